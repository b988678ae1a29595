"""The phong, ward, roughdiffuse, difftrans and thindielectric BSDFs on the
device: mtsg_bsdf_query against the float32 restatement of tests/bsdf_ref.py
and against the oracle for the older plugins, null events under hideEmitters,
`path` against `direct`, the tail kernel, twosided and instancing, the albedo
field, and the kernels each scene selects."""
import functools
import math
import os

import numpy as np
import pytest

import mtsg
from conftest import SCENES
import bsdf_ref as BR
import direct_ref as DR
import test_bsdf_chisquare as CS
from direct_ref import direct_desc
from multichannel_ref import Desc, xf
from test_gpu_direct import DIRECT, PATH, params

pytestmark = pytest.mark.gpu
f32 = np.float32

# (name, plugin, builder properties, the restatement's record)
MODELS = [
    ("phong", "phong", [("diffuseReflectance", "spectrum", (0.4, 0.3, 0.2)), ("specularReflectance", "spectrum", (0.5, 0.5, 0.4)),
                        ("exponent", "float", 18.0)], BR.phong((0.4, 0.3, 0.2), (0.5, 0.5, 0.4), 18.0)),
    ("ward", "ward", [("variant", "string", "ward"), ("diffuseReflectance", "spectrum", (0.3, 0.3, 0.3)),
                      ("specularReflectance", "spectrum", (0.5, 0.4, 0.5)), ("alphaU", "float", 0.15), ("alphaV", "float", 0.3)],
     BR.ward("ward", (0.3, 0.3, 0.3), (0.5, 0.4, 0.5), alphaU=0.15, alphaV=0.3)),
    ("ward-duer", "ward", [("variant", "string", "ward-duer"), ("diffuseReflectance", "spectrum", (0.3, 0.3, 0.3)),
                           ("specularReflectance", "spectrum", (0.5, 0.4, 0.5)), ("alphaU", "float", 0.3), ("alphaV", "float", 0.12)],
     BR.ward("ward-duer", (0.3, 0.3, 0.3), (0.5, 0.4, 0.5), alphaU=0.3, alphaV=0.12)),
    ("ward-balanced", "ward", [("diffuseReflectance", "spectrum", (0.3, 0.3, 0.3)), ("specularReflectance", "spectrum", (0.5, 0.4, 0.5)),
                               ("alphaU", "float", 0.2), ("alphaV", "float", 0.35)],
     BR.ward("balanced", (0.3, 0.3, 0.3), (0.5, 0.4, 0.5), alphaU=0.2, alphaV=0.35)),
    ("roughdiffuse", "roughdiffuse", [("reflectance", "spectrum", (0.5, 0.3, 0.8)), ("alpha", "float", 0.6)],
     BR.roughdiffuse((0.5, 0.3, 0.8), 0.6, False)),
    ("roughdiffuse-fast", "roughdiffuse", [("reflectance", "spectrum", (0.5, 0.3, 0.8)), ("alpha", "float", 0.6),
                                           ("useFastApprox", "boolean", True)], BR.roughdiffuse((0.5, 0.3, 0.8), 0.6, True)),
    ("difftrans", "difftrans", [("transmittance", "spectrum", (0.5, 0.3, 0.8))], BR.difftrans((0.5, 0.3, 0.8))),
    ("thindielectric", "thindielectric", [("specularReflectance", "spectrum", (0.9, 0.8, 1.0)),
                                          ("specularTransmittance", "spectrum", (0.7, 1.0, 0.9))],
     BR.thindielectric(specularReflectance=(0.9, 0.8, 1.0), specularTransmittance=(0.7, 1.0, 0.9))),
]
NAMES = [m[0] for m in MODELS]

# Largest relative difference between the device and the restatement over the
# queries of test_query_against_the_restatement, measured on an MI355X; the
# bound of each model is twice that (the config tests' convention).  0: every
# float of every query is bit-equal.
MEASURED = {n: 0.0 for n in NAMES}


def camera(b, width=DR.FILM_W, height=DR.FILM_H, sampler="independent", spp=4, film_props=()):
    b.sensor("perspective", [("fov", "float", 40.0), ("toWorld", "transform", xf([(-1, 0, 0), (0, 1, 0), (0, 0, -1)], (0.05, 0.1, 3.6)))])
    b.film("hdrfilm", [("width", "integer", width), ("height", "integer", height), ("pixelFormat", "string", "rgba")] + list(film_props),
           "gaussian", [])
    b.sampler(sampler, [("sampleCount", "integer", spp)])


def add_models(b, which=NAMES, group=-1):
    """One object per model in front of the box's back wall: cubes for the
    reflecting models, free-standing panes (lit from behind by the box's
    lights and walls) for difftrans and thindielectric.  Returns the BSDF ids."""
    ids = {}
    for k, (name, plugin, props, _ref) in enumerate(MODELS):
        if name not in which:
            continue
        ids[name] = b.bsdf(plugin, props)
        x = -0.95 + 0.27 * k
        if plugin in ("difftrans", "thindielectric"):
            b.shape("rectangle", [("toWorld", "transform", xf([(0.12, 0, 0), (0, 0.25, 0), (0, 0, 1)], (x, 0.15, 0.5)))], ids[name], -1, group)
        else:
            b.shape("cube", [("toWorld", "transform", xf([(0.1, 0, 0.03), (0, 0.12, 0), (-0.03, 0, 0.1)], (x, -0.25, 0.45)))], ids[name], -1, group)
    return ids


def models_scene(integrator="path", props=(("maxDepth", "integer", 2),), which=NAMES, sampler="independent", spp=4, instancing="flatten"):
    b = mtsg.SceneBuilder(SCENES, instancing=instancing)
    b.integrator(integrator, list(props))
    camera(b, sampler=sampler, spp=spp)
    DR.box_geometry(b, diffuse_only=True)
    ids = add_models(b, which)
    return b.finish(), ids


@pytest.fixture(scope="module")
def models():
    scene, ids = models_scene()
    g = mtsg.GPUScene(scene, 0)
    yield scene, g, ids
    g.close()


def queries(n, seed, both_sides):
    """wi over the sphere (or the upper hemisphere), with the poles, grazing and tangent directions; samples in [0, 1)."""
    rng = np.random.default_rng(seed)
    wi = rng.normal(size=(n, 3))
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    if not both_sides:
        wi[:, 2] = np.abs(wi[:, 2])
    wi = wi.astype(f32)
    g = math.sqrt(1 - 1e-6)
    wi[:8] = [(0, 0, 1), (0, 0, -1), (g, 0, 1e-3), (0, -g, 1e-3), (g, 0, -1e-3), (1, 0, 0), (0, 1, 0), (-math.sqrt(0.5), math.sqrt(0.5), 0)]
    u = rng.random((n, 3), dtype=np.float32)
    u[8:16, 0] = [0.0, 0.0, 0.5, 0.99999994, 0.25, 0.75, 0.5, 0.5]
    u[8:16, 1] = [0.0, 0.5, 0.0, 0.99999994, 0.5, 0.5, 0.25, 0.75]
    return wi, u


def rel_diff(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(got - want) / np.abs(want)
    d = np.where(got == want, 0.0, d)
    return float(np.nan_to_num(d, nan=np.inf).max()) if d.size else 0.0


@pytest.mark.parametrize("name", NAMES)
def test_query_against_the_restatement(models, name):
    """4096 queries per model, wi over both hemispheres with wi.z = +-1, grazing
    1e-3 and 0: sample mode (wo, weight, pdf, eta, flags), then eval mode at the
    sampled wo and at random wo.  The flags agree on every query; every float
    lies within 2 x MEASURED[name] relative of the restatement (0: bit-equal)."""
    scene, g, ids = models
    ref = MODELS[NAMES.index(name)][3]
    wi, u = queries(4096, 100 + NAMES.index(name), both_sides=True)
    wo, w, pdf, eta, flags = g.bsdf_query(ids[name], wi, sample=u)
    rwo, rw, rpdf, reta, rflags = BR.sample(ref, wi, u)
    worst = max(rel_diff(wo, rwo), rel_diff(w, rw), rel_diff(pdf, rpdf), rel_diff(eta, reta))
    mism = int((flags != rflags).sum())
    rng = np.random.default_rng(5)
    wr = rng.normal(size=(4096, 3))
    wr = (wr / np.linalg.norm(wr, axis=1, keepdims=True)).astype(f32)
    worst_e = 0.0
    for dirs in (np.where((rflags != 0)[:, None], rwo, wr), wr):
        val, p = g.bsdf_query(ids[name], wi, wo=dirs)
        rval, rp = BR.evaluate(ref, wi, dirs)
        worst_e = max(worst_e, rel_diff(val, rval), rel_diff(p, rp))
    print(f"bsdf query {name}: flags differ on {mism} of 4096, sample max rel diff {worst:.3e}, eval {worst_e:.3e}, "
          f"successful samples {int((rflags != 0).sum())}")
    assert mism == 0
    assert (rflags != 0).mean() > 0.2   # (half of the incident directions are below a reflecting model)
    bound = 2 * MEASURED[name]
    assert worst <= bound and worst_e <= bound, (name, worst, worst_e, bound)


@pytest.mark.parametrize("name", NAMES[:-1])
def test_query_histogram_matches_the_pdf(models, name):
    """The device's sampled wo over 10 x 20 cells against the restatement's pdf: the
    chi-square test of test_bsdf_chisquare.py (grid, 200k samples, significance)."""
    scene, g, ids = models
    ref = MODELS[NAMES.index(name)][3]
    wi = np.array([0.5, -0.3, math.sqrt(1 - 0.34)], f32)
    u = np.random.default_rng(21).random((CS.N_SAMPLES, 3), dtype=np.float32)
    wo, w, pdf, eta, flags = g.bsdf_query(ids[name], np.broadcast_to(wi, (CS.N_SAMPLES, 3)), sample=u)
    saved = CS.evaluate
    CS.evaluate = lambda b_, wi_, d: BR.evaluate(b_, wi_, d, exact=False)
    try:
        exp = CS.expected_counts(ref, wi, CS.N_SAMPLES, reachable_only=False)
    finally:
        CS.evaluate = saved
    p = CS.chi2_pvalue(CS.observed_counts(wo[flags != 0]), exp)
    assert p >= CS.SIGNIFICANCE, f"{name}: chi-square p-value {p:.3e}"


def test_older_plugins_through_the_query():
    """diffuse, GGX roughconductor, dielectric and roughplastic records through
    mtsg_bsdf_query against oracle_bsdf_sample3_n / oracle_bsdf_eval_n.  The
    oracle's libm and the device's restated glibc functions agree to the last bit
    but for rare arguments, and test_gpu_parity.py bounds what is left at 1e-3 of
    the value: the same bound holds here per query, with equal event types."""
    b = mtsg.SceneBuilder(SCENES)
    b.integrator("path", [])
    camera(b)
    DR.box_geometry(b, diffuse_only=True)
    ids = [b.bsdf("diffuse", [("reflectance", "spectrum", (0.5, 0.3, 0.8))]),
           b.bsdf("roughconductor", [("distribution", "string", "ggx"), ("alpha", "float", 0.25)]),
           b.bsdf("dielectric", []),
           b.bsdf("roughplastic", [("distribution", "string", "beckmann"), ("alpha", "float", 0.15), ("intIOR", "float", 1.49)])]
    for k, i in enumerate(ids):
        b.shape("cube", [("toWorld", "transform", xf([(0.1, 0, 0), (0, 0.1, 0), (0, 0, 0.1)], (-0.6 + 0.3 * k, -0.3, 0.5)))], i)
    scene = b.finish()
    recs = Desc(scene).bsdfs
    g = mtsg.GPUScene(scene, 0)
    try:
        assert g.kernel_sets() == (15 + 16, 0)   # no new type: the kernels such a scene always ran
        rng = np.random.default_rng(9)
        for i in ids:
            rec = recs[i]
            wis = CS.random_wi(rng, 6) + [np.array([0, 0, 1], f32), np.array([math.sqrt(1 - 1e-4), 0, 1e-2], f32)]
            if rec.type == CS.DIELECTRIC:
                wis = [w * (1 if k % 2 == 0 else -1) for k, w in enumerate(wis)]   # from inside too
            for wi in wis:
                n = 256
                u = rng.random((n, 3), dtype=np.float32)
                wo, w, pdf, eta, flags = g.bsdf_query(i, np.broadcast_to(wi, (n, 3)), sample=u)
                owo, opdf, ow, ot = CS.sample(rec, wi, u)
                ok = (opdf > 0) & (ow.max(1) > 0)
                assert (ok == (flags != 0)).mean() > 0.99, (rec.type, wi)
                sel = ok & (flags != 0)
                assert sel.mean() > 0.3
                np.testing.assert_allclose(wo[sel], owo[sel], rtol=1e-3, atol=1e-5)
                np.testing.assert_allclose(w[sel], ow[sel], rtol=1e-3, atol=1e-6)
                np.testing.assert_allclose(pdf[sel], opdf[sel], rtol=1e-3, atol=1e-6)
                assert (((flags[sel] & BR.DELTA) != 0) == ((ot[sel] & CS.DELTA) != 0)).all()
                assert ((flags & BR.NULL) == 0).all()
                val, p = g.bsdf_query(i, np.broadcast_to(wi, (int(sel.sum()), 3)), wo=owo[sel])
                oval, op = CS.evaluate(rec, wi, owo[sel])
                np.testing.assert_allclose(val, oval, rtol=1e-3, atol=1e-6)
                np.testing.assert_allclose(p, op, rtol=1e-3, atol=1e-6)
    finally:
        g.close()


# ---------------------------------------------------------------------------
# null events
# ---------------------------------------------------------------------------
def pane_scene(integrator, props):
    b = mtsg.SceneBuilder(SCENES)
    b.integrator(integrator, list(props))
    camera(b, 16, 16)
    b.emitter("constant", [("radiance", "spectrum", (1.0, 1.0, 1.0))])
    b.shape("rectangle", [("toWorld", "transform", xf([(0.8, 0, 0), (0, 0.5, 0), (0, 0, 1)], (0.1, 0.2, 0.0)))], b.bsdf("thindielectric", []))
    return b.finish()


def test_null_events_and_hide_emitters():
    """A constant emitter of radiance 1 and one default thindielectric pane,
    `path` with maxDepth -1.  Every sample is exactly 1; with hideEmitters a
    sample that misses the pane is 0, and one that hits it is 1 exactly when its
    BSDF draw has sample.x <= R' at its incidence cosine (the reflected ray left
    a scattering event behind, the transmitted one a null event: path.cpp:213,
    238).  `direct` (1, 1) with hideEmitters follows the same rule with its own
    draws (direct.cpp:288).  Without the null bit the transmitted samples are 1."""
    scene = pane_scene("path", [("maxDepth", "integer", -1)])
    g = mtsg.GPUScene(scene, 0)
    try:
        assert g.kernel_sets() == (15 + 16 + 32, 2)
        p = params(scene, PATH, max_depth=-1)
        shown = g.render_samples(p)
        assert (shown[..., :3] == 1).all()
        hit = shown[..., 3] == 1
        assert 0.2 < hit.mean() < 0.8
        ph = params(scene, PATH, max_depth=-1, hide_emitters=1)
        hidden = g.render_samples(ph)
        assert (hidden[~hit][:, :3] == 0).all()
        ys, xs, ss = np.nonzero(hit)
        rays = g.camera_rays(ph, np.stack([xs, ys, ss], 1))
        wi = np.zeros((len(xs), 3), f32)
        wi[:, 2] = -rays[:, 5]   # the pane's normal is +z: cosTheta(wi) = -d.z
        R = BR.thin_reflectance(BR.thindielectric(), wi)

        def check(got, p, kinds):
            """kinds: the sample's draws up to the BSDF's next2D, whose first number decides"""
            sx = np.array([g.sampler_draws(p, int(x), int(y), int(s), kinds)[2 * len(kinds) - 2] for x, y, s in zip(xs, ys, ss)], f32)
            want = (sx <= R).astype(f32)
            assert 0.02 < want.mean() < 0.5   # both events occur
            assert (got[~hit][:, :3] == 0).all()
            assert (got[ys, xs, ss][:, :3] == want[:, None]).all(), int((got[ys, xs, ss][:, 0] != want).sum())

        check(hidden, ph, [2, 2])   # the pixel sample, then the BSDF sample (no emitter sample: the BSDF is not smooth)
        g.set_direct(direct_desc(1, 1))
        pd = params(scene, DIRECT, hide_emitters=1)
        check(g.render_samples(pd), pd, [2, 2, 2])   # direct draws its emitter sample whatever the BSDF (direct.cpp:210-214)
    finally:
        g.close()


# ---------------------------------------------------------------------------
# path against direct, the tail kernel, wrappers and scene routes
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["independent", "sobol"])
def sampled(request):
    scene, ids = models_scene(sampler=request.param)
    g = mtsg.GPUScene(scene, 0)
    yield scene, g
    g.close()


@pytest.mark.parametrize("strict", [0, 1])
def test_one_one_equals_path_depth_two(sampled, strict):
    """test_gpu_direct's argument over a box that holds every model: direct (1, 1)
    and path maxDepth 2 draw the same numbers and weight them alike, sample for sample."""
    from test_gpu_direct import assert_bit_equal
    scene, g = sampled
    assert g.kernel_sets() == (15 + 16 + 32, 2)
    a = assert_bit_equal(g, scene, strict_normals=strict)
    assert set(np.unique(a[..., 3])) == {0.0, 1.0}


def test_tail_kernel_equals_the_bounce_kernels():
    """phong + thindielectric in the box, maxDepth 6: every path through k_finish
    after bounce 0 against the tail kernel off, bit for bit (test_gpu_finish.py's criterion)."""
    scene, _ = models_scene(props=[("maxDepth", "integer", 6)], which=("phong", "thindielectric"), spp=8)
    g = mtsg.GPUScene(scene, 0)
    try:
        g.set_finish_paths(0)
        bounce = g.render_samples(params(scene, PATH, max_depth=6))
        assert g.stats().launches_finish == 0
        g.set_finish_paths(1 << 30)
        tail = g.render_samples(params(scene, PATH, max_depth=6))
        st = g.stats()
        assert st.launches_finish == 1 and st.paths_finish > 0
        assert np.isfinite(bounce).all() and bounce[..., :3].max() > 0
        assert np.array_equal(bounce.view(np.uint32), tail.view(np.uint32))
    finally:
        g.close()


def test_twosided_phong_from_behind_equals_phong_on_a_flipped_pane():
    """A pane whose normal points away from the camera with twosided(phong)
    against the same pane turned round with plain phong: the wrapper negates
    wi.z and wo.z (twosided.cpp:103-170), the turned pane's frame negates the
    normal and one tangent, and phong depends on neither tangent's sign."""
    out = []
    for wrapped in (True, False):
        b = mtsg.SceneBuilder(SCENES)
        b.integrator("path", [("maxDepth", "integer", 3)])
        camera(b)
        DR.box_geometry(b, diffuse_only=True)
        ph = b.bsdf("phong", MODELS[0][2])
        if wrapped:   # local z = world -z: seen from behind
            b.shape("rectangle", [("toWorld", "transform", xf([(0.3, 0, 0), (0, -0.3, 0), (0, 0, -1)], (-0.4, 0.0, 0.5)))],
                    b.bsdf("twosided", [], nested=(ph,)))
        else:
            b.shape("rectangle", [("toWorld", "transform", xf([(0.3, 0, 0), (0, 0.3, 0), (0, 0, 1)], (-0.4, 0.0, 0.5)))], ph)
        scene = b.finish()
        g = mtsg.GPUScene(scene, 0)
        try:
            out.append(g.render_samples(params(scene, PATH, max_depth=3)))
        finally:
            g.close()
    assert out[0][..., :3].max() > 0
    # the two frames differ in the sign of one tangent: the lobe's azimuth is
    # mirrored sample by sample, so the films agree in the mean, not per sample
    DR.assert_same_mean(out[0][..., :3], out[1][..., :3], "twosided(phong) from behind vs phong on the turned pane")


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), (0.2, 0.05, 0.1)])
def test_roughdiffuse_in_an_instance_flattened_and_two_level(offset):
    """A roughdiffuse cube inside a shapegroup instance, flattened and two-level,
    with the identity and with a translation as the instance's toWorld.  The
    two-level traversal intersects the cube in the group's space and carries the
    hit back through the instance's transform (instance.cpp), the flattened scene
    holds world-space triangles: a path that meets the cube has the same hit up
    to the last bits, and at a silhouette it may go elsewhere.  Measured on an
    MI355X: 0.65% (identity) and 0.76% (translation) of the samples differ; the
    bound is twice the larger figure, so at least 98.48% of the samples must be
    the same floats.  At least 99% agree to 1e-4 of the value, and the two films
    have the same mean.  In each scene the tail kernel's
    instantiation (flat, two-level) gives the bounce kernels' samples bit for bit."""
    out = []
    for instancing in ("flatten", "two-level"):
        b = mtsg.SceneBuilder(SCENES, instancing=instancing)
        b.integrator("path", [("maxDepth", "integer", 3)])
        camera(b)
        DR.box_geometry(b, diffuse_only=True)
        grp = b.group("g")
        add_models(b, ("roughdiffuse",), group=grp)
        b.instance(grp, [("toWorld", "transform", xf([(1, 0, 0), (0, 1, 0), (0, 0, 1)], offset))])
        scene = b.finish()
        g = mtsg.GPUScene(scene, 0)
        try:
            assert g.kernel_sets()[0] == 15 + 16 + 32
            out.append(g.render_samples(params(scene, PATH, max_depth=3)))
            g.set_finish_paths(1 << 30)   # the tail kernel's two-level instantiation too
            tail = g.render_samples(params(scene, PATH, max_depth=3))
            assert np.array_equal(tail.view(np.uint32), out[-1].view(np.uint32))
        finally:
            g.close()
    same = (out[0].view(np.uint32) == out[1].view(np.uint32)).all(-1)
    print(f"roughdiffuse instance at {offset}: {same.mean():.4f} of the samples identical")
    close = np.isclose(out[0], out[1], rtol=1e-4, atol=1e-7).all(-1)
    assert same.mean() >= 1 - 2 * 0.0076 and close.mean() > 0.99, (same.mean(), close.mean())   # measured 0.9935 / 0.9924
    DR.assert_same_mean(out[0][..., :3], out[1][..., :3], "flattened vs two-level")


def test_albedo_field():
    """multichannel with path + albedo + shapeIndex over one pane per model: the
    parameter for phong, ward and roughdiffuse (their getDiffuseReflectance), zero for
    difftrans and thindielectric (the base class's eval(EDiffuseReflection) * pi, bsdf.cpp:82-86)."""
    b = mtsg.SceneBuilder(SCENES)
    for c in ("path", "albedo", "shapeIndex"):
        if c == "path":
            b.integrator_child("path", [("maxDepth", "integer", 2)])
        else:
            b.integrator_child("field", [("field", "string", c)])
    b.multichannel()
    b.sensor("perspective", [("fov", "float", 40.0), ("toWorld", "transform", xf([(-1, 0, 0), (0, 1, 0), (0, 0, -1)], (0.05, 0.1, 3.6)))])
    b.film("hdrfilm", [("width", "integer", 40), ("height", "integer", 24), ("pixelFormat", "string", "rgb, rgb, rgb"),
                       ("channelNames", "string", "a, b, c")], "gaussian", [])
    b.sampler("independent", [("sampleCount", "integer", 4)])
    want = {}
    for k, (name, plugin, props, ref) in enumerate(MODELS):
        i = b.bsdf(plugin, props)
        b.shape("rectangle", [("toWorld", "transform", xf([(0.14, 0, 0), (0, 0.6, 0), (0, 0, 1)], (-1.0 + 0.29 * k, 0.1, 0.0)))], i)
        want[k] = ref.reflectance if plugin in ("phong", "ward", "roughdiffuse") else np.zeros(3, f32)
    light = b.emitter("area", [("radiance", "spectrum", (5.0, 5.0, 5.0))])
    b.shape("rectangle", [("toWorld", "transform", xf([(0.4, 0, 0), (0, 0, 0.4), (0, -1, 0)], (0, 1.5, 1.0)))], -1, light)
    scene = b.finish()
    g = mtsg.GPUScene(scene, 0)
    try:
        g.set_aov(scene)
        s = g.render_samples_multi(scene.params())
    finally:
        g.close()
    albedo, shape, alpha = s[..., 3:6], s[..., 6], s[..., 9]
    seen = 0
    for k, w in want.items():
        on = (alpha == 1) & (shape == k)
        assert on.sum() > 20, (k, int(on.sum()))
        assert (albedo[on] == w).all(), (MODELS[k][0], albedo[on][:2], w)
        seen += 1
    assert seen == len(MODELS)


@pytest.mark.parametrize("name,sets", [("cbox", (1, 0)), ("env_glass", (1 | 2 | 8, 1)), ("cbox_roughplastic", (15 + 16, 0)),
                                       ("cbox_textured", (15 + 16, 0))])
def test_existing_scenes_keep_their_kernels(name, sets):
    """The material and emitter sets the launchers select for scenes without a new
    type, as the commit before the five plugins reports them."""
    scene = mtsg.Scene(os.path.join(SCENES, name + ".xml"), {"width": 40, "height": 24, "spp": 4, "envmap": os.path.join(SCENES, "sky512.pfm")})
    g = mtsg.GPUScene(scene, 0)
    try:
        assert g.kernel_sets() == sets
    finally:
        g.close()


# ---------------------------------------------------------------------------
# records the query had not met: twosided fronts and a textured parameter
# ---------------------------------------------------------------------------
def record_ref(rec):
    """The restatement's record of a descriptor record (its fields as the device reads them)."""
    r = BR.Record(rec.type, reflectance=list(rec.reflectance), spec_refl=list(rec.spec_refl), spec_trans=list(rec.spec_trans),
                  alpha_u=rec.alpha_u, alpha_v=rec.alpha_v, distribution=rec.distribution, nonlinear=rec.nonlinear,
                  ior_eta=rec.ior_eta, spec_sampling_weight=rec.spec_sampling_weight, smooth=rec.smooth, ref_n_zero=rec.ref_n_zero)
    return r


def assert_query_equals(g, bsdf, wi, u, want_sample, evaluate, alb=None):
    wo, w, pdf, eta, flags = g.bsdf_query(bsdf, wi, sample=u, alb=alb)
    rwo, rw, rpdf, reta, rflags = want_sample
    assert (flags == rflags).all()
    for a, b in ((wo, rwo), (w, rw), (pdf, rpdf), (eta, reta)):
        assert (a.view(np.uint32) == b.view(np.uint32)).all() or rel_diff(a, b) == 0, rel_diff(a, b)
    val, p = g.bsdf_query(bsdf, wi, wo=rwo, alb=alb)
    rval, rp = evaluate(rwo)
    assert rel_diff(val, rval) == 0 and rel_diff(p, rp) == 0, (rel_diff(val, rval), rel_diff(p, rp))
    return rflags


def test_twosided_front_record_through_the_query():
    """twosided(phong, roughdiffuse), front and back with different reflectances: a
    query with wi.z > 0 is the phong record's, one with wi.z < 0 is the roughdiffuse
    record's with wi.z and wo.z negated (twosided.cpp:103-170), bit for bit; wi.z = 0
    goes to the front record in sample mode and to the back record in eval mode."""
    b = mtsg.SceneBuilder(SCENES)
    b.integrator("path", [])
    camera(b)
    DR.box_geometry(b, diffuse_only=True)
    ph = b.bsdf("phong", MODELS[0][2])
    rd = b.bsdf("roughdiffuse", MODELS[4][2])
    two = b.bsdf("twosided", [], nested=(ph, rd))
    b.shape("rectangle", [("toWorld", "transform", xf([(0.3, 0, 0), (0, 0.3, 0), (0, 0, 1)], (-0.4, 0.0, 0.5)))], two)
    scene = b.finish()
    front, back = MODELS[0][3], MODELS[4][3]
    flip = np.array([1, 1, -1], f32)
    g = mtsg.GPUScene(scene, 0)
    try:
        wi, u = queries(2048, 77, both_sides=True)
        up, down = wi[:, 2] > 0, wi[:, 2] < 0
        ok = assert_query_equals(g, two, wi[up], u[up], BR.sample(front, wi[up], u[up]), lambda d: BR.evaluate(front, wi[up], d))
        assert ok.mean() > 0.8
        rwo, rw, rpdf, reta, rflags = BR.sample(back, wi[down] * flip, u[down])
        ok = assert_query_equals(g, two, wi[down], u[down], ((rwo * flip).astype(f32), rw, rpdf, reta, rflags),
                                 lambda d: BR.evaluate(back, wi[down] * flip, (d * flip).astype(f32)))
        assert ok.mean() > 0.9
        # the same wo for both sides, so that the back record's eval is not trivially zero
        rng = np.random.default_rng(3)
        wo = rng.normal(size=(int(down.sum()), 3))
        wo = (wo / np.linalg.norm(wo, axis=1, keepdims=True)).astype(f32)
        val, p = g.bsdf_query(two, wi[down], wo=wo)
        rval, rp = BR.evaluate(back, wi[down] * flip, (wo * flip).astype(f32))
        assert rel_diff(val, rval) == 0 and rel_diff(p, rp) == 0 and (rp > 0).mean() > 0.3
    finally:
        g.close()


def test_bitmap_diffuse_reflectance_reaches_the_models():
    """ward with a bitmap diffuseReflectance and specularReflectance 0.6 (the pair
    energy conservation scales the BSDF's copy of the texture): the value the
    shading kernels pass as `alb` is mtsg_tex_eval's times the texture's scale.
    Fed through the query at 2048 random uv, sample and eval are the restatement's
    with the same values, bit for bit: the texel reaches ward_eval's diffuse term, and
    the sampling weight is the one configure() derived from the scaled texture
    (tests/test_bsdfs_scene.py checks the record).  phong, roughdiffuse and difftrans
    take their texel through the same argument."""
    b = mtsg.SceneBuilder(SCENES)
    b.integrator("path", [])
    camera(b)
    DR.box_geometry(b, diffuse_only=True)
    tex = b.texture("bitmap", [("filename", "string", "tex_checker.png"), ("filterType", "string", "nearest")])
    ids = [b.bsdf("ward", [("diffuseReflectance", "texture", tex), ("specularReflectance", "spectrum", (0.6, 0.6, 0.6)),
                           ("alphaU", "float", 0.2), ("alphaV", "float", 0.3)]),
           b.bsdf("phong", [("diffuseReflectance", "texture", tex), ("specularReflectance", "spectrum", (0.6, 0.6, 0.6))]),
           b.bsdf("roughdiffuse", [("reflectance", "texture", tex)]),
           b.bsdf("difftrans", [("transmittance", "texture", tex)])]
    for k, i in enumerate(ids):
        b.shape("rectangle", [("toWorld", "transform", xf([(0.12, 0, 0), (0, 0.25, 0), (0, 0, 1)], (-0.6 + 0.3 * k, 0.15, 0.5)))], i)
    scene = b.finish()
    recs, texs = Desc(scene).bsdfs, scene.textures()
    g = mtsg.GPUScene(scene, 0)
    try:
        rng = np.random.default_rng(12)
        for i in ids:
            rec = recs[i]
            assert rec.texture > 0
            t = texs[rec.texture - 1]
            ref = record_ref(rec)
            wi, u = queries(2048, 300 + i, both_sides=True)
            uv = rng.random((2048, 2), dtype=np.float32)
            alb = (g.tex_eval(rec.texture - 1, uv) * f32(t.scale)).astype(f32)
            assert len(np.unique(alb, axis=0)) >= 2   # the checker's two colours
            ok = assert_query_equals(g, i, wi, u, BR.sample(ref, wi, u, alb=alb), lambda d: BR.evaluate(ref, wi, d, alb=alb), alb=alb)
            assert ok.mean() > 0.2
            # and the texel matters: the record's constant (the texture's average) gives other values
            val, _ = g.bsdf_query(i, wi, wo=BR.sample(ref, wi, u, alb=alb)[0])
            val2, _ = g.bsdf_query(i, wi, wo=BR.sample(ref, wi, u, alb=alb)[0], alb=alb)
            assert (val != val2).any()
    finally:
        g.close()


# ---------------------------------------------------------------------------
# whole `direct` renders against a per-sample restatement
# ---------------------------------------------------------------------------
# Largest error of a sample over sum |term_i| * 2^-23, per model, measured on an
# MI355X over both sample counts; the bound is twice that.  0: every sample is
# the restatement's float (measured: 0 of 3840 samples differ in all 16 cases;
# 118-156 lit samples on the cubes, 295 on the difftrans pane, 36 and 80 on the
# thindielectric pane).
RENDER_MEASURED = {n: 0.0 for n in NAMES}


def add_lit_object(b, name):
    """One object of the model where the box's rectangle light (at y = 0.99 over the
    middle of the box, facing down) reaches what the camera sees of it: a tilted cube
    behind the light's z for the reflecting models, so that its front and top faces
    are lit; an upright pane in front of the light for difftrans, lit from behind; and
    for thindielectric a pane tilted so that camera rays are mirrored towards the light."""
    _n, plugin, props, _ref = MODELS[NAMES.index(name)]
    i = b.bsdf(plugin, props)
    if plugin == "thindielectric":
        b.shape("rectangle", [("toWorld", "transform", xf([(0.35, 0, 0), (0, 0.505 * 0.35, -0.863 * 0.35), (0, 0.863, 0.505)], (0.0, 0.1, 0.5)))], i)
    elif plugin == "difftrans":
        b.shape("rectangle", [("toWorld", "transform", xf([(0.2, 0, 0), (0, 0.3, 0), (0, 0, 1)], (-0.3, 0.15, 0.5)))], i)
    else:
        b.shape("cube", [("toWorld", "transform", xf([(0.2, 0, 0.06), (0, 0.2, 0), (-0.06, 0, 0.2)], (-0.1, -0.2, -0.5)))], i)


@functools.lru_cache(maxsize=None)
def _lit_primary(name):
    """The oracle's camera samples and hits of the box with the model's object, shared by the two sample counts."""
    import bsdf_render_ref as RR
    return RR.primary(4, lambda b: add_lit_object(b, name))


@pytest.mark.parametrize("counts", [(1, 1), (4, 2)])
@pytest.mark.parametrize("name", NAMES)
def test_direct_render_against_the_restatement(name, counts):
    """`direct` with (emitterSamples, bsdfSamples) = (1, 1) and (4, 2) over the
    diffuse box with one object of the model (a cube; a back-lit pane for difftrans
    and thindielectric): every sample against bsdf_render_ref.direct_reference, which
    takes the oracle's camera rays, hits, BSDF-ray hits and shadow rays, the counter
    RNG's draws and the numpy BSDFs.  No sample is left out: every one lies within
    2 x RENDER_MEASURED[name] x 2^-23 x sum |term_i| of the restatement (0: the same
    float).  Samples that see the object itself are among them."""
    import bsdf_render_ref as RR
    ne, nb = counts
    add = lambda b: add_lit_object(b, name)
    P = _lit_primary(name)
    want, mag, fragile = RR.direct_reference(P, ne, nb)
    scene = RR.scene(add, ne, nb)
    g = mtsg.GPUScene(scene, 0)
    try:
        assert g.kernel_sets() == (15 + 16 + 32, 2)
        g.set_direct(direct_desc(ne, nb))
        got = g.render_samples(params(scene, DIRECT)).reshape(-1, 4)
    finally:
        g.close()
    assert ((got[:, 3] == 1) == P.hit).all()
    model = np.array([P.D.bsdfs[k].type >= BR.PHONG if k >= 0 else False for k in P.bsdf])
    assert model.sum() > 40, int(model.sum())
    err = np.abs(got[:, :3].astype(np.float64) - want.astype(np.float64))
    unit = 2.0 ** -23 * mag.astype(np.float64)
    with np.errstate(all="ignore"):
        rel = np.where(err == 0, 0.0, err / unit)
    worst = float(np.nan_to_num(rel, nan=np.inf).max())
    differ = (err != 0).any(1)
    print(f"direct {name} ({ne}, {nb}): {int(differ.sum())} of {len(err)} samples differ ({int((differ & model).sum())} on the object), "
          f"max error {worst:.3f} x 2^-23 x sum|terms|, fragile shadow rays on {int(fragile.sum())} samples, object samples {int(model.sum())}, "
          f"lit object samples {int(((want != 0).any(1) & model).sum())}")
    assert ((want != 0).any(1) & model).sum() > 20
    assert worst <= 2 * RENDER_MEASURED[name], (name, counts, worst)
