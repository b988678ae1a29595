"""The point / spot / directional / constant emitters on the GPU
(kernels.h emitter_sample_ext; the EM_ALL instantiations of k_shade, k_finish,
k_direct_shade and k_direct_resolve).  Films are 40 x 24 (not a multiple of the
16-pixel tile), at most 16 spp.  The oracle's `render` does not know these
emitters; the per-sample reference is emitter_ref's float32 restatement."""
import hashlib
import json
import os

import numpy as np
import pytest

import mtsg
from conftest import REPO, SCENES
import emitter_ref as E
from direct_ref import FILM_H, FILM_W, assert_same_mean, direct_desc
from test_gpu_direct import DIRECT, PATH, assert_bit_equal, params

pytestmark = pytest.mark.gpu

SMALL = {"width": FILM_W, "height": FILM_H, "spp": 4}
GOLDEN = os.path.join(REPO, "tests", "golden", "emitters_parent_samples.json")

# float32 roundings of one term value * bsdfVal / ne, from its.p and the shading
# frame to the term, in the longer of the two chains (the kernel's and the
# restatement's are the same operations):
#   common tail  value * (1 / emPdf): 2; toLocal(d).z: 5; the diffuse BSDF
#                (INV_PI * cos, * reflectance): 2; value * bsdfVal: 1; 1 / ne and
#                the product with it: 2                                   = 12
#   point        p - ref: 1; dot: 5; sqrt: 1; 1 / dist: 1; d * invDist: 1;
#                invDist^2: 1; intensity * it: 1                          = 11 -> 23
#   spot         point's 11, and dot(row, -d): 5; acosf: 1; cutoff - it: 1;
#                * invTransitionWidth: 1; intensity * falloff: 1          = 20 -> 32
#   directional  the value is the irradiance itself (d, the sphere and the
#                distance shape the shadow ray only)                      =  0 -> 12
#   constant     squareToCosineHemisphere: 10; INV_PI * z: 1; coordinateSystem:
#                6; cross: 3; toWorld: 5; 1 / pdf and radiance * it: 2    = 27 -> 39
ROUNDINGS = {"point": 23, "spot": 32, "directional": 12, "constant": 39}


def samples_of(scene, p):
    g = mtsg.GPUScene(scene, 0)
    try:
        return g.render_samples(p), g.kernel_sets()
    finally:
        g.close()


@pytest.mark.parametrize("ne", [1, 4])
@pytest.mark.parametrize("kind", ["point", "spot", "directional", "constant"])
def test_per_sample_restatement(kind, ne):
    """`direct` with emitterSamples 1 and 4, bsdfSamples 0, on the diffuse box
    lit by one emitter of the kind: per sample the unoccluded terms
    value * bsdfVal / ne of emitter_ref.emitters_reference.  A sample is fragile
    when one of its shadow rays changes its oracle answer under a 4-ulp move of
    a direction component (at most 2%, asserted on the CPU in
    test_emitters_scene.py); every other sample lies within
    k * 2^-23 * sum |term_i| with k = 2 * ROUNDINGS[kind] (counted above).  The
    spot's samples fall outside the cutoff, on the ramp and inside the beam.
    A primary miss under `constant` is the radiance exactly, and zero with
    hideEmitters.
    Measured on an MI355X, all eight cases: fragile share 0, maximum error 0 of
    the bound (every sample bit-equal to the restatement); lit samples of 3840:
    point 3321, spot 219, directional 2797, constant 3321."""
    scene = E.kind_scene(kind, "direct", [("emitterSamples", "integer", ne), ("bsdfSamples", "integer", 0)])
    P = E.primary(4)
    want, mag, fragile, branches = E.emitters_reference(P, E.kind_records(kind), ne)
    got, sets = samples_of(scene, scene.params())
    assert sets == (15 + 16, 2)   # every material class and BSDF plugin, every emitter kind
    a = got.reshape(-1, 4)
    assert ((a[:, 3] == 1) == P.hit).all()
    bound = 2 * ROUNDINGS[kind] * 2.0 ** -23 * mag.astype(np.float64)
    err = np.abs(a[:, :3].astype(np.float64) - want.astype(np.float64))
    ok = ~fragile
    lit = bound > 0
    worst = (err[ok][lit[ok]] / bound[ok][lit[ok]]).max()
    print(f"emitters {kind} ne={ne}: fragile {fragile.mean():.4f}, max error {worst:.3f} of the bound, "
          f"{np.abs(err[ok]).max():.3e} absolute, lit terms {int(lit.any(1).sum())}")
    assert fragile.mean() <= 0.02
    assert (err[ok] <= bound[ok]).all(), (kind, ne, worst)
    assert lit.any(1).mean() > (0.03 if kind == "spot" else 0.2)   # the check is not empty (the spot's cone is narrow)
    if kind == "spot":
        assert all((branches == k).sum() > 20 for k in (0, 1, 2))
    if kind == "constant":
        rad = np.array([0.8, 0.9, 1.0], np.float32)
        assert (a[P.miss, :3] == rad).all() and P.miss.any()
        hidden, _ = samples_of(scene, scene.params(hide_emitters=1))
        assert (hidden.reshape(-1, 4)[P.miss, :3] == 0).all()
    else:
        assert (a[P.miss, :3] == 0).all()


def test_spot_equals_point_inside_the_beam():
    """cutoffAngle 179, beamWidth 178: every direction the box sees is inside
    the beam, where falloffCurve is 1, so `path` maxDepth 3 is bit-equal."""
    pos = (0.1, 0.45, 2.9)
    m = E.xf([(1, 0, 0), (0, 1, 0), (0, 0, 1)], pos)
    m[:3, :3] = E.DOWN[:3, :3]
    inten = ("intensity", "spectrum", (9.0, 8.0, 7.0))
    out = []
    for em in (("point", [("position", "point", pos), inten]),
               ("spot", [("toWorld", "transform", m), inten, ("cutoffAngle", "float", 179.0), ("beamWidth", "float", 178.0)])):
        scene = E.mixed_scene(props=[("maxDepth", "integer", 3)], emitters=[em])
        out.append(samples_of(scene, scene.params())[0])
    # the spot looks down from above the box: everything below it is inside the beam
    assert out[0][..., :3].max() > 0
    assert (out[0].view(np.uint32) == out[1].view(np.uint32)).all()


@pytest.fixture(scope="module", params=["independent", "sobol"])
def mixed(request):
    scene = E.mixed_scene(sampler=request.param)
    g = mtsg.GPUScene(scene, 0)
    yield scene, g
    g.close()


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("hide", [0, 1])
def test_one_one_equals_path_depth_two(mixed, strict, hide):
    """test_gpu_direct's argument on the full box with a point, a spot, a
    directional and a constant emitter at unequal sampling weights: the weight
    of a delta emitter's sample is 1 in both integrators."""
    scene, g = mixed
    assert g.kernel_sets()[1] == 2
    a = assert_bit_equal(g, scene, strict_normals=strict, hide_emitters=hide)
    assert set(np.unique(a[..., 3])) == {0.0, 1.0}


def test_one_one_equals_path_in_a_two_level_scene(tmp_path):
    xml = open(os.path.join(SCENES, "cbox_inst.xml")).read()
    xml = xml.replace("</scene>", '<emitter type="point"><point name="position" x="0.2" y="1.2" z="0.5"/>'
                                  '<rgb name="intensity" value="2, 2, 2"/></emitter></scene>')
    for name in os.listdir(SCENES):   # the scene's meshes, by absolute path
        if name.endswith((".ply", ".obj", ".serialized")):
            xml = xml.replace(f'value="{name}"', f'value="{os.path.join(SCENES, name)}"')
    p = tmp_path / "cbox_inst_point.xml"
    p.write_text(xml)
    scene = mtsg.Scene(str(p), SMALL, instancing="two-level")
    g = mtsg.GPUScene(scene, 0)
    try:
        assert g.kernel_sets()[1] == 2
        assert_bit_equal(g, scene)
    finally:
        g.close()


def test_fans_and_the_tail_kernel():
    """`direct` (4, 2) under one seed against `path` maxDepth 2 under another:
    the same mean within 5 standard errors (film and six regions).  `path`
    maxDepth 5 at 16 spp from the bounce kernels against the same render with
    the tail kernel taking every path over after bounce 0: bit-equal, which
    pins k_finish's copy of the emitter sampling."""
    scene = E.mixed_scene(spp=16)
    g = mtsg.GPUScene(scene, 0)
    try:
        ref = g.render_samples(params(scene, PATH, seed=77))
        g.set_direct(direct_desc(4, 2))
        fan = g.render_samples(params(scene, DIRECT, seed=5))
        assert_same_mean(fan[..., :3], ref[..., :3], "direct (4,2) vs path")
        g.set_finish_paths(0)
        bounce = g.render_samples(params(scene, PATH, max_depth=5))
        assert g.stats().launches_finish == 0
        g.set_finish_paths(1 << 30)
        tail = g.render_samples(params(scene, PATH, max_depth=5))
        st = g.stats()
        assert st.launches_finish == 1 and st.paths_finish > 0
        assert np.array_equal(bounce, tail)
    finally:
        g.close()


def test_constant_against_a_uniform_envmap(tmp_path):
    """A 64 x 32 environment map of one value is the same light; the two sample
    the hemisphere differently, so only the means are compared."""
    rad = (0.8, 0.9, 1.0)
    pfm = tmp_path / "uniform.pfm"
    mtsg.write_pfm(str(pfm), np.broadcast_to(np.array(rad, np.float32), (32, 64, 3)).copy())
    out = []
    for seed, em in ((3, ("constant", [("radiance", "spectrum", rad)])), (11, ("envmap", [("filename", "string", str(pfm))]))):
        scene = E.mixed_scene(props=[("maxDepth", "integer", 3)], emitters=[em], spp=16)
        out.append(samples_of(scene, scene.params(seed=seed))[0])
    assert_same_mean(out[0][..., :3], out[1][..., :3], "constant vs uniform envmap")


@pytest.mark.parametrize("name,sets", [("cbox", (1, 0)), ("env_glass", (1 | 2 | 8, 1))])
def test_existing_scenes_keep_their_kernels(name, sets):
    """cbox.xml and env_glass.xml (with sky512.pfm) at 40 x 24 x 4: the per-sample
    values are those of the parent commit's build (SHA-256 of the float32 bytes,
    recorded on an MI355X from the parent's library), and the launchers select
    the material set and emitter set those scenes always ran."""
    scene = mtsg.Scene(os.path.join(SCENES, name + ".xml"), dict(SMALL, envmap=os.path.join(SCENES, "sky512.pfm")))
    got, selected = samples_of(scene, scene.params())
    assert selected == sets
    want = json.load(open(GOLDEN))[name]
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == want
