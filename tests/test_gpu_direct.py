"""The `direct` integrator on the GPU (csrc/direct.hip; direct.cpp:146-309).

Parity is pinned through `path`: with emitterSamples = bsdfSamples = 1,
`direct` is algebraically `path` with maxDepth 2 on scenes whose BSDFs are all
smooth -- both draw the emitter 2D sample, then the BSDF 2D sample
(direct.cpp:210-263, path.cpp:168-221), miWeight(a/2, b/2) == miWeight(a, b) in
float, and `path` adds nothing at depth 2 -- so the per-sample values must be
equal bit for bit, and the film must pass the oracle's `path` check.  Larger
fans (sample arrays) are unbiased estimators of the same image: their means
agree with `path` within the samples' own standard errors, and the
emitters-only fan (4, 0) equals, per sample, a float32 numpy restatement from
oracle pieces (direct_ref.emitters_only_reference).  Films are 40 x 24 (not a
multiple of the 16-pixel tile), at most 16 spp."""
import ctypes as C
import os

import numpy as np
import pytest

import mtsg
from oracle import pyoracle as O
from conftest import SCENES
import direct_ref
from direct_ref import FILM_H, FILM_W, assert_same_mean, box_scene, direct_desc
from test_gpu_parity import check_render

pytestmark = pytest.mark.gpu

PATH, DIRECT = mtsg.MTSG_INTEGRATOR_PATH, mtsg.MTSG_INTEGRATOR_DIRECT
SMALL = {"width": FILM_W, "height": FILM_H, "spp": 4}


def params(scene, integrator, **over):
    over.setdefault("max_depth", 2)
    p = scene.params(**over)
    p.integrator = integrator
    return p


def assert_bit_equal(g, scene, **over):
    """direct (1,1) and path maxDepth 2, per sample: radiance and alpha."""
    g.set_direct(direct_desc(1, 1))
    a = g.render_samples(params(scene, DIRECT, **over))
    b = g.render_samples(params(scene, PATH, **over))
    assert a.shape == (FILM_H, FILM_W, scene.params().spp, 4)
    assert np.isfinite(b).all() and b[..., :3].max() > 0
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), (int(diff.sum()), a[diff][:4], b[diff][:4])
    return a


@pytest.fixture(scope="module", params=["independent", "sobol"])
def box(request):
    scene = box_scene(sampler=request.param)
    g = mtsg.GPUScene(scene, 0)
    yield scene, g
    g.close()


@pytest.fixture(scope="module")
def box16():
    """The box at 16 spp, with its `path` maxDepth 2 samples under another seed."""
    scene = box_scene(spp=16)
    g = mtsg.GPUScene(scene, 0)
    ref = g.render_samples(params(scene, PATH, seed=77))
    yield scene, g, ref
    g.close()


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("hide", [0, 1])
def test_one_one_equals_path_depth_two(box, strict, hide):
    scene, g = box
    a = assert_bit_equal(g, scene, strict_normals=strict, hide_emitters=hide)
    alpha = a[..., 3]
    assert set(np.unique(alpha)) == {0.0, 1.0}   # the open quarter of the back: misses


def test_one_one_equals_path_with_an_environment(tmp_path):
    """env_glass.xml with its glass swapped for a rough conductor: primary
    misses see the environment through the camera's differentials, emitter
    samples go to the environment, BSDF rays that leave the scene are weighted
    with its pdf."""
    xml = open(os.path.join(SCENES, "env_glass.xml")).read()
    glass = xml[xml.index('<bsdf type="dielectric">'):]
    glass = glass[:glass.index("</bsdf>") + len("</bsdf>")]
    xml = xml.replace(glass, '<bsdf type="roughconductor"><float name="alpha" value="0.15"/></bsdf>')
    xml = xml.replace('value="bunny.ply"', f'value="{os.path.join(SCENES, "bunny.ply")}"')
    p = tmp_path / "env_rough.xml"
    p.write_text(xml)
    scene = mtsg.Scene(str(p), dict(SMALL, envmap=os.path.join(SCENES, "sky512.pfm")))
    g = mtsg.GPUScene(scene, 0)
    try:
        for hide in (0, 1):
            assert_bit_equal(g, scene, hide_emitters=hide)
    finally:
        g.close()


def test_one_one_equals_path_in_a_two_level_scene():
    scene = mtsg.Scene(os.path.join(SCENES, "cbox_inst.xml"), SMALL, instancing="two-level")
    g = mtsg.GPUScene(scene, 0)
    try:
        assert_bit_equal(g, scene)
    finally:
        g.close()


def test_one_one_film_passes_the_oracles_path_check(box):
    scene, g = box
    g.set_direct(direct_desc(1, 1))
    img_c, _ = O.render(scene.desc, params(scene, PATH), scene.border, rng=O.RNG_COUNTER)
    img_g = g.render(params(scene, DIRECT), scene.border)
    check_render(img_c, img_g)


def test_scene_route_applies_the_descriptor():
    """A scene whose integrator is `direct` renders through its own parameters."""
    scene = box_scene("direct", [])
    g = mtsg.GPUScene(scene, 0)
    try:
        a = g.render_samples(scene.params())
        b = g.render_samples(params(scene, PATH))
        assert (a.view(np.uint32) == b.view(np.uint32)).all()
    finally:
        g.close()


def test_emitters_only_per_sample_restatement():
    """emitterSamples = 4, bsdfSamples = 0 on diffuse surfaces with one rectangle
    light: per sample Le + the unoccluded terms value * bsdfVal / 4, from the
    array draws, Rectangle::samplePosition, oracle_bsdf_eval and
    oracle.trace_shadow.  A sample is fragile when one of its shadow rays
    changes its oracle answer under a 4-ulp move of a direction component
    (at most 2% may be); every other sample is within 64 * 2^-23 * sum |term_i|:
    each term is a chain of fewer than 32 float32 roundings on either side.
    Measured on an MI355X: fragile share 0, maximum error 0.04 of the bound
    (2.4e-7 absolute)."""
    scene = box_scene("direct", [("emitterSamples", "integer", 4), ("bsdfSamples", "integer", 0)], diffuse_only=True, mesh_light=False)
    P = direct_ref.primary(4, True, False)
    want, mag, fragile = direct_ref.emitters_only_reference(P, 4)
    g = mtsg.GPUScene(scene, 0)
    try:
        a = g.render_samples(scene.params()).reshape(-1, 4)
    finally:
        g.close()
    assert ((a[:, 3] == 1) == P.hit).all()
    bound = (64 * 2.0 ** -23 * mag.astype(np.float64))
    err = np.abs(a[:, :3].astype(np.float64) - want.astype(np.float64))
    ok = ~fragile
    lit = bound > 0
    worst = (err[ok][lit[ok]] / bound[ok][lit[ok]]).max()
    print(f"direct (4,0): fragile {fragile.mean():.4%}, maximum error / bound on the other samples {worst:.4f}, "
          f"maximum absolute error {err[ok].max():.3e}, mean radiance {want.mean():.4f}")
    assert fragile.mean() <= 0.02
    assert (err[ok] <= bound[ok]).all(), (int((err[ok] > bound[ok]).sum()), worst)
    assert want.max() > 1 and (mag.sum(1) > 0).mean() > 0.3


@pytest.mark.parametrize("ne,nb", [(4, 4), (1, 4), (4, 1), (0, 4), (4, 0)])
def test_fans_are_unbiased(box16, ne, nb):
    scene, g, ref = box16
    g.set_direct(direct_desc(ne, nb))
    a = g.render_samples(params(scene, DIRECT))
    assert np.isfinite(a).all()
    assert_same_mean(a[..., :3], ref[..., :3], (ne, nb))


def test_more_shading_samples_lower_the_variance(box16):
    scene, g, _ = box16
    var = {}
    for n in (1, 4):
        g.set_direct(direct_desc(n, n))
        a = g.render_samples(params(scene, DIRECT))[..., :3].astype(np.float64)
        var[n] = a.var(axis=2).mean()   # per pixel over its samples
    assert var[4] < var[1], var


def test_one_one_is_unbiased_where_path_draws_in_another_order():
    """cbox_glass.xml: a dielectric takes no emitter draw in `path`, `direct` always does."""
    scene = mtsg.Scene(os.path.join(SCENES, "cbox_glass.xml"), dict(SMALL, spp=16))
    g = mtsg.GPUScene(scene, 0)
    try:
        g.set_direct(direct_desc(1, 1))
        a = g.render_samples(params(scene, DIRECT))
        b = g.render_samples(params(scene, PATH, seed=77))
        assert_same_mean(a[..., :3], b[..., :3], "cbox_glass")
    finally:
        g.close()


# ---- splits (the comparison of tests/test_gpu_c4.py: rtol 2e-5, atol 2e-6)
@pytest.mark.parametrize("sampler", ["independent", "sobol"])
def test_tile_shares_and_batches_and_the_path_job(sampler):
    scene = box_scene("direct", [("emitterSamples", "integer", 2), ("bsdfSamples", "integer", 3)], sampler=sampler)
    g = mtsg.GPUScene(scene, 0)
    b = scene.border
    try:
        p = scene.params()
        whole = g.render(p, b)
        whole_samples = g.render_samples(p)
        assert whole[..., 4].max() > 0
        acc = np.zeros_like(whole)
        for off in range(2):
            q = p.copy()
            q.tile_stride, q.tile_offset = 2, off
            acc += g.render(q, b)
        np.testing.assert_allclose(acc, whole, rtol=2e-5, atol=2e-6)
        # a tile list
        g.set_tile_list([4, 1])
        part = g.render(p, b)
        g.set_tile_list([0, 2, 3, 5])
        np.testing.assert_allclose(part + g.render(p, b), whole, rtol=2e-5, atol=2e-6)
        g.set_tile_list(None)
        # small batches: 512 slots = one tile x two samples, each with its fan of 5
        g.set_batch_paths(512)
        np.testing.assert_allclose(g.render(p, b), whole, rtol=2e-5, atol=2e-6)
        st = g.stats()
        assert st.launches_trace_closest == 2 * 6 * 2   # 6 tiles x 2 sample batches, two launches each
        g.set_batch_paths(1 << 20)
        # per sample, the arrays do not depend on the rectangle a call renders ...
        q = p.copy()
        q.tile_x, q.tile_y, q.tile_w, q.tile_h = 16, 0, 24, 24
        assert (g.render_samples(q).view(np.uint32) == whole_samples[0:24, 16:40].view(np.uint32)).all()
        # ... nor on the batches rendered before
        assert (g.render_samples(p).view(np.uint32) == whole_samples.view(np.uint32)).all()
    finally:
        g.close()
    job = mtsg.PathJob(scene, 1)
    try:
        rc, img, _ = job.render(p, b)
        assert rc == 0, job.last_error()
        np.testing.assert_allclose(img, whole, rtol=2e-5, atol=2e-6)
    finally:
        job.close()


def test_tile_callback_and_cancel():
    scene = box_scene("direct", [("shadingSamples", "integer", 2)])
    g = mtsg.GPUScene(scene, 0)
    try:
        seen = []
        g.set_tile_callback(lambda key, x, y, w, h: seen.append((key, x, y, w, h)))
        g.render(scene.params(), scene.border)
        g.set_tile_callback(None)
        assert sorted(k for k, *_ in seen) == list(range(6))
        assert sum(w * h for _k, _x, _y, w, h in seen) == FILM_W * FILM_H
        g.cancel()   # set before the render: it cancels the next one
        with pytest.raises(RuntimeError, match="-4"):
            g.render(scene.params(), scene.border)
        g.render(scene.params(), scene.border)   # the flag was consumed
    finally:
        g.close()


@pytest.mark.parametrize("ne,nb", [(1, 1), (4, 2), (0, 3)])
def test_stats(box, ne, nb):
    scene, g = box
    g.set_direct(direct_desc(ne, nb))
    g.render(params(scene, DIRECT), scene.border)
    st = g.stats()
    samples = FILM_W * FILM_H * scene.params().spp
    assert st.samples == samples
    assert st.launches_trace_closest + st.launches_trace_shadow == 2 and st.launches_finish == 0
    assert 0 < st.rays_shadow <= samples * ne or ne == 0 and st.rays_shadow == 0
    assert samples < st.rays_closest <= samples * (1 + nb)


def test_errors(box):
    scene, g = box
    g.set_direct(None)
    out = np.zeros((FILM_H + 2 * scene.border, FILM_W + 2 * scene.border, 5), np.float32)
    p = params(scene, DIRECT)
    rc = mtsg.device_lib().mtsg_render(g._h, C.byref(p), out.ctypes.data_as(C.c_void_p))
    assert rc == -1
    with pytest.raises(RuntimeError, match="no mtsg_direct_desc"):
        g.render(p, scene.border)
    g.set_direct(direct_desc(0, 0))
    with pytest.raises(RuntimeError, match="greater than zero"):
        g.render(p, scene.border)
    with pytest.raises(RuntimeError, match="shading samples"):
        g.set_direct(direct_desc(70000, 1))
    g.set_direct(direct_desc(1, 1))
    g.render(p, scene.border)
