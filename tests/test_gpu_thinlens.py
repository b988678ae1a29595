"""The thinlens sensor on the GPU (kernels.h k_camera_lens, lens_ray;
thinlens.cpp:324-361).  The oracle does not know the sensor and never renders
these scenes: the camera rays are compared with thinlens_ref's float32
restatement, everything downstream with references built from those rays and
oracle pieces (closest hits, shadow rays, sampler draws), and with identities
between the GPU's own integrators.  Films are the 40 x 24 box of
direct_ref.box_scene at 4 spp (not a multiple of the 16-pixel tile), aperture
radius 0.05, focus distance 3.4."""
import hashlib
import json
import os

import numpy as np
import pytest

import mtsg
from oracle import pyoracle as O
from conftest import REPO, SCENES
import direct_ref
from direct_ref import FILM_H, FILM_W, direct_desc
import multichannel_ref as R
from multichannel_ref import f32, xf
import thinlens_ref as T
from test_gpu_direct import PATH, assert_bit_equal, params

pytestmark = pytest.mark.gpu

SPP = 4
N = FILM_W * FILM_H * SPP
AO = mtsg.MTSG_INTEGRATOR_AO
SMALL = {"width": FILM_W, "height": FILM_H, "spp": SPP}


def gpu(scene):
    return mtsg.GPUScene(scene, 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def assert_rays_equal(got, want, what):
    diff = bits(got) != bits(want)
    assert not diff.any(), (what, int(diff.any(1).sum()), np.nonzero(diff.any(0))[0], got[diff.any(1)][:2], want[diff.any(1)][:2])


# ---- 5. camera rays ---------------------------------------------------------
def test_camera_rays_independent_all_samples():
    """All 3840 samples: the 14 words of k_camera_lens equal the restatement fed
    with the counter RNG's draws 0-3 (pinned to the oracle's sampler below)."""
    scene = T.lens_box_scene()
    p = scene.params()
    xys = T.all_samples(SPP)
    u = T.counter_draws(xys, SPP, FILM_W, range(4))
    for i in (0, N // 3, N - 1):
        want = O.sampler_draws(scene.desc, p, int(xys[i, 0]), int(xys[i, 1]), int(xys[i, 2]), [2, 2])
        assert (bits(u[i]) == bits(want)).all()
    cam = T.Cam(scene)
    assert cam.sensor_type == 1
    want = T.lens_rays(cam, SPP, xys[:, 0], xys[:, 1], u[:, :2], u[:, 2:])
    g = gpu(scene)
    try:
        got = g.camera_rays(p, xys)
    finally:
        g.close()
    assert_rays_equal(got, want, "independent")
    # the rays leave the aperture, not one point, and the differentials are not the ray
    o = got[:, :3].astype(np.float64)
    spread = np.linalg.norm(o - np.array([0.05, 0.1, 3.6]), axis=1)   # from the camera's position
    assert 0.9 * T.RADIUS <= spread.max() <= T.RADIUS * (1 + 1e-5) and len(np.unique(bits(got[:, :3]), axis=0)) > N // 2
    assert (got[:, 8:11] != got[:, 3:6]).any(1).all() and (got[:, 11:14] != got[:, 3:6]).any(1).all()
    assert (got[:, 6] > 0).all() and (got[:, 7] > got[:, 6]).all()


@pytest.mark.parametrize("sampler", ["sobol", "halton", "ldsampler"])
def test_camera_rays_qmc(sampler):
    """Three pixels x all samples, the draws from the oracle's sampler: the
    aperture sample is the second 2D request (dimensions 2-3)."""
    scene = T.lens_box_scene(sampler=sampler)
    p = scene.params()
    xys = np.array([(x, y, s) for (x, y) in ((0, 0), (17, 9), (FILM_W - 1, FILM_H - 1)) for s in range(SPP)], np.int32)
    u = np.stack([O.sampler_draws(scene.desc, p, int(x), int(y), int(s), [2, 2]) for x, y, s in xys])
    want = T.lens_rays(T.Cam(scene), SPP, xys[:, 0], xys[:, 1], u[:, :2], u[:, 2:])
    g = gpu(scene)
    try:
        got = g.camera_rays(p, xys)
    finally:
        g.close()
    assert_rays_equal(got, want, sampler)


def test_camera_rays_crop_window_and_rotated_camera():
    c, s = np.cos(0.3), np.sin(0.3)
    to_world = xf([(-c, 0, s), (0, 1, 0), (-s, 0, -c)], (0.05, 0.1, 3.6))
    crop = [("cropOffsetX", "integer", 5), ("cropOffsetY", "integer", 3), ("cropWidth", "integer", 21), ("cropHeight", "integer", 17)]
    scene = T.lens_box_scene(film_props=crop, to_world=to_world)
    p = scene.params()
    assert (p.tile_x, p.tile_y, p.tile_w, p.tile_h) == (5, 3, 21, 17)
    xys = T.all_samples(SPP, 21, 17, 5, 3)
    u = T.counter_draws(xys, SPP, FILM_W, range(4))
    want = T.lens_rays(T.Cam(scene), SPP, xys[:, 0], xys[:, 1], u[:, :2], u[:, 2:])
    g = gpu(scene)
    try:
        got = g.camera_rays(p, xys)
        with pytest.raises(RuntimeError, match="outside the rectangle"):
            g.camera_rays(p, [(4, 3, 0)])
    finally:
        g.close()
    assert_rays_equal(got, want, "crop")


def test_camera_rays_of_a_perspective_scene_are_the_oracles():
    P = direct_ref.primary(SPP)
    g = gpu(P.scene)
    try:
        got = g.camera_rays(P.scene.params(), T.all_samples(SPP))
    finally:
        g.close()
    assert_rays_equal(got[:, :8], P.rays, "perspective")
    assert (got[:, 8:11] != got[:, 3:6]).any(1).all()


# ---- 6. fields --------------------------------------------------------------
def test_fields_per_sample():
    """position and distance of every sample: oracle.trace_closest of the
    restated rays through multichannel_ref.expected_fields, at the bar of
    test_gpu_multichannel.check_fields (distance equal, position within 4 ulp,
    a miss `undefined` exactly, the same set of misses)."""
    scene = T.lens_fields_scene(["position", "distance"])
    p = scene.params()
    xys = T.all_samples(SPP)
    u = T.counter_draws(xys, SPP, FILM_W, range(4))
    rays = np.ascontiguousarray(T.lens_rays(T.Cam(scene), SPP, xys[:, 0], xys[:, 1], u[:, :2], u[:, 2:])[:, :8])
    t, uu, v, prim = O.trace_closest(scene.desc, rays)
    want, miss = R.expected_fields(R.Desc(scene), scene.aov(), rays, t, uu, v, prim, lambda tex, uv: O.tex_eval(scene.desc, tex, uv))
    g = gpu(scene)
    try:
        got = g.render_samples_multi(p).reshape(N, 7)
    finally:
        g.close()
    np.testing.assert_array_equal(got[:, 6] == 0, miss)
    assert 0.02 < miss.mean() < 0.6
    hit = ~miss
    for k, name in enumerate(("position", "distance")):
        a = got[:, 3 * k:3 * k + 3]
        np.testing.assert_array_equal(a[miss], np.tile(f32(R.UNDEFINED), (int(miss.sum()), 1)))
        if name == "distance":
            np.testing.assert_array_equal(a[hit], want[name][hit])
        else:
            worst = R.ulps(a[hit], want[name][hit]).max()
            print("position: largest deviation", worst, "ulp")
            assert worst <= 4


# ---- 7. ao and direct, per sample -------------------------------------------
@pytest.mark.parametrize("n", [1, 4])
def test_ao_per_sample_restatement(n):
    """The bar of test_gpu_ao.test_per_sample_restatement, fragile share at most 1%."""
    scene = T.lens_box_scene("ao", [("shadingSamples", "integer", 4)])
    P = T.lens_primary(SPP)
    want, fragile = direct_ref.ao_reference(P, n, 0.45)
    g = gpu(scene)
    try:
        g.set_direct(direct_desc(ao=n, length=0.45))
        p = scene.params()
        assert p.integrator == AO
        a = g.render_samples(p).reshape(-1, 4)
    finally:
        g.close()
    assert ((a[:, 3] == 1) == P.hit).all()
    wrong = (a[:, 0] != want) & ~fragile
    print(f"thinlens ao N={n}: fragile {fragile.mean():.4%}, differing non-fragile samples {int(wrong.sum())} of {len(want)}")
    assert fragile.mean() <= 0.01
    assert not wrong.any(), (np.nonzero(wrong)[0][:8], a[wrong][:8, 0], want[wrong][:8])


@pytest.mark.parametrize("ne", [1, 4])
def test_direct_emitters_only_per_sample_restatement(ne):
    """The bar of test_gpu_direct.test_emitters_only_per_sample_restatement
    (64 * 2^-23 * sum |term|), fragile share at most 1%.  ne = 1 draws the
    regular 2D sample after the aperture's (dimensions 4-5), ne = 4 its array.
    Measured on an MI355X: fragile share 0 in both cases, maximum error 0.068
    (ne = 1) and 0.039 (ne = 4) of the bound."""
    scene = T.lens_box_scene("direct", [("emitterSamples", "integer", ne), ("bsdfSamples", "integer", 0)], diffuse_only=True, mesh_light=False)
    P = T.lens_primary(SPP, True, False)
    want, mag, fragile = direct_ref.emitters_only_reference(P, ne)
    g = gpu(scene)
    try:
        a = g.render_samples(scene.params()).reshape(-1, 4)
    finally:
        g.close()
    assert ((a[:, 3] == 1) == P.hit).all()
    bound = 64 * 2.0 ** -23 * mag.astype(np.float64)
    err = np.abs(a[:, :3].astype(np.float64) - want.astype(np.float64))
    ok = ~fragile
    lit = bound > 0
    worst = (err[ok][lit[ok]] / bound[ok][lit[ok]]).max()
    print(f"thinlens direct ({ne},0): fragile {fragile.mean():.4%}, maximum error / bound {worst:.4f}, absolute {err[ok].max():.3e}")
    assert fragile.mean() <= 0.01
    assert (err[ok] <= bound[ok]).all(), (int((err[ok] > bound[ok]).sum()), worst)
    assert want.max() > 1 and (mag.sum(1) > 0).mean() > 0.3


# ---- 8. identities between the GPU's integrators ----------------------------
@pytest.mark.parametrize("sampler", ["independent", "sobol"])
def test_one_one_equals_path_depth_two(sampler):
    scene = T.lens_box_scene(sampler=sampler)
    g = gpu(scene)
    try:
        for strict in (0, 1):
            a = assert_bit_equal(g, scene, strict_normals=strict)
        assert set(np.unique(a[..., 3])) == {0.0, 1.0}
    finally:
        g.close()


def test_one_one_equals_path_with_an_environment(tmp_path):
    """env_glass.xml, its glass swapped for a rough conductor, through the lens:
    the differentials of a primary miss are the carried ones (cam_diffs)."""
    xml = open(os.path.join(SCENES, "env_glass.xml")).read()
    glass = xml[xml.index('<bsdf type="dielectric">'):]
    glass = glass[:glass.index("</bsdf>") + len("</bsdf>")]
    xml = xml.replace(glass, '<bsdf type="roughconductor"><float name="alpha" value="0.15"/></bsdf>')
    xml = xml.replace('value="bunny.ply"', f'value="{os.path.join(SCENES, "bunny.ply")}"')
    assert xml.count('<sensor type="perspective">') == 1
    lens = xml.replace('<sensor type="perspective">',
                       '<sensor type="thinlens"><float name="apertureRadius" value="0.05"/><float name="focusDistance" value="3.2"/>')
    out = {}
    for name, text in (("pin", xml), ("lens", lens)):
        path = tmp_path / (name + ".xml")
        path.write_text(text)
        scene = mtsg.Scene(str(path), dict(SMALL, envmap=os.path.join(SCENES, "sky512.pfm")))
        g = gpu(scene)
        try:
            out[name] = assert_bit_equal(g, scene)
        finally:
            g.close()
    # (the film has no alpha channel: a miss shows as the environment's radiance only)
    assert (out["lens"] != out["pin"]).any()


def test_one_one_equals_path_on_an_ewa_texture():
    scene = T.lens_box_scene(textured=True)
    plain = T.lens_box_scene()
    g, h = gpu(scene), gpu(plain)
    try:
        a = assert_bit_equal(g, scene)
        assert (a != h.render_samples(params(plain, PATH))).any()   # the textured rectangle is seen
    finally:
        g.close()
        h.close()


def test_flat_equals_two_level():
    """The box with one more mesh in a shapegroup, instanced with the identity:
    the flattened scene holds the same world-space triangles."""
    out = {}
    for mode in ("flatten", "two-level"):
        scene = T.lens_box_scene(instancing=mode, instanced=True)
        g = gpu(scene)
        try:
            out[mode] = assert_bit_equal(g, scene)
        finally:
            g.close()
    assert (bits(out["flatten"]) == bits(out["two-level"])).all()
    assert (out["flatten"] != direct_samples_plain()).any()   # the instanced mesh is seen


def direct_samples_plain():
    scene = T.lens_box_scene()
    g = gpu(scene)
    try:
        return g.render_samples(params(scene, PATH))
    finally:
        g.close()


def test_shares_rectangles_and_the_path_job():
    scene = T.lens_box_scene()
    g = gpu(scene)
    b = scene.border
    try:
        p = scene.params()
        whole = g.render(p, b)
        samples = g.render_samples(p)
        assert whole[..., 4].max() > 0
        g.set_tile_list([4, 1])
        part = g.render(p, b)
        g.set_tile_list([0, 2, 3, 5])
        np.testing.assert_allclose(part + g.render(p, b), whole, rtol=2e-5, atol=2e-6)
        g.set_tile_list(None)
        acc = np.zeros_like(whole)
        for off in range(2):
            q = p.copy()
            q.tile_stride, q.tile_offset = 2, off
            acc += g.render(q, b)
        np.testing.assert_allclose(acc, whole, rtol=2e-5, atol=2e-6)
        # per sample, nothing depends on the rectangle a call renders
        q = p.copy()
        q.tile_x, q.tile_y, q.tile_w, q.tile_h = 16, 0, 24, 24
        assert (bits(g.render_samples(q)) == bits(samples[0:24, 16:40])).all()
        seen = []
        g.set_tile_callback(lambda key, x, y, w, h: seen.append(key))
        g.render(p, b)
        g.set_tile_callback(None)
        assert sorted(seen) == list(range(6))
    finally:
        g.close()
    job = mtsg.PathJob(scene, 1)
    try:
        rc, img, _ = job.render(p, b)
        assert rc == 0, job.last_error()
        np.testing.assert_allclose(img, whole, rtol=2e-5, atol=2e-6)
    finally:
        job.close()


def test_tail_kernel_starts_at_the_right_dimension():
    """path, maxDepth -1: the tail kernel taking every path over after bounce 0
    (its bounce 0 reads camera_meta) equals the bounce kernels, at shade
    thresholds 1 and 16."""
    scene = T.lens_box_scene(props=[("maxDepth", "integer", -1)])
    g = gpu(scene)
    try:
        p = params(scene, PATH, max_depth=-1)
        g.set_finish_paths(0)
        bounce = g.render_samples(p)
        assert g.stats().launches_finish == 0
        g.set_finish_paths(1 << 30)
        for shade_min in (1, 16):
            g.set_option(mtsg.MTSG_OPT_FINISH_SHADE_MIN, shade_min)
            tail = g.render_samples(p)
            st = g.stats()
            assert st.launches_finish == 1 and st.paths_finish > 0
            assert (bits(tail) == bits(bounce)).all(), shade_min
    finally:
        g.close()


def test_multichannel_path_child_is_the_plain_render():
    multi = T.lens_fields_scene(["path", "position"])
    plain = T.lens_box_scene()
    g, h = gpu(multi), gpu(plain)
    try:
        a = g.render_samples_multi(multi.params())
        b = h.render_samples(params(plain, PATH))
    finally:
        g.close()
        h.close()
    assert (bits(a[..., :3]) == bits(b[..., :3])).all() and b[..., :3].max() > 0


# ---- 9. circle of confusion -------------------------------------------------
@pytest.mark.parametrize("rel", [1.0, 2.0, 0.5])
def test_circle_of_confusion(rel):
    """One rectangle perpendicular to the optical axis at depth z, seen through
    the lens and through the pinhole at the same seed: the jitter, so nearP and
    the focal point F = nearP f / nearP.z, are the same.  The lens ray leaves
    A on the aperture (|A| <= R) towards F and meets the plane at
    A + (F - A) z / f; the pinhole's meets it at F z / f.  Their distance is
    |A| |z - f| / f <= R |z - f| / f: zero in focus, where only the rounding of
    two routes to one point remains (1e-4 f is far above it and far below any
    blur).  The concentric map reaches |A| >= 0.9 R with probability 0.19 per
    sample, so the largest of 3840 distances lies below 0.9 of the bound with
    probability 0.81^3840."""
    f, radius = 2.0, T.RADIUS
    z = rel * f
    pos = {}
    for sensor in ("thinlens", "perspective"):
        scene = T.plane_scene(z, sensor, f)
        g = gpu(scene)
        try:
            a = g.render_samples_multi(scene.params()).reshape(N, 4)
        finally:
            g.close()
        assert (a[:, 3] == 1).all()
        assert np.abs(a[:, 2] - z).max() <= 1e-5 * z
        pos[sensor] = a[:, :3].astype(np.float64)
    dist = np.linalg.norm(pos["thinlens"] - pos["perspective"], axis=1)
    coc = radius * abs(z - f) / f
    print(f"z = {rel} f: largest distance {dist.max():.6f}, R |z - f| / f = {coc:.6f}")
    if rel == 1.0:
        assert dist.max() <= 1e-4 * f
    else:
        assert dist.max() <= coc * (1 + 1e-3)
        assert dist.max() >= 0.9 * coc


# ---- 10. perspective scenes are untouched ------------------------------------
@pytest.mark.parametrize("name,sets", [("cbox", (1, 0)), ("env_glass", (1 | 2 | 8, 1))])
def test_perspective_scenes_keep_their_kernels_and_samples(name, sets):
    scene = mtsg.Scene(os.path.join(SCENES, name + ".xml"), dict(SMALL, envmap=os.path.join(SCENES, "sky512.pfm")))
    g = gpu(scene)
    try:
        got, selected = g.render_samples(scene.params()), g.kernel_sets()
    finally:
        g.close()
    assert selected == sets
    want = json.load(open(os.path.join(REPO, "tests", "golden", "emitters_parent_samples.json")))[name]
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == want
