"""Ray queries (mtsg_trace_closest / mtsg_trace_shadow -> k_trace_s) around
rectangles, with the rectangles tested at ray setup (MTSG_OPT_RECT_SETUP 1, the
default) and in the kd-tree leaves (0), against the oracle's Havran
restatement.  A builder scene with everything in easy numbers:

  floor   rectangle  y = 0, x, z in [-1, 1]          (rectangle 0)
  wall    rectangle  x = 1, y in [0, 2], z in [-1, 1] (rectangle 1, the light;
                     it lies on the +x face of the scene's box, the floor on
                     the -y face)
  patch   two triangles in y = 0, x, z in [-0.5, 0.5]: coplanar with the
          middle of the floor.  A ray through it meets a triangle and the
          floor at exactly the same distance -- both tests compute
          (0 - o.y) / d.y -- so the winner is Mitsuba's mailbox order, which
          only the tie retrace knows: the setup mode must flag every such ray.

The lists: the coplanar region from above and from below; maxt and mint
exactly at the floor's distance and one ulp either side; origins on the floor;
rays parallel to it (in its plane too); rays that miss the scene's box; shadow
rays that only a rectangle blocks and rays nothing blocks.  And a scene with
one rectangle more than the setup mode takes (MTSG_RECT_SETUP_CAP), which must
fall back to the in-leaf kernels."""
import numpy as np
import pytest

import mtsg
from conftest import SCENES
from multichannel_ref import f32, xf
from oracle import pyoracle as O
from test_gpu_parity import compare_closest

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
N = 512   # rays per list
FLOOR, WALL = 0x80000000, 0x80000001


def build(extra_rects=0):
    b = mtsg.SceneBuilder(SCENES)
    b.integrator("path", [("maxDepth", "integer", 4)])
    # above the patch, looking down: every camera ray through it meets a tie
    b.sensor("perspective", [("fov", "float", 50.0), ("toWorld", "transform", xf([(1, 0, 0), (0, 0, 1), (0, -1, 0)], (0, 1.5, 0)))])
    b.film("hdrfilm", [("width", "integer", 32), ("height", "integer", 32), ("pixelFormat", "string", "rgba")], "gaussian", [])
    b.sampler("independent", [("sampleCount", "integer", 4)])
    grey = b.bsdf("diffuse", [("reflectance", "spectrum", (0.6, 0.6, 0.6))])
    green = b.bsdf("diffuse", [("reflectance", "spectrum", (0.2, 0.7, 0.3))])
    light = b.emitter("area", [("radiance", "spectrum", (6.0, 6.0, 6.0))])
    b.shape("rectangle", [("toWorld", "transform", xf([(1, 0, 0), (0, 0, -1), (0, 1, 0)], (0, 0, 0)))], grey)
    b.shape("rectangle", [("toWorld", "transform", xf([(0, 0, 1), (0, 1, 0), (-1, 0, 0)], (1, 1, 0)))], grey, light)
    pos = np.array([(-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), (-0.5, 0, 0.5)], f32)
    b.mesh(pos, np.array([(0, 2, 1), (0, 3, 2)], np.uint32), face_normals=True, bsdf=green, name="patch")
    for k in range(extra_rects):   # small tiles floating above the floor, outside the patch's column
        b.shape("rectangle", [("toWorld", "transform", xf([(0.1, 0, 0), (0, 0, -0.1), (0, 1, 0)], (-0.8 + 0.2 * k, 0.25, 0.8)))], green)
    return b.finish()


class Pair:
    def __init__(self):
        self.scene = build()
        assert self.scene.info.n_triangles == 2
        self.gpu = {m: mtsg.GPUScene(self.scene, 0) for m in (1, 0)}
        self.gpu[0].set_option(mtsg.MTSG_OPT_RECT_SETUP, 0)

    def close(self):
        for g in self.gpu.values():
            g.close()


@pytest.fixture(scope="module")
def pair():
    p = Pair()
    yield p
    p.close()


@pytest.fixture(params=[1, 0], ids=["setup", "in-leaf"])
def mode(request):
    return request.param


def unit(d):
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def rays_of(o, d, mint=1e-4, maxt=np.inf):
    r = np.zeros((len(o), 8), f32)
    r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = o, d, mint, maxt
    return r


def down_rays(seed, half, y0=1.0, n=N, tilt=0.05):
    """From height y0 onto the floor's square |x|, |z| <= half (a tilt of a
    few degrees: its tangent is normal with deviation `tilt`; y0 < 0: from
    below, upwards)."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-half, half, n), np.full(n, y0), rng.uniform(-half, half, n)], 1).astype(f32)
    d = unit(np.stack([rng.normal(0, tilt, n), np.full(n, -np.sign(y0)), rng.normal(0, tilt, n)], 1))
    return rays_of(o, d)


def ring_rays(seed, n=N):
    """Onto the floor between the patch and the wall (0.6 <= |x| <= 0.76 at
    the start, within 0.1 of that on the floor): only a rectangle there."""
    r = down_rays(seed, 0.08, n=n, tilt=0.02)
    r[:, 0] += np.where(np.arange(n) % 2, 0.68, -0.68).astype(f32)
    return r


def exact(pair, mode, rays):
    """Every answer the oracle's, bit for bit, ties included."""
    t0, u0, v0, p0 = O.trace_closest(pair.scene.desc, rays)
    t1, u1, v1, p1 = pair.gpu[mode].trace_closest(rays)
    hit = p0 != MISS
    np.testing.assert_array_equal(p1, p0)
    np.testing.assert_array_equal(t1[hit], t0[hit])
    np.testing.assert_array_equal(u1[hit], u0[hit])
    np.testing.assert_array_equal(v1[hit], v0[hit])
    assert np.isposinf(t1[~hit]).all()
    return t0, p0


def test_coplanar_region(pair, mode):
    for seed, y0 in ((1, 1.0), (2, 0.37), (3, -0.5)):
        rays = down_rays(seed, 0.45, y0)
        compare_closest(pair.scene, pair.gpu[mode], rays)
        t0, p0 = exact(pair, mode, rays)
        assert np.isin(p0, (0, 1, FLOOR)).all()
        # the tie is exact: the distance both tests compute
        np.testing.assert_array_equal(t0, (f32(0) - rays[:, 1]) / rays[:, 4])


def test_tie_retraces_are_counted(pair, mode):
    """A counting render from the camera above the patch: the rays through it
    are traced again by k_tie in either mode (a missing flag is the bug)."""
    g = mtsg.GPUScene(pair.scene, 0)
    try:
        g.set_option(mtsg.MTSG_OPT_RECT_SETUP, mode)
        g.set_flags(mtsg.MTSG_FLAG_COUNT)
        g.render(pair.scene.params(), pair.scene.border)
        st = g.stats()
        # the camera sees the patch in about a quarter of its 32 x 32 x 4 samples
        assert st.tie_retraces >= 32 * 32 * 4 // 8
        # a rectangle record stepped over is a leaf reference, not a test
        if mode == 1:
            assert st.tri_tests < st.leaf_refs and st.shadow_tri_tests <= st.shadow_leaf_refs
        else:
            assert st.tri_tests == st.leaf_refs and st.shadow_tri_tests == st.shadow_leaf_refs
    finally:
        g.close()


def test_interval_ends_at_the_rectangle(pair, mode):
    base = ring_rays(4)
    t0, p0 = exact(pair, mode, base)
    assert (p0 == FLOOR).all()
    lo, hi = np.nextafter(t0, f32(0)), np.nextafter(t0, f32(np.inf))
    for what, col, values, hits in (("maxt", 7, (lo, t0, hi), (False, True, True)), ("mint", 6, (lo, t0, hi), (True, True, False))):
        for value, hit in zip(values, hits):
            rays = base.copy()
            rays[:, col] = value
            compare_closest(pair.scene, pair.gpu[mode], rays)
            _, p = exact(pair, mode, rays)
            assert ((p == FLOOR) == hit).all(), (what, hit)
            occ = pair.gpu[mode].trace_shadow(rays)
            np.testing.assert_array_equal(occ, O.trace_shadow(pair.scene.desc, rays), err_msg=what)
            assert (occ != 0).all() == hit and (occ != 0).any() == hit, (what, hit)


def test_origins_on_the_rectangle(pair, mode):
    rng = np.random.default_rng(5)
    o = np.stack([rng.uniform(-0.95, 0.95, 3 * N), np.zeros(3 * N), rng.uniform(-0.95, 0.95, 3 * N)], 1).astype(f32)
    d = rng.normal(size=(3 * N, 3))
    d[N:2 * N, 1] = -np.abs(d[N:2 * N, 1])   # leaving through the floor
    d[2 * N:, 1] = np.abs(d[2 * N:, 1])      # into the scene
    rays = rays_of(o, unit(d))
    compare_closest(pair.scene, pair.gpu[mode], rays)
    exact(pair, mode, rays)
    rays[:, 6] = 0.0   # no epsilon: the origin itself is a candidate
    exact(pair, mode, rays)
    np.testing.assert_array_equal(pair.gpu[mode].trace_shadow(rays), O.trace_shadow(pair.scene.desc, rays))


def test_rays_parallel_to_the_rectangle(pair, mode):
    rng = np.random.default_rng(6)
    o = np.stack([rng.uniform(-0.9, 0.9, 2 * N), rng.uniform(0.05, 1.9, 2 * N), rng.uniform(-0.9, 0.9, 2 * N)], 1).astype(f32)
    o[N:, 1] = 0.0   # in the floor's plane: 0 / 0 in the rectangle test
    d = rng.normal(size=(2 * N, 3))
    d[:, 1] = 0.0
    rays = rays_of(o, unit(d))
    compare_closest(pair.scene, pair.gpu[mode], rays)
    _, p = exact(pair, mode, rays)
    assert (p == WALL).any() and (p == MISS).any() and not (p[:N] == FLOOR).any()
    np.testing.assert_array_equal(pair.gpu[mode].trace_shadow(rays), O.trace_shadow(pair.scene.desc, rays))


def test_rays_that_miss_the_scene_box(pair, mode):
    rng = np.random.default_rng(7)
    o = rng.uniform(-0.9, 0.9, (N, 3)).astype(f32)
    o[:, 1] = rng.uniform(2.5, 4.0, N)   # above the box (y <= 2)
    d = rng.normal(size=(N, 3))
    d[:, 1] = np.abs(d[:, 1]) + 0.01     # and leaving: the floor's plane lies behind
    rays = rays_of(o, unit(d))
    _, p = exact(pair, mode, rays)
    assert (p == MISS).all()
    assert not pair.gpu[mode].trace_shadow(rays).any()
    # towards the box but beside it: the floor's plane is crossed outside the box
    o[:, 0] = rng.uniform(3.0, 5.0, N)
    d = np.stack([rng.normal(0, 0.02, N), -np.ones(N), rng.normal(0, 0.02, N)], 1)
    rays = rays_of(o, unit(d))
    _, p = exact(pair, mode, rays)
    assert (p == MISS).all()
    assert not pair.gpu[mode].trace_shadow(rays).any()


def test_shadow_rays(pair, mode):
    g = pair.gpu[mode]
    # from below the floor to above it, outside the patch: only the floor is between
    blocked = ring_rays(8)
    blocked[:, 1] = -0.5
    blocked[:, 4] = -blocked[:, 4]
    blocked[:, 7] = 1.0
    want = O.trace_shadow(pair.scene.desc, blocked)
    assert want.all()
    np.testing.assert_array_equal(g.trace_shadow(blocked), want)
    # from above towards the wall: only the wall is between
    rng = np.random.default_rng(9)
    o = np.stack([rng.uniform(-0.9, 0.5, N), rng.uniform(0.4, 1.6, N), rng.uniform(-0.6, 0.6, N)], 1).astype(f32)
    wall = rays_of(o, unit(np.stack([np.ones(N), rng.normal(0, 0.02, N), rng.normal(0, 0.02, N)], 1)), maxt=3.0)
    want = O.trace_shadow(pair.scene.desc, wall)
    assert want.all()
    np.testing.assert_array_equal(g.trace_shadow(wall), want)
    # the same rays ending short of it, and rays into the open sides: nothing between
    free = wall.copy()
    free[:, 7] = f32(0.4) * (f32(1) - o[:, 0])
    up = rays_of(o, unit(np.stack([-np.ones(N), np.abs(rng.normal(0, 0.3, N)) + 0.01, rng.normal(0, 0.3, N)], 1)), maxt=50.0)
    for rays in (free, up):
        want = O.trace_shadow(pair.scene.desc, rays)
        assert not want.any()
        np.testing.assert_array_equal(g.trace_shadow(rays), want)
    # a mix, in one list with closest-free shadow rays of every kind above
    mix = np.concatenate([blocked, free, wall, up])[np.random.default_rng(10).permutation(4 * N)]
    np.testing.assert_array_equal(g.trace_shadow(mix), O.trace_shadow(pair.scene.desc, mix))


def test_one_rectangle_over_the_cap_falls_back():
    """MTSG_RECT_SETUP_CAP + 1 rectangles: the option at 1 renders with the
    in-leaf kernels -- the counting pass books every leaf reference as a test,
    as with the option at 0 -- and the samples are those of the option at 0."""
    scene = build(extra_rects=mtsg.MTSG_RECT_SETUP_CAP + 1 - 2)
    out = {}
    for opt in (1, 0):
        g = mtsg.GPUScene(scene, 0)
        try:
            g.set_option(mtsg.MTSG_OPT_RECT_SETUP, opt)
            g.set_finish_paths(0)
            out[opt] = g.render_samples(scene.params())
            g.set_flags(mtsg.MTSG_FLAG_COUNT)
            g.render(scene.params(), scene.border)
            st = g.stats()
            assert st.tri_tests == st.leaf_refs > 0 and st.shadow_tri_tests == st.shadow_leaf_refs > 0
        finally:
            g.close()
    assert np.isfinite(out[1]).all() and out[1][..., :3].max() > 0
    assert np.array_equal(out[1], out[0])
