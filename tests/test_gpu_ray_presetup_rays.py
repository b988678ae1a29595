"""Ray queries with rectangle pre-records (MTSG_OPT_RAY_PRESETUP 1: k_query_pre
does for a query's rays what k_camera / k_shade do for theirs, then
k_trace_s_pre) against the refill's own rectangle loop (0), bit for bit, and
against the oracle where the oracle's order is the answer.  A builder scene:

  A   rectangle  y = 0, x, z in [-1, 1]                        (rectangle 0)
  B   rectangle  y = 0, x in [-0.5, 1.5], z in [-1, 1]: A moved by 0.5 in its
      own plane, the light                                      (rectangle 1)
      Both have the same rotation and no scale, so the third row of their
      to_object matrices is the same (0, 1, 0 | 0) and both tests compute the
      same distance -o.y / d.y for a ray: where they overlap every ray meets
      an exact tie of two rectangles, which only k_tie's mailbox order decides.
  T   one triangle in y = 0.5 over x, z in [-0.3, 0.3]

The camera looks straight down on the overlap, so a counting render must send
its rays to the tie list under either option."""
import numpy as np
import pytest

import mtsg
from conftest import SCENES
from multichannel_ref import f32, xf
from oracle import pyoracle as O
from test_gpu_rect_setup_rays import MISS, rays_of, unit

pytestmark = pytest.mark.gpu

N = 256
RECT_A, RECT_B = 0x80000000, 0x80000001


def build():
    b = mtsg.SceneBuilder(SCENES)
    b.integrator("path", [("maxDepth", "integer", 3)])
    b.sensor("perspective", [("fov", "float", 30.0), ("toWorld", "transform", xf([(1, 0, 0), (0, 0, 1), (0, -1, 0)], (0.5, 1.5, 0.5)))])
    b.film("hdrfilm", [("width", "integer", 32), ("height", "integer", 32), ("pixelFormat", "string", "rgba")], "gaussian", [])
    b.sampler("independent", [("sampleCount", "integer", 4)])
    grey = b.bsdf("diffuse", [("reflectance", "spectrum", (0.6, 0.6, 0.6))])
    light = b.emitter("area", [("radiance", "spectrum", (4.0, 4.0, 4.0))])
    rot = [(1, 0, 0), (0, 0, -1), (0, 1, 0)]
    b.shape("rectangle", [("toWorld", "transform", xf(rot, (0, 0, 0)))], grey)
    b.shape("rectangle", [("toWorld", "transform", xf(rot, (0.5, 0, 0)))], grey, light)
    pos = np.array([(-0.3, 0.5, -0.3), (0.3, 0.5, -0.3), (0.0, 0.5, 0.3)], f32)
    b.mesh(pos, np.array([(0, 2, 1)], np.uint32), face_normals=True, bsdf=grey, name="tri")
    return b.finish()


@pytest.fixture(scope="module")
def pair():
    scene = build()
    assert scene.info.n_triangles == 1
    gpu = {m: mtsg.GPUScene(scene, 0) for m in (1, 0)}
    for m, g in gpu.items():
        g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, m)
    yield scene, gpu
    for g in gpu.values():
        g.close()


def same_closest(pair, rays):
    """Both options bit for bit; returns option 1's answer."""
    _, gpu = pair
    a, b = gpu[1].trace_closest(rays), gpu[0].trace_closest(rays)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    return a


def same_shadow(pair, rays):
    scene, gpu = pair
    a, b = gpu[1].trace_shadow(rays), gpu[0].trace_shadow(rays)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, O.trace_shadow(scene.desc, rays))
    return a


def down(seed, x0, x1, z0, z1, y0=1.0, tilt=0.03, n=N):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(x0, x1, n), np.full(n, y0), rng.uniform(z0, z1, n)], 1).astype(f32)
    d = unit(np.stack([rng.normal(0, tilt, n), np.full(n, -np.sign(y0)), rng.normal(0, tilt, n)], 1))
    return rays_of(o, d)


def test_one_rectangle_and_the_triangle(pair):
    scene, _ = pair
    # A alone (x < -0.5), B alone (x > 1), and through the triangle onto the overlap
    for seed, box, prims in ((1, (-0.9, -0.65, -0.8, 0.8), (RECT_A,)), (2, (1.15, 1.4, -0.8, 0.8), (RECT_B,)),
                             (3, (-0.05, 0.05, -0.12, 0.0), (0,))):
        rays = down(seed, *box)
        t, u, v, p = same_closest(pair, rays)
        assert np.isin(p, prims).all()
        t0, u0, v0, p0 = O.trace_closest(scene.desc, rays)
        np.testing.assert_array_equal(p, p0)
        for x, y in ((t, t0), (u, u0), (v, v0)):
            np.testing.assert_array_equal(x, y)


def test_two_rectangles_at_the_same_distance(pair):
    scene, _ = pair
    rays = down(4, 0.4, 0.9, 0.4, 0.9)   # the overlap, beside the triangle's column
    t, u, v, p = same_closest(pair, rays)
    np.testing.assert_array_equal(t, (f32(0) - rays[:, 1]) / rays[:, 4])   # the distance both tests compute
    t0, _, _, p0 = O.trace_closest(scene.desc, rays)
    np.testing.assert_array_equal(t, t0)
    np.testing.assert_array_equal(p, p0)   # Mitsuba's mailbox order: k_tie
    assert np.isin(p, (RECT_A, RECT_B)).all()


def test_ties_reach_the_tie_list(pair):
    """A counting render from the camera above the overlap: every camera ray
    meets both rectangles at one distance and is retraced, under either option
    (the flag travels in the pre-record)."""
    scene, _ = pair
    counts = {}
    for pre in (1, 0):
        g = mtsg.GPUScene(scene, 0)
        try:
            g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, pre)
            g.set_flags(mtsg.MTSG_FLAG_COUNT)
            g.render(scene.params(), scene.border)
            counts[pre] = g.stats().tie_retraces
        finally:
            g.close()
    assert counts[1] == counts[0] >= 32 * 32 * 4


def test_origins_in_a_rectangles_plane(pair):
    rng = np.random.default_rng(5)
    o = np.stack([rng.uniform(-0.95, 1.45, 2 * N), np.zeros(2 * N), rng.uniform(-0.95, 0.95, 2 * N)], 1).astype(f32)
    d = rng.normal(size=(2 * N, 3))
    d[:N, 1] = np.abs(d[:N, 1])   # into the scene; the rest leave through the floor
    d[N:, 1] = -np.abs(d[N:, 1])
    rays = rays_of(o, unit(d))
    same_closest(pair, rays)
    same_shadow(pair, rays)
    rays[:, 6] = 0.0   # no epsilon: the origin itself is a candidate
    same_closest(pair, rays)
    same_shadow(pair, rays)
    # in the plane and along it: 0 / 0 in the rectangle test
    d[:, 1] = 0.0
    same_closest(pair, rays_of(o, unit(d)))


def test_rays_without_an_interval(pair):
    rng = np.random.default_rng(6)
    o = rng.uniform(-0.9, 0.9, (N, 3)).astype(f32)
    o[:, 1] = rng.uniform(1.0, 3.0, N)   # above the scene's box (y <= 0.5) ...
    d = rng.normal(size=(N, 3))
    d[:, 1] = np.abs(d[:, 1]) + 0.01     # ... and leaving
    rays = rays_of(o, unit(d))
    t, _, _, p = same_closest(pair, rays)
    assert (p == MISS).all() and np.isposinf(t).all()
    assert not same_shadow(pair, rays).any()
    # dead slots: a negative maxt, as k_camera stores them; their records are never written
    dead = down(7, -0.9, 1.4, -0.9, 0.9)
    dead[:, 7] = -1.0
    t, _, _, p = same_closest(pair, dead)
    assert (p == MISS).all() and np.isposinf(t).all()
    # among live rays in one list
    mix = np.concatenate([dead, down(8, -0.9, 1.4, -0.9, 0.9), rays])[np.random.default_rng(9).permutation(3 * N)]
    _, _, _, p = same_closest(pair, mix)
    assert (p != MISS).sum() == N


def test_shadow_rays(pair):
    # from below the floor to above it, beside the triangle: only a rectangle is between
    blocked = down(10, -0.9, -0.65, -0.8, 0.8, y0=-0.5)
    blocked[:, 7] = 1.0
    assert same_shadow(pair, blocked).all()
    # from above the triangle to below the floor: the triangle in front of the rectangles
    both = down(11, -0.05, 0.05, -0.12, 0.0, y0=1.0)
    both[:, 7] = 1.4
    assert same_shadow(pair, both).all()
    # the same rays ending between the triangle and the floor: the triangle alone
    tri = both.copy()
    tri[:, 7] = 0.75
    assert same_shadow(pair, tri).all()
    # ending above the triangle, and beside it short of the floor: nothing between
    free = both.copy()
    free[:, 7] = 0.4
    short = down(12, 0.4, 0.9, 0.4, 0.9)
    short[:, 7] = 0.9
    assert not same_shadow(pair, free).any() and not same_shadow(pair, short).any()
    # every kind in one list: the occluded rays leave no contribution, the others theirs
    mix = np.concatenate([blocked, both, tri, free, short])[np.random.default_rng(13).permutation(5 * N)]
    assert same_shadow(pair, mix).sum() == 3 * N
