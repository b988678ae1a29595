"""The filtered leaf addressing of the flat traversal's setup mode
(MTSG_OPT_LEAF_FILTER 1, the default: the timed kernels walk leaves without
rectangle records, kd_layout.h blocksRS) against the walk that steps over those
records in the scene's own leaves (MTSG_OPT_LEAF_FILTER 0): the same samples and
the same ray answers, bit for bit, in one process.

Scenes: bunny15 (2 rectangles) and env_glass (1) and their samples from before
the setup mode existed (tests/golden/rect_setup_parent_digests.json); the
builder scene of tests/golden/leaf_filter_scene.txt -- a floor (y = 0), a wall
that is the light (x = 1), twelve small triangles -- under its hand-made tree
(tools/check_kd_layout.cpp: leaves of rectangle records only, with a rectangle
record first, in the middle and last) and under a one-leaf tree (the kd root a
leaf); and the scene of test_gpu_rect_setup_rays, a triangle patch coplanar with
a rectangle, whose tied rays k_tie retraces through the unfiltered layout.
Each with the tail kernel at its default threshold (it keeps the scene's own
leaves: a path changes layout in mid-flight) and with set_finish_paths(0)."""
import hashlib
import json
import os

import numpy as np
import pytest

import mtsg
from conftest import GOLDEN, SCENES
from direct_ref import direct_desc
from multichannel_ref import f32, xf
from oracle import pyoracle as O
from test_gpu_rect_setup_rays import build as coplanar_scene

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
FLOOR, WALL = 0x80000000, 0x80000001
DIGESTS = os.path.join(GOLDEN, "rect_setup_parent_digests.json")
XML = {
    "bunny15": ("bunny15.xml", {"width": 64, "height": 36, "spp": 4}),
    "env_glass": ("env_glass.xml", {"width": 64, "height": 36, "spp": 4, "maxDepth": 8}),
}


def read_fixture():
    tok = open(os.path.join(GOLDEN, "leaf_filter_scene.txt")).read().split()
    out, i = {}, 0
    for key, width, kind in (("vertices", 3, float), ("triangles", 3, int), ("nodes", 2, int), ("indices", 1, int)):
        assert tok[i] == key
        n = int(tok[i + 1]) * width
        out[key] = [kind(x) for x in tok[i + 2:i + 2 + n]]
        i += 2 + n
    assert tok[i] == "aabb" and tok[i + 7] == "max_depth"
    out["aabb"] = [float(x) for x in tok[i + 1:i + 7]]
    out["max_depth"] = int(tok[i + 8])
    return out


def builder_scene(tree="hand", integrator="path"):
    """tools/check_kd_layout.cpp builder_scene, with the fixture's tree or a one-leaf tree."""
    F = read_fixture()
    b = mtsg.SceneBuilder(SCENES)
    b.integrator(integrator, [("maxDepth", "integer", 4)] if integrator == "path" else [])
    b.sensor("perspective", [("fov", "float", 70.0), ("toWorld", "transform", xf([(1, 0, 0), (0, 0, 1), (0, -1, 0)], (0, 1.9, 0)))])
    b.film("hdrfilm", [("width", "integer", 32), ("height", "integer", 32), ("pixelFormat", "string", "rgba")], "gaussian", [])
    b.sampler("independent", [("sampleCount", "integer", 4)])
    grey = b.bsdf("diffuse", [("reflectance", "spectrum", (0.6, 0.6, 0.6))])
    light = b.emitter("area", [("radiance", "spectrum", (6.0, 6.0, 6.0))])
    b.shape("rectangle", [("toWorld", "transform", xf([(1, 0, 0), (0, 0, -1), (0, 1, 0)], (0, 0, 0)))], grey)
    b.shape("rectangle", [("toWorld", "transform", xf([(0, 0, 1), (0, 1, 0), (-1, 0, 0)], (1, 1, 0)))], grey, light)
    b.mesh(np.array(F["vertices"], f32).reshape(-1, 3), np.array(F["triangles"], np.uint32).reshape(-1, 3), face_normals=True,
           bsdf=grey, name="chips")
    s = b.finish()
    assert s.info.n_triangles == 12 and s.info.n_rects == 2
    lo, hi = np.array(F["aabb"][:3], f32), np.array(F["aabb"][3:], f32)
    if tree == "hand":
        s.set_kdtree(dict(nodes=np.array(F["nodes"], np.uint32).reshape(-1, 2), indices=np.array(F["indices"], np.uint32),
                          aabb_min=lo, aabb_max=hi, max_depth=F["max_depth"]))
    else:   # every primitive in one leaf, the rectangles (12, 13) inside the list
        s.set_kdtree(dict(nodes=np.array([[0x80000000, 14]], np.uint32), indices=(np.arange(14, dtype=np.uint32) * 5) % 14,
                          aabb_min=lo, aabb_max=hi, max_depth=0))
    return s


SCENE_MAKERS = {
    "bunny15": lambda: mtsg.Scene(os.path.join(SCENES, XML["bunny15"][0]), XML["bunny15"][1]),
    "env_glass": lambda: mtsg.Scene(os.path.join(SCENES, XML["env_glass"][0]), XML["env_glass"][1]),
    "builder": lambda: builder_scene("hand"),
    "builder-root-leaf": lambda: builder_scene("leaf"),
    "coplanar": lambda: coplanar_scene(),
}
_scenes = {}


def scene_of(name):
    if name not in _scenes:
        _scenes[name] = SCENE_MAKERS[name]()
    return _scenes[name]


def digest(samples):
    return hashlib.sha256(np.ascontiguousarray(samples).tobytes()).hexdigest()


def render(scene, leaf_filter, finish0, options=(), direct=False):
    g = mtsg.GPUScene(scene, 0)
    try:
        g.set_option(mtsg.MTSG_OPT_LEAF_FILTER, leaf_filter)
        for key, value in options:
            g.set_option(key, value)
        if finish0:
            g.set_finish_paths(0)
        p = scene.params()
        if direct:
            g.set_direct(direct_desc(2, 1))
            p.integrator = mtsg.MTSG_INTEGRATOR_DIRECT
        samples = g.render_samples(p)
        if finish0 and not direct:
            assert g.stats().launches_finish == 0
        return samples
    finally:
        g.close()


@pytest.mark.parametrize("finish0", [False, True], ids=["tail", "no-tail"])
@pytest.mark.parametrize("name", list(SCENE_MAKERS))
def test_filtered_and_unfiltered_leaves_render_the_same_samples(name, finish0):
    scene = scene_of(name)
    a, b = render(scene, 1, finish0), render(scene, 0, finish0)
    assert np.isfinite(a).all() and a[..., :3].max() > 0
    assert np.array_equal(a, b)
    if name in XML:
        want = json.load(open(DIGESTS))[f"{name}-{'no-tail' if finish0 else 'tail'}"]
        assert digest(a) == want
        assert digest(b) == want


def test_through_the_direct_integrator():
    scene = scene_of("builder")
    a, b = render(scene, 1, True, direct=True), render(scene, 0, True, direct=True)
    assert np.isfinite(a).all() and a[..., :3].max() > 0
    assert np.array_equal(a, b)


def test_with_pre_records():
    """MTSG_OPT_RAY_PRESETUP 1: k_trace_s_pre walks the filtered leaves too."""
    scene = scene_of("builder")
    pre = ((mtsg.MTSG_OPT_RAY_PRESETUP, 1),)
    want = render(scene, 0, True)
    for finish0 in (True, False):
        a, b = render(scene, 1, finish0, pre), render(scene, 0, finish0, pre)
        assert np.array_equal(a, b)
        assert np.array_equal(a, want)


def unit(d):
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def rays_of(o, d, mint=1e-4, maxt=np.inf):
    r = np.zeros((len(o), 8), f32)
    r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = np.asarray(o, f32), d, mint, maxt
    return r


def query_rays():
    """Named ray lists on the builder scene (cells of the hand-made tree:
    x < 0, z > 0 below y = 1 holds the floor alone; x > 0.5, z < 0 above
    y = 1 holds the wall alone: both leaves are empty in the filtered layout)."""
    n, rng, out = 512, np.random.default_rng(11), {}
    # down onto the floor inside the emptied floor-only cell
    o = np.stack([rng.uniform(-0.9, -0.1, n), rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.9, n)], 1)
    out["into the emptied floor leaf"] = rays_of(o, unit(np.stack([rng.normal(0, 0.02, n), -np.ones(n), rng.normal(0, 0.02, n)], 1)))
    # towards the wall inside the emptied wall-only cell
    o = np.stack([rng.uniform(0.55, 0.9, n), rng.uniform(1.1, 1.9, n), rng.uniform(-0.9, -0.1, n)], 1)
    out["into the emptied wall leaf"] = rays_of(o, unit(np.stack([np.ones(n), rng.normal(0, 0.02, n), rng.normal(0, 0.02, n)], 1)))
    # origins in the floor's plane, any direction; and without the epsilon
    o = np.stack([rng.uniform(-0.95, 0.95, n), np.zeros(n), rng.uniform(-0.95, 0.95, n)], 1)
    d = rng.normal(size=(n, 3))
    d[: n // 4, 1] = 0.0   # in the plane
    out["from the floor's plane"] = rays_of(o, unit(d))
    out["from the floor's plane, mint 0"] = rays_of(o, unit(d), mint=0.0)
    # origins in the wall's plane
    o = np.stack([np.ones(n), rng.uniform(0.05, 1.95, n), rng.uniform(-0.95, 0.95, n)], 1)
    out["from the wall's plane"] = rays_of(o, unit(rng.normal(size=(n, 3))))
    # anywhere to anywhere: every leaf kind
    o = np.stack([rng.uniform(-0.95, 0.95, 4 * n), rng.uniform(0.05, 1.95, 4 * n), rng.uniform(-0.95, 0.95, 4 * n)], 1)
    out["random"] = rays_of(o, unit(rng.normal(size=(4 * n, 3))))
    # dead slots (an empty interval) among live rays
    mix = out["random"][:n].copy()
    mix[::3, 7] = -1.0
    out["dead slots"] = mix
    return out


@pytest.fixture(scope="module", params=["builder", "builder-root-leaf"])
def query_pair(request):
    scene = scene_of(request.param)
    gpu = {m: mtsg.GPUScene(scene, 0) for m in (1, 0)}
    for m, g in gpu.items():
        g.set_option(mtsg.MTSG_OPT_LEAF_FILTER, m)
    yield scene, gpu
    for g in gpu.values():
        g.close()


def test_single_ray_queries(query_pair):
    scene, gpu = query_pair
    seen = set()
    for what, rays in query_rays().items():
        t0, u0, v0, p0 = O.trace_closest(scene.desc, rays)
        ans = {m: gpu[m].trace_closest(rays) for m in (1, 0)}
        for k in range(4):   # t, u, v, primitive: bit for bit between the options
            np.testing.assert_array_equal(ans[1][k].view(np.uint32), ans[0][k].view(np.uint32), err_msg=what)
        t1, u1, v1, p1 = ans[1]
        hit = p0 != MISS
        np.testing.assert_array_equal(p1, p0, err_msg=what)
        np.testing.assert_array_equal(t1[hit], t0[hit], err_msg=what)
        np.testing.assert_array_equal(u1[hit], u0[hit], err_msg=what)
        np.testing.assert_array_equal(v1[hit], v0[hit], err_msg=what)
        assert np.isposinf(t1[~hit]).all(), what
        occ = {m: gpu[m].trace_shadow(rays) for m in (1, 0)}
        np.testing.assert_array_equal(occ[1], occ[0], err_msg=what)
        np.testing.assert_array_equal(occ[1], O.trace_shadow(scene.desc, rays), err_msg=what)
        if what == "into the emptied floor leaf":
            assert (p0 == FLOOR).all()
        if what == "into the emptied wall leaf":
            assert (p0 == WALL).all()
        if what == "dead slots":
            assert (p0[::3] == MISS).all() and (p0 != MISS).any()
        seen |= set(np.unique(p0).tolist())
    assert {FLOOR, WALL, MISS} <= seen and any(p < 12 for p in seen)


def int_fields(st):
    out = {}
    for name, kind in mtsg.Stats._fields_:
        v = getattr(st, name)
        if kind is not mtsg.C.c_double:
            out[name] = list(v) if hasattr(v, "__len__") else int(v)
    return out


# Loop iterations of a wave, with an inner node or a primitive in any lane:
# they depend on which rays share a wave, and that is decided by the order in
# which the waves of a launch win the work list's atomic fetches.  Two counting
# renders of one handle with nothing changed between them differ in these
# (measured on the builder scene, option 0 three times: wave_steps 1613 / 1633 /
# 1594, option 1: 1627 / 1622 / 1620; no other field moved), so they say
# nothing about the option.  Every other integer field is a sum over
# rays (wave_active_lanes too: the lane-iterations) and must be equal.
WAVE_SCHEDULE_FIELDS = {"wave_node_iters", "wave_test_iters", "wave_steps",
                        "shadow_wave_node_iters", "shadow_wave_test_iters", "shadow_wave_steps"}


def counting_render(scene, leaf_filter):
    g = mtsg.GPUScene(scene, 0)
    try:
        g.set_option(mtsg.MTSG_OPT_LEAF_FILTER, leaf_filter)
        g.set_finish_paths(0)
        g.set_flags(mtsg.MTSG_FLAG_COUNT)
        g.render(scene.params(), scene.border)
        return int_fields(g.stats())
    finally:
        g.close()


def test_counting_renders_count_the_same():
    """MTSG_FLAG_COUNT renders walk the scene's own leaves under either option."""
    scene = scene_of("builder")
    got = {m: counting_render(scene, m) for m in (1, 0)}
    for name in got[1]:
        print(name, got[1][name], got[0][name])
    assert got[1]["leaf_refs"] > got[1]["tri_tests"] > 0
    assert set(got[1]) - WAVE_SCHEDULE_FIELDS > {"nodes_visited", "leaf_refs", "tri_tests", "wave_active_lanes", "iter_hist_closest"}
    for name in got[1]:
        if name not in WAVE_SCHEDULE_FIELDS:
            assert got[1][name] == got[0][name], name


def test_the_option_takes_zero_and_one_only():
    scene = mtsg.Scene(os.path.join(SCENES, "cbox.xml"), {"width": 16, "height": 16, "spp": 1})
    g = mtsg.GPUScene(scene, 0)
    try:
        for value in (-1, 2):
            with pytest.raises(RuntimeError):
                g.set_option(mtsg.MTSG_OPT_LEAF_FILTER, value)
        g.set_option(mtsg.MTSG_OPT_LEAF_FILTER, 0)
        g.set_option(mtsg.MTSG_OPT_LEAF_FILTER, 1)
    finally:
        g.close()
