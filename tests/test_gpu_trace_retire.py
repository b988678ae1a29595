"""Batched retirement in the persistent traversal kernel (k_trace_s,
MTSG_RETIRE_BATCH): a finished ray's tie-list entry, error flag, miss record
or unoccluded shadow contribution is written when its wave refills, and at the
latest in the wave's last pass, instead of in the iteration that finished the
ray.  The records must be the ones the oracle gives, for every ray, at the
list sizes around the refill threshold (16 idle lanes), the wave (64) and the
fetch pool (128): a small list is retired in the last pass only, 60000 rays
make every wave retire and refill many times.  Through mtsg_trace_closest /
mtsg_trace_shadow and a render whose every bounce goes through k_trace_s, over
the Cornell box, the flattened C3 scene and the two-level C3 scene."""
import os

import numpy as np
import pytest

import mtsg
from conftest import SCENES
from oracle import pyoracle as O
from test_gpu_parity import check_render, compare_closest

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
SIZES = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 60000]
SMALL = [n for n in SIZES if n <= 129]


def bounds(scene):
    b = scene.prim_bounds()
    live = (b[:, :3] <= b[:, 3:]).all(1)
    return b[live, :3].min(0).astype(np.float32), b[live, 3:].max(0).astype(np.float32)


def inside_rays(lo, hi, n, seed):
    """Random rays that start inside the scene bounds."""
    rng = np.random.default_rng(seed)
    rays = np.zeros((n, 8), np.float32)
    ext = hi - lo
    rays[:, 0:3] = rng.uniform(lo + 0.02 * ext, hi - 0.02 * ext, (n, 3))
    d = rng.normal(size=(n, 3))
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 6] = 1e-4
    rays[:, 7] = np.inf
    return rays


class Pair:
    """A scene on the host and on the device, with pools of rays the oracle
    sorted into those that hit something and those that hit nothing."""

    def __init__(self, name):
        inst = "two-level" if name.endswith("two-level") else "flatten"
        xml = "cbox.xml" if name == "cbox" else "bunny15.xml"
        self.scene = mtsg.Scene(os.path.join(SCENES, xml), {"width": 32, "height": 24, "spp": 1}, instancing=inst)
        self.gpu = mtsg.GPUScene(self.scene, 0)
        self.lo, self.hi = bounds(self.scene)
        pool = inside_rays(self.lo, self.hi, 8192, 7)
        prim = O.trace_closest(self.scene.desc, pool)[3]
        self.hitting, self.missing = pool[prim != MISS], pool[prim == MISS]
        assert len(self.hitting) >= 129 and len(self.missing) >= 129, (len(self.hitting), len(self.missing))


@pytest.fixture(scope="module", params=["cbox", "bunny15", "bunny15-two-level"])
def pair(request):
    p = Pair(request.param)
    yield p
    p.gpu.close()


def test_closest_rays_at_the_refill_boundaries(pair):
    for n in SIZES:
        rays = inside_rays(pair.lo, pair.hi, n, 100 + n)
        compare_closest(pair.scene, pair.gpu, rays)
        p0 = O.trace_closest(pair.scene.desc, rays)[3]
        t1, _, _, p1 = pair.gpu.trace_closest(rays)
        np.testing.assert_array_equal(p1 == MISS, p0 == MISS, err_msg=f"n={n}")
        assert np.isposinf(t1[p1 == MISS]).all(), n


def miss_list(pair, n, seed):
    """n rays that hit nothing: in-bounds rays the oracle found to miss, rays
    that miss the scene bounds altogether (they never enter the loop: the
    refill retires them) and empty intervals."""
    rng = np.random.default_rng(seed)
    rays = pair.missing[rng.integers(0, len(pair.missing), n)].copy()
    kind = np.arange(n) % 4          # 0, 1: in-bounds miss; 2: outside the bounds; 3: empty interval
    ext = pair.hi - pair.lo
    out = kind == 2
    rays[out, 0:3] = pair.hi + ext * rng.uniform(0.5, 2.0, (int(out.sum()), 3)).astype(np.float32)
    rays[out, 3:6] = np.abs(rays[out, 3:6]) + np.float32(1e-3)   # away from the box
    empty = kind == 3
    rays[empty, 6] = 5.0
    rays[empty, 7] = 1.0
    return rays


def test_all_miss_lists_write_the_miss_record(pair):
    for n in SMALL:
        rays = miss_list(pair, n, 200 + n)
        assert (O.trace_closest(pair.scene.desc, rays)[3] == MISS).all()
        t, _, _, p = pair.gpu.trace_closest(rays)
        assert (p == MISS).all(), n
        assert np.isposinf(t).all(), n


def test_shadow_rays_at_the_refill_boundaries(pair):
    ext = float((pair.hi - pair.lo).max())
    for n in SIZES:
        rng = np.random.default_rng(300 + n)
        # every lane runs the deferred read-modify-write
        free = pair.missing[rng.integers(0, len(pair.missing), n)]
        got = pair.gpu.trace_shadow(free)
        np.testing.assert_array_equal(got, O.trace_shadow(pair.scene.desc, free), err_msg=f"unoccluded n={n}")
        assert not got.any(), n
        # no lane does
        blocked = pair.hitting[rng.integers(0, len(pair.hitting), n)]
        got = pair.gpu.trace_shadow(blocked)
        np.testing.assert_array_equal(got, O.trace_shadow(pair.scene.desc, blocked), err_msg=f"occluded n={n}")
        assert got.all(), n
        # a mix
        rays = inside_rays(pair.lo, pair.hi, n, 400 + n)
        rays[:, 7] = rng.uniform(0.01, ext, n)
        got = pair.gpu.trace_shadow(rays)
        np.testing.assert_array_equal(got, O.trace_shadow(pair.scene.desc, rays), err_msg=f"random n={n}")
        if n >= 60000:
            assert 0.01 < got.mean() < 0.99
        # the lists above with the lists of the all-miss test mixed in
        if n <= 129:
            rays = miss_list(pair, n, 500 + n)
            assert not pair.gpu.trace_shadow(rays).any(), n


@pytest.mark.parametrize("name", ["cbox", "bunny15", "bunny15-two-level"])
def test_tiny_render_through_the_per_bounce_launches(name):
    """32 x 24 x 4 spp with the tail kernel off, so that every bounce's closest
    and shadow rays go through k_trace_s: the samples against the oracle's
    (counter-mode random numbers: identical draws per pixel, sample and
    dimension), with the bar of the render parity tests."""
    inst = "two-level" if name.endswith("two-level") else "flatten"
    xml = "cbox.xml" if name == "cbox" else "bunny15.xml"
    s = mtsg.Scene(os.path.join(SCENES, xml), {"width": 32, "height": 24, "spp": 4}, instancing=inst)
    p = s.params()
    g = mtsg.GPUScene(s, 0)
    try:
        g.set_finish_paths(0)
        samples = g.render_samples(p)
        assert g.stats().launches_finish == 0
        img_g = g.render(p, s.border)
    finally:
        g.close()
    img_c, _ = O.render(s.desc, p, s.border, rng=O.RNG_COUNTER)
    check_render(img_c, img_g)
    # the per-sample radiance against the oracle's samples: each pixel's sample
    # mean as a box-filtered block (weight 1), through the same comparison
    assert np.isfinite(samples).all()
    ref = np.stack([np.stack([O.pixel_samples(s.desc, p, x, y) for x in range(32)]) for y in range(24)])

    def block(rgb):
        out = np.ones(rgb.shape[:2] + (5,), np.float32)
        out[..., :3] = rgb.mean(2, dtype=np.float64)
        return out

    l1, mean = check_render(block(ref), block(samples[..., :3]))
    print(f"{name}: per-pixel L1 of the sample means {l1:.3e}, mean {mean:.5f}")
