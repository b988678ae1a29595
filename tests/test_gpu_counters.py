"""MTSG_FLAG_COUNT: the traversal counters a counting render copies into
mtsg_stats (kernels.h CTR_*: the kernels write the words, the render's final
drain reads them by the same names).  One flat and one two-level render of a
32x32 rectangle, 4 spp, maxDepth 4 (both sides multiples of the tile, so every
path slot is a sample), and the relations that hold between the fields
whatever the scene: a counter word that moved would break them."""
import ctypes as C
import os

import numpy as np
import pytest

import mtsg
from conftest import SCENES

pytestmark = pytest.mark.gpu

INT_FIELDS = [n for n, t in mtsg.Stats._fields_ if t is not C.c_double]


def count_stats(scene):
    """The integer fields of mtsg_stats after one counting render, and the
    number of straggler records."""
    g = mtsg.GPUScene(scene, 0)
    g.set_flags(mtsg.MTSG_FLAG_COUNT)
    g.render(scene.params(tile_w=32, tile_h=32, spp=4, max_depth=4), scene.border)
    st = g.stats()
    buf = np.zeros((64, 12), np.float32)
    n = mtsg.device_lib().mtsg_debug_stragglers(g._h, C.c_void_p(buf.ctypes.data), 64)
    g.close()
    out = {}
    for name in INT_FIELDS:
        v = getattr(st, name)
        out[name] = list(v) if hasattr(v, "__len__") else int(v)
    out["stragglers"] = int(n)
    return out


def flat_scene():
    return mtsg.Scene(os.path.join(SCENES, "cbox.xml"), {"width": 64, "height": 48, "spp": 8})


def instanced_scene():
    return mtsg.Scene(os.path.join(SCENES, "bunny15.xml"), {"width": 160, "height": 90, "spp": 4}, instancing="two-level")


def check_common(st):
    print({k: v for k, v in st.items()})
    assert st["samples"] == 32 * 32 * 4
    for kind in ("closest", "shadow"):
        hist, rays, top = st[f"iter_hist_{kind}"], st[f"rays_{kind}"], st[f"iter_max_{kind}"]
        # a ray whose clip against the scene's box leaves no interval never
        # enters the tree (spec_init) and has no histogram entry
        assert 0 < sum(hist) <= rays
        k = max(i for i, h in enumerate(hist) if h)
        assert top >= 1 << k and (k == 15 or top < 2 << k), (kind, top, k)
    for name in ("nodes_visited", "leaf_refs", "tri_tests", "shadow_nodes_visited", "shadow_leaf_refs", "shadow_tri_tests"):
        assert st[name] > 0, name
    assert 0 < st["wave_active_lanes"] <= 64 * st["wave_steps"]
    assert st["guard_rays_closest"] <= st["restarts_closest"]
    assert st["guard_rays_shadow"] <= st["restarts_shadow"]
    assert 0 <= st["stragglers"] <= 64


def test_counters_flat_scene():
    st = count_stats(flat_scene())
    check_common(st)
    for name in ("instance_visits", "shadow_instance_visits", "instance_rejects", "instance_prefiltered"):
        assert st[name] == 0, name


def test_counters_two_level_scene():
    st = count_stats(instanced_scene())
    check_common(st)
    assert st["instance_visits"] > 0
    # an instance node a ray met in a leaf was prefiltered or visited, and the
    # group-box clip rejects only visits (include/mtsg.h), so of the
    # prefiltered + visited encounters at most the visits are rejected
    assert st["instance_rejects"] <= st["instance_visits"] + st["shadow_instance_visits"]
