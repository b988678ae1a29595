"""Rectangles tested at ray setup (k_trace_s's production flat kernels,
kernels.h spec_init<true>; MTSG_OPT_RECT_SETUP 1, the default) against the
in-leaf test every other traversal keeps (MTSG_OPT_RECT_SETUP 0): the same
samples, bit for bit, in one process, and the samples the library rendered
before the setup mode existed (tests/golden/rect_setup_parent_digests.json:
sha256 of render_samples, recorded from the parent commit's library).  The
flattened C3 scene (2 rectangles among the triangles) and the dielectric
environment scene (1 rectangle) take the setup mode; the Cornell box (6
rectangles, over MTSG_RECT_SETUP_CAP) renders with the in-leaf kernel
k_trace_s_leaf under either option, so its case holds that kernel to the
parent's samples.  Each with the
tail kernel at its default threshold -- the tail kernel keeps the in-leaf test,
so a path changes mode in mid-flight -- and with every bounce in k_trace_s
(set_finish_paths(0))."""
import hashlib
import json
import os

import numpy as np
import pytest

import mtsg
from conftest import GOLDEN, SCENES

pytestmark = pytest.mark.gpu

CASES = {
    "cbox": ("cbox.xml", {"width": 64, "height": 64, "spp": 4}),
    "bunny15": ("bunny15.xml", {"width": 64, "height": 36, "spp": 4}),
    "env_glass": ("env_glass.xml", {"width": 64, "height": 36, "spp": 4, "maxDepth": 8}),
}
DIGESTS = os.path.join(GOLDEN, "rect_setup_parent_digests.json")


def digest(samples):
    return hashlib.sha256(np.ascontiguousarray(samples).tobytes()).hexdigest()


def render(scene, setup, finish0):
    g = mtsg.GPUScene(scene, 0)
    try:
        if setup is not None:
            g.set_option(mtsg.MTSG_OPT_RECT_SETUP, setup)
        if finish0:
            g.set_finish_paths(0)
        samples = g.render_samples(scene.params())
        if finish0:
            assert g.stats().launches_finish == 0
        return samples
    finally:
        g.close()


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    xml, defines = CASES[request.param]
    return request.param, mtsg.Scene(os.path.join(SCENES, xml), defines)


@pytest.mark.parametrize("finish0", [False, True], ids=["tail", "no-tail"])
def test_setup_and_in_leaf_render_the_same_samples(case, finish0):
    name, scene = case
    a, b = render(scene, 1, finish0), render(scene, 0, finish0)
    assert np.isfinite(a).all() and a[..., :3].max() > 0
    assert np.array_equal(a, b)
    want = json.load(open(DIGESTS))[f"{name}-{'no-tail' if finish0 else 'tail'}"]
    assert digest(a) == want
    assert digest(b) == want


def test_the_option_takes_zero_and_one_only():
    scene = mtsg.Scene(os.path.join(SCENES, "cbox.xml"), {"width": 16, "height": 16, "spp": 1})
    g = mtsg.GPUScene(scene, 0)
    try:
        for value in (-1, 2):
            with pytest.raises(RuntimeError):
                g.set_option(mtsg.MTSG_OPT_RECT_SETUP, value)
        g.set_option(mtsg.MTSG_OPT_RECT_SETUP, 0)
        g.set_option(mtsg.MTSG_OPT_RECT_SETUP, 1)
    finally:
        g.close()
