"""Rectangle pre-records (MTSG_OPT_RAY_PRESETUP 1; the default is 0): on a flat scene
in the setup mode the kernels that make the `path` integrator's rays -- k_camera,
k_camera_lens, k_shade -- run the rectangle tests of kernels.h ray_prerecord and
the traversal's refill reads the 16-B result (k_trace_s_pre), against the refill
running the loop itself (0, k_trace_s).  The same function on the same words, so
the same samples bit for bit, and the samples the library rendered before either
existed (tests/golden/rect_setup_parent_digests.json).

The flattened C3 scene (2 rectangles) and the dielectric environment scene (1)
take the mode; the Cornell box (6 rectangles, over MTSG_RECT_SETUP_CAP) must be
untouched by it.  Each with the tail kernel at its default threshold, without it
(every bounce through the per-bounce launches), and with a threshold so large
that the tail takes over right after bounce 0.  Then the same equality through
the thinlens camera, with two lanes, with the order buffer (allocated only once
MTSG_OPT_RAY_ORDER 1 asks for it), with the other refill width, and on the
routes whose launches carry no pre-records (direct, multichannel)."""
import hashlib
import json
import os

import numpy as np
import pytest

import mtsg
from conftest import GOLDEN, SCENES
from direct_ref import direct_desc

pytestmark = pytest.mark.gpu

CASES = {
    "cbox": ("cbox.xml", {"width": 64, "height": 64, "spp": 4}),
    "bunny15": ("bunny15.xml", {"width": 64, "height": 36, "spp": 4}),
    "env_glass": ("env_glass.xml", {"width": 64, "height": 36, "spp": 4, "maxDepth": 8}),
}
TAILS = {"tail": None, "no-tail": 0, "tail-after-bounce-0": 1 << 30}
DIGESTS = os.path.join(GOLDEN, "rect_setup_parent_digests.json")


def digest(samples):
    return hashlib.sha256(np.ascontiguousarray(samples).tobytes()).hexdigest()


def render(scene, pre, finish=None, options=(), params=None):
    g = mtsg.GPUScene(scene, 0)
    try:
        g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, pre)
        for key, value in options:
            g.set_option(key, value)
        if finish is not None:
            g.set_finish_paths(finish)
        samples = g.render_samples(params if params is not None else scene.params())
        st = g.stats()
        if finish == 0:
            assert st.launches_finish == 0
        elif finish:
            assert st.launches_finish == 1 and st.launches_trace_closest == 2   # bounce 0, bounce 1, then the tail
        return samples, st
    finally:
        g.close()


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    xml, defines = CASES[request.param]
    return request.param, mtsg.Scene(os.path.join(SCENES, xml), defines)


@pytest.mark.parametrize("tail", list(TAILS))
def test_producer_and_refill_tests_render_the_same_samples(case, tail):
    name, scene = case
    (a, sa), (b, sb) = render(scene, 1, TAILS[tail]), render(scene, 0, TAILS[tail])
    assert np.isfinite(a).all() and a[..., :3].max() > 0
    assert np.array_equal(a, b)
    want = json.load(open(DIGESTS)).get(f"{name}-{tail}")
    if want is not None:
        assert digest(a) == want
        assert digest(b) == want
    assert sa.rays_closest == sb.rays_closest
    if name == "cbox":
        # over the cap: no pre-records, no shadow ray dropped where it is made
        assert sa.rays_shadow == sb.rays_shadow
    elif tail == "no-tail":
        # the shadow rays a rectangle occludes are not sent to the traversal:
        # env_glass's rays towards the lower half of the environment meet its
        # ground; bunny15's go up to the light, few can meet the ground
        assert 0 < sa.rays_shadow <= sb.rays_shadow
        assert name != "env_glass" or sa.rays_shadow < sb.rays_shadow


def lens_bunny15(tmp_path):
    xml = open(os.path.join(SCENES, "bunny15.xml")).read()
    assert xml.count('<sensor type="perspective">') == 1 and xml.count('value="bunny.ply"') == 1
    xml = xml.replace('<sensor type="perspective">',
                      '<sensor type="thinlens"><float name="apertureRadius" value="0.1"/><float name="focusDistance" value="7"/>')
    xml = xml.replace('value="bunny.ply"', f'value="{os.path.join(SCENES, "bunny.ply")}"')
    p = tmp_path / "bunny15_lens.xml"
    p.write_text(xml)
    return mtsg.Scene(str(p), {"width": 32, "height": 32, "spp": 4})


@pytest.fixture(scope="module")
def bunny32():
    return mtsg.Scene(os.path.join(SCENES, "bunny15.xml"), {"width": 32, "height": 32, "spp": 4})


def test_through_the_thinlens_camera(tmp_path, bunny32):
    scene = lens_bunny15(tmp_path)
    for finish in (None, 0):
        a, b = render(scene, 1, finish)[0], render(scene, 0, finish)[0]
        assert np.isfinite(a).all() and a[..., :3].max() > 0
        assert np.array_equal(a, b)
    # (the lens is in use: not the pinhole's samples)
    assert not np.array_equal(a, render(bunny32, 1, 0)[0])


@pytest.mark.parametrize("options", [
    ((mtsg.MTSG_OPT_LANES, 2),),                     # two batches in flight: each lane has its own pre-records
    ((mtsg.MTSG_OPT_RAY_ORDER, 1),),                 # the order buffer, allocated on demand; the refill reads pre[order[i]]
    ((mtsg.MTSG_OPT_TRACE_REFILL, 32),),             # k_trace_s_pre<.., 32>
], ids=["lanes-2", "ray-order", "refill-32"])
def test_with_other_schedules(bunny32, options):
    want = render(bunny32, 0, 0)[0]
    # 2 x 2 tiles of 4 spp in batches of 2 tiles: several batches per lane
    p = bunny32.params()
    g = mtsg.GPUScene(bunny32, 0)
    try:
        g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, 1)
        for key, value in options:
            g.set_option(key, value)
        g.set_finish_paths(0)
        if options[0][0] == mtsg.MTSG_OPT_LANES:
            # the lanes run only outside the debug dump, so films are compared.
            # A film value sums at most 4 spp x 5 x 5 pixels of the gaussian's
            # footprint with float atomics in any order: (n - 1) 2^-24 of the sum
            # of its positive terms, 6e-6 (the bound of the staggered-lane test)
            g.set_batch_paths(2 * 256 * 4)
            film = g.render(p, bunny32.border)
            g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, 0)
            np.testing.assert_allclose(film, g.render(p, bunny32.border), rtol=2e-5, atol=2e-5)
            assert film[..., :3].max() > 0
        else:
            np.testing.assert_array_equal(g.render_samples(p), want)
            # back and forth on one handle: the buffers of a batch serve both
            g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, 0)
            np.testing.assert_array_equal(g.render_samples(p), want)
            g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, 1)
            g.set_option(mtsg.MTSG_OPT_RAY_ORDER, 0)
            np.testing.assert_array_equal(g.render_samples(p), want)
    finally:
        g.close()


@pytest.mark.parametrize("name", ["cbox", "bunny15"])
def test_direct_route_is_untouched(name, bunny32):
    """The fan's launches carry no pre-records: the same samples and the same
    ray counts under either option (the Cornell box, and bunny15: a scene
    whose `path` renders do take the mode)."""
    scene = bunny32 if name == "bunny15" else mtsg.Scene(os.path.join(SCENES, "cbox.xml"), {"width": 32, "height": 32, "spp": 4})
    out = {}
    for pre in (1, 0):
        g = mtsg.GPUScene(scene, 0)
        try:
            g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, pre)
            g.set_direct(direct_desc(2, 1))
            q = scene.params()
            q.integrator = mtsg.MTSG_INTEGRATOR_DIRECT
            out[pre] = (g.render_samples(q), g.stats().rays_shadow)
        finally:
            g.close()
    assert np.isfinite(out[1][0]).all() and out[1][0][..., :3].max() > 0
    assert np.array_equal(out[1][0], out[0][0]) and out[1][1] == out[0][1] > 0


def multichannel_cbox(tmp_path):
    xml = open(os.path.join(SCENES, "cbox.xml")).read()
    a, b = xml.index("<integrator"), xml.index("</integrator>") + len("</integrator>")
    multi = ('<integrator type="multichannel"><integrator type="path"><integer name="maxDepth" value="4"/></integrator>'
             '<integrator type="field"><string name="field" value="distance"/></integrator></integrator>')
    xml = xml[:a] + multi + xml[b:]
    assert xml.count('<film type="hdrfilm">') == 1
    xml = xml.replace('<film type="hdrfilm">',
                      '<film type="hdrfilm"><string name="pixelFormat" value="rgb, luminance"/><string name="channelNames" value="c, d"/>')
    p = tmp_path / "cbox_multi.xml"
    p.write_text(xml)
    return mtsg.Scene(str(p), {"width": 32, "height": 32, "spp": 4})


def test_multichannel_route_is_untouched(tmp_path):
    scene = multichannel_cbox(tmp_path)
    out = {}
    for pre in (1, 0):
        g = mtsg.GPUScene(scene, 0)
        try:
            g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, pre)
            g.set_aov(scene)
            out[pre] = g.render_samples_multi(scene.params())
        finally:
            g.close()
    assert np.isfinite(out[1]).all() and out[1].max() > 0
    assert np.array_equal(out[1], out[0])


def test_turning_the_option_on_after_a_render(bunny32):
    """The pre-records are allocated by the first render that asks for them:
    a handle that has rendered without them renders the same samples with them."""
    p = bunny32.params()
    g = mtsg.GPUScene(bunny32, 0)
    try:
        g.set_finish_paths(0)
        g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, 0)
        plain = g.render_samples(p)
        g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, 1)
        np.testing.assert_array_equal(g.render_samples(p), plain)
    finally:
        g.close()


def test_the_option_takes_zero_and_one_only():
    scene = mtsg.Scene(os.path.join(SCENES, "cbox.xml"), {"width": 16, "height": 16, "spp": 1})
    g = mtsg.GPUScene(scene, 0)
    try:
        for value in (-1, 2):
            with pytest.raises(RuntimeError):
                g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, value)
        g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, 0)
        g.set_option(mtsg.MTSG_OPT_RAY_PRESETUP, 1)
    finally:
        g.close()
