"""The `adaptive` integrator on the GPU (src/integrators/misc/adaptive.cpp)
against its float32 restatement (adaptive_ref) over the plain `path` render's
per-sample values: sample s of a pixel under `adaptive` is sample s of the
`path` render at spp = cap, so the counts must agree at every pixel."""
import ctypes as C

import numpy as np
import pytest

import mtsg
import adaptive_ref as A
import direct_ref as DR
import multichannel_ref as R
from conftest import SCENES

pytestmark = pytest.mark.gpu
f32 = np.float32
N = A.N_BASE
FACTOR = 4
CAP = FACTOR * N
# chosen on the CPU oracle's samples of the box so that the restated counts
# hold pixels that stop at N, between N and the cap, and at the cap
MAX_ERROR = 0.4
W, H = DR.FILM_W, DR.FILM_H


def render_adaptive(scene, setup=None, params=None):
    g = mtsg.GPUScene(scene, 0)
    try:
        if setup:
            setup(g)
        p = params or scene.params()
        block = g.render(p, scene.border)
        return block, g.adaptive_info(p), g.stats()
    finally:
        g.close()


def path_samples(scene, params=None):
    g = mtsg.GPUScene(scene, 0)
    try:
        return g.render_samples(params or scene.params())
    finally:
        g.close()


class Box:
    """The plain `path` render's samples at spp = cap and the adaptive render, once."""

    def __init__(self, **kw):
        self.kw = kw
        self.plain = A.path_scene(CAP, **kw)
        self.samples = path_samples(self.plain)
        self.scene = A.adaptive_scene(MAX_ERROR, FACTOR, **kw)
        self.D = R.Desc(self.scene)
        self.params = self.scene.params()
        self.block, self.info, self.stats = render_adaptive(self.scene)
        self.restated = A.restate_counts(self.samples, N, FACTOR, MAX_ERROR, self.info["quantile"], self.info["average_luminance"])
        self.jitter = A.jitter_of(W, H, CAP)
        self.want, self.mag = A.film_reference(self.D, self.jitter, self.samples, self.restated, W, H)
        self.terms = A.film_terms(self.D, CAP)


@pytest.fixture(scope="module")
def box():
    return Box()


def test_counts_and_film_against_the_restatement(box):
    """1. Every pixel's count equals the restated rule's, all three classes of
    pixels are present, and the block is sum (1 / n_p) sum w v within
    n_terms 2^-24 sum|w v| per texel, n_terms = 25 (cap + 3).
    Measured on an MI355X: every count equal; the largest film deviation is
    0.0051 of the bound (counts: 260 pixels at N, 187 at the cap, 513 between)."""
    c = box.restated
    assert (c == N).any() and ((c > N) & (c < CAP)).any() and (c == CAP).any(), np.bincount(c.ravel())
    np.testing.assert_array_equal(box.info["counts"], c)
    assert box.info["total_samples"] == int(c.sum()) == box.stats.samples
    assert box.info["quantile"] == f32(1.959963984540054)
    worst = A.film_error(box.block, box.want, box.mag, box.terms)
    print(f"adaptive film: largest deviation {worst:.4f} of the bound; counts {np.bincount(c.ravel())[N:]}")
    assert worst <= 1.0


def test_max_sample_factor_one_is_the_plain_render():
    """2. maxSampleFactor = 1: every count is N and the developed image is the
    plain `path` render's at N spp (the block is that render's times 1 / N: the
    bound of test 1 on the scaled block); maxSampleFactor = 0: one sample."""
    plain = A.path_scene(N)
    g = mtsg.GPUScene(plain, 0)
    try:
        want = g.render(plain.params(), plain.border)
    finally:
        g.close()
    scene = A.adaptive_scene(0.05, 1)
    block, info, _ = render_adaptive(scene)
    assert (info["counts"] == N).all() and info["rounds"] == 1
    scale = (f32(1) / f32(N)).astype(np.float64)
    bound = A.film_terms(R.Desc(scene), N) * 2.0 ** -24 * np.abs(want.astype(np.float64)) * scale
    assert np.all(np.abs(block.astype(np.float64) - want.astype(np.float64) * scale) <= bound)
    a, b = mtsg.develop(block), mtsg.develop(want)
    assert np.abs(a - b).max() <= 64 * 2.0 ** -24 * max(1.0, float(b.max()))
    assert b.max() > 0
    _, info0, _ = render_adaptive(A.adaptive_scene(0.05, 0))
    assert (info0["counts"] == 1).all() and info0["total_samples"] == W * H


@pytest.mark.parametrize("how", ["batch_paths", "round_size"])
def test_counts_do_not_depend_on_scheduling(box, how):
    """3. A small wavefront batch (the rounds are cut along tiles and samples)
    and another round size leave every count as it was and the film within
    test 1's bound.  The film is not bit-identical: a pixel's window is summed
    in sample order whatever the cut, but the film adds the windows of the
    pixels that stop in one batch together, so its sums are regrouped."""
    setup = (lambda g: g.set_batch_paths(3 * 256)) if how == "batch_paths" else (lambda g: g.set_option(mtsg.MTSG_OPT_ADAPTIVE_ROUND, 5))
    block, info, _ = render_adaptive(box.scene, setup)
    np.testing.assert_array_equal(info["counts"], box.restated)
    assert info["average_luminance"] == box.info["average_luminance"]
    assert A.film_error(block, box.want, box.mag, box.terms) <= 1.0
    if how == "round_size":
        assert info["rounds"] > box.info["rounds"] - 1 and info["rounds"] >= 2


LENS = ("thinlens", [("fov", "float", 40.0), ("apertureRadius", "float", 0.08), ("focusDistance", "float", 3.4),
                     ("toWorld", "transform", R.xf([(-1, 0, 0), (0, 1, 0), (0, 0, -1)], (0.05, 0.1, 3.6)))])
CROP = [("cropOffsetX", "integer", 9), ("cropOffsetY", "integer", 5), ("cropWidth", "integer", 21), ("cropHeight", "integer", 13)]


def test_thinlens_counts_and_a_crop_window():
    """4. thinlens: the aperture draw moves the path's dimensions and the
    counts still equal the restatement's.  A crop window renders its pixels
    only, with the counts of the same pixels of the full render's restatement
    given the crop render's own pre-pass value, which still samples the full film."""
    plain = A.path_scene(CAP, sensor=LENS)
    samples = path_samples(plain)
    scene = A.adaptive_scene(MAX_ERROR, FACTOR, sensor=LENS)
    _, info, _ = render_adaptive(scene)
    want = A.restate_counts(samples, N, FACTOR, MAX_ERROR, info["quantile"], info["average_luminance"])
    np.testing.assert_array_equal(info["counts"], want)
    assert len(np.unique(want)) > 2
    crop = A.adaptive_scene(MAX_ERROR, FACTOR, sensor=LENS, film_props=CROP)
    p = crop.params()
    assert (p.tile_x, p.tile_y, p.tile_w, p.tile_h) == (9, 5, 21, 13)
    block, cinfo, _ = render_adaptive(crop)
    assert block.shape[:2] == (13 + 2 * crop.border, 21 + 2 * crop.border)
    # the pre-pass does not see the crop: the same 10000 full-film samples
    assert cinfo["average_luminance"] == info["average_luminance"]
    np.testing.assert_array_equal(cinfo["counts"], want[5:18, 9:30])


def test_prepass_average_luminance(box):
    """5. averageLuminance against the mean sample luminance of the plain
    render over the full film, within 5 standard errors of the difference (the
    two sample variances are the film samples' and the pre-pass's own, which
    mtsg_adaptive_info reports); two renders give the same bits."""
    lum = A.luminance(box.samples[..., :3]).astype(np.float64).ravel()
    got = float(box.info["average_luminance"])
    assert box.info["luminance_variance"] > 0
    se = np.sqrt(lum.var(ddof=1) / lum.size + box.info["luminance_variance"] / A.PREPASS_SAMPLES)
    assert abs(got - lum.mean()) <= 5 * se, (got, lum.mean(), se)
    assert got > 0
    _, again, _ = render_adaptive(box.scene)
    assert again["average_luminance"].tobytes() == box.info["average_luminance"].tobytes()


def dark_light_geometry(b):
    """A wall and, in front of it, a rectangle whose emitter has a negative
    radiance: every sample of the pixels that see it is negative and
    ImageBlock::put rejects it; a second, ordinary light keeps the rest lit."""
    wall = b.bsdf("diffuse", [("reflectance", "spectrum", (0.7, 0.65, 0.6))])
    bad = b.emitter("area", [("radiance", "spectrum", (-4.0, -4.0, -4.0))])
    light = b.emitter("area", [("radiance", "spectrum", (15.0, 14.0, 12.0))])
    b.shape("rectangle", [("toWorld", "transform", R.xf([(1.5, 0, 0), (0, 1.0, 0), (0, 0, 1)], (0, 0, -1.0)))], wall)
    b.shape("rectangle", [("toWorld", "transform", R.xf([(0.3, 0, 0), (0, 0.3, 0), (0, 0, 1)], (-0.4, 0.1, 0.5)))], -1, bad)
    b.shape("rectangle", [("toWorld", "transform", R.xf([(0.4, 0, 0), (0, 0, 0.4), (0, -1, 0)], (0.5, 0.99, 0)))], -1, light)


def test_rejected_samples_count_with_luminance_zero():
    """6. The pixels that see the negative emitter have every sample rejected:
    they stop at N (mean = meanSqr = 0), add nothing to the block, weight
    included, and the render ends; the counts equal the restatement's."""
    kw = dict(geometry=dark_light_geometry, path_props=(("maxDepth", "integer", 1),))
    samples = path_samples(A.path_scene(CAP, **kw))
    ok = A.accepted(samples)
    dead = ~ok.any(-1)
    assert dead.sum() >= 4 and ok.all(-1).sum() >= 4
    scene = A.adaptive_scene(MAX_ERROR, FACTOR, **kw)
    block, info, _ = render_adaptive(scene)
    want = A.restate_counts(samples, N, FACTOR, MAX_ERROR, info["quantile"], info["average_luminance"])
    np.testing.assert_array_equal(info["counts"], want)
    assert (info["counts"][dead] == N).all()
    D = R.Desc(scene)
    ref, mag = A.film_reference(D, A.jitter_of(W, H, CAP), samples, want, W, H)
    assert A.film_error(block, ref, mag, A.film_terms(D, CAP)) <= 1.0
    # a texel whose whole footprint lies in the rejected region has weight 0
    assert (mag[..., 4] == 0).any() and np.all(block[..., 4][mag[..., 4] == 0] == 0)


CANCEL_ERROR = 1.5   # the box's tiles then finish in different rounds (chosen on the CPU oracle's samples)


def test_cancel_from_the_tile_callback(box):
    """7. A cancel from the first tile callback ends the render with the
    cancel status between rounds; the handle then renders as before.  The
    callback fires when a tile's last pixel stops, after the round in which it does."""
    want = A.restate_counts(box.samples, N, FACTOR, CANCEL_ERROR, box.info["quantile"], box.info["average_luminance"])
    last = np.array([[want[y:y + 16, x:x + 16].max() for x in range(0, W, 16)] for y in range(0, H, 16)])
    rounds = (last + N - 1) // N   # rounds of N samples a tile takes
    assert rounds.min() < rounds.max()
    scene = A.adaptive_scene(CANCEL_ERROR, FACTOR)
    g = mtsg.GPUScene(scene, 0)
    try:
        lib = mtsg.device_lib()
        seen = []

        def on_tile(user, key, x, y, w, h):
            if not seen:
                lib.mtsg_cancel(g._h)
            seen.append(key)

        fn = mtsg.TILE_FN(on_tile)
        assert lib.mtsg_set_tile_callback(g._h, fn, None) == mtsg.MTSG_OK
        p = scene.params()
        out = np.zeros((p.tile_h + 2 * scene.border, p.tile_w + 2 * scene.border, 5), f32)
        rc = lib.mtsg_render(g._h, C.byref(p), out.ctypes.data_as(C.c_void_p))
        assert rc == mtsg.MTSG_ERR_CANCELLED
        first = int((rounds == rounds.min()).sum())
        assert len(seen) == first   # the tiles of the first round that finished any
        block = g.render(p, scene.border)
        assert len(seen) == first + last.size   # every tile once, as its last pixel stops
        info = g.adaptive_info(p)
        np.testing.assert_array_equal(info["counts"], want)
        ref, mag = A.film_reference(box.D, box.jitter, box.samples, want, W, H)
        assert A.film_error(block, ref, mag, box.terms) <= 1.0
    finally:
        g.close()


def textured_geometry(b):
    """The box with a bitmap texture, filtered through the camera rays' differentials, on the back wall and the floor
    (seen at a grazing angle: anisotropic footprints)."""
    tex = b.texture("bitmap", [("filename", "string", "tex_checker.png"), ("filterType", "string", "ewa"), ("uscale", "float", 6.0),
                               ("vscale", "float", 6.0)])
    wall = b.bsdf("diffuse", [("reflectance", "texture", tex)])
    light = b.emitter("area", [("radiance", "spectrum", (15.0, 14.0, 12.0))])
    b.shape("rectangle", [("toWorld", "transform", R.xf([(1.2, 0, 0), (0, 1, 0), (0, 0, 1)], (0, 0, -1.0)))], wall)
    b.shape("rectangle", [("toWorld", "transform", R.xf([(1.2, 0, 0), (0, 0, -1.2), (0, 1, 0)], (0, -0.5, 0.2)))], wall)
    b.shape("rectangle", [("toWorld", "transform", R.xf([(0.4, 0, 0), (0, 0, 0.4), (0, -1, 0)], (0, 0.99, 0)))], -1, light)


def test_textured_scene_keeps_the_base_count_differentials():
    """8. A filtered texture under maxSampleFactor = 1 against plain `path` at
    N spp, as test 2: the filtered lookups go through the adaptive camera
    kernel's differentials.  With a factor of 1 the cap equals N, so this case
    cannot tell 1 / sqrt(N) from 1 / sqrt(cap): the test below does."""
    kw = dict(geometry=textured_geometry, path_props=(("maxDepth", "integer", 2),))
    plain = A.path_scene(N, **kw)
    g = mtsg.GPUScene(plain, 0)
    try:
        want = g.render(plain.params(), plain.border)
    finally:
        g.close()
    scene = A.adaptive_scene(0.05, 1, **kw)
    block, info, _ = render_adaptive(scene)
    assert (info["counts"] == N).all()
    scale = (f32(1) / f32(N)).astype(np.float64)
    bound = A.film_terms(R.Desc(scene), N) * 2.0 ** -24 * np.abs(want.astype(np.float64)) * scale
    assert np.all(np.abs(block.astype(np.float64) - want.astype(np.float64) * scale) <= bound)
    assert want[..., :3].max() > 0


def test_entries_that_refuse_adaptive_scenes(box):
    """mtsg_render_samples and the tile-window entry return MTSG_ERR_INVALID with a message."""
    g = mtsg.GPUScene(box.scene, 0)
    try:
        with pytest.raises(RuntimeError, match="adaptive"):
            g.render_samples(box.scene.params())
        lib = mtsg.device_lib()
        p = box.scene.params()
        buf = C.c_void_p()
        assert lib.mtsg_device_alloc(g._h, 4096 * 64, C.byref(buf)) == mtsg.MTSG_OK
        assert lib.mtsg_render_device_tiles(g._h, C.byref(p), buf) == mtsg.MTSG_ERR_INVALID
        lib.mtsg_device_free(g._h, buf)
        # a tile share renders: the two halves of the deal sum to the whole film
        halves = []
        for off in (0, 1):
            q = box.scene.params(tile_stride=2, tile_offset=off)
            halves.append((g.render(q, box.scene.border), g.adaptive_info(q)["counts"]))
        np.testing.assert_array_equal(halves[0][1] + halves[1][1], box.restated)
        assert ((halves[0][1] == 0) | (halves[1][1] == 0)).all()
        assert A.film_error(halves[0][0] + halves[1][0], box.want, box.mag, box.terms + 1) <= 1.0
    finally:
        g.close()


def test_environment_scene_carries_the_differentials(tmp_path):
    """An environment scene (scenes/env_glass.xml, 40x24): a camera ray that
    misses looks the environment up through its differentials, which an adaptive
    render always carries in the path state, scaled by 1 / sqrt(N).  With
    maxSampleFactor = 1 the block is the plain render's at N spp times 1 / N,
    within test 2's bound, and every count is N."""
    import os
    src = open(os.path.join(SCENES, "env_glass.xml")).read()
    a = src.index('<integrator type="path">')
    b = src.index('</integrator>', a) + len('</integrator>')
    xml = tmp_path / "env_adaptive.xml"
    xml.write_text((src[:a] + '<integrator type="adaptive"><integer name="maxSampleFactor" value="1"/>' + src[a:b] + '</integrator>'
                    + src[b:]).replace('"bunny.ply"', '"%s"' % os.path.join(SCENES, "bunny.ply")))
    defs = {"width": W, "height": H, "spp": N, "maxDepth": 6, "envmap": os.path.join(SCENES, "envmap.exr")}
    plain = mtsg.Scene(os.path.join(SCENES, "env_glass.xml"), defs)
    g = mtsg.GPUScene(plain, 0)
    try:
        want = g.render(plain.params(), plain.border)
    finally:
        g.close()
    scene = mtsg.Scene(str(xml), defs)
    block, info, _ = render_adaptive(scene)
    assert (info["counts"] == N).all() and info["average_luminance"] > 0
    scale = (f32(1) / f32(N)).astype(np.float64)
    bound = A.film_terms(R.Desc(scene), N) * 2.0 ** -24 * np.abs(want.astype(np.float64)) * scale
    assert np.all(np.abs(block.astype(np.float64) - want.astype(np.float64) * scale) <= bound)
    assert want[..., :3].max() > 0


def env_xml(tmp_path, props):
    import os
    src = open(os.path.join(SCENES, "env_glass.xml")).read()
    a = src.index('<integrator type="path">')
    b = src.index('</integrator>', a) + len('</integrator>')
    xml = tmp_path / "env_adaptive2.xml"
    xml.write_text((src[:a] + '<integrator type="adaptive">' + props + src[a:b] + '</integrator>' + src[b:])
                   .replace('"bunny.ply"', '"%s"' % os.path.join(SCENES, "bunny.ply")))
    return str(xml)


def test_differential_scale_is_the_base_count_under_a_larger_cap(tmp_path):
    """The sample id of sample s of film pixel (0, 0) is s whatever the cap, so
    its first N samples under `adaptive` with maxSampleFactor = 2 draw the
    random numbers of the plain render at N spp; a maxError that every pixel
    meets at N makes them the pixel's whole contribution.  On an 8x6 film of
    scenes/env_glass.xml the pixel's rays miss into the environment, whose EWA
    lookup depends on the differentials' scale: the plain render's samples at
    2N spp (scale 1 / sqrt(2N), the same random numbers) differ from those at N
    spp, and the adaptive block of the one-pixel rectangle is the N-spp block
    times 1 / N within test 2's bound."""
    import os
    defs = {"width": 8, "height": 6, "maxDepth": 6, "envmap": os.path.join(SCENES, "envmap.exr")}
    plain = mtsg.Scene(os.path.join(SCENES, "env_glass.xml"), dict(defs, spp=N))
    plain2 = mtsg.Scene(os.path.join(SCENES, "env_glass.xml"), dict(defs, spp=2 * N))
    one = dict(tile_x=0, tile_y=0, tile_w=1, tile_h=1)
    g = mtsg.GPUScene(plain, 0)
    try:
        want = g.render(plain.params(**one), plain.border)
        s1 = g.render_samples(plain.params(**one))
    finally:
        g.close()
    s2 = path_samples(plain2, plain2.params(**one))
    # the check can see the scale: same random numbers, another footprint, other values
    assert s1.shape[2] == N and (s1[0, 0, :, :3] != s2[0, 0, :N, :3]).any()
    assert s1[..., 3].max() == 0 or s1[..., :3].max() > 0
    scene = mtsg.Scene(env_xml(tmp_path, '<integer name="maxSampleFactor" value="2"/><float name="maxError" value="1e6"/>'), dict(defs, spp=N))
    p = scene.params(**one)
    block, info, _ = render_adaptive(scene, params=p)
    assert info["counts"].shape == (1, 1) and info["counts"][0, 0] == N
    scale = (f32(1) / f32(N)).astype(np.float64)
    bound = A.film_terms(R.Desc(scene), N) * 2.0 ** -24 * np.abs(want.astype(np.float64)) * scale
    assert np.all(np.abs(block.astype(np.float64) - want.astype(np.float64) * scale) <= bound)
    assert want[..., :3].max() > 0
