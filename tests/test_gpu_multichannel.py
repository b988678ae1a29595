"""The `multichannel` integrator with `path` and `field` children on the GPU
(multichannel.cpp:87-243, field.cpp:55-187; csrc/fields.hip): the colour of
the `path` child is the plain render's bit for bit, every field is checked
per sample against the CPU oracle's camera rays and closest hits, the film of
the fields against a restatement of ImageBlock::put, and the instanced,
split and fields-only renders and the entry points against each other.

The scene (multichannel_ref.box_scene): a box of a UV-mapped, vertex-normal,
textured floor, a face-normal plastic wall, a roughplastic wall, a back wall
that leaves an opening, a roughconductor cube, a twosided panel seen from
behind and a rectangle light; film 40 x 24 (no multiple of 16), 4 spp,
undefined = (-1, 0.5, 7)."""
import ctypes as C

import numpy as np
import pytest

import mtsg
import multichannel_ref as R
from oracle import pyoracle as O
from test_gpu_parity import check_render

pytestmark = pytest.mark.gpu
f32 = np.float32

# two child sets cover the nine fields within MTSG_MAX_SUBINTEGRATORS = 8
WITH_PATH = ["path", "position", "relPosition", "distance", "geoNormal", "shNormal", "uv", "albedo"]
FIELDS_ONLY = ["shapeIndex", "primIndex", "distance", "shNormal", "uv", "albedo", "position"]


def planes(block, children, name):
    k = children.index(name)
    return block[..., 3 * k:3 * k + 3]


def render_multi(scene, **over):
    g = mtsg.GPUScene(scene, 0)
    try:
        return g.render_multi(scene.params(**over), scene.border)
    finally:
        g.close()


def single_owner(shape, border, width, height):
    """Texels of a block (h + 2b, w + 2b) that one 16x16 tile's filter support
    covers alone.  A texel that several tiles reach is summed by float
    atomics of several workgroups in no fixed order (k_splat's flush), so two
    renders of the same samples -- two plain renders too -- can differ there
    in the last bit; everywhere else the film is a fixed-order sum."""
    def owners(n, size):
        c = np.zeros(n + 2 * border, np.int64)
        for t0 in range(0, size, 16):
            c[t0:min(t0 + 16, size) + 2 * border] += 1
        return c
    own = owners(height, height)[:, None] * owners(width, width)[None, :]
    assert own.shape == tuple(shape[:2])
    return own == 1


def assert_same_film(a, b, border, width=R.FILM_W, height=R.FILM_H):
    """Bit equality where one workgroup owns the texel; where tiles overlap,
    the comparison tests/test_gpu_c4.py uses for sums in another order."""
    one = single_owner(a.shape, border, width, height)
    assert one.mean() > 0.4
    np.testing.assert_array_equal(a[one], b[one])
    np.testing.assert_allclose(a, b, rtol=2e-5, atol=2e-6)


def render_plain_samples(scene):
    g = mtsg.GPUScene(scene, 0)
    try:
        return g.render_samples(scene.params())
    finally:
        g.close()


def render_plain(scene, **over):
    g = mtsg.GPUScene(scene, 0)
    try:
        return g.render(scene.params(**over), scene.border)
    finally:
        g.close()


@pytest.mark.parametrize("rfilter", [("gaussian", []), ("box", [("radius", "float", 0.5)])], ids=["gaussian", "box"])
@pytest.mark.parametrize("children", [WITH_PATH, WITH_PATH[1:] + ["path"]], ids=["path-first", "path-last"])
@pytest.mark.parametrize("sampler", ["independent", "sobol"])
def test_colour_is_the_plain_render(rfilter, children, sampler):
    """1. The `path` child is the plain `path` render (field children draw no
    random numbers; the multichannel block rejects no sample, and this scene's
    path produces none to reject): every sample's radiance and alpha bit for
    bit, and the film's planes, alpha and weight bit for bit wherever the film
    is a fixed-order sum (single_owner; measured on an MI355X: on the other
    texels 2 of the 3696 colour floats differed from the plain render's, by
    one unit in the last place)."""
    ps, ms = R.box_scene(None, rfilter, sampler), R.box_scene(children, rfilter, sampler)
    gp, gm = mtsg.GPUScene(ps, 0), mtsg.GPUScene(ms, 0)
    try:
        plain, plain_samples = gp.render(ps.params(), ps.border), gp.render_samples(ps.params())
        multi, multi_samples = gm.render_multi(ms.params(), ms.border), gm.render_samples_multi(ms.params())
    finally:
        gp.close()
        gm.close()
    assert multi.shape[-1] == 3 * len(children) + 2
    assert plain[..., :3].max() > 0
    np.testing.assert_array_equal(planes(multi_samples, children, "path"), plain_samples[..., :3])
    np.testing.assert_array_equal(multi_samples[..., -1], plain_samples[..., 3])
    colour = np.concatenate([planes(multi, children, "path"), multi[..., -2:]], -1)
    assert_same_film(colour, plain, ps.border)
    assert 0 < multi[..., -2].sum() < multi[..., -1].sum()   # some camera rays leave through the opening


class Reference:
    """Per sample: the oracle's camera ray and closest hit, the fields the
    reference's code gives for them, the jitter -- computed once."""

    def __init__(self, children):
        self.children = children
        self.scene = R.box_scene(children)
        self.aov = self.scene.aov()
        self.D = R.Desc(self.scene)
        p = self.scene.params()
        self.params = p
        L = O.lib()
        L.oracle_debug_path_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        h, w, spp = p.tile_h, p.tile_w, p.spp
        rays = np.zeros((h, w, spp, 8), f32)
        jit = np.zeros((h, w, spp, 2), f32)
        one = np.zeros(8, f32)
        for y in range(h):
            for x in range(w):
                for s in range(spp):
                    assert L.oracle_debug_path_rays(self.scene.desc, C.byref(p), x, y, s, O._p(one), 1) == 1
                    rays[y, x, s] = one
                    jit[y, x, s] = O.sampler_draws(self.scene.desc, p, x, y, s, [2])
        self.rays, self.jitter = rays, jit
        flat = rays.reshape(-1, 8)
        t, u, v, prim = O.trace_closest(self.scene.desc, flat)
        self.fields, miss = R.expected_fields(self.D, self.aov, flat, t, u, v, prim,
                                              lambda tex, uv: O.tex_eval(self.scene.desc, tex, uv))
        self.miss = miss.reshape(h, w, spp)
        self.prim = prim.reshape(h, w, spp)
        g = mtsg.GPUScene(self.scene, 0)
        try:
            self.samples = g.render_samples_multi(p)
            self.block = g.render_multi(p, self.scene.border)
        finally:
            g.close()

    def expected(self, name):
        return self.fields[name].reshape(self.miss.shape + (3,))

    def got(self, name):
        return planes(self.samples, self.children, name)


@pytest.fixture(scope="module")
def with_path():
    return Reference(WITH_PATH)


@pytest.fixture(scope="module")
def fields_only():
    return Reference(FIELDS_ONLY)


def check_fields(ref):
    alpha = ref.samples[..., -1]
    # the set of miss samples is the oracle's
    np.testing.assert_array_equal(alpha == 0, ref.miss)
    assert set(np.unique(alpha)) == {0.0, 1.0} and 0.02 < ref.miss.mean() < 0.6
    worst = {}
    for name in ref.children:
        if name == "path":
            continue
        got, want = ref.got(name), ref.expected(name)
        # a miss returns `undefined` exactly, in every field
        np.testing.assert_array_equal(got[ref.miss], np.tile(f32(R.UNDEFINED), (int(ref.miss.sum()), 1)))
        hit = ~ref.miss
        u = R.ulps(got[hit], want[hit])
        worst[name] = float(u.max())
        if name in ("distance", "primIndex", "shapeIndex"):
            np.testing.assert_array_equal(got[hit], want[hit])
        elif name in ("geoNormal", "shNormal"):
            # 4 ulp of 1
            assert np.abs(got[hit].astype(np.float64) - want[hit]).max() <= 4 * 2.0 ** -23, name
        else:
            assert u.max() <= 4, (name, u.max())
    print("largest deviation per field, in ulp of the vector's largest component:", worst)
    return worst


def test_fields_per_sample_against_the_oracle(with_path):
    """2. position, relPosition, distance, normals, uv and albedo of every
    sample.  Measured on an MI355X: 0 ulp in every field (bit equality)."""
    ref = with_path
    check_fields(ref)
    hit = ~ref.miss
    # every material of the scene is seen, constant albedos are exactly the descriptor's
    textured = ref.aov.bsdf_textured
    alb = ref.got("albedo")[hit]
    consts = {tuple(f) for f, t in zip(ref.aov.bsdf_factor.tolist(), textured) if not t}
    seen = {tuple(a) for a in alb.tolist()}
    assert (0.0, 0.0, 0.0) in seen                       # roughconductor (and the light's absorbing BSDF)
    assert tuple(f32([0.1, 0.75, 0.2]).tolist()) in seen  # the twosided panel from behind: its back colour
    assert tuple(f32([0.8, 0.1, 0.1]).tolist()) not in seen
    assert len(seen & consts) >= 5 and len(seen - consts) > 50   # + the textured floor's lookups
    # vertex-normal and face-normal meshes, rectangles
    assert (ref.prim[hit] < 0x80000000).mean() > 0.2 and (ref.prim[hit] >= 0x80000000).mean() > 0.2
    sn, gn = ref.got("shNormal")[hit], ref.got("geoNormal")[hit]
    assert (np.abs(sn - gn).max(-1) > 1e-3).mean() > 0.05   # the bumped floor's interpolated normals


def test_index_fields_per_sample_against_the_oracle(fields_only):
    """2. (second child set) shapeIndex, primIndex and the rest, fields only."""
    ref = fields_only
    check_fields(ref)
    hit = ~ref.miss
    si = ref.got("shapeIndex")[hit][:, 0]
    assert set(np.unique(si)) >= {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}   # floor, wall, two rectangles, cube, panel
    pi = ref.got("primIndex")[hit][:, 0]
    assert pi.max() > 20 and np.all(pi[ref.prim[hit] >= 0x80000000] == 0)


def film_check(ref, block, names):
    D = ref.D
    p = ref.params
    for name in names:
        want, mag = R.film_reference(D, ref.jitter, ref.expected(name), p.tile_w, p.tile_h)
        got = planes(block, ref.children, name).astype(np.float64)
        n_terms = (2 * D.border + 1) ** 2 * p.spp
        bound = n_terms * 2.0 ** -23 * mag
        assert np.all(np.abs(got - want) <= bound), (name, float((np.abs(got - want) - bound).max()))
    ones = np.ones(ref.miss.shape + (1,), f32)
    want, mag = R.film_reference(D, ref.jitter, np.concatenate([(~ref.miss)[..., None].astype(f32), ones], -1), p.tile_w, p.tile_h)
    n_terms = (2 * D.border + 1) ** 2 * p.spp
    assert np.all(np.abs(block[..., -2:] - want) <= n_terms * 2.0 ** -23 * mag)


def test_film_of_the_fields_gaussian(with_path, fields_only):
    """3. The block's field planes, alpha and weight against ImageBlock::put
    restated with the descriptor's filter table (float64 sums of float32
    weights); per texel within n_terms 2^-23 sum|w v|, n_terms = 25 spp."""
    film_check(with_path, with_path.block, WITH_PATH[1:])
    film_check(fields_only, fields_only.block, FIELDS_ONLY)


def test_film_of_the_fields_box(with_path):
    """3. Box filter.  With an effective radius of exactly 0.5 (the rfilter's
    radius + 1e-5, rfilter.cpp / box.cpp) the discretized weights are exactly
    1 and the border is 0: each texel is the float32 sum of its own samples'
    values in sample order, and the weight is spp -- exactly.  With the
    `radius` parameter itself at 0.5 the reference's normalised table holds
    1 / 1.00002 and a border of one texel, so that film is checked against
    the ImageBlock::put restatement like the Gaussian one."""
    # radius parameter 0.5: the general restatement
    scene = R.box_scene(WITH_PATH, ("box", [("radius", "float", 0.5)]))
    box = Reference.__new__(Reference)
    box.__dict__.update(with_path.__dict__)
    box.D = R.Desc(scene)
    assert box.D.border == 1 and box.D.filter_values[0] != 1
    film_check(box, render_multi(scene), WITH_PATH[1:])
    # effective radius 0.5: exact
    exact = R.box_scene(WITH_PATH, ("box", [("radius", "float", float(f32(0.5) - f32(1e-5)))]))
    De = R.Desc(exact)
    assert De.filter_radius == 0.5 and De.border == 0 and np.all(De.filter_values[:31] == 1)
    block = render_multi(exact)
    for name in WITH_PATH[1:]:
        v = with_path.got(name)   # the per-sample values of test 2 (they do not depend on the filter)
        acc = np.zeros(v.shape[:2] + (3,), f32)
        for s in range(v.shape[2]):
            acc = (acc + v[:, :, s]).astype(f32)
        np.testing.assert_array_equal(planes(block, WITH_PATH, name), acc)
    np.testing.assert_array_equal(block[..., -1], np.full(block.shape[:2], with_path.params.spp, f32))
    np.testing.assert_array_equal(block[..., -2], (~with_path.miss).sum(-1).astype(f32))


def test_instancing_modes_agree():
    """4. flatten and two-level: primIndex, shapeIndex (-1 on instanced hits)
    and the hit / miss sets equal; distance equal off the instances and to
    1e-5 relative on them; position and normals to 1e-5 (the two modes
    transform in different places; measured on an MI355X: distance 2.6e-7
    relative, position 7.2e-7, shNormal 9.6e-7, geoNormal 1.8e-7); colour as
    tests/test_gpu_instancing.py requires."""
    children = ["path", "distance", "primIndex", "shapeIndex", "position", "shNormal", "geoNormal"]
    out = {}
    for mode in ("flatten", "two-level"):
        s = R.instanced_scene(children, mode)
        g = mtsg.GPUScene(s, 0)
        try:
            out[mode] = (g.render_samples_multi(s.params()), g.render_multi(s.params(), s.border))
        finally:
            g.close()
    a, b = out["flatten"][0], out["two-level"][0]
    for name in ("primIndex", "shapeIndex"):
        np.testing.assert_array_equal(planes(a, children, name), planes(b, children, name))
    np.testing.assert_array_equal(a[..., -1], b[..., -1])
    si = planes(a, children, "shapeIndex")[..., 0]
    hit = a[..., -1] == 1
    # its.t: equal off the instances; on them the flattened scene intersects the
    # world-space triangle and the two-level one the group-space triangle with
    # the transformed ray (instance.cpp:115-130), the same distance in other
    # roundings -- like the position, not bit equality
    da, db = planes(a, children, "distance"), planes(b, children, "distance")
    np.testing.assert_array_equal(da[si != -1], db[si != -1])
    rel = np.abs(da[hit] - db[hit]) / db[hit]
    print(f"flatten vs two-level distance on instanced hits: max relative diff {rel.max():.2e}")
    assert rel.max() <= 1e-5
    # m_shapes: shapegroup 0, floor 1, instances 2 and 3, light 4; instanced hits report -1
    assert set(np.unique(si[hit])) == {-1.0, 1.0} and (si[hit] == -1).mean() > 0.1
    pi = planes(a, children, "primIndex")[..., 0]
    assert set(np.unique(pi[hit & (si == -1)])) <= {0.0, 1.0, 2.0, 3.0} and len(np.unique(pi[hit & (si == -1)])) >= 3
    for name in ("position", "shNormal", "geoNormal"):
        d = np.abs(planes(a, children, name) - planes(b, children, name)).max()
        print(f"flatten vs two-level {name}: max |diff| {d:.2e}")
        assert d <= 1e-5, (name, d)
    fa, fb = out["flatten"][1], out["two-level"][1]
    check_render(np.concatenate([fa[..., :3], fa[..., -2:]], -1), np.concatenate([fb[..., :3], fb[..., -2:]], -1))


def test_splits_sum_to_the_whole_block(with_path):
    """5. Tile shares and small batches against the single-batch block, under
    the comparison tests/test_gpu_c4.py uses for the colour film."""
    s, whole = with_path.scene, with_path.block
    g = mtsg.GPUScene(s, 0)
    try:
        acc = sum(g.render_multi(s.params(tile_stride=2, tile_offset=r), s.border) for r in range(2))
        np.testing.assert_allclose(acc, whole, rtol=2e-5, atol=2e-6)
        g.set_batch_paths(512)   # one tile x two samples per batch: 6 tile batches x 2 sample batches
        np.testing.assert_allclose(g.render_multi(s.params(), s.border), whole, rtol=2e-5, atol=2e-6)
    finally:
        g.close()


def test_fields_only_stops_after_the_first_trace(with_path, fields_only):
    """6. No `path` child: the planes of tests 2 and 3, one closest launch per
    batch, no shading."""
    b = with_path.scene.border
    for name in ("distance", "shNormal", "uv", "albedo", "position"):
        np.testing.assert_array_equal(fields_only.got(name), with_path.got(name))
        assert_same_film(planes(fields_only.block, FIELDS_ONLY, name), planes(with_path.block, WITH_PATH, name), b)
    np.testing.assert_array_equal(fields_only.samples[..., -1], with_path.samples[..., -1])
    assert_same_film(fields_only.block[..., -2:], with_path.block[..., -2:], b)
    s = fields_only.scene
    g = mtsg.GPUScene(s, 0)
    try:
        g.set_flags(mtsg.MTSG_FLAG_TIMING)
        g.render_multi(s.params(), s.border)
        st = g.stats()
        assert st.launches_trace_closest == 1 and st.launches_trace_shadow == 0 and st.launches_finish == 0
        assert st.rays_closest == st.samples == R.FILM_W * R.FILM_H * R.SPP and st.rays_shadow == 0
        assert st.ms_shade == 0 and st.ms_finish == 0 and st.ms_trace_closest > 0 and st.ms_splat > 0
        g.set_batch_paths(512)
        g.render_multi(s.params(), s.border)
        st = g.stats()
        assert st.launches_trace_closest == 12 and st.rays_closest == st.samples and st.ms_shade == 0
    finally:
        g.close()


def test_entry_points(with_path):
    """7. The path job renders the multichannel block; the single-film entries
    refuse a handle with fields active; set_aov(None) restores the plain render."""
    s = with_path.scene
    job = mtsg.PathJob(s, 1)
    try:
        rc, block, _ = job.render_multi(s.params(), s.border)
        assert rc == 0, job.last_error()
        assert_same_film(block, with_path.block, s.border)
        rc, _, _ = job.render(s.params(), s.border)
        assert rc == -1 and "multichannel" in job.last_error()
    finally:
        job.close()
    plain_scene = R.box_scene(None, pixel_format="rgb")
    fresh = render_plain(plain_scene)
    g = mtsg.GPUScene(s, 0)
    try:
        with pytest.raises(RuntimeError, match=r"\(-1\).*multichannel"):
            g.render(s.params(), s.border)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            g.render_samples(s.params())
        g.set_aov(None)
        with pytest.raises(RuntimeError):
            g.render_multi(s.params(), s.border)
        np.testing.assert_array_equal(g.render_samples(s.params()), render_plain_samples(plain_scene))
        assert_same_film(g.render(s.params(), s.border), fresh, s.border)
    finally:
        g.close()
    # a plain handle has no multichannel entry
    g = mtsg.GPUScene(plain_scene, 0)
    try:
        out = np.zeros(8, f32)
        assert mtsg.device_lib().mtsg_render_multi(g._h, C.byref(plain_scene.params()), mtsg._ptr(out)) == -1
    finally:
        g.close()
