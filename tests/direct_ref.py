"""Helpers of the `direct` / `ao` tests: the test scenes (built with
SceneBuilder on the model of multichannel_ref.box_scene) and the comparisons
the GPU tests share."""
import numpy as np

import mtsg
from conftest import SCENES
from multichannel_ref import grid_mesh, xf

f32 = np.float32
FILM_W, FILM_H = 40, 24   # not a multiple of the 16-pixel tile


def box_props(b, sampler="independent", spp=4, pixel_format="rgba", sampler_props=(), film_props=()):
    b.sensor("perspective", [("fov", "float", 40.0),
                             ("toWorld", "transform", xf([(-1, 0, 0), (0, 1, 0), (0, 0, -1)], (0.05, 0.1, 3.6)))])
    b.film("hdrfilm", [("width", "integer", FILM_W), ("height", "integer", FILM_H), ("pixelFormat", "string", pixel_format)] + list(film_props),
           "gaussian", [])
    b.sampler(sampler, [("sampleCount", "integer", spp)] + list(sampler_props))


def box_geometry(b, diffuse_only=False, mesh_light=True):
    """The box of multichannel_ref.box_scene with smooth BSDFs only: a bumpy
    floor with vertex normals, a left wall with face normals, rectangles, a
    rough metal cube, a rectangle light and a two-triangle mesh light.  The
    right quarter of the back is open: those camera rays miss."""
    wall = b.bsdf("diffuse", [("reflectance", "spectrum", (0.7, 0.65, 0.6))])
    floor = b.bsdf("diffuse", [("reflectance", "spectrum", (0.5, 0.6, 0.4))])
    red = b.bsdf("diffuse", [("reflectance", "spectrum", (0.8, 0.1, 0.1))])
    if diffuse_only:
        rplastic = metal = wall
    else:
        rplastic = b.bsdf("roughplastic", [("diffuseReflectance", "spectrum", (0.6, 0.3, 0.2)), ("alpha", "float", 0.2),
                                           ("intIOR", "float", 1.5), ("extIOR", "float", 1.0)])
        metal = b.bsdf("roughconductor", [("alpha", "float", 0.3)])
    light = b.emitter("area", [("radiance", "spectrum", (15.0, 14.0, 12.0))])
    fp, fuv, ft = grid_mesh((-1.2, -0.5, 1.2), (0.6, 0, 0), (0, 0, -0.55), 4, lambda i, j: 0.08 * np.sin(1.3 * i) * np.cos(0.9 * j),
                            (0, 1, 0))
    fn = np.zeros_like(fp)
    for k, (i, j) in enumerate((i, j) for j in range(5) for i in range(5)):
        dx = 0.08 * 1.3 * np.cos(1.3 * i) * np.cos(0.9 * j) / 0.6
        dz = -0.08 * 0.9 * np.sin(1.3 * i) * np.sin(0.9 * j) / -0.55
        n = np.array([-dx, 1.0, -dz])
        fn[k] = n / np.linalg.norm(n)
    b.mesh(fp, ft, normals=fn, texcoords=fuv, bsdf=floor, name="floor")
    lp, _luv, lt = grid_mesh((-1.2, -1.0, 1.2), (0, 0, -0.75), (0, 0.7, 0), 3, lambda i, j: 0.05 * ((i * 2 + j) % 3), (1, 0, 0))
    b.mesh(lp, lt, face_normals=True, bsdf=red, name="left")
    b.shape("rectangle", [("toWorld", "transform", xf([(0, 0, 1.1), (0, 1, 0), (-1, 0, 0)], (1.2, 0, 0.1)))], rplastic)
    b.shape("rectangle", [("toWorld", "transform", xf([(0.9, 0, 0), (0, 1, 0), (0, 0, 1)], (-0.3, 0, -1.0)))], wall)
    b.shape("cube", [("toWorld", "transform", xf([(0.25, 0, 0), (0, 0.25, 0), (0, 0, 0.25)], (0.45, -0.2, 0.2)))], metal)
    b.shape("rectangle", [("toWorld", "transform", xf([(0.4, 0, 0), (0, 0, 0.4), (0, -1, 0)], (0, 0.99, 0)))], -1, light)
    if mesh_light:
        light2 = b.emitter("area", [("radiance", "spectrum", (6.0, 8.0, 10.0))])
        pos = np.array([(-1.1, 0.6, -0.3), (-1.1, 0.6, 0.3), (-1.1, 0.9, 0.3), (-1.1, 0.9, -0.3)], f32)
        b.mesh(pos, np.array([(0, 2, 1), (0, 3, 2)], np.uint32), face_normals=True, bsdf=wall, emitter=light2, name="panel")


def box_scene(integrator="path", props=(("maxDepth", "integer", 2),), **kw):
    geo = {k: kw.pop(k) for k in ("diffuse_only", "mesh_light") if k in kw}
    b = mtsg.SceneBuilder(SCENES)
    b.integrator(integrator, list(props))
    box_props(b, **kw)
    box_geometry(b, **geo)
    return b.finish()


def direct_desc(ne=0, nb=0, ao=0, length=0.0):
    return mtsg.DirectDesc(ne, nb, ao, length)


def region_masks(h, w):
    """Six film regions: a 3 x 2 grid."""
    ys, xs = np.mgrid[0:h, 0:w]
    return [(ys * 2 // h == j) & (xs * 3 // w == i) for j in range(2) for i in range(3)]


def assert_same_mean(a, b, what):
    """Per-sample values a, b (h, w, spp, 3) of two unbiased estimators of one
    image: the channel means over the film and over six regions agree within
    5 standard errors, the variances taken from the samples themselves."""
    h, w = a.shape[:2]
    for name, m in [("film", np.ones((h, w), bool))] + [(f"region {k}", m) for k, m in enumerate(region_masks(h, w))]:
        for c in range(3):
            x, y = a[m][..., c].astype(np.float64).ravel(), b[m][..., c].astype(np.float64).ravel()
            bound = 5 * np.sqrt(x.var() / x.size + y.var() / y.size)
            assert abs(x.mean() - y.mean()) <= bound, (what, name, c, x.mean(), y.mean(), bound)


# ---------------------------------------------------------------------------
# Per-sample restatements from oracle pieces (CPU only): the oracle's camera
# rays, closest hits, BSDF functions and shadow rays, the reference's
# intersection record in float32 numpy (multichannel_ref), and the counter
# RNG's draws.  Sample i is ((y * FILM_W + x) * spp + s), the order of
# mtsg_render_samples.
# ---------------------------------------------------------------------------
import ctypes as C
import functools

from oracle import pyoracle as O
import multichannel_ref as R
import test_bsdf_chisquare as B

U64 = np.uint64
EPS = f32(1e-4)            # Epsilon (constants.h:28)
SHADOW_EPS = f32(1e-3)     # ShadowEpsilon


def _mix64(x):
    with np.errstate(over="ignore"):
        x = x.astype(U64)
        x = x ^ (x >> U64(30))
        x = x * U64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> U64(27))
        x = x * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def counter_key(seed, sample_id):
    with np.errstate(over="ignore"):
        return _mix64(np.asarray(sample_id, U64) * U64(0x9E3779B97F4A7C15) + U64(seed))


def counter_float(key, dim):
    """DESIGN "Random numbers": draw `dim` of the sample with this key."""
    with np.errstate(over="ignore"):
        u = (_mix64(key + U64(dim + 1) * U64(0xD1B54A32D192ED03)) >> U64(32)).astype(np.uint32)
    return (((u >> np.uint32(9)) | np.uint32(0x3F800000)).view(f32) - f32(1)).astype(f32)


def _v(a, b):   # componentwise product of (n, 3) by (n,), float32
    return (a * b[:, None]).astype(f32)


class Primary:
    """The camera samples of the box (independent sampler, seed 0): the
    oracle's camera rays and closest hits and, for each hit, its.p, the
    geometric normal and the shading frame of computeShadingFrame
    (util.cpp:603-608), the BSDF record and the emitter."""

    def __init__(self, spp, diffuse_only=False, mesh_light=True):
        b = mtsg.SceneBuilder(SCENES)
        b.integrator_child("field", [("field", "string", "position")])
        b.multichannel()
        box_props(b, spp=spp, pixel_format="rgb")
        box_geometry(b, diffuse_only=diffuse_only, mesh_light=mesh_light)
        self.scene = sc = b.finish()
        self.D = D = R.Desc(sc)
        self.spp = spp
        p = sc.params()
        L = O.lib()
        L.oracle_debug_path_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        n = FILM_H * FILM_W * spp
        rays = np.zeros((n, 8), f32)
        one = np.zeros(8, f32)
        i = 0
        for y in range(FILM_H):
            for x in range(FILM_W):
                for s in range(spp):
                    assert L.oracle_debug_path_rays(sc.desc, C.byref(p), x, y, s, O._p(one), 1) == 1
                    rays[i] = one
                    i += 1
        self.rays = rays
        t, u, v, prim = O.trace_closest(sc.desc, rays)
        fields, miss = R.expected_fields(D, sc.aov(), rays, t, u, v, prim, lambda tex, uv: O.tex_eval(sc.desc, tex, uv))
        self.miss, self.hit = miss, ~miss
        self.p, self.n, self.gn = fields["position"], fields["shNormal"], fields["geoNormal"]
        self.rd = rays[:, 3:6].astype(f32)
        sd = C.cast(sc.desc, C.POINTER(R.SceneDesc)).contents
        tri_dpdu = R._arr(sd.dpdu, f32, (sd.ntri, 3))
        tri = self.hit & (prim < 0x80000000)
        rec = self.hit & (prim >= 0x80000000)
        ri = (prim & 0x7FFFFFFF).astype(np.int64)
        dpdu = np.zeros((n, 3), f32)
        shape = np.zeros(n, np.int64)
        dpdu[tri] = tri_dpdu[prim[tri].astype(np.int64)]
        shape[tri] = D.tri_shape[prim[tri].astype(np.int64)]
        dpdu[rec] = D.rects[ri[rec], 33:36]
        shape[rec] = D.rect_shape[ri[rec]]
        self.bsdf = np.where(self.hit, D.shapes[shape, 1], -1)
        self.emitter = np.where(self.hit, D.shapes[shape, 2], -1)
        # computeShadingFrame: s = normalize(dpdu - n dot(n, dpdu)), t = cross(n, s)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.s = R._normalize((dpdu - _v(self.n, R._dot(self.n, dpdu))).astype(f32))
            self.t = R._cross(self.n, self.s)
        ids = np.arange(n, dtype=U64)
        self.key = counter_key(0, ids)
        # the restated draws are the oracle's: the pixel jitter and the next regular 2D draw of a few samples
        for i in (0, n // 3, n - 1):
            x, y, s = (i // spp) % FILM_W, i // spp // FILM_W, i % spp
            want = O.sampler_draws(sc.desc, p, x, y, s, [2, 2])
            got = np.array([counter_float(self.key[i:i + 1], d)[0] for d in range(4)], f32)
            assert (got.view(np.uint32) == want.view(np.uint32)).all()

    def draws(self, n, request=0):
        """The 2D numbers of a technique with n samples, (samples, n, 2): the
        regular draw after the jitter, or array `request` (sampler.h smp_array2D)."""
        if n <= 1:
            return np.stack([counter_float(self.key, 2), counter_float(self.key, 3)], -1)[:, None, :]
        base = 0x80000000 | (request << 24)
        return np.stack([np.stack([counter_float(self.key, base | (2 * k)), counter_float(self.key, base | (2 * k + 1))], -1)
                         for k in range(n)], 1)

    def to_world(self, v):
        return ((_v(self.s, v[:, 0]) + _v(self.t, v[:, 1])).astype(f32) + _v(self.n, v[:, 2])).astype(f32)

    def to_local(self, v):
        return np.stack([R._dot(v, self.s), R._dot(v, self.t), R._dot(v, self.n)], 1).astype(f32)

    def shadow(self, o, d, mint, maxt, active):
        """Per ray: occluded (oracle.trace_shadow), and whether that answer
        changes when one direction component moves by 4 ulps either way."""
        def trace(dd):
            rays = np.concatenate([o, dd, mint[:, None], maxt[:, None]], 1).astype(f32)
            rays[~active] = (0, 0, 0, 0, 0, 1, 0, 0)
            return O.trace_shadow(self.scene.desc, np.ascontiguousarray(rays)).astype(bool)
        occ = trace(d)
        fragile = np.zeros(len(d), bool)
        for c in range(3):
            for step in (4, -4):
                q = d.copy()
                q[:, c] = (q[:, c].view(np.int32) + np.int32(step)).view(f32)
                fragile |= trace(q) != occ
        return occ & active, fragile & active


@functools.lru_cache(maxsize=None)
def primary(spp, diffuse_only=False, mesh_light=True):
    return Primary(spp, diffuse_only, mesh_light)


def ao_reference(P, n, length):
    """ao.cpp:84-125 per sample: (value, fragile)."""
    S = len(P.key)
    u = P.draws(n).reshape(-1, 2)
    # squareToCosineHemisphere, as the diffuse BSDF samples it (diffuse.cpp)
    wo = B.sample(B.make_bsdf(B.DIFFUSE), np.array([0, 0, 1], f32), u)[0].reshape(S, n, 3)
    count = np.zeros(S, f32)
    fragile = np.zeros(S, bool)
    for k in range(n):
        d = P.to_world(wo[:, k])
        occ, fr = P.shadow(P.p, d, np.full(S, EPS), np.full(S, f32(length)), P.hit)
        count = (count + np.where(P.hit & ~occ, f32(1), f32(0))).astype(f32)
        fragile |= fr
    value = (count * (f32(1) / f32(n))).astype(f32)
    return np.where(P.miss, f32(1), value), fragile


def emitters_only_reference(P, ne):
    """direct.cpp:146-245 per sample with bsdfSamples = 0 on the diffuse box
    with its one rectangle light: (Li, sum of |terms|, fragile)."""
    D = P.D
    S = len(P.key)
    em_shape = int(np.nonzero(D.shapes[:, 2] >= 0)[0][0])
    assert (D.shapes[:, 2] >= 0).sum() == 1 and D.shapes[em_shape, 0] == 1   # one emitter, a rectangle
    rect = D.rects[D.shapes[em_shape, 6]]
    M = rect[12:24].reshape(3, 4)
    en, inv_area = rect[30:33], rect[39]
    sd = C.cast(P.scene.desc, C.POINTER(R.SceneDesc)).contents
    radiance = np.frombuffer((C.c_char * 12).from_address(sd.emitters + 16), f32).copy()   # mtsg_emitter: type, shape, cdf_offset, pdf_discrete, radiance[3]
    Li = np.zeros((S, 3), f32)
    facing = (P.emitter >= 0) & (R._dot(P.n, (-P.rd).astype(f32)) > 0)
    Li[facing] = radiance
    mag = np.zeros((S, 3), f32)
    fragile = np.zeros(S, bool)
    wi = P.to_local((-P.rd).astype(f32))
    u = P.draws(ne)
    weight = f32(1) / f32(ne)   # miWeight(pdf fracLum, 0) = 1, times weightLum
    for i in range(ne):
        x = (u[:, i, 0] * f32(2) - f32(1)).astype(f32)
        y = (u[:, i, 1] * f32(2) - f32(1)).astype(f32)
        ep = np.stack([((M[k, 0] * x).astype(f32) + (M[k, 1] * y).astype(f32)).astype(f32) + M[k, 3] for k in range(3)], 1).astype(f32)
        dd = (ep - P.p).astype(f32)
        d2 = R._dot(dd, dd)
        with np.errstate(invalid="ignore", divide="ignore"):
            dist = np.sqrt(d2).astype(f32)
            dd = (dd / dist[:, None]).astype(f32)
            den = np.broadcast_to(en, dd.shape).astype(f32)
            cos_e = R._dot(dd, den)
            dp = np.abs(cos_e)
            pdf = (inv_area * np.where(dp != 0, (d2 / dp).astype(f32), f32(0))).astype(f32)
            ok = P.hit & (R._dot(dd, P.n) >= 0) & (cos_e < 0) & (pdf != 0)
            value = (radiance[None, :] / pdf[:, None]).astype(f32)
        wo = P.to_local(dd)
        bval = np.zeros((S, 3), f32)
        for j in np.nonzero(ok)[0]:
            bval[j] = B.evaluate(D.bsdfs[P.bsdf[j]], wi[j], wo[j:j + 1])[0][0]
        term = ((value * bval).astype(f32) * weight).astype(f32)
        ok &= (bval != 0).any(1) & (term != 0).any(1)
        maxt = (dist * (f32(1) - SHADOW_EPS)).astype(f32)
        occ, fr = P.shadow(P.p, dd, np.full(S, EPS), maxt, ok)
        add = ok & ~occ
        Li[add] = (Li[add] + term[add]).astype(f32)
        mag[ok] += np.abs(term[ok])
        fragile |= fr
    return Li, mag, fragile
