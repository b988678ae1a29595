"""Per-sample restatement of `direct` (direct.cpp:146-306) over the diffuse
test box with one object of a phong / ward / roughdiffuse / difftrans /
thindielectric BSDF in it, for tests/test_gpu_bsdfs.py.

Built as direct_ref.emitters_only_reference is, from oracle pieces that do not
know these BSDFs: the oracle's camera rays, closest hits and shadow rays
(direct_ref.Primary over the same geometry), the counter RNG's draws, the
intersection record of multichannel_ref, and the numpy BSDFs of bsdf_ref (the
box's own diffuse records are restated here too: diffuse.cpp:107-150).  The
box has one rectangle light, so Scene::sampleEmitterDirect picks it with
probability 1 and leaves the sample's first coordinate as it is.  Every
operation is float32 in the reference's order; Spectrum / Float multiplies by
the reciprocal (spectrum.h:447-456)."""
import ctypes as C
import functools

import numpy as np

import direct_ref as DR
import multichannel_ref as R
import bsdf_ref as BR
from oracle import pyoracle as O
from direct_ref import EPS, SHADOW_EPS, _v, counter_float

f32 = np.float32
DIFFUSE = 1


def geometry(add_object):
    """direct_ref.box_geometry's diffuse box with its rectangle light, then add_object(builder)."""
    saved = DR.box_geometry

    def build(b, diffuse_only=False, mesh_light=True):
        saved(b, diffuse_only=True, mesh_light=False)
        add_object(b)
    return saved, build


def primary(spp, add_object):
    """direct_ref.Primary over the box with the object."""
    saved, build = geometry(add_object)
    DR.box_geometry = build
    try:
        return DR.Primary(spp)
    finally:
        DR.box_geometry = saved


def scene(add_object, ne, nb, spp=4):
    import mtsg
    from conftest import SCENES
    saved, build = geometry(add_object)
    b = mtsg.SceneBuilder(SCENES)
    b.integrator("direct", [("emitterSamples", "integer", ne), ("bsdfSamples", "integer", nb)])
    DR.box_props(b, spp=spp)
    build(b)
    return b.finish()


def _mis(a, b):   # miWeight (direct.cpp:309-313)
    with np.errstate(all="ignore"):
        a, b = (a * a).astype(f32), (b * b).astype(f32)
        return (a / (a + b)).astype(f32)


def _record(rec):
    return BR.Record(rec.type, reflectance=list(rec.reflectance), spec_refl=list(rec.spec_refl), spec_trans=list(rec.spec_trans),
                     alpha_u=rec.alpha_u, alpha_v=rec.alpha_v, distribution=rec.distribution, nonlinear=rec.nonlinear,
                     ior_eta=rec.ior_eta, spec_sampling_weight=rec.spec_sampling_weight, smooth=rec.smooth, ref_n_zero=rec.ref_n_zero)


class Bsdfs:
    """eval / sample over samples that hit different records."""

    def __init__(self, P):
        self.recs = P.D.bsdfs
        self.idx = P.bsdf
        self.kinds = sorted(set(int(k) for k in self.idx[self.idx >= 0]))
        n = len(self.idx)
        self.alb = np.zeros((n, 3), f32)
        self.smooth = np.zeros(n, bool)
        self.ref_n_zero = np.zeros(n, bool)
        for k in self.kinds:
            on = self.idx == k
            self.alb[on] = np.array(list(self.recs[k].reflectance), f32)
            self.smooth[on] = bool(self.recs[k].smooth)
            self.ref_n_zero[on] = bool(self.recs[k].ref_n_zero)

    def evaluate(self, wi, wo, active):
        n = len(wi)
        val, pdf = np.zeros((n, 3), f32), np.zeros(n, f32)
        for k in self.kinds:
            on = active & (self.idx == k)
            if not on.any():
                continue
            rec = self.recs[k]
            if rec.type == DIFFUSE:   # diffuse.cpp:107-126
                ok = (wi[on, 2] > 0) & (wo[on, 2] > 0) & bool(rec.smooth)
                p = np.where(ok, BR.INV_PI * wo[on, 2], f32(0)).astype(f32)
                val[on], pdf[on] = (self.alb[on] * p[:, None]).astype(f32), p
            else:
                val[on], pdf[on] = BR.evaluate(_record(rec), wi[on], wo[on], alb=self.alb[on])
        return val, pdf

    def sample(self, wi, u, active):
        """(wo, weight, pdf, delta, ok)"""
        n = len(wi)
        wo, w = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
        wo[:, 2] = 1
        pdf, delta, ok = np.zeros(n, f32), np.zeros(n, bool), np.zeros(n, bool)
        for k in self.kinds:
            on = active & (self.idx == k)
            if not on.any():
                continue
            rec = self.recs[k]
            if rec.type == DIFFUSE:   # diffuse.cpp:139-150
                d = BR.cosine_hemisphere(BR.Math(True), u[on, 0], u[on, 1])
                good = (wi[on, 2] > 0) & (self.alb[on] != 0).any(1)
                wo[on], w[on], pdf[on], ok[on] = d, self.alb[on], (BR.INV_PI * d[:, 2]).astype(f32), good
            else:
                a, b, c, _eta, fl = BR.sample(_record(rec), wi[on], u[on], alb=self.alb[on])
                wo[on], w[on], pdf[on], ok[on], delta[on] = a, b, c, fl != 0, (fl & BR.DELTA) != 0
        return wo, w, pdf, delta, ok & active


def direct_reference(P, ne, nb):
    """(Li (samples, 3), sum of |terms|, fragile) of `direct` with emitterSamples ne and bsdfSamples nb."""
    D = P.D
    S = len(P.key)
    em_shape = int(np.nonzero(D.shapes[:, 2] >= 0)[0][0])
    assert (D.shapes[:, 2] >= 0).sum() == 1 and D.shapes[em_shape, 0] == 1   # one emitter, a rectangle
    rect_index = int(D.shapes[em_shape, 6])
    rect = D.rects[rect_index]
    M = rect[12:24].reshape(3, 4)
    en, inv_area = rect[30:33], rect[39]
    sd = C.cast(P.scene.desc, C.POINTER(R.SceneDesc)).contents
    radiance = np.frombuffer((C.c_char * 12).from_address(sd.emitters + 16), f32).copy()
    B = Bsdfs(P)
    Li = np.zeros((S, 3), f32)
    facing = (P.emitter >= 0) & (R._dot(P.n, (-P.rd).astype(f32)) > 0)
    Li[facing] = radiance
    mag = np.abs(Li).copy()
    fragile = np.zeros(S, bool)
    wi = P.to_local((-P.rd).astype(f32))
    refN = np.where(B.ref_n_zero[:, None], f32(0), P.n).astype(f32)
    total = f32(ne + nb)
    frac_lum, frac_bsdf = f32(ne) / total, f32(nb) / total          # direct.cpp:100-102
    weight_lum, weight_bsdf = f32(1) / f32(max(ne, 1)), f32(1) / f32(max(nb, 1))
    den = np.broadcast_to(en, (S, 3)).astype(f32)
    # ---- emitter sampling (direct.cpp:210-245)
    u = P.draws(ne)
    for i in range(ne):
        x = (u[:, i, 0] * f32(2) - f32(1)).astype(f32)
        y = (u[:, i, 1] * f32(2) - f32(1)).astype(f32)
        ep = np.stack([((M[k, 0] * x).astype(f32) + (M[k, 1] * y).astype(f32)).astype(f32) + M[k, 3] for k in range(3)], 1).astype(f32)
        dd = (ep - P.p).astype(f32)
        d2 = R._dot(dd, dd)
        with np.errstate(all="ignore"):
            dist = np.sqrt(d2).astype(f32)
            dd = (dd * (f32(1) / dist)[:, None]).astype(f32)
            cos_e = R._dot(dd, den)
            dp = np.abs(cos_e)
            pdf = (inv_area * np.where(dp != 0, (d2 / dp).astype(f32), f32(0))).astype(f32)
            ok = P.hit & B.smooth & (R._dot(dd, refN) >= 0) & (cos_e < 0) & (pdf != 0)
            value = (radiance[None, :] * (f32(1) / pdf)[:, None]).astype(f32)
        wo = P.to_local(dd)
        bval, bpdf = B.evaluate(wi, wo, ok)
        ok &= (bval != 0).any(1)
        weight = (_mis((pdf * frac_lum).astype(f32), (bpdf * frac_bsdf).astype(f32)) * weight_lum).astype(f32)
        term = ((value * bval).astype(f32) * weight[:, None]).astype(f32)
        ok &= (term != 0).any(1)
        occ, fr = P.shadow(P.p, dd, np.full(S, EPS), (dist * (f32(1) - SHADOW_EPS)).astype(f32), ok)
        add = ok & ~occ
        Li[add] = (Li[add] + term[add]).astype(f32)
        mag[ok] += np.abs(term[ok])
        fragile |= fr
    # ---- BSDF sampling (direct.cpp:251-306)
    if nb == 1:
        d0 = 4 if ne <= 1 else 2   # the regular draw after the emitter technique's
        ub = np.stack([counter_float(P.key, d0), counter_float(P.key, d0 + 1)], -1)[:, None, :]
    else:
        ub = P.draws(nb, request=1 if ne > 1 else 0)
    for j in range(nb):
        wo, bw, bpdf, delta, ok = B.sample(wi, ub[:, j], P.hit)
        d = P.to_world(wo)
        rays = np.concatenate([P.p, d, np.full((S, 1), EPS), np.full((S, 1), np.inf, f32)], 1).astype(f32)
        rays[~ok] = (0, 0, 0, 0, 0, 1, 0, 0)
        t, _u, _v2, prim = O.trace_closest(P.scene.desc, np.ascontiguousarray(rays))
        on = ok & (prim == np.uint32(0x80000000 | rect_index))
        with np.errstate(all="ignore"):
            cos_l = R._dot(d, den)
            value = np.where((-cos_l > 0)[:, None], radiance[None, :], f32(0)).astype(f32)
            lum = np.where((R._dot(d, refN) >= 0) & (cos_l < 0), (inv_area * (t * t).astype(f32)).astype(f32) / np.abs(cos_l), f32(0))
            lum = np.where(delta, f32(0), lum).astype(f32)
            weight = (_mis((bpdf * frac_bsdf).astype(f32), (lum * frac_lum).astype(f32)) * weight_bsdf).astype(f32)
        term = ((value * bw).astype(f32) * weight[:, None]).astype(f32)
        Li[on] = (Li[on] + term[on]).astype(f32)
        mag[on] += np.abs(term[on])
    return Li, mag, fragile
