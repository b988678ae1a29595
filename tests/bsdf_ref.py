"""float32 numpy restatement of the phong, ward, roughdiffuse, difftrans and
thindielectric plugins: sample(bRec, pdf, sample), eval and pdf (ESolidAngle,
ERadiance, every component), and the values their configure() derives.

  phong           src/bsdfs/phong.cpp:60-240
  ward            src/bsdfs/ward.cpp:97-326
  roughdiffuse    src/bsdfs/roughdiffuse.cpp:88-251
  difftrans       src/bsdfs/difftrans.cpp:49-116
  thindielectric  src/bsdfs/thindielectric.cpp:73-232
  ensureEnergyConservation  src/librender/bsdf.cpp:88-146

Every operation is a float32 numpy operation in the reference's order (the
single-precision build's M_PI is a float, constants.h).  Where the reference
calls libm the restatement calls the C library's function per element
(`exact=True`, the default; emitter_ref does the same); `exact=False` takes
numpy's vectorised functions instead, which may differ by an ulp: the
chi-square tests draw 200k samples and do not need the last bit.
std::pow(Float, int) (ward.cpp:206,245) is the double function in C++11, so
those two factors are evaluated in double, as the compiled reference does.
math::fastexp / fastlog are the double functions rounded to float
(math.h:185-199).  Spectrum / Float and Vector / Float multiply by the
reciprocal (spectrum.h:447-456, vector.h)."""
import ctypes as C
import math

import numpy as np

f32 = np.float32
PHONG, WARD, ROUGHDIFFUSE, DIFFTRANS, THINDIELECTRIC = 8, 9, 10, 11, 12
WARD_WARD, WARD_DUER, WARD_BALANCED = 0, 1, 2
OK, DELTA, NULL = 1, 2, 4   # MTSG_BSDF_QUERY_*
PI = f32(3.14159265358979323846)
INV_PI = f32(0.31830988618379067154)
INV_TWOPI = f32(0.15915494309189533577)
EPS = f32(1e-4)

_libm = C.CDLL("libm.so.6")
for _n in ("sinf", "cosf", "tanf", "atanf", "acosf"):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float]
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]


class Math:
    """The transcendental functions, per element through libm or vectorised."""

    def __init__(self, exact=True):
        self.exact = exact

    def _un(self, name, x, np_fn):
        x = np.asarray(x, f32)
        if not self.exact:
            with np.errstate(all="ignore"):
                return np_fn(x).astype(f32)
        fn = getattr(_libm, name)
        return np.array([fn(float(v)) for v in x.ravel()], f32).reshape(x.shape)

    def sin(self, x): return self._un("sinf", x, np.sin)
    def cos(self, x): return self._un("cosf", x, np.cos)
    def tan(self, x): return self._un("tanf", x, np.tan)
    def atan(self, x): return self._un("atanf", x, np.arctan)
    def acos(self, x): return self._un("acosf", x, np.arccos)

    def pow(self, x, y):
        x, y = np.broadcast_arrays(np.asarray(x, f32), np.asarray(y, f32))
        if not self.exact:
            with np.errstate(all="ignore"):
                return np.power(x, y).astype(f32)
        return np.array([_libm.powf(float(a), float(b)) for a, b in zip(x.ravel(), y.ravel())], f32).reshape(x.shape)

    def fastexp(self, x):   # (float) exp((double) x)
        x = np.asarray(x, f32)
        if not self.exact:
            with np.errstate(all="ignore"):
                return np.exp(x.astype(np.float64)).astype(f32)
        out = []
        for v in x.ravel():
            try:
                out.append(math.exp(float(v)))
            except OverflowError:
                out.append(math.inf)
        with np.errstate(over="ignore"):
            return np.array(out, np.float64).astype(f32).reshape(x.shape)

    def fastlog(self, x):   # (float) log((double) x)
        x = np.asarray(x, f32)
        with np.errstate(all="ignore"):
            if not self.exact:
                return np.log(x.astype(np.float64)).astype(f32)
            return np.array([math.log(float(v)) if v > 0 else (-math.inf if v == 0 else math.nan) for v in x.ravel()],
                            np.float64).astype(f32).reshape(x.shape)

    def powd(self, x, k):   # std::pow(Float, int): double
        x = np.asarray(x, f32).astype(np.float64)
        if not self.exact:
            return np.power(x, float(k))
        return np.array([math.pow(float(v), float(k)) for v in x.ravel()], np.float64).reshape(x.shape)


# ---------------------------------------------------------------------------
# configure(): the record a plugin's properties give
# ---------------------------------------------------------------------------
def luminance(v):   # spectrum.h:638-640
    v = np.asarray(v, f32)
    return f32(v[0] * f32(0.212671) + v[1] * f32(0.715160) + v[2] * f32(0.072169))


def conserve(v):
    """ensureEnergyConservation(texture, name, 1) of a constant."""
    v = np.asarray(v, f32)
    mx = v.max()
    return v * f32(f32(0.99) * (f32(1.0) / mx)) if mx > 1 else v


def conserve_pair(spec, diff):
    """The pair form: both scaled by 0.99 / max(spec + diff) when that exceeds 1."""
    spec, diff = np.asarray(spec, f32), np.asarray(diff, f32)
    mx = (spec + diff).max()
    if mx > 1:
        s = f32(f32(0.99) * (f32(1.0) / mx))
        return spec * s, diff * s
    return spec, diff


class Record:
    """The fields of mtsg_bsdf the five models read."""

    def __init__(self, type, reflectance=(0, 0, 0), spec_refl=(0, 0, 0), spec_trans=(0, 0, 0), alpha_u=0.0, alpha_v=0.0,
                 distribution=0, nonlinear=0, ior_eta=0.0, spec_sampling_weight=0.0, smooth=1, ref_n_zero=0):
        self.type = type
        self.reflectance = np.asarray(reflectance, f32)
        self.spec_refl = np.asarray(spec_refl, f32)
        self.spec_trans = np.asarray(spec_trans, f32)
        self.alpha_u, self.alpha_v = f32(alpha_u), f32(alpha_v)
        self.distribution, self.nonlinear = distribution, nonlinear
        self.ior_eta = f32(ior_eta)
        self.ior_inv_eta = f32(f32(1) / f32(ior_eta)) if ior_eta else f32(0)
        self.spec_sampling_weight = f32(spec_sampling_weight)
        self.smooth, self.ref_n_zero = smooth, ref_n_zero


def _glossy(type, diffuse, specular, **kw):
    sr, dr = conserve_pair(np.full(3, specular, f32) if np.isscalar(specular) else specular,
                           np.full(3, diffuse, f32) if np.isscalar(diffuse) else diffuse)
    d, s = luminance(dr), luminance(sr)
    return Record(type, reflectance=dr, spec_refl=sr, spec_sampling_weight=f32(s / f32(d + s)), **kw)


def phong(diffuseReflectance=0.5, specularReflectance=0.2, exponent=30.0):
    return _glossy(PHONG, diffuseReflectance, specularReflectance, alpha_u=exponent)


def ward(variant="balanced", diffuseReflectance=0.5, specularReflectance=0.2, alpha=0.1, alphaU=None, alphaV=None):
    v = {"ward": WARD_WARD, "ward-duer": WARD_DUER, "balanced": WARD_BALANCED}[variant]
    return _glossy(WARD, diffuseReflectance, specularReflectance, distribution=v,
                   alpha_u=alpha if alphaU is None else alphaU, alpha_v=alpha if alphaV is None else alphaV)


def _spec(v):
    return np.full(3, v, f32) if np.isscalar(v) else np.asarray(v, f32)


def roughdiffuse(reflectance=0.5, alpha=0.2, useFastApprox=False):
    return Record(ROUGHDIFFUSE, reflectance=conserve(_spec(reflectance)), alpha_u=alpha, nonlinear=1 if useFastApprox else 0)


def difftrans(transmittance=0.5):
    return Record(DIFFTRANS, reflectance=conserve(_spec(transmittance)), ref_n_zero=1)


def thindielectric(intIOR=1.5046, extIOR=1.000277, specularReflectance=1.0, specularTransmittance=1.0):
    return Record(THINDIELECTRIC, spec_refl=conserve(_spec(specularReflectance)), spec_trans=conserve(_spec(specularTransmittance)),
                  ior_eta=f32(f32(intIOR) / f32(extIOR)), smooth=0, ref_n_zero=1)


# ---------------------------------------------------------------------------
# sample / eval / pdf
# ---------------------------------------------------------------------------
def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _scale(v, s):
    return v * s[:, None]


def cosine_hemisphere(M, sx, sy):
    """warp::squareToCosineHemisphere over squareToUniformDiskConcentric (warp.cpp:43-52,81-102)."""
    with np.errstate(all="ignore"):
        r1, r2 = f32(2) * sx - f32(1), f32(2) * sy - f32(1)
        a = r1 * r1 > r2 * r2
        zero = (r1 == 0) & (r2 == 0)
        r = np.where(a, r1, r2)
        phi = np.where(a, (PI / f32(4)) * (r2 / r1), (PI / f32(2)) - (r1 / r2) * (PI / f32(4))).astype(f32)
        r = np.where(zero, f32(0), r).astype(f32)
        phi = np.where(zero, f32(0), phi).astype(f32)
        px, py = r * M.cos(phi), r * M.sin(phi)
        z = np.sqrt(np.maximum(f32(0), f32(1) - px * px - py * py)).astype(f32)
        z = np.where(z == 0, f32(1e-10), z).astype(f32)
    return np.stack([px, py, z], 1).astype(f32)


def _coordinate_system(a):   # util.cpp:590-600: (b, c)
    with np.errstate(all="ignore"):
        big = np.abs(a[:, 0]) > np.abs(a[:, 1])
        i1 = f32(1) / np.sqrt(a[:, 0] * a[:, 0] + a[:, 2] * a[:, 2])
        i2 = f32(1) / np.sqrt(a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])
        zero = np.zeros_like(i1)
        c = np.where(big[:, None], np.stack([a[:, 2] * i1, zero, -a[:, 0] * i1], 1), np.stack([zero, a[:, 2] * i2, -a[:, 1] * i2], 1)).astype(f32)
        b = np.stack([c[:, 1] * a[:, 2] - c[:, 2] * a[:, 1], c[:, 2] * a[:, 0] - c[:, 0] * a[:, 2],
                      c[:, 0] * a[:, 1] - c[:, 1] * a[:, 0]], 1).astype(f32)
    return b, c


def fresnel_dielectric(cos_i, eta):
    """fresnelDielectricExt without the transmitted cosine (util.cpp:651-681)."""
    with np.errstate(all="ignore"):
        scale = np.where(cos_i > 0, f32(1) / eta, eta).astype(f32)
        c2 = f32(1) - (f32(1) - cos_i * cos_i) * (scale * scale)
        ci, ct = np.abs(cos_i), np.sqrt(np.maximum(c2, f32(0))).astype(f32)
        rs = (ci - eta * ct) / (ci + eta * ct)
        rp = (eta * ci - ct) / (eta * ci + ct)
        F = f32(0.5) * (rs * rs + rp * rp)
        F = np.where(c2 <= 0, f32(1), F).astype(f32)
    return np.zeros_like(F) if eta == 1 else F


def thin_reflectance(b, wi):
    """R' = R + T^2 R / (1 - R^2) (thindielectric.cpp:209-213)."""
    R = fresnel_dielectric(np.abs(wi[:, 2]), b.ior_eta)
    T = f32(1) - R
    with np.errstate(all="ignore"):
        return np.where(R < 1, R + T * T * R / (f32(1) - R * R), R).astype(f32)


def _sin_theta(v):
    t = f32(1) - v[:, 2] * v[:, 2]
    return np.where(t <= 0, f32(0), np.sqrt(np.maximum(t, f32(0)))).astype(f32)


def _phong(M, b, alb, wi, wo):
    n = wi.shape[0]
    R = np.stack([-wi[:, 0], -wi[:, 1], wi[:, 2]], 1)
    alpha, e = _dot(wo, R), b.alpha_u
    with np.errstate(all="ignore"):
        p = M.pow(np.where(alpha > 0, alpha, f32(1)), np.full(n, e, f32))
    spec = np.where(alpha > 0, (e + f32(2)) * INV_TWOPI * p, f32(0)).astype(f32)
    specProb = np.where(alpha > 0, p * (e + f32(1)) / (f32(2) * PI), f32(0)).astype(f32)
    result = b.spec_refl[None, :] * spec[:, None] + alb * INV_PI
    pdf = b.spec_sampling_weight * specProb + (f32(1) - b.spec_sampling_weight) * (INV_PI * wo[:, 2])
    return _scale(result, wo[:, 2]).astype(f32), pdf.astype(f32)


def _ward(M, b, alb, wi, wo):
    au, av = b.alpha_u, b.alpha_v
    with np.errstate(all="ignore"):
        H = wi + wo
        if b.distribution == WARD_WARD:
            f1 = f32(1) / (f32(4) * PI * au * av * np.sqrt(wi[:, 2] * wo[:, 2]))
        elif b.distribution == WARD_DUER:
            f1 = f32(1) / (f32(4) * PI * au * av * wi[:, 2] * wo[:, 2])
        else:
            f1 = (_dot(H, H).astype(np.float64) / (np.float64(f32(PI * au * av)) * M.powd(H[:, 2], 4))).astype(f32)
        f2, f3 = H[:, 0] / au, H[:, 1] / av
        ex = -(f2 * f2 + f3 * f3) / (H[:, 2] * H[:, 2])
        specRef = (f1 * M.fastexp(ex)).astype(f32)
        spec = np.where(specRef > f32(1e-10), specRef, f32(0)).astype(f32)
        result = b.spec_refl[None, :] * spec[:, None] + alb * INV_PI
        Hs = wi + wo
        Hn = _scale(Hs, f32(1) / np.sqrt(_dot(Hs, Hs)))
        g1 = (1.0 / ((f32(4) * PI * au * av * _dot(Hn, wi)).astype(np.float64) * M.powd(Hn[:, 2], 3))).astype(f32)
        g2, g3 = Hn[:, 0] / au, Hn[:, 1] / av
        ex2 = -(g2 * g2 + g3 * g3) / (Hn[:, 2] * Hn[:, 2])
        specProb = (g1 * M.fastexp(ex2)).astype(f32)
        pdf = b.spec_sampling_weight * specProb + (f32(1) - b.spec_sampling_weight) * (INV_PI * wo[:, 2])
    return _scale(result, wo[:, 2]).astype(f32), pdf.astype(f32)


def _clamp1(v):
    return np.where(v < -1, f32(-1), np.where(v > 1, f32(1), v)).astype(f32)


def _roughdiffuse(M, b, alb, wi, wo):
    with np.errstate(all="ignore"):
        conv = f32(1) / np.sqrt(f32(2))
        sigma = f32(b.alpha_u * conv)
        s2 = f32(sigma * sigma)
        sI, sO = _sin_theta(wi), _sin_theta(wo)
        both = (sI > EPS) & (sO > EPS)
        sPI, cPI = _clamp1(wi[:, 1] / sI), _clamp1(wi[:, 0] / sI)
        sPO, cPO = _clamp1(wo[:, 1] / sO), _clamp1(wo[:, 0] / sO)
        cpd = np.where(both, cPI * cPO + sPI * sPO, f32(0)).astype(f32)
        iGt = wi[:, 2] > wo[:, 2]
        sinAlpha = np.where(iGt, sO, sI).astype(f32)
        sinBeta = np.where(iGt, sI, sO).astype(f32)
        tanBeta = np.where(iGt, sI / wi[:, 2], sO / wo[:, 2]).astype(f32)
        cosO = wo[:, 2]
        if b.nonlinear:
            A = f32(1) - f32(0.5) * s2 / (s2 + f32(0.33))
            Bc = f32(0.45) * s2 / (s2 + f32(0.09))
            val = alb * (INV_PI * cosO * (A + Bc * np.maximum(cpd, f32(0)) * sinAlpha * tanBeta))[:, None]
        else:
            tI = M.acos(np.minimum(f32(1), np.maximum(f32(-1), wi[:, 2])))
            tO = M.acos(np.minimum(f32(1), np.maximum(f32(-1), wo[:, 2])))
            alpha, beta = np.maximum(tI, tO), np.minimum(tI, tO)
            tmp = f32(s2 / (s2 + f32(0.09)))
            tmp2 = (f32(4) * INV_PI * INV_PI) * alpha * beta
            tmp3 = f32(2) * beta * INV_PI
            C1 = f32(1) - f32(0.5) * s2 / (s2 + f32(0.33))
            C2 = f32(f32(0.45) * tmp)
            C3 = f32(0.125) * tmp * tmp2 * tmp2
            C4 = f32(0.17) * s2 / (s2 + f32(0.13))
            C2 = np.where(cpd > 0, C2 * sinAlpha, C2 * (sinAlpha - tmp3 * tmp3 * tmp3)).astype(f32)
            sq = lambda v: np.sqrt(np.maximum(f32(0), v)).astype(f32)
            tanHalf = (sinAlpha + sinBeta) / (sq(f32(1) - sinAlpha * sinAlpha) + sq(f32(1) - sinBeta * sinBeta))
            sngl = alb * (C1 + cpd * C2 * tanBeta + (f32(1) - np.abs(cpd)) * C3 * tanHalf)[:, None]
            dbl = alb * alb * (C4 * (f32(1) - cpd * tmp3 * tmp3))[:, None]
            val = (sngl + dbl) * (INV_PI * cosO)[:, None]
    return val.astype(f32), (INV_PI * cosO).astype(f32)


def evaluate(b, wi, wo, exact=True, alb=None):
    """(eval * cos (n, 3), pdf (n,)) for wi (3,) or (n, 3) and wo (n, 3)."""
    M = Math(exact)
    wo = np.ascontiguousarray(wo, f32).reshape(-1, 3)
    wi = np.broadcast_to(np.asarray(wi, f32).reshape(-1, 3), wo.shape).copy()
    n = wo.shape[0]
    alb = np.broadcast_to(b.reflectance if alb is None else np.asarray(alb, f32), (n, 3)).astype(f32)
    val, pdf = np.zeros((n, 3), f32), np.zeros(n, f32)
    if b.type == THINDIELECTRIC:
        return val, pdf
    if b.type == DIFFTRANS:
        on = wi[:, 2] * wo[:, 2] < 0
        a = np.abs(wo[:, 2])
        return np.where(on[:, None], alb * (INV_PI * a)[:, None], f32(0)).astype(f32), np.where(on, a * INV_PI, f32(0)).astype(f32)
    on = (wi[:, 2] > 0) & (wo[:, 2] > 0)
    if on.any():
        fn = {PHONG: _phong, WARD: _ward, ROUGHDIFFUSE: _roughdiffuse}[b.type]
        v, p = fn(M, b, alb[on], wi[on], wo[on])
        val[on], pdf[on] = v, p
    return val, pdf


def sample(b, wi, u, exact=True, alb=None):
    """(wo, weight, pdf, eta, flags) for wi (3,) or (n, 3) and u (n, >= 2):
    a failed sample (zero weight) has flags 0 and zeros elsewhere."""
    M = Math(exact)
    u = np.ascontiguousarray(u, f32)
    n = u.shape[0]
    wi = np.broadcast_to(np.asarray(wi, f32).reshape(-1, 3), (n, 3)).copy()
    albs = np.broadcast_to(b.reflectance if alb is None else np.asarray(alb, f32), (n, 3)).astype(f32)
    sx, sy = u[:, 0].copy(), u[:, 1].copy()
    wo, weight = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    pdf, flags = np.zeros(n, f32), np.zeros(n, np.uint32)
    ok = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        if b.type in (PHONG, WARD):
            w = b.spec_sampling_weight
            spec = sx <= w
            sx = np.where(spec, sx / w, (sx - w) / (f32(1) - w)).astype(f32)
            d = ~spec
            if d.any():
                wo[d] = cosine_hemisphere(M, sx[d], sy[d])
            alive = np.ones(n, bool)
            if spec.any():
                s, xs, ys, wis = np.flatnonzero(spec), sx[spec], sy[spec], wi[spec]
                if b.type == PHONG:
                    R = np.stack([-wis[:, 0], -wis[:, 1], wis[:, 2]], 1)
                    e = np.full(len(s), b.alpha_u, f32)
                    sinA = np.sqrt(f32(1) - M.pow(ys, f32(2) / (e + f32(1)))).astype(f32)
                    cosA = M.pow(ys, f32(1) / (e + f32(1)))
                    phi = (f32(2) * PI) * xs
                    loc = np.stack([sinA * M.cos(phi), sinA * M.sin(phi), cosA], 1)
                    fs, ft = _coordinate_system(R)
                    w_s = _scale(fs, loc[:, 0]) + _scale(ft, loc[:, 1]) + _scale(R, loc[:, 2])
                else:
                    au, av = b.alpha_u, b.alpha_v
                    phiH = M.atan(av / au * M.tan(f32(2) * PI * ys))
                    phiH = np.where(ys > f32(0.5), phiH + PI, phiH).astype(f32)
                    cP, sPtrue = M.cos(phiH), M.sin(phiH)
                    sP = np.sqrt(np.maximum(f32(0), f32(1) - cP * cP)).astype(f32)
                    arg = -M.fastlog(xs) / ((cP * cP) / (au * au) + (sP * sP) / (av * av))
                    thetaH = M.atan(np.sqrt(np.maximum(f32(0), arg)).astype(f32))
                    sT, cT = M.sin(thetaH), M.cos(thetaH)
                    H = np.stack([sT * cP, sT * sPtrue, cT], 1).astype(f32)
                    w_s = _scale(H, f32(2) * _dot(wis, H)) - wis
                wo[s] = w_s
                alive[s] = w_s[:, 2] > 0
            val, p = evaluate(b, wi, wo, exact, albs)
            good = alive & (p != 0)
            weight = np.where(good[:, None], val * (f32(1) / p)[:, None], f32(0)).astype(f32)
            pdf = p
            ok = good & (weight != 0).any(1)
        elif b.type == ROUGHDIFFUSE:
            wo = cosine_hemisphere(M, sx, sy)
            val, _ = evaluate(b, wi, wo, exact, albs)
            pdf = (INV_PI * wo[:, 2]).astype(f32)
            weight = (val * (f32(1) / pdf)[:, None]).astype(f32)
            ok = (wi[:, 2] > 0) & (weight != 0).any(1)
        elif b.type == DIFFTRANS:
            wo = cosine_hemisphere(M, sx, sy)
            wo[:, 2] = np.where(wi[:, 2] > 0, wo[:, 2] * f32(-1), wo[:, 2])
            pdf = (np.abs(wo[:, 2]) * INV_PI).astype(f32)
            weight = albs.copy()
            ok = (weight != 0).any(1)
        else:
            R = thin_reflectance(b, wi)
            refl = sx <= R
            wo = np.where(refl[:, None], np.stack([-wi[:, 0], -wi[:, 1], wi[:, 2]], 1), -wi).astype(f32)
            pdf = np.where(refl, R, f32(1) - R).astype(f32)
            weight = np.where(refl[:, None], b.spec_refl[None, :], b.spec_trans[None, :]).astype(f32)
            ok = (weight != 0).any(1)
            flags = np.where(refl, DELTA, DELTA | NULL).astype(np.uint32)
    flags = np.where(ok, flags | OK, 0).astype(np.uint32)
    z = ~ok
    wo[z], weight[z], pdf[z] = 0, 0, 0
    eta = np.where(ok, f32(1), f32(0)).astype(f32)
    return wo.astype(f32), weight.astype(f32), pdf.astype(f32), eta, flags
