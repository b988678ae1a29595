"""Helpers of the point / spot / directional / constant emitter tests: ctypes
views of mtsg_emitter and mtsg_emitter_ext, the test scenes, and a float32
numpy restatement of the four emitters' sampleDirect (point.cpp:127-142,
spot.cpp:105-127,179-193, directional.cpp:159-180, constant.cpp:173-215) inside
`direct`'s emitter loop (direct.cpp:146-245, Scene::sampleEmitterDirect,
scene.cpp:910-947).

The restatement is built from oracle pieces as direct_ref.emitters_only_reference
is: the oracle's camera rays, closest hits, BSDF evaluation and shadow rays, the
intersection record of multichannel_ref and the counter RNG's draws, with
DiscreteDistribution::sampleReuse's rescaled first coordinate.  Where the
reference calls libm (acosf, sincosf) the restatement calls the C library's
function per element, not numpy's vectorised one.  The oracle's `render` does
not know these emitters and is never asked to render such a scene."""
import ctypes as C
import functools

import numpy as np

import mtsg
from conftest import SCENES
import direct_ref as DR
import multichannel_ref as R
import test_bsdf_chisquare as B
from direct_ref import EPS, SHADOW_EPS, _v, box_geometry, box_props
from multichannel_ref import f32, grid_mesh, xf

F, I, U, P = C.c_float, C.c_int32, C.c_uint32, C.c_void_p
AREA, ENVMAP, POINT, SPOT, DIRECTIONAL, CONSTANT = 1, 2, 3, 4, 5, 6
INV_PI = f32(0.31830988618379067154)
INV_FOURPI = f32(0.07957747154594766788)

_libm = C.CDLL("libm.so.6")
_libm.acosf.restype = F
_libm.acosf.argtypes = [F]


def acosf(x):
    return np.array([_libm.acosf(float(v)) for v in x], f32)


class Emitter(C.Structure):
    """mtsg_emitter (include/mtsg.h)."""
    _fields_ = [("type", I), ("shape", I), ("cdf_offset", U), ("pdf_discrete", F), ("radiance", F * 3), ("inv_area", F)]


class EmitterExt(C.Structure):
    """mtsg_emitter_ext (include/mtsg.h)."""
    _fields_ = [("position", F * 3), ("direction", F * 3), ("to_local", F * 9), ("cos_beam_width", F), ("cos_cutoff_angle", F),
                ("cutoff_angle", F), ("inv_transition_width", F), ("bsphere_center", F * 3), ("bsphere_radius", F), ("pad", F)]


class SceneDescX(C.Structure):
    """mtsg_scene_desc with the field appended after ABI 8's."""
    _fields_ = list(R.SceneDesc._fields_) + [("emitter_ext", P)]


assert C.sizeof(Emitter) == 32 and C.sizeof(EmitterExt) == 96


def emitter_records(scene):
    """(emitters, extension records or None, the discrete CDF) of a scene descriptor, copied."""
    d = C.cast(scene.desc, C.POINTER(SceneDescX)).contents
    n = d.nemitters
    ems = [Emitter.from_buffer_copy(bytes(C.cast(d.emitters, C.POINTER(Emitter))[k])) for k in range(n)]
    ext = None
    if d.emitter_ext:
        ext = [EmitterExt.from_buffer_copy(bytes(C.cast(d.emitter_ext, C.POINTER(EmitterExt))[k])) for k in range(n)]
    return ems, ext, R._arr(d.emitter_cdf, f32, (n + 1,))


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
DOWN = xf([(1, 0, 0), (0, 0, 1), (0, -1, 0)], (0.0, 0.9, 0.9))   # local z = world -y: a spot that looks at the floor

# One emitter per kind for the per-sample restatement.  The point light sits
# close to the camera's axis (the camera is at (0.05, 0.1, 3.6)), so the cube's
# hard shadow lies behind the cube as the camera sees it and few visible points
# see the light graze the cube's silhouette; the spot hangs over the open
# floor in front of the cube and its 25-degree cone ends on the floor, so
# camera samples fall outside the cutoff, on the ramp and inside the 12-degree
# beam; the directional light comes from above and in front.
KIND_EMITTERS = {
    "point": ("point", [("position", "point", (0.1, 0.45, 2.9)), ("intensity", "spectrum", (9.0, 8.0, 7.0))]),
    "spot": ("spot", [("toWorld", "transform", DOWN), ("intensity", "spectrum", (20.0, 22.0, 25.0)),
                      ("cutoffAngle", "float", 25.0), ("beamWidth", "float", 12.0)]),
    "directional": ("directional", [("direction", "vector", (-0.3, -1.0, -0.4)), ("irradiance", "spectrum", (2.0, 2.5, 3.0))]),
    "constant": ("constant", [("radiance", "spectrum", (0.8, 0.9, 1.0))]),
}

# the four kinds beside the full box's area lights, at unequal sampling weights
MIXED_EMITTERS = [
    ("point", [("position", "point", (0.1, 0.45, 2.9)), ("intensity", "spectrum", (9.0, 8.0, 7.0)), ("samplingWeight", "float", 0.5)]),
    ("spot", [("toWorld", "transform", DOWN), ("intensity", "spectrum", (20.0, 22.0, 25.0)), ("cutoffAngle", "float", 25.0),
              ("beamWidth", "float", 12.0), ("samplingWeight", "float", 2.0)]),
    ("directional", [("direction", "vector", (-0.3, -1.0, -0.4)), ("irradiance", "spectrum", (2.0, 2.5, 3.0)),
                     ("samplingWeight", "float", 1.5)]),
    ("constant", [("radiance", "spectrum", (0.8, 0.9, 1.0)), ("samplingWeight", "float", 0.7)]),
]


def diffuse_box(b):
    """direct_ref.box_geometry(diffuse_only=True) without its area lights: the
    bumpy floor with vertex normals, the left wall with face normals, the two
    wall rectangles and the cube, all diffuse.  The right quarter of the back
    is open: those camera rays miss."""
    wall = b.bsdf("diffuse", [("reflectance", "spectrum", (0.7, 0.65, 0.6))])
    floor = b.bsdf("diffuse", [("reflectance", "spectrum", (0.5, 0.6, 0.4))])
    red = b.bsdf("diffuse", [("reflectance", "spectrum", (0.8, 0.1, 0.1))])
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
    b.shape("rectangle", [("toWorld", "transform", xf([(0, 0, 1.1), (0, 1, 0), (-1, 0, 0)], (1.2, 0, 0.1)))], wall)
    b.shape("rectangle", [("toWorld", "transform", xf([(0.9, 0, 0), (0, 1, 0), (0, 0, 1)], (-0.3, 0, -1.0)))], wall)
    b.shape("cube", [("toWorld", "transform", xf([(0.25, 0, 0), (0, 0.25, 0), (0, 0, 0.25)], (0.45, -0.2, 0.2)))], wall)


def kind_scene(kind, integrator="direct", props=(), **kw):
    """The diffuse box lit by the one emitter of `kind`."""
    b = mtsg.SceneBuilder(SCENES)
    b.integrator(integrator, list(props))
    box_props(b, **kw)
    diffuse_box(b)
    b.emitter(*KIND_EMITTERS[kind])
    return b.finish()


def mixed_scene(integrator="path", props=(("maxDepth", "integer", 2),), emitters=MIXED_EMITTERS, instancing="flatten", **kw):
    """The full box (rough plastic, metal cube, area lights) with the four new emitters added."""
    b = mtsg.SceneBuilder(SCENES, instancing=instancing)
    b.integrator(integrator, list(props))
    box_props(b, **kw)
    box_geometry(b)
    for plugin, p in emitters:
        b.emitter(plugin, p)
    return b.finish()


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def primary(spp):
    """direct_ref.Primary over the diffuse box: its camera samples, hits,
    shading frames, draws and shadow rays.  The oracle walks a path to log the
    camera ray and knows area lights only, so its copy of the box is lit by a
    millimetre-sized rectangle light 50 units below the floor instead of the
    emitter under test: farther away than any shadow ray of these tests is
    long, so it occludes none, and the hits of the box do not depend on it."""
    saved = DR.box_geometry

    def geometry(b, diffuse_only=False, mesh_light=True):
        diffuse_box(b)
        far = b.emitter("area", [("radiance", "spectrum", (1.0, 1.0, 1.0))])
        b.shape("rectangle", [("toWorld", "transform", xf([(1e-3, 0, 0), (0, 0, 1e-3), (0, -1, 0)], (0, -50.0, 0)))], -1, far)
    DR.box_geometry = geometry
    try:
        return DR.Primary(spp)
    finally:
        DR.box_geometry = saved


@functools.lru_cache(maxsize=None)
def kind_records(kind):
    """(emitters, extension records, CDF) of kind_scene(kind)."""
    return emitter_records(kind_scene(kind))


def _coordinate_system(a):
    """coordinateSystem (util.cpp:590-600) per row: (b, c)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        wide = np.abs(a[:, 0]) > np.abs(a[:, 1])
        l1 = f32(1) / np.sqrt(((a[:, 0] * a[:, 0]).astype(f32) + (a[:, 2] * a[:, 2]).astype(f32)).astype(f32)).astype(f32)
        l2 = f32(1) / np.sqrt(((a[:, 1] * a[:, 1]).astype(f32) + (a[:, 2] * a[:, 2]).astype(f32)).astype(f32)).astype(f32)
        zero = np.zeros(len(a), f32)
        c = np.where(wide[:, None], np.stack([a[:, 2] * l1, zero, -a[:, 0] * l1], 1), np.stack([zero, a[:, 2] * l2, -a[:, 1] * l2], 1)).astype(f32)
    return R._cross(c, a), c


def _sphere(center, radius, o, d):
    """BSphere::rayIntersect + solveQuadratic (bsphere.h:88-95, util.cpp:447-485): (hit, nearT, farT)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        oc = (o - center[None, :]).astype(f32)
        A, Bq = R._dot(d, d), (f32(2) * R._dot(oc, d)).astype(f32)
        Cq = (R._dot(oc, oc) - f32(radius * radius)).astype(f32)
        disc = ((Bq * Bq).astype(f32) - ((f32(4) * A).astype(f32) * Cq).astype(f32)).astype(f32)
        hit = (A != 0) & (disc >= 0)
        sq = np.sqrt(np.where(hit, disc, 0)).astype(f32)
        temp = np.where(Bq < 0, (f32(-0.5) * (Bq - sq).astype(f32)).astype(f32), (f32(-0.5) * (Bq + sq).astype(f32)).astype(f32))
        x0, x1 = (temp / A).astype(f32), (Cq / temp).astype(f32)
    return hit, np.minimum(x0, x1), np.maximum(x0, x1)


def sample_direct(em, ext, ref, ref_n, u):
    """Emitter::sampleDirect of one point / spot / directional / constant
    emitter for n reference points: (ok, d, dist, value, branch).  branch (spot):
    0 outside the cutoff, 1 on the ramp, 2 inside the beam."""
    n = len(ref)
    rad = np.array(list(em.radiance), f32)
    branch = np.full(n, -1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if em.type in (POINT, SPOT):
            d = (np.array(list(ext.position), f32)[None, :] - ref).astype(f32)
            dist = np.sqrt(R._dot(d, d)).astype(f32)
            inv = (f32(1) / dist).astype(f32)
            d = _v(d, inv)
            value = np.broadcast_to(rad, (n, 3)).astype(f32)
            ok = np.ones(n, bool)
            if em.type == SPOT:
                row = np.broadcast_to(np.array(list(ext.to_local), f32)[6:9], (n, 3)).astype(f32)
                cos_t = R._dot(row, (-d).astype(f32))
                ok = cos_t > f32(ext.cos_cutoff_angle)
                ramp = ok & ~(cos_t >= f32(ext.cos_beam_width))
                fall = ((f32(ext.cutoff_angle) - acosf(np.where(ramp, cos_t, f32(1)))).astype(f32) * f32(ext.inv_transition_width)).astype(f32)
                value = np.where(ramp[:, None], _v(value, fall), value)
                branch = np.where(~ok, 0, np.where(ramp, 1, 2))
            value = _v(value, (inv * inv).astype(f32))
            return ok, d, dist, value, branch
        if em.type == DIRECTIONAL:
            dv = np.array(list(ext.direction), f32)
            disk = (np.array(list(ext.bsphere_center), f32) - (dv * f32(ext.bsphere_radius)).astype(f32)).astype(f32)
            dn = np.broadcast_to(dv, (n, 3)).astype(f32)
            distance = R._dot((ref - disk[None, :]).astype(f32), dn)
            return distance >= 0, (-dn).astype(f32), distance, np.broadcast_to(rad, (n, 3)).astype(f32), branch
        assert em.type == CONSTANT and not (ref_n == 0).all(1).any()   # the diffuse box: refN is the shading normal
        local = B.sample(B.make_bsdf(B.DIFFUSE), np.array([0, 0, 1], f32), u)[0]   # squareToCosineHemisphere
        pdf = (INV_PI * local[:, 2]).astype(f32)
        s, t = _coordinate_system(ref_n)
        d = ((_v(s, local[:, 0]) + _v(t, local[:, 1])).astype(f32) + _v(ref_n, local[:, 2])).astype(f32)
        hit, near, far = _sphere(np.array(list(ext.bsphere_center), f32), f32(ext.bsphere_radius), ref, d)
        ok = hit & (near < 0) & (far > 0) & (R._dot(d, ref_n) > 0)
        value = _v(np.broadcast_to(rad, (n, 3)).astype(f32), (f32(1) / pdf).astype(f32))
        return ok, d, far, value, branch


def emitters_reference(Pr, records, ne, hide_emitters=False):
    """direct.cpp:146-245 per sample with bsdfSamples = 0 on the diffuse box lit
    by emitters without a shape: (Li, sum of |terms|, fragile, spot branches).
    Both MIS weights are 1 (a delta emitter's BSDF pdf is 0; a constant
    emitter's is multiplied by fracBSDF = 0), so a term is value * bsdfVal / ne."""
    ems, ext, cdf = records
    assert ext is not None and all(e.type >= POINT for e in ems)
    S = len(Pr.key)
    Li = np.zeros((S, 3), f32)
    const = [e for e in ems if e.type == CONSTANT]
    if const and not hide_emitters:
        Li[Pr.miss] = np.array(list(const[0].radiance), f32)   # evalEnvironment of a primary miss
    mag = np.zeros((S, 3), f32)
    fragile = np.zeros(S, bool)
    branches = np.full((S, ne), -1)
    wi = Pr.to_local((-Pr.rd).astype(f32))
    u = Pr.draws(ne)
    weight = f32(1) / f32(ne)
    for i in range(ne):
        sx, sy = u[:, i, 0].copy(), u[:, i, 1]
        # DiscreteDistribution::sampleReuse (pmf.h): lower_bound - 1, then the rescaled sample
        idx = np.clip(np.searchsorted(cdf, sx, "left") - 1, 0, len(ems) - 1)
        c0, c1 = cdf[idx], cdf[idx + 1]
        em_pdf = (c1 - c0).astype(f32)
        sx = ((sx - c0).astype(f32) / em_pdf).astype(f32)
        ok = np.zeros(S, bool)
        d = np.zeros((S, 3), f32)
        dist = np.zeros(S, f32)
        value = np.zeros((S, 3), f32)
        for k, em in enumerate(ems):
            m = Pr.hit & (idx == k)
            if not m.any():
                continue
            o, dk, tk, vk, bk = sample_direct(em, ext[k], Pr.p[m], Pr.n[m], np.stack([sx[m], sy[m]], 1))
            ok[m], d[m], dist[m], value[m] = o, dk, tk, vk
            branches[m, i] = bk
        with np.errstate(invalid="ignore", divide="ignore"):
            value = _v(value, (f32(1) / em_pdf).astype(f32))
        wo = Pr.to_local(d)
        bval = np.zeros((S, 3), f32)
        for j in np.nonzero(ok)[0]:
            bval[j] = B.evaluate(Pr.D.bsdfs[Pr.bsdf[j]], wi[j], wo[j:j + 1])[0][0]
        term = ((value * bval).astype(f32) * weight).astype(f32)
        ok &= (bval != 0).any(1) & (term != 0).any(1)
        maxt = (dist * (f32(1) - SHADOW_EPS)).astype(f32)
        occ, fr = Pr.shadow(Pr.p, d, np.full(S, EPS), maxt, ok)
        add = ok & ~occ
        Li[add] = (Li[add] + term[add]).astype(f32)
        mag[ok] += np.abs(term[ok])
        fragile |= fr
    return Li, mag, fragile, branches
