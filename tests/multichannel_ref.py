"""Helpers of tests/test_gpu_multichannel.py: the test scenes (built with
SceneBuilder), a ctypes view of mtsg_scene_desc, and float32 numpy
restatements of the reference code the `field` integrator reads its values
from -- ShapeKDTree::fillIntersectionRecord (skdtree.h:349-426),
Rectangle::fillIntersectionRecord (rectangle.cpp:155-164), field.cpp:124-177
-- and of ImageBlock::put (imageblock.h:153-187)."""
import ctypes as C
import os

import numpy as np

import mtsg
from conftest import SCENES
from test_bsdf_chisquare import Bsdf

f32 = np.float32
UNDEFINED = (-1.0, 0.5, 7.0)
FILM_W, FILM_H, SPP = 40, 24, 4

P, U, I, F = C.c_void_p, C.c_uint32, C.c_int32, C.c_float


class Camera(C.Structure):
    """mtsg_camera (include/mtsg.h)."""
    _fields_ = [("s2c", F * 16), ("c2w", F * 12), ("dx", F * 3), ("dy", F * 3), ("near_clip", F), ("far_clip", F),
                ("inv_res_x", F), ("inv_res_y", F), ("film_w", I), ("film_h", I), ("crop", I * 4), ("filter_type", I),
                ("filter_radius", F), ("filter_scale", F), ("border", I), ("filter_values", F * 32), ("has_alpha", I),
                ("pad", I * 3)]


class SceneDesc(C.Structure):
    """mtsg_scene_desc (include/mtsg.h); the environment record as raw words."""
    _fields_ = [("abi", U), ("nv", U), ("pos", P), ("nrm", P), ("ntri", U), ("tri_idx", P), ("dpdu", P), ("nrects", U),
                ("rects", P), ("nshapes", U), ("shapes", P), ("nbsdfs", U), ("bsdfs", P), ("nemitters", U), ("emitters", P),
                ("emitter_cdf", P), ("n_emitter_tri_cdf", U), ("emitter_tri_cdf", P), ("n_nodes", U), ("nodes", P),
                ("n_indices", U), ("indices", P), ("n_prims", U), ("triaccel", P), ("aabb_min", F * 3), ("aabb_max", F * 3),
                ("max_depth", U), ("camera", Camera), ("has_envmap", I), ("n_env_texels", U), ("env_texels", P),
                ("env_cdf_rows", P), ("env_cdf_cols", P), ("env_row_weights", P), ("envmap", U * 222), ("sampler", I * 4),
                ("qmc_primes", P), ("qmc_perm_offset", P), ("qmc_perm", P), ("sobol_scramble", C.c_uint64),
                ("sobol_matrices", P), ("sobol_vdc_rows", U), ("sobol_vdc_inv_rows", U), ("sobol_vdc", P),
                ("sobol_vdc_inv", P), ("n_instances", U), ("instances", P), ("n_groups", U), ("groups", P),
                ("n_group_nodes", U), ("group_nodes", P), ("n_group_indices", U), ("group_indices", P), ("n_textures", U),
                ("textures", P), ("n_tex_texels", U), ("tex_texels", P), ("tri_uv", P), ("tri_dpdv", P), ("om", P),
                ("om_bits", P)]


def _arr(ptr, dtype, shape):
    n = int(np.prod(shape))
    if n == 0 or not ptr:
        return np.zeros(shape, dtype)
    buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype).reshape(shape).copy()


class Desc:
    """The arrays of a scene descriptor the restatements need."""

    def __init__(self, scene):
        d = C.cast(scene.desc, C.POINTER(SceneDesc)).contents
        assert d.abi == 8 and d.n_prims == d.ntri + d.nrects + d.n_instances   # the struct above matches the header
        self.pos = _arr(d.pos, f32, (d.nv, 3))
        self.nrm = _arr(d.nrm, f32, (d.nv, 3))
        self.tri = _arr(d.tri_idx, np.uint32, (d.ntri, 3))
        self.tri_uv = _arr(d.tri_uv, f32, (d.ntri, 6)) if d.tri_uv else None
        self.shapes = _arr(d.shapes, np.int32, (d.nshapes, 8))   # type, bsdf, emitter, face_normals, tri_begin, tri_count, rect, instance
        self.rects = _arr(d.rects, f32, (d.nrects, 41))
        self.rect_shape = _arr(d.rects, np.uint32, (d.nrects, 41))[:, 40]
        self.bsdfs = list(C.cast(d.bsdfs, C.POINTER(Bsdf))[:d.nbsdfs])
        self.n_textures = d.n_textures
        cam = d.camera
        self.border = cam.border
        self.filter_values = np.array(list(cam.filter_values), f32)
        self.filter_scale = f32(cam.filter_scale)
        self.filter_radius = f32(cam.filter_radius)
        self.tri_shape = np.zeros(d.ntri, np.int64)
        for si, sh in enumerate(self.shapes):
            if sh[0] == 0:
                self.tri_shape[sh[4]:sh[4] + sh[5]] = si


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
def xf(cols, t):
    """4x4 from the images of the local x, y, z axes and the translation."""
    m = np.eye(4, dtype=f32)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = cols[0], cols[1], cols[2], t
    return m


def grid_mesh(origin, du, dv, n, bump, normal):
    """(n+1)^2 vertices origin + i du + j dv + bump(i, j) normal, 2 n^2 triangles, uv = (i, j) / n."""
    pos, uv = [], []
    for j in range(n + 1):
        for i in range(n + 1):
            pos.append(np.asarray(origin, np.float64) + i * np.asarray(du) + j * np.asarray(dv) + bump(i, j) * np.asarray(normal))
            uv.append((i / n, j / n))
    tris = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            tris += [(a, a + 1, a + n + 2), (a, a + n + 2, a + n + 1)]
    return np.asarray(pos, f32), np.asarray(uv, f32), np.asarray(tris, np.uint32)


ALL_FIELDS = ["position", "relPosition", "distance", "geoNormal", "shNormal", "uv", "albedo", "shapeIndex", "primIndex"]


def box_scene(children, rfilter=("gaussian", []), sampler="independent", pixel_format=None):
    """The closed test box.  children: None = the plain `path` integrator, else
    the multichannel children in order ("path" or a field name)."""
    b = mtsg.SceneBuilder(SCENES)
    path_props = [("maxDepth", "integer", 4)]
    if children is None:
        b.integrator("path", path_props)
        fmt = [("pixelFormat", "string", pixel_format or "rgba")]
    else:
        for c in children:
            if c == "path":
                b.integrator_child("path", path_props)
            else:
                b.integrator_child("field", [("field", "string", c), ("undefined", "spectrum", UNDEFINED)])
        b.multichannel()
        fmt = [("pixelFormat", "string", ", ".join(["rgb"] * len(children))),
               ("channelNames", "string", ", ".join(f"c{k}" for k in range(len(children))))]
    b.sensor("perspective", [("fov", "float", 40.0),
                             ("toWorld", "transform", xf([(-1, 0, 0), (0, 1, 0), (0, 0, -1)], (0.05, 0.1, 3.6)))])
    b.film("hdrfilm", [("width", "integer", FILM_W), ("height", "integer", FILM_H)] + fmt, rfilter[0], rfilter[1])
    b.sampler(sampler, [("sampleCount", "integer", SPP)])
    tex = b.texture("bitmap", [("filename", "string", "tex_checker.png")])
    checker = b.bsdf("diffuse", [("reflectance", "texture", tex)])
    plastic = b.bsdf("plastic", [("diffuseReflectance", "spectrum", (0.4, 0.5, 0.6)), ("intIOR", "float", 1.5),
                                 ("extIOR", "float", 1.0)])
    rplastic = b.bsdf("roughplastic", [("diffuseReflectance", "spectrum", (0.6, 0.3, 0.2)), ("alpha", "float", 0.2),
                                       ("intIOR", "float", 1.5), ("extIOR", "float", 1.0)])
    metal = b.bsdf("roughconductor", [("alpha", "float", 0.3)])
    wall = b.bsdf("diffuse", [("reflectance", "spectrum", (0.7, 0.65, 0.6))])
    red = b.bsdf("diffuse", [("reflectance", "spectrum", (0.8, 0.1, 0.1))])
    green = b.bsdf("diffuse", [("reflectance", "spectrum", (0.1, 0.75, 0.2))])
    panel = b.bsdf("twosided", [], nested=(red, green))
    light = b.emitter("area", [("radiance", "spectrum", (15.0, 14.0, 12.0))])
    # floor: UV-mapped, vertex normals (a smooth bump), textured
    fp, fuv, ft = grid_mesh((-1.2, -0.5, 1.2), (0.6, 0, 0), (0, 0, -0.55), 4, lambda i, j: 0.08 * np.sin(1.3 * i) * np.cos(0.9 * j),
                            (0, 1, 0))
    fn = np.zeros_like(fp)
    for k, (i, j) in enumerate((i, j) for j in range(5) for i in range(5)):
        dx = 0.08 * 1.3 * np.cos(1.3 * i) * np.cos(0.9 * j) / 0.6
        dz = -0.08 * 0.9 * np.sin(1.3 * i) * np.sin(0.9 * j) / -0.55
        n = np.array([-dx, 1.0, -dz])
        fn[k] = n / np.linalg.norm(n)
    b.mesh(fp, ft, normals=fn, texcoords=fuv, bsdf=checker, name="floor")
    # left wall: face normals, no texture coordinates
    lp, _luv, lt = grid_mesh((-1.2, -1.0, 1.2), (0, 0, -0.75), (0, 0.7, 0), 3, lambda i, j: 0.05 * ((i * 2 + j) % 3), (1, 0, 0))
    b.mesh(lp, lt, face_normals=True, bsdf=plastic, name="left")
    # right wall, back wall (leaves the right quarter open: those camera rays miss), light
    b.shape("rectangle", [("toWorld", "transform", xf([(0, 0, 1.1), (0, 1, 0), (-1, 0, 0)], (1.2, 0, 0.1)))], rplastic)
    b.shape("rectangle", [("toWorld", "transform", xf([(0.9, 0, 0), (0, 1, 0), (0, 0, 1)], (-0.3, 0, -1.0)))], wall)
    b.shape("cube", [("toWorld", "transform", xf([(0.25, 0, 0), (0, 0.25, 0), (0, 0, 0.25)], (0.45, -0.2, 0.2)))], metal)
    # a twosided panel whose front faces away from the camera
    b.shape("rectangle", [("toWorld", "transform", xf([(-0.3, 0, 0), (0, 0.3, 0), (0, 0, -1)], (-0.5, -0.1, 0.3)))], panel)
    b.shape("rectangle", [("toWorld", "transform", xf([(0.4, 0, 0), (0, 0, 0.4), (0, -1, 0)], (0, 0.99, 0)))], -1, light)
    return b.finish()


def instanced_scene(children, instancing):
    b = mtsg.SceneBuilder(SCENES, instancing=instancing)
    for c in children:
        if c == "path":
            b.integrator_child("path", [("maxDepth", "integer", 4)])
        else:
            b.integrator_child("field", [("field", "string", c), ("undefined", "spectrum", UNDEFINED)])
    b.multichannel()
    b.sensor("perspective", [("fov", "float", 45.0),
                             ("toWorld", "transform", xf([(-1, 0, 0), (0, 1, 0), (0, 0, -1)], (0, 0.3, 3.2)))])
    b.film("hdrfilm", [("width", "integer", 32), ("height", "integer", 24),
                       ("pixelFormat", "string", ", ".join(["rgb"] * len(children))),
                       ("channelNames", "string", ", ".join(f"c{k}" for k in range(len(children))))], "gaussian", [])
    b.sampler("independent", [("sampleCount", "integer", SPP)])
    white = b.bsdf("diffuse", [("reflectance", "spectrum", (0.7, 0.7, 0.7))])
    blue = b.bsdf("diffuse", [("reflectance", "spectrum", (0.2, 0.3, 0.8))])
    light = b.emitter("area", [("radiance", "spectrum", (12.0, 12.0, 12.0))])
    g = b.group("pyramids")
    pos = np.array([(-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, 1.5, 0)], f32) * f32(0.3)
    tris = np.array([(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)], np.uint32)
    b.mesh(pos, tris, bsdf=blue, group=g, name="pyramid")           # computed vertex normals
    b.mesh(pos * f32(0.5) + f32([0.5, 0, 0]), tris, face_normals=True, bsdf=white, group=g, name="small")
    b.shape("rectangle", [("toWorld", "transform", xf([(2, 0, 0), (0, 0, -2), (0, 1, 0)], (0, -0.4, 0)))], white)
    c, s = np.cos(0.6), np.sin(0.6)
    b.instance(g, [("toWorld", "transform", xf([(c, 0, -s), (0, 1, 0), (s, 0, c)], (-0.6, -0.4, 0)))])
    b.instance(g, [("toWorld", "transform", xf([(1.4 * c, 0, 1.4 * s), (0, 1.4, 0), (-1.4 * s, 0, 1.4 * c)], (0.5, -0.4, -0.5)))])
    b.shape("rectangle", [("toWorld", "transform", xf([(0.5, 0, 0), (0, 0, 0.5), (0, -1, 0)], (0, 1.6, 0)))], -1, light)
    return b.finish()


# ---------------------------------------------------------------------------
# the reference's intersection record and fields, float32
# ---------------------------------------------------------------------------
def _dot(a, b):
    return ((a[:, 0] * b[:, 0]).astype(f32) + (a[:, 1] * b[:, 1]).astype(f32)).astype(f32) + (a[:, 2] * b[:, 2]).astype(f32)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(f32)


def _normalize(a):
    with np.errstate(divide="ignore", invalid="ignore"):   # (unused vertex normals of face-normal meshes are zero)
        return _normalize_(a)


def _normalize_(a):
    inv = (f32(1) / np.sqrt(_dot(a, a)).astype(f32)).astype(f32)
    return (a * inv[:, None]).astype(f32)


def _bary(a, b, c, bx, by, bz):
    return ((a * bx[:, None]).astype(f32) + (b * by[:, None]).astype(f32) + (c * bz[:, None]).astype(f32)).astype(f32)


def expected_fields(D, aov, rays, t, u, v, prim, tex_eval):
    """Per sample the nine fields of field.cpp:124-177 from the camera ray and
    its closest hit; tex_eval(tex, uv) = the unfiltered texture lookup."""
    n = len(t)
    out = {k: np.tile(f32(UNDEFINED), (n, 1)) for k in ALL_FIELDS}
    miss = prim == 0xFFFFFFFF
    o, d = rays[:, 0:3].astype(f32), rays[:, 3:6].astype(f32)
    tri = ~miss & (prim < 0x80000000)
    rec = ~miss & (prim >= 0x80000000)
    p = np.zeros((n, 3), f32)
    gn = np.zeros((n, 3), f32)
    sn = np.zeros((n, 3), f32)
    uv = np.zeros((n, 2), f32)
    shape = np.zeros(n, np.int64)
    primidx = np.zeros(n, f32)
    # ---- triangles (skdtree.h:349-426)
    k = np.nonzero(tri)[0]
    tp = prim[k].astype(np.int64)
    i0, i1, i2 = D.tri[tp, 0], D.tri[tp, 1], D.tri[tp, 2]
    p0, p1, p2 = D.pos[i0], D.pos[i1], D.pos[i2]
    by, bz = u[k].astype(f32), v[k].astype(f32)
    bx = ((f32(1) - by).astype(f32) - bz).astype(f32)
    p[k] = _bary(p0, p1, p2, bx, by, bz)
    fn = _cross((p1 - p0).astype(f32), (p2 - p0).astype(f32))
    fn = _normalize(fn)
    sh = D.tri_shape[tp]
    shape[k] = sh
    face = D.shapes[sh, 3] != 0
    vn = _normalize(_bary(D.nrm[i0], D.nrm[i1], D.nrm[i2], bx, by, bz))
    with np.errstate(invalid="ignore"):
        flip = ~face & (_dot(fn, np.where(face[:, None], fn, vn)) < 0)
    fn = np.where(flip[:, None], -fn, fn)
    gn[k] = fn
    sn[k] = np.where(face[:, None], fn, vn)
    if D.tri_uv is not None:
        T = D.tri_uv[tp]
        uv[k, 0] = ((T[:, 0] * bx).astype(f32) + (T[:, 2] * by).astype(f32)).astype(f32) + (T[:, 4] * bz).astype(f32)
        uv[k, 1] = ((T[:, 1] * bx).astype(f32) + (T[:, 3] * by).astype(f32)).astype(f32) + (T[:, 5] * bz).astype(f32)
    # its.primIndex counts within the triangle's own mesh (skdtree.h:418); elements of a compound shape start over
    local = tp - D.shapes[sh, 4]
    starts = [np.asarray(aov.shape_elems[s]) for s in sh]
    primidx[k] = [loc - st[st <= loc].max() for loc, st in zip(local, starts)]
    elem = np.array([int((st <= loc).sum()) - 1 for loc, st in zip(local, starts)], np.int64)
    # ---- rectangles (rectangle.cpp:155-164): its.p = ray(t), uv = 0.5 (local + 1)
    r = np.nonzero(rec)[0]
    ri = (prim[r] & 0x7FFFFFFF).astype(np.int64)
    p[r] = (o[r] + (d[r] * t[r][:, None]).astype(f32)).astype(f32)
    gn[r] = sn[r] = D.rects[ri, 30:33]
    uv[r, 0] = (f32(0.5) * (u[r] + f32(1)).astype(f32)).astype(f32)
    uv[r, 1] = (f32(0.5) * (v[r] + f32(1)).astype(f32)).astype(f32)
    shape[r] = D.rect_shape[ri]
    elem_all = np.zeros(n, np.int64)
    elem_all[k] = elem
    hit = ~miss
    out["position"][hit] = p[hit]
    m = aov.world_to_camera.astype(f32)
    q = [((m[a, 0] * p[:, 0]).astype(f32) + (m[a, 1] * p[:, 1]).astype(f32)).astype(f32) + (m[a, 2] * p[:, 2]).astype(f32) + m[a, 3]
         for a in range(4)]
    rel = np.stack(q[:3], axis=1).astype(f32)
    assert np.all(q[3][hit] == 1)   # an affine sensor transform: the homogeneous divide is skipped
    out["relPosition"][hit] = rel[hit]
    out["distance"][hit] = t[hit, None]
    out["geoNormal"][hit] = gn[hit]
    out["shNormal"][hit] = sn[hit]
    out["uv"][hit] = np.concatenate([uv, np.zeros((n, 1), f32)], axis=1)[hit]
    si = aov.shape_scene_index[shape]
    out["shapeIndex"][hit] = np.where(si < 0, -1, si + elem_all).astype(f32)[hit, None]
    out["primIndex"][hit] = primidx[hit, None]
    # albedo: its.shape->getBSDF()->getDiffuseReflectance(its); twosided by its.wi.z > 0 (shading frame)
    bs = D.shapes[shape, 1]
    wiz = _dot(sn, (-d).astype(f32))
    alb = np.zeros((n, 3), f32)
    for j in np.nonzero(hit)[0]:
        b = D.bsdfs[bs[j]]
        e = b.back if (b.twosided and not wiz[j] > 0) else bs[j]
        fac = aov.bsdf_factor[e]
        if aov.bsdf_textured[e]:
            alb[j] = (tex_eval(D.bsdfs[e].texture - 1, uv[j:j + 1])[0] * fac).astype(f32)
        else:
            alb[j] = fac
    out["albedo"][hit] = alb[hit]
    return out, miss


def ulps(got, want):
    """|got - want| in units of the last place of each vector's largest component."""
    scale = np.maximum(np.abs(want).max(axis=-1, keepdims=True), np.finfo(f32).tiny).astype(np.float64)
    ulp = 2.0 ** (np.floor(np.log2(scale)) - 23)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp


def film_reference(D, jitter, values, width, height):
    """ImageBlock::put (imageblock.h:153-187) of every sample into the block of
    the whole film + border: float64 sums of float32 filter weights x values,
    and the sums of |w v| for the error bound.  jitter (h, w, spp, 2), values
    (h, w, spp, C)."""
    b = D.border
    ch = values.shape[-1]
    acc = np.zeros((height + 2 * b, width + 2 * b, ch), np.float64)
    mag = np.zeros_like(acc)
    fv, scale, radius = D.filter_values, D.filter_scale, D.filter_radius
    ys, xs = np.mgrid[0:height, 0:width]
    for s in range(values.shape[2]):
        # the sample's position in its 32x32 render block (+ border), as Mitsuba forms it
        ox, oy = (xs & ~31) - b, (ys & ~31) - b
        px = ((xs.astype(f32) + jitter[:, :, s, 0]).astype(f32) - f32(0.5)).astype(f32) - ox.astype(f32)
        py = ((ys.astype(f32) + jitter[:, :, s, 1]).astype(f32) - f32(0.5)).astype(f32) - oy.astype(f32)
        for dy in range(-b, b + 1):
            for dx in range(-b, b + 1):
                cx, cy = (xs + dx - ox).astype(f32), (ys + dy - oy).astype(f32)
                inx = (cx >= np.ceil(px - radius)) & (cx <= np.floor(px + radius))
                iny = (cy >= np.ceil(py - radius)) & (cy <= np.floor(py + radius))
                wx = fv[np.minimum((np.abs((cx - px).astype(f32)) * scale).astype(f32).astype(np.int64), 31)]
                wy = fv[np.minimum((np.abs((cy - py).astype(f32)) * scale).astype(f32).astype(np.int64), 31)]
                w = np.where(inx & iny, (wx * wy).astype(f32), f32(0)).astype(np.float64)
                ty, tx = ys + dy + b, xs + dx + b
                term = w[..., None] * values[:, :, s, :].astype(np.float64)
                np.add.at(acc, (ty, tx), term)
                np.add.at(mag, (ty, tx), np.abs(term))
    return acc, mag
