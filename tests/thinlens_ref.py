"""Helpers of the thinlens sensor tests: the box of direct_ref.box_scene seen
through a thin lens, and a float32 numpy restatement of
ThinLens::sampleRayDifferential (thinlens.cpp:324-361) with
warp::squareToUniformDiskConcentric (warp.cpp:81-102) and the scaling of the
differentials by 1/sqrt(spp) (integrator.cpp:148-149, ray.h:163-168).  Every
step is one correctly rounded float32 operation; sincosf is the C library's,
called per element.  The oracle does not know the sensor: it is asked for
sampler draws, closest hits and shadow rays only."""
import ctypes as C
import functools

import numpy as np

import mtsg
from conftest import SCENES
import direct_ref
from direct_ref import FILM_H, FILM_W, U64, box_geometry, counter_float, counter_key
import multichannel_ref as R
from multichannel_ref import f32, xf

RADIUS, FOCUS = 0.05, 3.4   # the focal plane lies roughly at the cube
PI = f32(3.14159265358979323846)
BOX_TO_WORLD = xf([(-1, 0, 0), (0, 1, 0), (0, 0, -1)], (0.05, 0.1, 3.6))

_libm = C.CDLL("libm.so.6")
_libm.sincosf.restype = None
_libm.sincosf.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]


def sincosf(x):
    s, c = C.c_float(), C.c_float()
    out = np.zeros((len(x), 2), f32)
    for i, v in enumerate(x):
        _libm.sincosf(float(v), C.byref(s), C.byref(c))
        out[i] = s.value, c.value
    return out[:, 0], out[:, 1]


def lens_sensor(radius=RADIUS, focus=FOCUS, to_world=BOX_TO_WORLD, extra=()):
    props = [("fov", "float", 40.0), ("toWorld", "transform", to_world)]
    if radius is not None:
        props.append(("apertureRadius", "float", radius))
    if focus is not None:
        props.append(("focusDistance", "float", focus))
    return props + list(extra)


def lens_props(b, sampler="independent", spp=4, pixel_format="rgba", sampler_props=(), film_props=(), sensor="thinlens", **lens):
    """direct_ref.box_props with the sensor swapped."""
    if sensor == "thinlens":
        b.sensor("thinlens", lens_sensor(**lens))
    else:
        b.sensor("perspective", [("fov", "float", 40.0), ("toWorld", "transform", lens.get("to_world", BOX_TO_WORLD))])
    b.film("hdrfilm", [("width", "integer", FILM_W), ("height", "integer", FILM_H), ("pixelFormat", "string", pixel_format)] + list(film_props),
           "gaussian", [])
    b.sampler(sampler, [("sampleCount", "integer", spp)] + list(sampler_props))


def lens_box_scene(integrator="path", props=(("maxDepth", "integer", 2),), instancing="flatten", textured=False, instanced=False, **kw):
    """direct_ref.box_scene through the thin lens; textured: one more rectangle
    with an EWA-filtered bitmap reflectance, facing the camera; instanced: one
    more mesh, in a shapegroup with one instance."""
    geo = {k: kw.pop(k) for k in ("diffuse_only", "mesh_light") if k in kw}
    b = mtsg.SceneBuilder(SCENES, instancing=instancing)
    b.integrator(integrator, list(props))
    lens_props(b, **kw)
    box_geometry(b, **geo)
    if instanced:
        # a small pyramid in a shapegroup, instanced once with the identity:
        # flattened it is the same world-space triangles
        g = b.group("pyramid")
        pos = np.array([(-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, 1.5, 0)], f32) * f32(0.2) + f32([-0.6, -0.45, 0.5])
        tris = np.array([(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)], np.uint32)
        b.mesh(pos, tris, face_normals=True, bsdf=b.bsdf("diffuse", [("reflectance", "spectrum", (0.2, 0.3, 0.8))]), group=g, name="pyramid")
        b.instance(g, [("toWorld", "transform", np.eye(4, dtype=f32))])
    if textured:
        tex = b.texture("bitmap", [("filename", "string", "tex_checker.png"), ("filterType", "string", "ewa")])
        checker = b.bsdf("diffuse", [("reflectance", "texture", tex)])
        b.shape("rectangle", [("toWorld", "transform", xf([(0.3, 0, 0), (0, 0.3, 0), (0, 0, 1)], (-0.5, -0.1, 0.3)))], checker)
    return b.finish()


def lens_fields_scene(fields, **kw):
    """multichannel over the box: `path` (maxDepth 2) or a field name per child."""
    b = mtsg.SceneBuilder(SCENES)
    for f in fields:
        if f == "path":
            b.integrator_child("path", [("maxDepth", "integer", 2)])
        else:
            b.integrator_child("field", [("field", "string", f), ("undefined", "spectrum", R.UNDEFINED)])
    b.multichannel()
    lens_props(b, pixel_format=", ".join(["rgb"] * len(fields)),
               film_props=[("channelNames", "string", ", ".join(f"c{k}" for k in range(len(fields))))] if len(fields) > 1 else [], **kw)
    box_geometry(b)
    return b.finish()


def plane_scene(z, sensor, focus, radius=RADIUS):
    """One rectangle perpendicular to the optical axis at depth z (the camera
    at the origin looks along +z), with the `position` field."""
    b = mtsg.SceneBuilder(SCENES)
    b.integrator_child("field", [("field", "string", "position"), ("undefined", "spectrum", R.UNDEFINED)])
    b.multichannel()
    lens_props(b, pixel_format="rgb", sensor=sensor, radius=radius, focus=focus, to_world=np.eye(4, dtype=f32))
    light = b.emitter("area", [("radiance", "spectrum", (1.0, 1.0, 1.0))])
    b.shape("rectangle", [("toWorld", "transform", xf([(50, 0, 0), (0, 50, 0), (0, 0, 1)], (0, 0, z)))], -1, light)
    return b.finish()


class Cam:
    """The words of mtsg_camera the restatement reads."""

    def __init__(self, scene):
        d = C.cast(scene.desc, C.POINTER(R.SceneDesc)).contents
        assert d.abi == 8
        c = d.camera
        self.s2c = np.array(list(c.s2c), f32)
        self.c2w = np.array(list(c.c2w), f32)
        self.dx, self.dy = np.array(list(c.dx), f32), np.array(list(c.dy), f32)
        self.near, self.far = f32(c.near_clip), f32(c.far_clip)
        self.inv_res = f32(c.inv_res_x), f32(c.inv_res_y)
        words = np.array(list(c.pad), np.int32)   # the struct's last three words: sensor_type, aperture_radius, focus_distance
        self.sensor_type = int(words[0])
        self.radius, self.focus = words[1:].view(f32)


def _disk(u, v):
    """warp.cpp:81-102."""
    r1 = (f32(2) * u - f32(1)).astype(f32)
    r2 = (f32(2) * v - f32(1)).astype(f32)
    zero = (r1 == 0) & (r2 == 0)
    first = (r1 * r1).astype(f32) > (r2 * r2).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        phi1 = ((PI / f32(4)) * (r2 / r1).astype(f32)).astype(f32)
        phi2 = ((PI / f32(2)) - ((r1 / r2).astype(f32) * (PI / f32(4))).astype(f32)).astype(f32)
    r = np.where(zero, f32(0), np.where(first, r1, r2)).astype(f32)
    phi = np.where(zero, f32(0), np.where(first, phi1, phi2)).astype(f32)
    s, c = sincosf(phi)
    return (r * c).astype(f32), (r * s).astype(f32)


def _near(cam, x, y, a, b):
    """sampleToCamera of the film position (Transform::operator()(Point), transform.h:131-146)."""
    sx = ((x.astype(f32) + a).astype(f32) * cam.inv_res[0]).astype(f32)
    sy = ((y.astype(f32) + b).astype(f32) * cam.inv_res[1]).astype(f32)
    m = cam.s2c
    row = lambda k: (((m[4 * k] * sx).astype(f32) + (m[4 * k + 1] * sy).astype(f32)).astype(f32) + m[4 * k + 3]).astype(f32)
    p = np.stack([row(0), row(1), row(2)], 1)
    w = row(3)
    inv = (f32(1) / w).astype(f32)
    return np.where((w == 1)[:, None], p, (p * inv[:, None]).astype(f32)).astype(f32)


def _to_world_dir(cam, d):
    t = cam.c2w
    return np.stack([(((t[4 * k] * d[:, 0]).astype(f32) + (t[4 * k + 1] * d[:, 1]).astype(f32)).astype(f32)
                      + (t[4 * k + 2] * d[:, 2]).astype(f32)).astype(f32) for k in range(3)], 1)


def _to_world_point(cam, p):
    t = cam.c2w
    return (_to_world_dir(cam, p) + np.array([t[3], t[7], t[11]], f32)[None, :]).astype(f32)


def lens_rays(cam, spp, x, y, jitter, aperture):
    """thinlens.cpp:324-361 for the samples at pixels (x, y): (n, 14) = origin,
    direction, mint, maxt, rx and ry directions scaled by 1/sqrt(spp)."""
    tx, ty = _disk(aperture[:, 0].astype(f32), aperture[:, 1].astype(f32))
    ap = np.stack([(tx * cam.radius).astype(f32), (ty * cam.radius).astype(f32), np.zeros(len(tx), f32)], 1)
    near = _near(cam, np.asarray(x), np.asarray(y), jitter[:, 0].astype(f32), jitter[:, 1].astype(f32))
    fdist = (cam.focus / near[:, 2]).astype(f32)

    def through(p):
        return R._normalize_(((p * fdist[:, None]).astype(f32) - ap).astype(f32))
    d = through(near)
    inv_z = (f32(1) / d[:, 2]).astype(f32)
    o = _to_world_point(cam, ap)
    wd = _to_world_dir(cam, d)
    scale = f32(1) / np.sqrt(f32(spp))
    out = [o, wd, (cam.near * inv_z).astype(f32)[:, None], (cam.far * inv_z).astype(f32)[:, None]]
    for delta in (cam.dx, cam.dy):
        r = _to_world_dir(cam, through((near + delta[None, :]).astype(f32)))
        out.append((wd + ((r - wd).astype(f32) * scale).astype(f32)).astype(f32))
    return np.concatenate(out, 1).astype(f32)


def all_samples(spp, w=FILM_W, h=FILM_H, x0=0, y0=0):
    """(x, y, s) of every sample in the order of mtsg_render_samples."""
    ys, xs, ss = np.meshgrid(np.arange(h) + y0, np.arange(w) + x0, np.arange(spp), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), ss.ravel()], 1).astype(np.int32)


def counter_draws(xys, spp, film_w, dims, seed=0):
    """Draws `dims` of the independent sampler for the samples xys (n, 3)."""
    ids = ((xys[:, 1].astype(U64) * U64(film_w) + xys[:, 0].astype(U64)) * U64(spp) + xys[:, 2].astype(U64)).astype(U64)
    key = counter_key(seed, ids)
    return np.stack([counter_float(key, d) for d in dims], 1)


class LensPrimary(direct_ref.Primary):
    """direct_ref.Primary through the thin lens: the camera rays are the
    restated ones (draws 0-3 of the counter RNG: pixel jitter, aperture sample),
    and the regular draw after the camera's sits at dimensions 4-5.  Sample
    arrays keep their keys."""

    def __init__(self, spp, diffuse_only=False, mesh_light=True):
        from oracle import pyoracle as O
        b = mtsg.SceneBuilder(SCENES)
        b.integrator_child("field", [("field", "string", "position")])
        b.multichannel()
        lens_props(b, spp=spp, pixel_format="rgb")
        box_geometry(b, diffuse_only=diffuse_only, mesh_light=mesh_light)
        self.scene = sc = b.finish()
        self.D = D = R.Desc(sc)
        self.spp = spp
        p = sc.params()
        n = FILM_H * FILM_W * spp
        xys = all_samples(spp)
        self.key = counter_key(0, np.arange(n, dtype=U64))
        # the restated draws are the oracle's: jitter, aperture and the next regular 2D draw of a few samples
        for i in (0, n // 3, n - 1):
            want = O.sampler_draws(sc.desc, p, int(xys[i, 0]), int(xys[i, 1]), int(xys[i, 2]), [2, 2, 2])
            got = np.array([counter_float(self.key[i:i + 1], d)[0] for d in range(6)], f32)
            assert (got.view(np.uint32) == want.view(np.uint32)).all()
        u = np.stack([counter_float(self.key, d) for d in range(4)], 1)
        self.rays14 = lens_rays(Cam(sc), spp, xys[:, 0], xys[:, 1], u[:, 0:2], u[:, 2:4])
        self.rays = rays = np.ascontiguousarray(self.rays14[:, :8])
        t, uu, v, prim = O.trace_closest(sc.desc, rays)
        fields, miss = R.expected_fields(D, sc.aov(), rays, t, uu, v, prim, lambda tex, uv: O.tex_eval(sc.desc, tex, uv))
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
        with np.errstate(invalid="ignore", divide="ignore"):
            self.s = R._normalize((dpdu - direct_ref._v(self.n, R._dot(self.n, dpdu))).astype(f32))
            self.t = R._cross(self.n, self.s)

    def draws(self, n, request=0):
        if n <= 1:
            return np.stack([counter_float(self.key, 4), counter_float(self.key, 5)], -1)[:, None, :]
        return super().draws(n, request)


@functools.lru_cache(maxsize=None)
def lens_primary(spp, diffuse_only=False, mesh_light=True):
    return LensPrimary(spp, diffuse_only, mesh_light)
