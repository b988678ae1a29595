"""The `multichannel` integrator with `path` / `field` children and the
multi-entry `hdrfilm` (reference: src/integrators/misc/multichannel.cpp:87-243,
field.cpp:55-187, src/films/hdrfilm.cpp:216-295), host side: loading through
the XML and the builder routes, the descriptor handed to the device
(mtsg_aov_desc), the develop step (bitmap.cpp:1608-1673) and the EXR writer.
No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import scene_walker as W
from conftest import REPO

HEAD = """<?xml version="1.0"?>
<scene version="0.5.0">
"""
SENSOR = """
  <sensor type="perspective">
    <float name="fov" value="40"/>
    <transform name="toWorld"><lookat origin="0, 0.2, 3.5" target="0, 0, 0" up="0, 1, 0"/></transform>
    <sampler type="{sampler}"><integer name="sampleCount" value="4"/></sampler>
    <film type="hdrfilm"><integer name="width" value="40"/><integer name="height" value="24"/>
      {film}
      <rfilter type="gaussian"/></film>
  </sensor>
"""
CONTENT = """
  <bsdf type="diffuse" id="white"><rgb name="reflectance" value="0.7, 0.6, 0.5"/></bsdf>
  <shape type="rectangle"><transform name="toWorld"><translate z="-1"/></transform><ref id="white"/></shape>
  <shape type="cube"><transform name="toWorld"><scale value="0.3"/></transform><ref id="white"/></shape>
  <shape type="rectangle">
    <transform name="toWorld"><scale x="0.3" y="0.3" z="1"/><rotate x="1" angle="90"/><translate y="0.99"/></transform>
    <emitter type="area"><rgb name="radiance" value="10, 10, 10"/></emitter></shape>
</scene>
"""
# the reference's own example (multichannel.cpp:51-74)
EXAMPLE = """
  <integrator type="multichannel">
    <integrator type="path"/>
    <integrator type="field"><string name="field" value="shNormal"/></integrator>
    <integrator type="field"><string name="field" value="distance"/></integrator>
  </integrator>
"""
EXAMPLE_FILM = """<string name="pixelFormat" value="rgb, rgb, luminance"/>
      <string name="channelNames" value="color, normal, distance"/>"""


def scene_xml(integrator, film, sampler="halton", content=CONTENT):
    return HEAD + integrator + SENSOR.format(sampler=sampler, film=film) + content


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def differing(a, b):
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


class MultiWalker(W.Walker):
    """scene_walker's Mitsuba stand-in, extended by what a plugin does with a
    multichannel integrator: its nested integrators first, then the parent."""

    def props(self, e, key):
        out, nested = super().props(e, key)
        if key == "integrator":
            self._children = nested
        return out, nested

    def call(self, what, *args, **kw):
        if what == "integrator" and args[0] == "multichannel":
            self.log.append("multichannel")
            for c in self._children:
                self.b.integrator_child(self.attr(c, "type"), super().props(c, None)[0])
            return self.b.multichannel(args[1])
        return super().call(what, *args, **kw)


def test_reference_example_scene_loads(tmp_path):
    import mtsg
    s = mtsg.Scene(write(tmp_path, "example.xml", scene_xml(EXAMPLE, EXAMPLE_FILM)))
    a = s.aov()
    assert a is not None and a.m == 3 and a.path_child == 0
    assert a.children == [(mtsg.AOV_PATH, (0.0, 0.0, 0.0)), (mtsg.FIELD_IDS["shNormal"], (0.0, 0.0, 0.0)),
                          (mtsg.FIELD_IDS["distance"], (0.0, 0.0, 0.0))]
    assert [mtsg.FORMAT_NAMES[f] for f in a.formats] == ["rgb", "rgb", "luminance"]
    assert a.channels == ["color.R", "color.G", "color.B", "normal.R", "normal.G", "normal.B", "distance.Y"]
    p = s.params()
    assert (p.max_depth, p.rr_depth, p.spp, p.integrator) == (-1, 5, 4, 0)
    # the plain scene has no descriptor
    assert mtsg.Scene(write(tmp_path, "plain.xml", scene_xml('<integrator type="path"/>', ""))).aov() is None


def test_children_order_undefined_and_path_properties(tmp_path):
    import mtsg
    integ = """
  <integrator type="multichannel">
    <integrator type="field"><string name="field" value="uv"/><spectrum name="undefined" value="-1, 0.5, 7"/></integrator>
    <integrator type="field"><string name="field" value="albedo"/><float name="undefined" value="2.5"/></integrator>
    <integrator type="path"><integer name="maxDepth" value="3"/><integer name="rrDepth" value="2"/></integrator>
    <integrator type="field"><string name="field" value="relPosition"/></integrator>
  </integrator>
"""
    film = '<string name="pixelFormat" value="xyz, rgba, luminanceAlpha, xyza"/><string name="channelNames" value="a, b, c, d"/>'
    a = mtsg.Scene(write(tmp_path, "s.xml", scene_xml(integ, film))).aov()
    assert [c[0] for c in a.children] == [mtsg.FIELD_IDS["uv"], mtsg.FIELD_IDS["albedo"], mtsg.AOV_PATH,
                                          mtsg.FIELD_IDS["relPosition"]]
    assert a.children[0][1] == (-1.0, 0.5, 7.0) and a.children[1][1] == (2.5, 2.5, 2.5)
    assert a.path_child == 2
    assert a.channels == ["a.X", "a.Y", "a.Z", "b.R", "b.G", "b.B", "b.A", "c.Y", "c.A", "d.X", "d.Y", "d.Z", "d.A"]
    s = mtsg.Scene(write(tmp_path, "s.xml", scene_xml(integ, film)))
    assert (s.params().max_depth, s.params().rr_depth) == (3, 2)


def test_scene_arrays_equal_the_plain_path_scene(tmp_path):
    """multichannel changes no array of the scene descriptor; a `uv` field
    adds tri_uv / tri_dpdv (the scene has no texture that would)."""
    import mtsg
    plain = mtsg.Scene(write(tmp_path, "plain.xml", scene_xml('<integrator type="path"/>', ""))).digest()
    multi = mtsg.Scene(write(tmp_path, "multi.xml", scene_xml(EXAMPLE, EXAMPLE_FILM))).digest()
    assert differing(plain, multi) == []
    uv = EXAMPLE.replace("shNormal", "uv")
    with_uv = mtsg.Scene(write(tmp_path, "uv.xml", scene_xml(uv, EXAMPLE_FILM))).digest()
    assert differing(plain, with_uv) == ["tri_dpdv", "tri_uv"]
    assert with_uv["tri_uv"][0] == 12 * 6 * 4   # the cube's 12 triangles


@pytest.mark.parametrize("instancing", ["flatten", "two-level"])
def test_xml_and_builder_routes_agree(tmp_path, instancing):
    import mtsg
    path = shape_index_scene(tmp_path)
    by_xml = mtsg.Scene(path, instancing=instancing)
    walker = MultiWalker(path, instancing=instancing)
    by_builder = walker.walk()
    assert "multichannel" in walker.log
    assert differing(by_xml.digest(), by_builder.digest()) == []
    assert by_xml.aov().to_bytes() == by_builder.aov().to_bytes()
    assert by_xml.aov().channels == by_builder.aov().channels and by_xml.aov().formats == by_builder.aov().formats


@pytest.mark.parametrize("integrator,film,message", [
    (EXAMPLE, '<string name="pixelFormat" value="rgb, rgb"/><string name="channelNames" value="a, b"/>', "pixelFormat"),
    (EXAMPLE.replace("shNormal", "tangent"), EXAMPLE_FILM, "field"),
    (EXAMPLE.replace('type="field"><string name="field" value="shNormal"/>', 'type="path">'), EXAMPLE_FILM, "one 'path'"),
    (EXAMPLE.replace('<integrator type="path"/>', '<integrator type="multichannel"><integrator type="path"/></integrator>'),
     EXAMPLE_FILM, "nested"),
    (EXAMPLE.replace('type="path"', 'type="myPath2_OM"'), EXAMPLE_FILM, "myPath2_OM"),
    ('<integrator type="multichannel">' + '<integrator type="field"><string name="field" value="uv"/></integrator>' * 9 +
     "</integrator>", '<string name="pixelFormat" value="%s"/><string name="channelNames" value="%s"/>' %
     (", ".join(["rgb"] * 9), ", ".join("c%d" % i for i in range(9))), "more than 8"),
    (EXAMPLE, '<string name="pixelFormat" value="rgb, rgb, spectrum"/><string name="channelNames" value="a, b, c"/>',
     "pixelFormat"),
    ('<integrator type="path"/>', EXAMPLE_FILM, "multichannel"),
])
def test_load_errors(tmp_path, integrator, film, message):
    import mtsg
    with pytest.raises(RuntimeError, match=message):
        mtsg.Scene(write(tmp_path, "bad.xml", scene_xml(integrator, film)))


OBJ = """
v -1 -1 0.5
v 1 -1 0.5
v 1 1 0.5
v -1 1 0.5
v 0 0 0.9
g first
f 1 2 3
f 1 3 4
g second
f 1 2 5
f 2 3 5
f 3 4 5
g empty
"""


def shape_index_scene(tmp_path):
    (tmp_path / "two_groups.obj").write_text(OBJ)
    content = """
  <bsdf type="diffuse" id="white"><rgb name="reflectance" value="0.7, 0.6, 0.5"/></bsdf>
  <shape type="obj"><string name="filename" value="two_groups.obj"/>
    <transform name="toWorld"><scale value="0.2"/><translate x="-0.6"/></transform><ref id="white"/></shape>
  <shape type="shapegroup" id="grp">
    <shape type="cube"><transform name="toWorld"><scale value="0.1"/></transform><ref id="white"/></shape>
  </shape>
  <shape type="instance"><ref id="grp"/><transform name="toWorld"><translate x="0.6"/></transform></shape>
  <shape type="rectangle"><transform name="toWorld"><translate z="-1"/></transform><ref id="white"/></shape>
  <shape type="cube"><transform name="toWorld"><scale value="0.2"/></transform><ref id="white"/></shape>
  <shape type="instance"><ref id="grp"/><transform name="toWorld"><translate x="0.6" y="0.5"/></transform></shape>
  <shape type="rectangle">
    <transform name="toWorld"><scale x="0.3" y="0.3" z="1"/><rotate x="1" angle="90"/><translate y="0.99"/></transform>
    <emitter type="area"><rgb name="radiance" value="10, 10, 10"/></emitter></shape>
</scene>
"""
    integ = """
  <integrator type="multichannel">
    <integrator type="field"><string name="field" value="shapeIndex"/></integrator>
    <integrator type="field"><string name="field" value="primIndex"/></integrator>
  </integrator>
"""
    film = '<string name="pixelFormat" value="luminance, luminance"/><string name="channelNames" value="shape, prim"/>'
    return write(tmp_path, "shapes.xml", scene_xml(integ, film, sampler="independent", content=content))


def test_shape_index_table(tmp_path):
    """Scene::m_shapes after initialize (scene.cpp:345-357,608-647): the obj's
    two groups are entries 0 and 1 (its trailing group without faces makes no
    mesh, obj.cpp:616-617), the shapegroup is entry 2, the instance 3, the
    rectangle 4, the cube 5, the second instance 6, the light 7.  Instanced
    geometry reports -1 in both modes."""
    import mtsg
    path = shape_index_scene(tmp_path)
    flat = mtsg.Scene(path, instancing="flatten").aov()
    # shapes: obj, instance copy of the cube, rectangle, cube, second copy, light
    assert flat.shape_scene_index.tolist() == [0, -1, 4, 5, -1, 7]
    assert flat.shape_elems == [[0, 2], [0], [0], [0], [0], [0]]
    two = mtsg.Scene(path, instancing="two-level").aov()
    # shapes: obj, the group's cube, instance, rectangle, cube, instance, light
    assert two.shape_scene_index.tolist() == [0, -1, 3, 4, 5, 6, 7]
    assert two.shape_elems == [[0, 2], [0], [0], [0], [0], [0], [0]]


def test_albedo_records(tmp_path):
    """getDiffuseReflectance per BSDF record: diffuse the reflectance, plastic
    x (1 - fdrExt), roughplastic x Ftr, conductors 0, a textured reflectance
    flagged (its factor multiplies the lookup)."""
    import mtsg
    tex = os.path.join(REPO, "scenes", "tex_checker.png")
    content = f"""
  <bsdf type="diffuse" id="d"><rgb name="reflectance" value="0.7, 0.6, 0.5"/></bsdf>
  <bsdf type="plastic" id="p"><rgb name="diffuseReflectance" value="0.4, 0.5, 0.6"/><float name="intIOR" value="1.5"/>
    <float name="extIOR" value="1"/></bsdf>
  <bsdf type="roughplastic" id="rp"><rgb name="diffuseReflectance" value="0.4, 0.5, 0.6"/><float name="alpha" value="0.2"/>
    <float name="intIOR" value="1.5"/><float name="extIOR" value="1"/></bsdf>
  <bsdf type="roughconductor" id="rc"/>
  <bsdf type="diffuse" id="t"><texture type="bitmap" name="reflectance"><string name="filename" value="{tex}"/></texture></bsdf>
  <bsdf type="twosided" id="ts"><ref id="d"/><ref id="p"/></bsdf>
""" + "".join(f"""
  <shape type="rectangle"><transform name="toWorld"><translate z="{-1 - k}"/></transform><ref id="{b}"/></shape>"""
              for k, b in enumerate(["d", "p", "rp", "rc", "t", "ts"])) + CONTENT
    integ = '<integrator type="multichannel"><integrator type="field"><string name="field" value="albedo"/></integrator></integrator>'
    s = mtsg.Scene(write(tmp_path, "albedo.xml", scene_xml(integ, "", content=content)))
    a = s.aov()
    f, t = a.bsdf_factor, a.bsdf_textured
    assert t[:6].tolist() == [0, 0, 0, 0, 1, 0]
    np.testing.assert_array_equal(f[0], np.float32([0.7, 0.6, 0.5]))
    # fresnelDiffuseReflectance(1.5, false): the quadrature of util.cpp:814-860, here by the midpoint rule in float64
    xi = (np.arange(200000) + 0.5) / 200000
    c = np.sqrt(xi)
    ct = np.sqrt(1 - (1 - c * c) / 1.5 ** 2)
    rs, rp = (c - 1.5 * ct) / (c + 1.5 * ct), (1.5 * c - ct) / (1.5 * c + ct)
    fdr = float(np.mean(0.5 * (rs * rs + rp * rp)))
    np.testing.assert_allclose(f[1], np.float32([0.4, 0.5, 0.6]) * np.float32(1 - fdr), rtol=2e-6)
    # roughplastic: Ftr = the external rough transmittance's diffuse value
    trans = np.zeros(8, np.float32)
    ftr = mtsg.C.c_float()
    assert mtsg.host_lib().mtsh_rough_transmittance(0, mtsg.C.c_float(0.2), mtsg.C.c_float(1.5), 8, mtsg._ptr(trans),
                                                    mtsg.C.byref(ftr)) == 0
    np.testing.assert_array_equal(f[2], np.float32([0.4, 0.5, 0.6]) * np.float32(ftr.value))
    assert 0.5 < ftr.value < 1.0
    np.testing.assert_array_equal(f[3], np.float32([0, 0, 0]))
    np.testing.assert_array_equal(f[4], np.float32([1, 1, 1]))
    np.testing.assert_array_equal(f[5], f[0])   # the twosided front record is its first nested BSDF's
    # a textured albedo needs the per-triangle texture records
    assert "tri_uv" in s.digest() and s.digest()["tri_uv"][0] > 0


def develop_reference(block, formats):
    """Bitmap::convertMultiSpectrumAlphaWeight (bitmap.cpp:1617-1672) in float32."""
    f32 = np.float32
    m = len(formats)
    w = block[..., -1]
    inv = np.where(w == 0, f32(0), f32(1) / np.where(w == 0, f32(1), w)).astype(f32)
    alpha = (block[..., -2] * inv).astype(f32)
    out = []
    for i, fmt in enumerate(formats):
        r, g, b = [(block[..., 3 * i + c] * inv).astype(f32) for c in range(3)]
        lum = ((r * f32(0.212671)).astype(f32) + (g * f32(0.715160)).astype(f32)).astype(f32)
        lum = (lum + (b * f32(0.072169)).astype(f32)).astype(f32)
        if fmt.startswith("luminance"):
            out.append(lum)
        elif fmt.startswith("xyz"):
            x = ((r * f32(0.412453)).astype(f32) + (g * f32(0.357580)).astype(f32)).astype(f32)
            x = (x + (b * f32(0.180423)).astype(f32)).astype(f32)
            z = ((r * f32(0.019334)).astype(f32) + (g * f32(0.119193)).astype(f32)).astype(f32)
            z = (z + (b * f32(0.950227)).astype(f32)).astype(f32)
            out += [x, lum, z]
        else:
            out += [r, g, b]
        if fmt in ("luminanceAlpha", "rgba", "xyza"):
            out.append(alpha)
    return np.stack(out, axis=-1)


def test_develop_multi_matches_the_reference_formula():
    import mtsg
    rng = np.random.default_rng(5)
    formats = ["rgb", "luminance", "luminanceAlpha", "rgba", "xyz", "xyza"]
    block = rng.normal(0, 3, (7, 9, 3 * len(formats) + 2)).astype(np.float32)   # fields may be negative
    block[..., -1] = rng.uniform(0.5, 4, (7, 9)).astype(np.float32)
    block[..., -2] = block[..., -1] * rng.uniform(0, 1, (7, 9)).astype(np.float32)
    block[2, 3, -1] = 0.0          # zero-weight texels develop to 0, whatever they hold
    block[0, 0, :] = 0.0
    block[4, 4, 0] = np.inf        # nothing is rejected
    with np.errstate(invalid="ignore", over="ignore"):
        want = develop_reference(block, formats)
    got = mtsg.develop_multi(block, formats)
    assert got.shape == (7, 9, 3 + 1 + 2 + 4 + 3 + 4)
    np.testing.assert_array_equal(got, want)
    assert np.all(got[2, 3] == 0) and np.all(got[0, 0] == 0) and np.isinf(got[4, 4, 0])
    with pytest.raises(ValueError):
        mtsg.develop_multi(block, formats[:-1])


def read_exr(path):
    """Header and scanlines of an uncompressed scanline OpenEXR file."""
    d = open(path, "rb").read()
    assert struct.unpack_from("<II", d, 0) == (20000630, 2)
    o, attrs = 8, {}

    def cstr(o):
        e = d.index(b"\0", o)
        return d[o:e].decode(), e + 1
    while d[o] != 0:
        name, o = cstr(o)
        typ, o = cstr(o)
        size, = struct.unpack_from("<i", d, o)
        attrs[name] = (typ, d[o + 4:o + 4 + size])
        o += 4 + size
    o += 1
    chans, c, q = [], attrs["channels"][1], 0
    while c[q] != 0:
        e = c.index(b"\0", q)
        ptype, _lin, xs, ys = struct.unpack_from("<iIii", c, e + 1)
        chans.append((c[q:e].decode(), ptype, xs, ys))
        q = e + 17
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    offsets = struct.unpack_from("<%dQ" % h, d, o)
    planes = {n: np.zeros((h, w), np.float32) for n, *_ in chans}
    for y in range(h):
        yy, size = struct.unpack_from("<ii", d, offsets[y])
        assert yy == y and size == 4 * w * len(chans)
        row = np.frombuffer(d, "<f4", w * len(chans), offsets[y] + 8).reshape(len(chans), w)
        for k, (n, *_r) in enumerate(chans):
            planes[n][y] = row[k]
    assert offsets[-1] + 8 + 4 * w * len(chans) == len(d)
    return attrs, chans, planes


def test_write_exr_round_trip(tmp_path):
    import mtsg
    names = ["color.R", "color.G", "color.B", "normal.R", "normal.G", "normal.B", "distance.Y", "A"]
    rng = np.random.default_rng(9)
    img = rng.normal(0, 2, (5, 7, len(names))).astype(np.float32)
    img[1, 2, 3] = -np.inf
    path = str(tmp_path / "out.exr")
    mtsg.write_exr(path, img, names)
    attrs, chans, planes = read_exr(path)
    assert [c[0] for c in chans] == sorted(names)          # the format stores channels by name
    assert all(c[1:] == (2, 1, 1) for c in chans)          # FLOAT, no subsampling
    assert attrs["compression"] == ("compression", b"\0") and attrs["lineOrder"] == ("lineOrder", b"\0")
    assert attrs["displayWindow"][1] == attrs["dataWindow"][1] == struct.pack("<4i", 0, 0, 6, 4)
    for k, n in enumerate(names):
        np.testing.assert_array_equal(planes[n], img[..., k])
    # the scene loader's own reader takes the file (R, G, B by name)
    assert mtsg.read_image(path).shape == (5, 7, 3)
    with pytest.raises(RuntimeError):
        mtsg.write_exr(path, img[..., :2], ["same", "same"])


def test_host_program_under_sanitizers(tmp_path):
    """tools/check_multichannel_host.cpp: load, descriptor, develop, write -- a
    stand-alone program that the Makefile builds with ASan + UBSan together
    with the host sources (`make` builds it; current = a no-op here)."""
    exe = os.path.join(REPO, "tools", "check_multichannel_host")
    subprocess.check_call(["make", "-C", REPO, "tools/check_multichannel_host"], stdout=subprocess.DEVNULL)
    xml = write(tmp_path, "example.xml", scene_xml(EXAMPLE, EXAMPLE_FILM))
    out = str(tmp_path / "host.exr")
    r = subprocess.run([exe, xml, out], capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    _attrs, chans, planes = read_exr(out)
    assert [c[0] for c in chans] == sorted(["color.R", "color.G", "color.B", "normal.R", "normal.G", "normal.B", "distance.Y"])
    assert planes["distance.Y"].shape == (24, 40)
