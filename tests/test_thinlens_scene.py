"""The thinlens sensor and the focalLength property on the host (builder.cpp
SceneBuilder::sensor, build.cpp; thinlens.cpp:122-143, sensor.cpp:156-278):
the XML and the builder route, defaults and error messages, the descriptor
words, and the descriptors of the perspective test scenes, which must not move.
No GPU."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import mtsg
import scene_walker as W
from conftest import GOLDEN, SCENES
import direct_ref
import thinlens_ref as T
from multichannel_ref import f32

SMALL = {"width": 40, "height": 24, "spp": 4}
_libm = C.CDLL("libm.so.6")
_libm.atanf.restype = C.c_float
_libm.atanf.argtypes = [C.c_float]


def lens_xml(tmp_path, radius="0.05", focus="3.4", name="lens.xml"):
    """cbox.xml seen through a thin lens."""
    xml = open(os.path.join(SCENES, "cbox.xml")).read()
    lens = '<sensor type="thinlens">'
    if radius is not None:
        lens += f'<float name="apertureRadius" value="{radius}"/>'
    if focus is not None:
        lens += f'<float name="focusDistance" value="{focus}"/>'
    assert xml.count('<sensor type="perspective">') == 1
    p = tmp_path / name
    p.write_text(xml.replace('<sensor type="perspective">', lens))
    return str(p)


def small_xml(tmp_path, sensor, integrator="path", name="s.xml"):
    p = tmp_path / name
    p.write_text(f"""<?xml version="1.0"?>
<scene version="0.5.0">
  <integrator type="{integrator}"/>
  {sensor}
  <shape type="rectangle"><emitter type="area"><rgb name="radiance" value="1, 1, 1"/></emitter></shape>
</scene>""")
    return str(p)


def sensor_xml(kind, body):
    return (f'<sensor type="{kind}">{body}<film type="hdrfilm"><integer name="width" value="40"/>'
            '<integer name="height" value="24"/></film></sensor>')


def differing(a, b):
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


def test_xml_and_builder_routes_agree(tmp_path):
    path = lens_xml(tmp_path)
    by_xml = mtsg.Scene(path, SMALL)
    by_builder = W.Walker(path, SMALL).walk()
    assert differing(by_xml.digest(), by_builder.digest()) == []
    cam = T.Cam(by_xml)
    assert cam.sensor_type == 1 and cam.radius == f32(0.05) and cam.focus == f32(3.4)
    # the two lens words reach the digest, and only the scalar part of the descriptor moves
    base = by_xml.digest()
    for k, (r, f) in enumerate((("0.06", "3.4"), ("0.05", "3.5"))):
        other = mtsg.Scene(lens_xml(tmp_path, r, f, f"l{k}.xml"), SMALL).digest()
        moved = differing(base, other)
        assert len(moved) == 1, moved
    # the same box through the pinhole differs in the sensor words only
    pin = mtsg.Scene(os.path.join(SCENES, "cbox.xml"), SMALL)
    assert differing(base, pin.digest()) == moved
    pc, lc = T.Cam(pin), cam
    assert pc.sensor_type == 0 and pc.radius == 0 and pc.focus == 0
    assert (pc.s2c == lc.s2c).all() and (pc.c2w == lc.c2w).all() and (pc.dx == lc.dx).all() and (pc.dy == lc.dy).all()


def test_defaults_and_errors(tmp_path):
    # focusDistance defaults to farClip (sensor.cpp:162), a zero radius becomes Epsilon (thinlens.cpp:134-138)
    cam = T.Cam(mtsg.Scene(lens_xml(tmp_path, "0", None), SMALL))
    assert cam.sensor_type == 1 and cam.radius == f32(1e-4) and cam.focus == f32(1e4)
    sc = mtsg.Scene(small_xml(tmp_path, sensor_xml("thinlens", '<float name="apertureRadius" value="0.1"/><float name="farClip" value="50"/>')))
    assert T.Cam(sc).focus == f32(50)
    with pytest.raises(RuntimeError, match='Property "apertureRadius" has not been specified!'):
        mtsg.Scene(lens_xml(tmp_path, None, "3.4"), SMALL)
    b = mtsg.SceneBuilder(SCENES)
    with pytest.raises(RuntimeError, match='Property "apertureRadius" has not been specified!'):
        b.sensor("thinlens", T.lens_sensor(radius=None))
    scaled = np.eye(4, dtype=f32)
    scaled[0, 0] = 2
    with pytest.raises(RuntimeError, match="Scale factors in the camera-to-world transformation are not allowed!"):
        b.sensor("thinlens", T.lens_sensor(to_world=scaled))
    b.sensor("perspective", [("toWorld", "transform", scaled)])   # the pinhole takes it (perspective.cpp has no such check)
    with pytest.raises(RuntimeError, match="Scale factors in the camera-to-world transformation are not allowed!"):
        mtsg.Scene(small_xml(tmp_path, sensor_xml("thinlens", '<float name="apertureRadius" value="0.1"/>'
                                                  '<transform name="toWorld"><scale x="2"/></transform>')))
    with pytest.raises(RuntimeError, match="myPath2_OM: the thinlens sensor is outside this build's scope"):
        mtsg.Scene(small_xml(tmp_path, sensor_xml("thinlens", '<float name="apertureRadius" value="0.1"/>'), integrator="myPath2_OM"))
    for kind, extra in (("perspective", ""), ("thinlens", '<float name="apertureRadius" value="0.1"/>')):
        with pytest.raises(RuntimeError, match=r"Please specify either a focal length \('focalLength'\) or a field of view \('fov'\)!"):
            mtsg.Scene(small_xml(tmp_path, sensor_xml(kind, extra + '<float name="fov" value="40"/><string name="focalLength" value="35mm"/>')))
        with pytest.raises(RuntimeError, match=r"Could not parse the focal length \(must be of the form <x>mm, where <x> is a positive integer\)!"):
            mtsg.Scene(small_xml(tmp_path, sensor_xml(kind, extra + '<string name="focalLength" value="35cm"/>')))
        with pytest.raises(RuntimeError, match="The 'fovAxis' parameter must be set to one of 'smaller', 'larger', 'diagonal', 'x', or 'y'!"):
            mtsg.Scene(small_xml(tmp_path, sensor_xml(kind, extra + '<float name="fov" value="40"/><string name="fovAxis" value="z"/>')))
        for axis in ("x", "y", "diagonal", "smaller", "larger", "Diagonal"):
            mtsg.Scene(small_xml(tmp_path, sensor_xml(kind, extra + f'<float name="fov" value="40"/><string name="fovAxis" value="{axis}"/>')))
    with pytest.raises(RuntimeError, match="outside this build's scope"):
        mtsg.Scene(small_xml(tmp_path, sensor_xml("orthographic", "")))


def focal_fov(mm):
    """sensor.cpp:276 as this build reads it: the float sqrt, quotient and
    atan, the double 2 * 180 / M_PI, rounded to float on entry to setDiagonalFov."""
    value = f32(mm)
    q = f32(np.sqrt(f32(36 * 36 + 24 * 24)) / f32(f32(2) * value))
    return float(f32(2 * 180 / math.pi * float(_libm.atanf(float(q)))))


@pytest.mark.parametrize("kind,extra", [("perspective", ""), ("thinlens", '<float name="apertureRadius" value="0.1"/>')])
def test_focal_length(tmp_path, kind, extra):
    def s2c(body, name):
        sc = mtsg.Scene(small_xml(tmp_path, sensor_xml(kind, extra + body), name=name))
        return T.Cam(sc).s2c.view(np.uint32)
    default = s2c("", "a.xml")
    assert (default == s2c('<string name="focalLength" value="50mm"/>', "b.xml")).all()
    mm35 = s2c('<string name="focalLength" value="35mm"/>', "c.xml")
    assert (mm35 == s2c('<string name="focalLength" value="35"/>', "d.xml")).all()
    assert (mm35 != default).any()
    for mm, got in ((50, default), (35, mm35)):
        want = s2c(f'<float name="fov" value="{focal_fov(mm)!r}"/><string name="fovAxis" value="diagonal"/>', f"e{mm}.xml")
        assert (got == want).all(), (mm, focal_fov(mm))
    # fovAxis is not read without fov (sensor.cpp:244-265)
    assert (mm35 == s2c('<string name="focalLength" value="35mm"/><string name="fovAxis" value="y"/>', "f.xml")).all()


def test_perspective_scenes_are_untouched():
    """The descriptors of the perspective test scenes are those the parent
    commit's host library built (names and FNV-1a digests, recorded from it)."""
    want = json.load(open(os.path.join(GOLDEN, "thinlens_parent_digests.json")))
    scenes = {"box": direct_ref.box_scene()}
    for n in ("cbox", "env_glass"):
        scenes[n] = mtsg.Scene(os.path.join(SCENES, n + ".xml"), dict(SMALL, envmap=os.path.join(SCENES, "sky512.pfm")))
    assert sorted(want) == sorted(scenes)
    for name, sc in scenes.items():
        got = {k: "%016x" % h for k, (_b, h) in sc.digest().items()}
        assert got == want[name], (name, differing(got, want[name]))
        assert T.Cam(sc).sensor_type == 0


def test_restatements_have_few_fragile_samples():
    """The share of fragile samples (a shadow ray whose oracle answer changes
    under a 4-ulp move of a direction component) of the references the GPU tests
    compare with, on the box through the lens: at most 1%."""
    P = T.lens_primary(4)
    assert P.hit.mean() > 0.5 and P.miss.any()
    for n in (1, 4):
        _value, fragile = direct_ref.ao_reference(P, n, 0.45)
        assert fragile.mean() <= 0.01, ("ao", n, fragile.mean())
    Q = T.lens_primary(4, True, False)
    for ne in (1, 4):
        _li, mag, fragile = direct_ref.emitters_only_reference(Q, ne)
        assert fragile.mean() <= 0.01, ("direct", ne, fragile.mean())
        assert (mag.sum(1) > 0).mean() > 0.3
