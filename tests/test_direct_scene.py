"""The scene side of the `direct` and `ao` integrators (direct.cpp:93-144,
ao.cpp:46-82): property parsing and defaults, the load errors, ao's default
ray length, the render parameters and the mtsg_direct_desc beside the scene
descriptor, both scene routes, and the batch plan's fan factor.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mtsg
import scene_walker as W
from conftest import REPO, SCENES
import direct_ref
from direct_ref import box_geometry, box_props, box_scene
from multichannel_ref import Desc, SceneDesc

XML = """<?xml version="1.0"?>
<scene version="0.5.0">
  <default name="ns" value="3"/>
  <integrator type="{integrator}">{props}</integrator>
  <sensor type="perspective">
    <float name="fov" value="39.3"/>
    <transform name="toWorld"><lookat origin="0.3, 0.2, 3.9" target="0, 0, 0" up="0, 1, 0"/></transform>
    <sampler type="{sampler}"><integer name="sampleCount" value="4"/></sampler>
    <film type="hdrfilm"><integer name="width" value="40"/><integer name="height" value="24"/>
      <rfilter type="gaussian"/></film>
  </sensor>
  <bsdf type="diffuse" id="white"><rgb name="reflectance" value="0.725, 0.71, 0.68"/></bsdf>
  <shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="-90"/><translate y="-1"/></transform>
    <ref id="white"/></shape>
  <shape type="cube"><transform name="toWorld"><scale value="0.3"/><translate x="0.2" y="-0.7"/></transform><ref id="white"/></shape>
  <shape type="rectangle">
    <transform name="toWorld"><scale x="0.23" y="0.19" z="1"/><rotate x="1" angle="90"/><translate y="0.99"/></transform>
    <emitter type="area"><rgb name="radiance" value="17, 12, 4"/></emitter></shape>
</scene>
"""


def write_xml(tmp_path, integrator, props="", sampler="independent", name="s.xml"):
    p = tmp_path / name
    p.write_text(XML.format(integrator=integrator, props=props, sampler=sampler))
    return str(p)


def desc_tuple(d):
    return (d.emitter_samples, d.bsdf_samples, d.ao_samples, d.ao_ray_length)


@pytest.mark.parametrize("props,want,flags", [
    ("", (1, 1), (0, 0)),
    ('<integer name="shadingSamples" value="4"/>', (4, 4), (0, 0)),
    ('<integer name="shadingSamples" value="4"/><integer name="bsdfSamples" value="2"/>', (4, 2), (0, 0)),
    ('<integer name="emitterSamples" value="0"/><integer name="bsdfSamples" value="5"/>', (0, 5), (0, 0)),
    ('<integer name="emitterSamples" value="$ns"/><boolean name="strictNormals" value="true"/>'
     '<boolean name="hideEmitters" value="true"/>', (3, 1), (1, 1)),
])
def test_direct_properties_and_render_params(tmp_path, props, want, flags):
    s = mtsg.Scene(write_xml(tmp_path, "direct", props))
    d = s.direct()
    assert d is not None and desc_tuple(d) == (want[0], want[1], 0, 0.0)
    p = s.params()
    assert p.integrator == mtsg.MTSG_INTEGRATOR_DIRECT == 2
    assert (p.strict_normals, p.hide_emitters) == flags
    assert (p.spp, p.tile_w, p.tile_h) == (4, 40, 24)
    assert s.aov() is None


def test_defines_reach_the_sample_counts(tmp_path):
    s = mtsg.Scene(write_xml(tmp_path, "direct", '<integer name="emitterSamples" value="$ns"/>'), {"ns": "7"})
    assert desc_tuple(s.direct())[:2] == (7, 1)


def test_ao_properties_and_default_ray_length(tmp_path):
    s = mtsg.Scene(write_xml(tmp_path, "ao", '<integer name="shadingSamples" value="4"/><float name="rayLength" value="0.25"/>'))
    assert desc_tuple(s.direct()) == (0, 0, 4, 0.25)
    assert s.params().integrator == mtsg.MTSG_INTEGRATOR_AO == 3
    # the default: half the radius of the bounding sphere of the kd-tree AABB
    # expanded by the sensor position (ao.cpp:77-80, scene.cpp:412-440,
    # aabb.h getBSphere: centre, distance to the maximum corner), in float
    s = mtsg.Scene(write_xml(tmp_path, "ao"))
    d = s.direct()
    assert (d.emitter_samples, d.bsdf_samples, d.ao_samples) == (0, 0, 1)
    sd = C.cast(s.desc, C.POINTER(SceneDesc)).contents
    f32 = np.float32
    cam = np.array(list(sd.camera.c2w), f32).reshape(3, 4)[:, 3]
    np.testing.assert_allclose(cam, [0.3, 0.2, 3.9], rtol=1e-6)
    mn = np.minimum(np.array(list(sd.aabb_min), f32), cam)
    mx = np.maximum(np.array(list(sd.aabb_max), f32), cam)
    centre = ((mn + mx).astype(f32) * f32(0.5)).astype(f32)
    e = (centre - mx).astype(f32)
    radius = np.sqrt(((e[0] * e[0]).astype(f32) + (e[1] * e[1]).astype(f32)).astype(f32) + (e[2] * e[2]).astype(f32)).astype(f32)
    assert d.ao_ray_length == f32(radius * f32(0.5))
    assert 0.5 < d.ao_ray_length < 5
    # a negative value is the default too (ao.cpp:77)
    s2 = mtsg.Scene(write_xml(tmp_path, "ao", '<float name="rayLength" value="-3"/>'))
    assert s2.direct().ao_ray_length == d.ao_ray_length


def test_other_integrators_have_no_descriptor():
    s = mtsg.Scene(os.path.join(SCENES, "cbox.xml"), {"width": 16, "height": 16, "spp": 1})
    assert s.direct() is None and s.params().integrator == 0


def test_load_errors(tmp_path):
    with pytest.raises(RuntimeError, match="emitterSamples.*bsdfSamples.*greater than zero"):
        mtsg.Scene(write_xml(tmp_path, "direct", '<integer name="shadingSamples" value="0"/>'))
    # Mitsuba's wording (hammersley.cpp:297-301)
    msg = "request2DArray\\(\\): Not supported for the Hammersley QMC sequence! If you used this sampler together with the " \
          "'direct' or 'ao' integrators, you will have to set the 'shadingSamples' parameter to 1 to use this sampler."
    with pytest.raises(RuntimeError, match=msg):
        mtsg.Scene(write_xml(tmp_path, "direct", '<integer name="bsdfSamples" value="2"/>', sampler="hammersley"))
    with pytest.raises(RuntimeError, match=msg):
        mtsg.Scene(write_xml(tmp_path, "ao", '<integer name="shadingSamples" value="2"/>', sampler="hammersley"))
    # without an array hammersley loads; the other samplers take arrays
    assert mtsg.Scene(write_xml(tmp_path, "direct", "", sampler="hammersley")).direct() is not None
    for smp in ("independent", "halton", "sobol", "ldsampler"):
        s = mtsg.Scene(write_xml(tmp_path, "ao", '<integer name="shadingSamples" value="3"/>', sampler=smp))
        assert s.direct().ao_samples == 3
    with pytest.raises(RuntimeError, match="outside this build's scope"):
        mtsg.Scene(write_xml(tmp_path, "irrcache"))


@pytest.mark.parametrize("child", ["direct", "ao"])
def test_multichannel_children_stay_rejected(child):
    b = mtsg.SceneBuilder(SCENES)
    with pytest.raises(RuntimeError, match=f'multichannel: child integrator "{child}" is outside this build\'s scope '
                                           "\\(only 'path' and 'field'\\)"):
        b.integrator_child(child, [])


@pytest.mark.parametrize("integrator,props", [
    ("direct", '<integer name="emitterSamples" value="4"/><integer name="bsdfSamples" value="2"/><boolean name="strictNormals" value="true"/>'),
    ("ao", '<integer name="shadingSamples" value="4"/>'),
])
def test_xml_and_builder_routes_are_byte_identical(tmp_path, integrator, props):
    path = write_xml(tmp_path, integrator, props)
    by_xml = mtsg.Scene(path)
    by_builder = W.Walker(path, {}).walk()
    assert by_xml.digest() == by_builder.digest()
    assert bytes(by_xml.direct()) == bytes(by_builder.direct())
    assert bytes(by_xml.params()) == bytes(by_builder.params())


def test_builder_made_scene_and_overrides():
    s = box_scene("direct", [("shadingSamples", "integer", 2), ("hideEmitters", "boolean", True)])
    assert desc_tuple(s.direct()) == (2, 2, 0, 0.0) and s.params().hide_emitters == 1
    s = box_scene("ao", [("shadingSamples", "integer", 4), ("rayLength", "float", 0.5)])
    assert desc_tuple(s.direct()) == (0, 0, 4, 0.5)
    # the plugin's in-memory values: strictNormals / hideEmitters apply to `direct`
    b = mtsg.SceneBuilder(SCENES)
    b.integrator("direct", [("emitterSamples", "integer", 3)])
    box_props(b)
    box_geometry(b)
    ov = mtsg.SceneOverrides()
    ov.mask = 4 | 2   # MTSH_OVERRIDE_INTEGRATOR | MTSH_OVERRIDE_SAMPLE_COUNT
    ov.sample_count, ov.max_depth, ov.rr_depth, ov.strict_normals, ov.hide_emitters = 8, 0, 0, 1, 0   # no depths in `direct`
    s = b.finish(ov)
    p = s.params()
    assert (p.integrator, p.spp, p.strict_normals, p.hide_emitters) == (2, 8, 1, 0)
    assert desc_tuple(s.direct())[:2] == (3, 1)


def test_render_plan_fan_sweep():
    """tools/check_render_plan sweeps the fan factor of direct / ao batches:
    nslots * fan entries per batch, never more than 2^31."""
    exe = os.path.join(REPO, "tools", "check_render_plan")
    subprocess.check_call(["make", "-C", REPO, "tools/check_render_plan"], stdout=subprocess.DEVNULL)
    r = subprocess.run([exe], capture_output=True, text=True, cwd=REPO, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plans ok" in r.stdout


def test_restatements_have_few_fragile_samples():
    """The per-sample references of tests/test_gpu_ao.py and
    tests/test_gpu_direct.py (direct_ref.py), on the CPU alone: a sample is
    fragile when one of its shadow rays changes its oracle answer under a 4-ulp
    move of a direction component; at most 2% of the samples of the chosen
    scenes may be."""
    P = direct_ref.primary(4)
    assert 0.5 < P.hit.mean() < 1
    for n, length in ((1, 0.45), (4, 0.45)):
        value, fragile = direct_ref.ao_reference(P, n, length)
        assert fragile.mean() <= 0.02
        assert (value[P.miss] == 1).all() and 0.5 < value[P.hit].mean() < 1
    Q = direct_ref.primary(4, True, False)
    Li, mag, fragile = direct_ref.emitters_only_reference(Q, 4)
    assert fragile.mean() <= 0.02
    assert (Li.mean(0) > 0.05).all() and (mag >= 0).all()
