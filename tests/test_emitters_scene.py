"""The scene side of the point / spot / directional / constant emitters
(src/emitters/point.cpp, spot.cpp, directional.cpp, constant.cpp): property
parsing and defaults on both scene routes, the descriptor's records, the
reference's load errors, the bounding spheres, the identity of the two routes,
and the fragile-sample share of the GPU tests' restatement.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import mtsg
import scene_walker as W
from conftest import SCENES
import emitter_ref as E
from emitter_ref import AREA, CONSTANT, DIRECTIONAL, POINT, SPOT, emitter_records
from direct_ref import box_props
from multichannel_ref import SceneDesc

f32 = np.float32

XML = """<?xml version="1.0"?>
<scene version="0.5.0">
  <integrator type="{integrator}"/>
  <sensor type="perspective">
    <float name="fov" value="39.3"/>
    <transform name="toWorld"><lookat origin="0.3, 0.2, 3.9" target="0, 0, 0" up="0, 1, 0"/></transform>
    <sampler type="independent"><integer name="sampleCount" value="4"/></sampler>
    <film type="hdrfilm"><integer name="width" value="40"/><integer name="height" value="24"/>
      <rfilter type="gaussian"/></film>
  </sensor>
  <bsdf type="diffuse" id="white"><rgb name="reflectance" value="0.725, 0.71, 0.68"/></bsdf>
  <shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="-90"/><translate y="-1"/></transform>
    <ref id="white"/></shape>
  {shapes}
  {emitters}
</scene>
"""
CUBE = '<shape type="cube"><transform name="toWorld"><scale value="0.3"/><translate x="0.2" y="-0.7"/></transform><ref id="white"/></shape>'
GROUP = ('<shape type="shapegroup" id="g"><shape type="cube"><transform name="toWorld"><scale value="0.3"/></transform>'
         '<ref id="white"/></shape></shape>'
         '<shape type="instance"><ref id="g"/><transform name="toWorld"><translate x="0.2" y="-0.7"/></transform></shape>'
         '<shape type="instance"><ref id="g"/><transform name="toWorld"><translate x="-0.7" y="-0.7" z="-0.5"/></transform></shape>')
AREA_LIGHT = ('<shape type="rectangle"><transform name="toWorld"><scale x="0.23" y="0.19" z="1"/><rotate x="1" angle="90"/>'
              '<translate y="0.99"/></transform><emitter type="area"><rgb name="radiance" value="17, 12, 4"/>'
              '<float name="samplingWeight" value="3"/></emitter></shape>')
FOUR = """
  <emitter type="point"><point name="position" x="0.4" y="0.8" z="1.5"/><rgb name="intensity" value="3, 4, 5"/>
    <float name="samplingWeight" value="0.5"/></emitter>
  <emitter type="spot"><transform name="toWorld"><lookat origin="-0.5, 0.9, 0.5" target="0, -1, 0" up="0, 0, 1"/></transform>
    <rgb name="intensity" value="20, 22, 25"/><float name="cutoffAngle" value="30"/><float name="beamWidth" value="10"/>
    <spectrum name="texture" value="0.5"/><float name="samplingWeight" value="2"/></emitter>
  <emitter type="directional"><vector name="direction" x="-0.3" y="-1" z="-0.4"/><spectrum name="irradiance" value="2, 2.5, 3"/>
    <float name="samplingWeight" value="1.5"/></emitter>
  <emitter type="constant"><rgb name="radiance" value="0.8, 0.9, 1"/><float name="samplingWeight" value="0.7"/></emitter>
"""


def write_xml(tmp_path, emitters, shapes=CUBE, integrator="path", name="s.xml"):
    p = tmp_path / name
    p.write_text(XML.format(integrator=integrator, shapes=shapes, emitters=emitters))
    return str(p)


def builder(emitters, integrator="path"):
    b = mtsg.SceneBuilder(SCENES)
    b.integrator(integrator, [])
    box_props(b)
    E.diffuse_box(b)
    for plugin, props in emitters:
        b.emitter(plugin, props)
    return b


def header(scene):
    return C.cast(scene.desc, C.POINTER(SceneDesc)).contents


def tree_sphere(sd, with_sensor):
    """AABB::getBSphere (aabb.cpp:44-47) of the kd-tree's box, expanded by the sensor or not, in float32."""
    mn, mx = np.array(list(sd.aabb_min), f32), np.array(list(sd.aabb_max), f32)
    if with_sensor:
        cam = np.array(list(sd.camera.c2w), f32).reshape(3, 4)[:, 3]
        mn, mx = np.minimum(mn, cam), np.maximum(mx, cam)
    return sphere_of(mn, mx)


def sphere_of(mn, mx):
    centre = ((mn + mx).astype(f32) * f32(0.5)).astype(f32)
    e = (centre - mx).astype(f32)
    return centre, np.sqrt(((e[0] * e[0]).astype(f32) + (e[1] * e[1]).astype(f32)).astype(f32) + (e[2] * e[2]).astype(f32)).astype(f32)


def deg(v):   # degToRad (util.h:297)
    return f32(float(f32(v)) * (math.pi / 180.0))


def test_defaults_through_both_routes(tmp_path):
    xml = "".join(f'<emitter type="{k}"/>' for k in ("point", "spot", "directional", "constant"))
    by_xml = mtsg.Scene(write_xml(tmp_path, xml))
    by_builder = builder([(k, []) for k in ("point", "spot", "directional", "constant")]).finish()
    for scene in (by_xml, by_builder):
        ems, ext, cdf = emitter_records(scene)
        assert [e.type for e in ems] == [POINT, SPOT, DIRECTIONAL, CONSTANT]
        for e in ems:
            assert list(e.radiance) == [1, 1, 1] and e.shape == -1 and e.pdf_discrete == f32(0.25)
        assert list(cdf) == [0, 0.25, 0.5, 0.75, 1]
        assert list(ext[0].position) == [0, 0, 0] and list(ext[1].position) == [0, 0, 0]
        # spot: cutoffAngle 20, beamWidth 3/4 of it, configure() in float (spot.cpp:73-93)
        cut, beam = deg(20), deg(f32(20) * f32(3) / f32(4))
        assert ext[1].cutoff_angle == cut
        assert ext[1].cos_cutoff_angle == f32(math.cos(cut)) and ext[1].cos_beam_width == f32(math.cos(beam))
        assert ext[1].inv_transition_width == f32(1) / f32(cut - beam)
        assert list(ext[1].to_local) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
        assert list(ext[2].direction) == [0, 0, 1]


def test_every_property_and_the_descriptor(tmp_path):
    """point + spot + directional + constant + one area light at unequal
    sampling weights: type, constants, spheres and pdf_discrete."""
    scene = mtsg.Scene(write_xml(tmp_path, FOUR, shapes=CUBE + AREA_LIGHT))
    sd = header(scene)
    ems, ext, cdf = emitter_records(scene)
    assert [e.type for e in ems] == [AREA, POINT, SPOT, DIRECTIONAL, CONSTANT]
    weights = np.array([3, 0.5, 2, 1.5, 0.7], f32)
    total = f32(0)
    for w in weights:
        total = f32(total + w)
    norm = f32(1) / total
    assert [e.pdf_discrete for e in ems] == [f32(w * norm) for w in weights]
    assert cdf[0] == 0 and cdf[-1] == 1 and (np.diff(cdf) > 0).all()
    assert list(ems[1].radiance) == [3, 4, 5] and list(ext[1].position) == [f32(0.4), f32(0.8), f32(1.5)]
    assert list(ems[2].radiance) == [20, 22, 25] and list(ext[2].position) == [f32(-0.5), f32(0.9), f32(0.5)]
    assert ext[2].cutoff_angle == deg(30) and ext[2].cos_beam_width == f32(math.cos(deg(10)))
    assert ext[2].inv_transition_width == f32(1) / f32(deg(30) - deg(10))
    # the spot's local z axis is the lookat direction: toWorld^-1 maps it to (0, 0, 1)
    look = np.array([0.5, -1.9, -0.5]) / np.linalg.norm([0.5, -1.9, -0.5])
    rot = np.array(list(ext[2].to_local)).reshape(3, 3)
    np.testing.assert_allclose(rot @ look, [0, 0, 1], atol=1e-6)
    np.testing.assert_allclose(rot @ rot.T, np.eye(3), atol=1e-6)
    # directional: the frame of directional.cpp:62-68 looks along the normalised direction
    want = np.array([-0.3, -1, -0.4]) / np.linalg.norm([-0.3, -1, -0.4])
    np.testing.assert_allclose(list(ext[3].direction), want, atol=1e-6)
    assert list(ems[3].radiance) == [2, 2.5, 3]
    # its sphere: the kd-tree box's, radius x 1.1 (directional.cpp:88-93)
    centre, radius = tree_sphere(sd, False)
    assert list(ext[3].bsphere_center) == list(centre) and ext[3].bsphere_radius == f32(radius * f32(1.1))
    # constant: the sphere of the tree's box expanded by the sensor, x 1.5 (constant.cpp:67-71)
    centre, radius = tree_sphere(sd, True)
    assert list(ext[4].bsphere_center) == list(centre) and ext[4].bsphere_radius == f32(radius * f32(1.5))
    assert [round(v, 6) for v in ems[4].radiance] == [0.8, 0.9, 1.0]
    # scenes without such an emitter carry no extension records
    assert emitter_records(mtsg.Scene(write_xml(tmp_path, "", shapes=CUBE + AREA_LIGHT)))[1] is None


def test_position_and_direction_against_toworld():
    pos = builder([("point", [("position", "point", (1, 2, 3))])]).finish()
    m = np.eye(4, dtype=f32)
    m[:3, 3] = (1, 2, 3)
    tw = builder([("point", [("toWorld", "transform", m)])]).finish()
    assert list(emitter_records(pos)[1][0].position) == list(emitter_records(tw)[1][0].position) == [1, 2, 3]
    rot = E.xf([(0, 0, 1), (0, 1, 0), (-1, 0, 0)], (0, 0, 0))   # local z -> world -x
    d = emitter_records(builder([("directional", [("toWorld", "transform", rot)])]).finish())[1][0]
    assert list(d.direction) == [-1, 0, 0]


def test_the_references_errors(tmp_path):
    m = np.eye(4, dtype=f32)
    with pytest.raises(RuntimeError, match="Only one of the parameters 'position' and 'toWorld' can be used!"):
        builder([("point", [("position", "point", (1, 2, 3)), ("toWorld", "transform", m)])])
    with pytest.raises(RuntimeError, match="Only one of the parameters 'direction' and 'toWorld'"):
        builder([("directional", [("direction", "vector", (0, -1, 0)), ("toWorld", "transform", m)])])
    with pytest.raises(RuntimeError, match="Scale factors in the emitter-to-world transformation are not allowed!"):
        builder([("directional", [("toWorld", "transform", m * f32(2))])])
    with pytest.raises(RuntimeError, match="only one environment emitter"):
        builder([("constant", []), ("envmap", [("filename", "string", "sky512.pfm")])])
    with pytest.raises(RuntimeError, match="only one environment emitter"):
        builder([("envmap", [("filename", "string", "sky512.pfm")]), ("constant", [])])
    with pytest.raises(RuntimeError, match="only one environment emitter"):
        builder([("constant", []), ("constant", [])])
    with pytest.raises(RuntimeError, match="spot: a nested <texture> is outside this build's scope"):
        mtsg.Scene(write_xml(tmp_path, '<emitter type="spot"><texture name="texture" type="bitmap">'
                                       '<string name="filename" value="tex_checker.png"/></texture></emitter>'))
    b = mtsg.SceneBuilder(SCENES)
    tex = b.texture("bitmap", [("filename", "string", "tex_checker.png")])
    with pytest.raises(RuntimeError, match="spot: a nested <texture> is outside this build's scope"):
        b.emitter("spot", [("texture", "texture", tex)])
    # a shape's emitter stays an area light, on both routes
    with pytest.raises(RuntimeError, match="a shape's emitter must be an 'area' emitter"):
        mtsg.Scene(write_xml(tmp_path, "", shapes='<shape type="cube"><emitter type="point"/></shape>'))
    b = builder([])
    pt = b.emitter("point", [])
    with pytest.raises(RuntimeError, match="a shape's emitter must be an 'area' emitter"):
        b.shape("cube", [], -1, pt)
    with pytest.raises(RuntimeError, match="myPath2_OM: point, spot, directional and constant emitters are outside"):
        mtsg.Scene(write_xml(tmp_path, '<emitter type="point"/>', integrator="myPath2_OM"))
    # still no emitter at all, and still no sun / sky
    with pytest.raises(RuntimeError, match="scene has no emitters"):
        mtsg.Scene(write_xml(tmp_path, ""))
    with pytest.raises(RuntimeError, match="outside this build's scope"):
        mtsg.Scene(write_xml(tmp_path, '<emitter type="sunsky"/>'))


def test_scene_bounding_spheres_with_a_far_point_light(tmp_path):
    """Scene::initializeBidirectional (scene.cpp:410-440) resets m_aabb to the
    kd-tree's box expanded by the sensor before it calls the emitters'
    createShape, and adds their getAABB() to it only after the loop.  So the
    sphere a constant or envmap emitter takes from scene->getAABB() does not see
    a point light, however far away, while Scene::getBSphere() afterwards
    (ao's default ray length, ao.cpp:77-80) does.  Both values by hand."""
    far = '<emitter type="point"><point name="position" x="40" y="3" z="-2"/></emitter>'
    for env in ('<emitter type="constant"/>', '<emitter type="envmap"><string name="filename" value="{}/sky512.pfm"/></emitter>'.format(SCENES)):
        scene = mtsg.Scene(write_xml(tmp_path, env + far))
        sd = header(scene)
        centre, radius = tree_sphere(sd, True)
        if "constant" in env:
            x = emitter_records(scene)[1][0]
            got = list(x.bsphere_center), x.bsphere_radius
        else:
            words = np.array(list(sd.envmap), np.uint32).view(f32)   # mtsg_envmap: mip (192 words), scale, to_world, to_local, sphere
            got = list(words[211:214]), words[214]
        assert got[0] == list(centre) and got[1] == f32(radius * f32(1.5))
    ao = mtsg.Scene(write_xml(tmp_path, '<emitter type="constant"/>' + far, integrator="ao"))
    sd = header(ao)
    cam = np.array(list(sd.camera.c2w), f32).reshape(3, 4)[:, 3]
    pts = [cam, np.array([40, 3, -2], f32), tree_sphere(sd, True)[0]]   # sensor, point light, the constant emitter's centre
    mn, mx = np.array(list(sd.aabb_min), f32), np.array(list(sd.aabb_max), f32)
    for p in pts:
        mn, mx = np.minimum(mn, p), np.maximum(mx, p)
    assert ao.direct().ao_ray_length == f32(sphere_of(mn, mx)[1] * f32(0.5))
    near = mtsg.Scene(write_xml(tmp_path, '<emitter type="constant"/>', integrator="ao"))
    assert ao.direct().ao_ray_length > 4 * near.direct().ao_ray_length


@pytest.mark.parametrize("instancing", ["flatten", "two-level"])
def test_xml_and_builder_routes_are_byte_identical(tmp_path, instancing):
    path = write_xml(tmp_path, FOUR, shapes=GROUP + AREA_LIGHT)
    by_xml = mtsg.Scene(path, instancing=instancing)
    by_builder = W.Walker(path, {}, instancing=instancing).walk()
    dx, db = by_xml.digest(), by_builder.digest()
    assert "emitter_ext" in str(dx) and dx == db
    assert len(emitter_records(by_xml)[0]) == 5
    assert (header(by_xml).n_instances > 0) == (instancing == "two-level")


@pytest.mark.parametrize("kind", ["point", "spot", "directional", "constant"])
def test_restatement_has_few_fragile_samples(kind):
    """The per-sample reference of tests/test_gpu_emitters.py on the CPU alone:
    a sample is fragile when one of its shadow rays changes its oracle answer
    under a 4-ulp move of a direction component (Primary.shadow); at most 2% of
    the samples of each test scene may be.  The point light is placed near the
    camera's axis so that the cube's hard shadow edge is mostly hidden behind
    the cube (emitter_ref.KIND_EMITTERS)."""
    P = E.primary(4)
    assert 0.5 < P.hit.mean() < 1
    for ne in (1, 4):
        Li, mag, fragile, branches = E.emitters_reference(P, E.kind_records(kind), ne)
        assert fragile.mean() <= 0.02, (kind, ne, fragile.mean())
        assert (Li[P.hit].mean(0) > 0.01).all() and (mag >= 0).all()
        if kind == "spot":   # all three falloff branches occur
            assert all((branches == k).sum() > 20 for k in (0, 1, 2)), [(branches == k).sum() for k in (0, 1, 2)]
