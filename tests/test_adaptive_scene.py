"""The scene side of the `adaptive` integrator (adaptive.cpp:70-121,161-178):
properties and defaults, the quantile, the load errors with the reference's
wording, both scene routes, the digests, and the round bookkeeping's sweep.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import mtsg
import adaptive_ref as A
from conftest import REPO, SCENES
import scene_walker as W

f32 = np.float32

XML = """<?xml version="1.0"?>
<scene version="0.5.0">
  {integrator}
  <sensor type="perspective">
    <float name="fov" value="39.3"/>
    <transform name="toWorld"><lookat origin="0.3, 0.2, 3.9" target="0, 0, 0" up="0, 1, 0"/></transform>
    <sampler type="{sampler}"><integer name="sampleCount" value="{spp}"/></sampler>
    <film type="hdrfilm"><integer name="width" value="40"/><integer name="height" value="24"/>
      <rfilter type="gaussian"/></film>
  </sensor>
  <bsdf type="diffuse" id="white"><rgb name="reflectance" value="0.725, 0.71, 0.68"/></bsdf>
  <shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="-90"/><translate y="-1"/></transform>
    <ref id="white"/></shape>
  <shape type="rectangle">
    <transform name="toWorld"><scale x="0.23" y="0.19" z="1"/><rotate x="1" angle="90"/><translate y="0.99"/></transform>
    <emitter type="area"><rgb name="radiance" value="17, 12, 4"/></emitter></shape>
</scene>
"""
PATH = '<integrator type="path"><integer name="maxDepth" value="3"/></integrator>'


def adaptive_xml(props="", child=PATH):
    return f'<integrator type="adaptive">{props}{child}</integrator>'


def load(tmp_path, integrator, sampler="independent", spp=8, name="s.xml"):
    p = tmp_path / name
    p.write_text(XML.format(integrator=integrator, sampler=sampler, spp=spp))
    return mtsg.Scene(str(p))


def desc_tuple(d):
    return (d.max_error, d.quantile, d.max_sample_factor, d.base_count)


def test_defaults_and_render_params(tmp_path):
    s = load(tmp_path, adaptive_xml(), spp=16)
    d = s.adaptive()
    assert d is not None
    assert desc_tuple(d) == (f32(0.05), f32(1.959963984540054), 32, 16)
    p = s.params()
    # the child's properties are the render's
    assert (p.integrator, p.max_depth, p.rr_depth, p.spp) == (mtsg.MTSG_INTEGRATOR_PATH, 3, 5, 16)
    assert s.aov() is None and s.direct() is None
    plain = load(tmp_path, PATH, spp=16, name="p.xml")
    assert plain.adaptive() is None


@pytest.mark.parametrize("p_value,want", [("0.05", 1.959963984540054), ("0.01", 2.5758293035489004), ("0.1", 1.6448536269514722),
                                          ("0.5", 0.6744897501960817)])
def test_quantile(tmp_path, p_value, want):
    s = load(tmp_path, adaptive_xml(f'<float name="pValue" value="{p_value}"/>'))
    assert s.adaptive().quantile == f32(want)


class Walker(W.Walker):
    """scene_walker's replay of an XML file through the builder calls, with the
    nested integrators of the <integrator> element added first, as a plugin
    hands them over (mtsh_scene_add_integrator_child, then the parent)."""

    def walk(self, overrides=None):
        import xml.etree.ElementTree as ET
        for e in ET.parse(self.path).getroot():
            if e.tag == "integrator":
                for c in self.props(e, "integrator")[1]:
                    assert c.tag == "integrator"
                    self.call("integrator_child", self.attr(c, "type"), self.props(c, "integrator")[0])
        return super().walk(overrides)


def write(tmp_path, integrator, sampler="independent", spp=8, name="s.xml"):
    p = tmp_path / name
    p.write_text(XML.format(integrator=integrator, sampler=sampler, spp=spp))
    return str(p)


def test_both_routes_give_the_same_descriptor_and_digest(tmp_path):
    """One scene file through mtsh_scene_load and, replayed call by call, through the builder: the same adaptive
    descriptor, render parameters and scene digest; and the digest is the plain `path` file's, route by route."""
    props = '<float name="maxError" value="0.125"/><integer name="maxSampleFactor" value="4"/><float name="pValue" value="0.01"/>'
    path = write(tmp_path, adaptive_xml(props))
    by_xml = mtsg.Scene(path)
    walker = Walker(path, {})
    by_builder = walker.walk()
    assert walker.log.count("integrator_child") == 1
    assert desc_tuple(by_xml.adaptive()) == (f32(0.125), f32(2.5758293035489004), 4, 8)
    assert bytes(by_xml.adaptive()) == bytes(by_builder.adaptive())
    assert bytes(by_xml.params()) == bytes(by_builder.params())
    assert by_xml.digest() == by_builder.digest()
    # `adaptive` leaves the scene descriptor alone: the same file under its `path` child alone
    plain = write(tmp_path, PATH, name="p.xml")
    assert mtsg.Scene(plain).digest() == by_xml.digest() == W.Walker(plain, {}).walk().digest()
    # the defaults on the builder route
    assert desc_tuple(A.adaptive_scene(defaults=True).adaptive()) == (f32(0.05), f32(1.959963984540054), 32, 8)


# FNV-1a 64 of the descriptor arrays of scenes/cbox.xml at 32x32, 8 spp under its own `path` integrator, recorded on
# the commit before `adaptive` existed
CBOX_DIGEST = {
    "bsdfs": "899682ba0ea01c59", "emitter_cdf": "49b12a7eb10017aa", "emitter_tri_cdf": "14650fb0739d0383",
    "emitters": "bac5fbe8403574d1", "group_indices": "14650fb0739d0383", "group_nodes": "14650fb0739d0383",
    "groups": "14650fb0739d0383", "indices": "6a2691504d958251", "instances": "14650fb0739d0383", "nodes": "bc958164391693a0",
    "rects": "8efa89633d3150c2", "scalars": "009a2d438cdd0564", "shapes": "37a2b17881cd4042", "tex_texels": "14650fb0739d0383",
    "textures": "14650fb0739d0383", "tri_dpdu": "f6c6ae6960156abd", "tri_idx": "e6363a2bd64af303", "triaccel": "b81b56cdd9d51587",
    "vtx_nrm": "f9e7b9bfde9bfa63", "vtx_pos": "9a7462bfca428f4f",
}


def test_a_plain_path_scene_digest_is_what_it_was(tmp_path):
    """scenes/cbox.xml: every descriptor array's hash is the one recorded before this feature, and wrapping its
    integrator in `adaptive` moves none of them."""
    sc = mtsg.Scene(os.path.join(SCENES, "cbox.xml"), {"width": 32, "height": 32, "spp": 8})
    got = {k: "%016x" % h for k, (_b, h) in sc.digest().items()}
    assert got == CBOX_DIGEST
    assert sc.adaptive() is None
    src = open(os.path.join(SCENES, "cbox.xml")).read()
    i = src.index('<integrator type="path">')
    j = src.index("</integrator>", i) + len("</integrator>")
    wrapped = tmp_path / "cbox_adaptive.xml"
    wrapped.write_text(src[:i] + '<integrator type="adaptive">' + src[i:j] + "</integrator>" + src[j:])
    ad = mtsg.Scene(str(wrapped), {"width": 32, "height": 32, "spp": 8})
    assert ad.adaptive() is not None
    assert {k: "%016x" % h for k, (_b, h) in ad.digest().items()} == CBOX_DIGEST


def test_load_errors(tmp_path):
    with pytest.raises(RuntimeError, match="The error-controlling integrator should only be used in conjunction with the independent sampler"):
        load(tmp_path, adaptive_xml(), sampler="halton")
    with pytest.raises(RuntimeError, match="Starting the adaptive integrator with less than 8 samples per pixel does not make much sense -- giving up."):
        load(tmp_path, adaptive_xml(), spp=7)
    with pytest.raises(RuntimeError, match="No sub-integrator was specified!"):
        load(tmp_path, adaptive_xml(child=""))
    for child in ("direct", "ao", "multichannel", "myPath2_OM", "adaptive"):
        with pytest.raises(RuntimeError, match="outside this build's scope"):
            load(tmp_path, adaptive_xml(child=f'<integrator type="{child}"/>'))
    with pytest.raises(RuntimeError, match="outside this build's scope"):
        load(tmp_path, adaptive_xml(child=adaptive_xml()))
    # a `path` child with nested objects is refused, as multichannel's children are
    with pytest.raises(RuntimeError, match="adaptive: a child integrator with nested objects is not supported"):
        load(tmp_path, adaptive_xml(child='<integrator type="path"><integrator type="path"/></integrator>'))
    # adaptive as a child of multichannel stays refused
    with pytest.raises(RuntimeError):
        load(tmp_path, f'<integrator type="multichannel">{adaptive_xml()}</integrator>')
    with pytest.raises(RuntimeError, match="multichannel: child integrator \"adaptive\" is outside this build's scope"):
        load(tmp_path, '<integrator type="multichannel"><integrator type="adaptive"/></integrator>')
    # the reference's "infinity": a bound is required
    with pytest.raises(RuntimeError, match="maxSampleFactor.*a bound on the samples per pixel is required"):
        load(tmp_path, adaptive_xml('<integer name="maxSampleFactor" value="-1"/>'))


def test_builder_route_errors():
    b = mtsg.SceneBuilder(SCENES)
    with pytest.raises(RuntimeError, match="No sub-integrator was specified!"):
        b.integrator("adaptive", [])
    b = mtsg.SceneBuilder(SCENES)
    with pytest.raises(RuntimeError, match="outside this build's scope"):
        b.integrator_child("direct", [])
    b = mtsg.SceneBuilder(SCENES)
    b.integrator_child("field", [("field", "string", "position")])
    with pytest.raises(RuntimeError, match="outside this build's scope"):
        b.integrator("adaptive", [])
    b = mtsg.SceneBuilder(SCENES)
    b.integrator_child("path", [])
    with pytest.raises(RuntimeError, match="a bound on the samples per pixel is required"):
        b.integrator("adaptive", [("maxSampleFactor", "integer", -1)])
    with pytest.raises(RuntimeError, match="less than 8 samples per pixel"):
        A.adaptive_scene(spp=4)
    with pytest.raises(RuntimeError, match="independent sampler"):
        A.adaptive_scene(sampler="ldsampler")


def test_restatement_on_hand_made_samples():
    """adaptive_ref.restate_counts on pixels whose stop is known: constant
    samples stop at N (variance 0), a pixel of one bright sample among zeros
    runs to the cap, a rejected pixel counts zeros and stops at N, and a
    factor of 0 or 1 ends at 1 or N."""
    n, cap = 8, 32
    q = A.adaptive_scene(defaults=True).adaptive().quantile
    assert q == f32(1.959963984540054)
    s = np.zeros((1, 4, cap, 4), f32)
    s[0, 0, :, :3] = 0.5
    s[0, 1, 3, :3] = 100.0
    s[0, 2, :, 0] = -1.0
    s[0, 3, :, :3] = np.where(np.arange(cap) % 2 == 0, f32(0.443), f32(0.557))[:, None]   # sd 0.057: about 22 samples
    c = A.restate_counts(s, n, 4, 0.05, q, f32(0.3))
    assert c[0, 0] == n and c[0, 1] == cap and c[0, 2] == n and n + 8 < c[0, 3] < cap
    assert (A.restate_counts(s, n, 1, 0.05, q, f32(0.3)) == n).all()
    assert (A.restate_counts(s[:, :, :1], n, 0, 0.05, q, f32(0.3)) == 1).all()
    assert not A.accepted(s)[0, 2].any() and A.accepted(s)[0, :2].all()


def test_round_bookkeeping_sweep():
    """tools/check_adaptive_plan: csrc/adaptive_plan.h over a sweep of base
    counts, factors, round sizes, rectangles and path budgets (its own main,
    compiled with the address and undefined-behaviour sanitizers, CPU only)."""
    exe = os.path.join(REPO, "tools", "check_adaptive_plan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "simulated renders ok" in r.stdout
