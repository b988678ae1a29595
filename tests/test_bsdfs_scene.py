"""The scene side of the phong, ward, roughdiffuse, difftrans and thindielectric
BSDFs (src/bsdfs/phong.cpp, ward.cpp, roughdiffuse.cpp, difftrans.cpp,
thindielectric.cpp): the records of both scene routes against the configure()
values of tests/bsdf_ref.py, the load errors, the restatement's own
sample-vs-pdf consistency (the chi-square settings of test_bsdf_chisquare.py),
and the descriptors of the scenes that existed before these plugins.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

import mtsg
import scene_walker as W
from conftest import REPO, SCENES
import bsdf_ref as BR
import test_bsdf_chisquare as CS
from multichannel_ref import Desc

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
  {bsdfs}
  <shape type="rectangle"><transform name="toWorld"><rotate x="1" angle="-90"/><translate y="-1"/></transform>
    <ref id="b0"/></shape>
  <shape type="shapegroup" id="g"><shape type="cube"><transform name="toWorld"><scale value="0.3"/></transform>
    <ref id="b0"/></shape></shape>
  <shape type="instance"><ref id="g"/><transform name="toWorld"><translate x="0.2" y="-0.7"/></transform></shape>
  <shape type="rectangle"><transform name="toWorld"><scale x="0.23" y="0.19" z="1"/><rotate x="1" angle="90"/>
    <translate y="0.99"/></transform><emitter type="area"><rgb name="radiance" value="17, 12, 4"/></emitter></shape>
</scene>
"""


def write_xml(tmp_path, bsdfs, integrator="path", name="s.xml"):
    """bsdfs: the inner XML of <bsdf> elements; they get the ids b0, b1, ..."""
    body = "".join(f'<bsdf type="{t}" id="b{k}">{inner}</bsdf>' for k, (t, inner) in enumerate(bsdfs))
    p = tmp_path / name
    p.write_text(XML.format(integrator=integrator, bsdfs=body))
    return str(p)


DEFAULTS = [("phong", ""), ("ward", ""), ("roughdiffuse", ""), ("difftrans", ""), ("thindielectric", "")]
# one non-default set per plugin: the three ward variants (one anisotropic), a
# named intIOR, and the pair energy conservation (0.8 + 0.6 > 1)
CUSTOM = [
    ("phong", '<spectrum name="diffuseReflectance" value="0.8"/><spectrum name="specularReflectance" value="0.6"/>'
              '<float name="exponent" value="12.5"/>'),
    ("ward", '<string name="variant" value="ward"/><rgb name="diffuseReflectance" value="0.3, 0.2, 0.1"/>'
             '<float name="alphaU" value="0.05"/><float name="alphaV" value="0.3"/>'),
    ("ward", '<string name="variant" value="ward-duer"/><float name="alpha" value="0.25"/>'
             '<spectrum name="specularReflectance" value="0.4"/>'),
    ("ward", '<string name="variant" value="Balanced"/><rgb name="diffuseReflectance" value="0.8, 0.5, 0.2"/>'
             '<rgb name="specularReflectance" value="0.6, 0.1, 0.1"/>'),
    ("roughdiffuse", '<rgb name="diffuseReflectance" value="0.2, 1.4, 0.6"/><float name="alpha" value="0.7"/>'
                     '<boolean name="useFastApprox" value="true"/>'),
    ("difftrans", '<rgb name="transmittance" value="0.1, 0.9, 0.4"/>'),
    ("thindielectric", '<string name="intIOR" value="diamond"/><float name="extIOR" value="1.33"/>'
                       '<spectrum name="specularReflectance" value="0.9"/><rgb name="specularTransmittance" value="0.5, 2.0, 1.0"/>'),
]
CUSTOM_REF = [
    BR.phong(0.8, 0.6, 12.5),
    BR.ward("ward", (0.3, 0.2, 0.1), 0.2, alphaU=0.05, alphaV=0.3),
    BR.ward("ward-duer", 0.5, 0.4, alpha=0.25),
    BR.ward("balanced", (0.8, 0.5, 0.2), (0.6, 0.1, 0.1)),
    BR.roughdiffuse((0.2, 1.4, 0.6), 0.7, True),
    BR.difftrans((0.1, 0.9, 0.4)),
    BR.thindielectric(2.419, 1.33, 0.9, (0.5, 2.0, 1.0)),
]
DEFAULT_REF = [BR.phong(), BR.ward(), BR.roughdiffuse(), BR.difftrans(), BR.thindielectric()]


def check_record(got, want, what):
    assert got.type == want.type, what
    assert (got.smooth, got.ref_n_zero, got.twosided, got.texture) == (want.smooth, want.ref_n_zero, 0, 0), what
    assert list(got.reflectance) == list(want.reflectance), what
    assert list(got.spec_refl) == list(want.spec_refl), what
    assert list(got.spec_trans) == list(want.spec_trans), what
    assert (got.alpha_u, got.alpha_v) == (want.alpha_u, want.alpha_v), what
    assert (got.distribution, got.nonlinear) == (want.distribution, want.nonlinear), what
    assert (got.ior_eta, got.ior_inv_eta) == (want.ior_eta, want.ior_inv_eta), what
    assert got.spec_sampling_weight == want.spec_sampling_weight, what
    assert list(got.pad_tex) == [0, 0, 0] and not any(got.rtrans) and got.fdr_int == 0 and got.sample_visible == 0, what


@pytest.mark.parametrize("name,bsdfs,refs", [("defaults", DEFAULTS, DEFAULT_REF), ("custom", CUSTOM, CUSTOM_REF)])
@pytest.mark.parametrize("instancing", ["flatten", "two-level"])
def test_records_of_both_routes(tmp_path, name, bsdfs, refs, instancing):
    path = write_xml(tmp_path, bsdfs)
    by_xml = mtsg.Scene(path, instancing=instancing)
    by_builder = W.Walker(path, {}, instancing=instancing).walk()
    assert by_xml.digest() == by_builder.digest()
    for scene in (by_xml, by_builder):
        recs = Desc(scene).bsdfs
        for k, want in enumerate(refs):
            check_record(recs[k], want, (name, k, bsdfs[k][0]))


def test_pair_energy_conservation_scales_both():
    """diffuseReflectance 0.8 + specularReflectance 0.6: both times 0.99 / 1.4 (bsdf.cpp:115-146)."""
    r = CUSTOM_REF[0]
    s = f32(f32(0.99) * (f32(1.0) / f32(f32(0.8) + f32(0.6))))
    assert r.reflectance[0] == f32(0.8) * s and r.spec_refl[0] == f32(0.6) * s
    assert (r.reflectance + r.spec_refl).max() <= 1
    # ward "balanced" above: the maximum of the sum is the red channel's 1.4
    assert CUSTOM_REF[3].spec_refl[1] == f32(0.1) * s


def test_the_load_errors(tmp_path):
    with pytest.raises(RuntimeError, match='ward: Specified an invalid model type "wardx", must be "ward", "ward-duer", or "balanced"!'):
        mtsg.Scene(write_xml(tmp_path, [("ward", '<string name="variant" value="wardx"/>')]))
    with pytest.raises(RuntimeError, match="thindielectric: the interior and exterior indices of refraction must differ"):
        mtsg.Scene(write_xml(tmp_path, [("thindielectric", '<float name="intIOR" value="1.3"/><float name="extIOR" value="1.3"/>')]))
    tex = '<texture name="{}" type="bitmap"><string name="filename" value="' + os.path.join(SCENES, "tex_checker.png") + '"/></texture>'
    for plugin, param in (("phong", "exponent"), ("ward", "alphaU"), ("roughdiffuse", "alpha"), ("thindielectric", "specularReflectance")):
        with pytest.raises(RuntimeError, match=f'{plugin}: a texture for parameter "{param}" is outside this build\'s scope'):
            mtsg.Scene(write_xml(tmp_path, [(plugin, tex.format(param))]))
    mtsg.Scene(write_xml(tmp_path, [("ward", tex.format("diffuseReflectance"))]))   # the one parameter that takes a bitmap
    for inner in ("difftrans", "thindielectric"):
        with pytest.raises(RuntimeError, match=f"twosided: Only materials without a transmission component can be nested!.*{inner}"):
            mtsg.Scene(write_xml(tmp_path, [("twosided", f'<bsdf type="{inner}"/>')]))
    for plugin in ("phong", "ward", "roughdiffuse", "difftrans", "thindielectric"):
        with pytest.raises(RuntimeError, match=f"myPath2_OM: the {plugin} BSDF is outside this build's scope"):
            mtsg.Scene(write_xml(tmp_path, [(plugin, "")], integrator="myPath2_OM"))


def test_textured_pair_energy_conservation(tmp_path):
    """A bitmap diffuseReflectance on ward and phong with specularReflectance
    0.6: the texture's maximum plus 0.6 exceeds 1, so the BSDF gets its own copy
    of the texture scaled by 0.99 / max(sum), the specular constant is scaled
    alike, and the sampling weight comes from the scaled texture's average
    (bsdf.cpp:115-146, ward.cpp:158-162).  Without the rescale the texture is
    shared and unscaled.  Both scene routes."""
    tex = ('<texture name="diffuseReflectance" type="bitmap"><string name="filename" value="'
           + os.path.join(SCENES, "tex_checker.png") + '"/></texture>')
    spec = '<spectrum name="specularReflectance" value="0.6"/>'
    path = write_xml(tmp_path, [("ward", tex + spec), ("phong", tex + spec),
                                ("ward", tex + spec + '<boolean name="ensureEnergyConservation" value="false"/>')])
    by_xml = mtsg.Scene(path)
    by_builder = W.Walker(path, {}).walk()
    assert by_xml.digest() == by_builder.digest()
    for scene in (by_xml, by_builder):
        recs, texs = Desc(scene).bsdfs, scene.textures()
        for k in (0, 1):
            r = recs[k]
            assert r.texture > 0
            t = texs[r.texture - 1]
            mx = np.array(list(t.maximum), f32)
            assert mx.max() + f32(0.6) > 1   # the case under test
            s = f32(f32(0.99) * (f32(1.0) / (mx + f32(0.6)).max()))
            assert t.scale == s, (t.scale, s)
            assert list(r.spec_refl) == [f32(0.6) * s] * 3
            avg = np.array(list(t.average), f32) * s
            d, sp = BR.luminance(avg), BR.luminance(np.array(list(r.spec_refl), f32))
            assert r.spec_sampling_weight == f32(sp / f32(d + sp))
            assert list(r.reflectance) == list(avg)   # the value getAverage() saw
            assert ((mx * s) + np.array(list(r.spec_refl), f32)).max() <= 1
        assert recs[0].texture != recs[1].texture   # each BSDF scales a copy of its own
        r = recs[2]
        assert texs[r.texture - 1].scale == 1 and list(r.spec_refl) == [f32(0.6)] * 3


def test_twosided_takes_the_reflecting_models(tmp_path):
    scene = mtsg.Scene(write_xml(tmp_path, [("twosided", '<bsdf type="phong"/><bsdf type="roughdiffuse"/>'),
                                            ("twosided", '<bsdf type="ward"/>')]))
    recs = Desc(scene).bsdfs
    fronts = [r for r in recs if r.twosided]
    assert [r.type for r in fronts] == [BR.PHONG, BR.WARD]
    assert recs[fronts[0].back].type == BR.ROUGHDIFFUSE and recs[fronts[1].back].type == BR.WARD


# ---------------------------------------------------------------------------
# the restatement checks itself
# ---------------------------------------------------------------------------
MODELS = [
    ("phong", BR.phong(0.4, 0.5, 18.0)),
    ("ward", BR.ward("ward", 0.3, 0.5, alphaU=0.15, alphaV=0.3)),
    ("ward-duer", BR.ward("ward-duer", 0.3, 0.5, alphaU=0.3, alphaV=0.12)),
    ("ward-balanced", BR.ward("balanced", 0.3, 0.5, alphaU=0.2, alphaV=0.35)),
    ("roughdiffuse", BR.roughdiffuse((0.5, 0.3, 0.8), 0.6, False)),
    ("roughdiffuse-fast", BR.roughdiffuse((0.5, 0.3, 0.8), 0.6, True)),
    ("difftrans", BR.difftrans((0.5, 0.3, 0.8))),
]


def expected_counts(b, wi, n_samples, gl=32):
    """test_bsdf_chisquare.expected_counts over the restatement's pdf."""
    saved = CS.evaluate
    CS.evaluate = lambda b_, wi_, wo: BR.evaluate(b_, wi_, wo, exact=False)
    try:
        return CS.expected_counts(b, wi, n_samples, gl, reachable_only=False)
    finally:
        CS.evaluate = saved


@pytest.mark.parametrize("name,b", MODELS, ids=[m[0] for m in MODELS])
def test_restatement_sampling_matches_its_pdf(name, b):
    rng = np.random.default_rng(11)
    n_wi = 2
    alpha = 1 - (1 - CS.SIGNIFICANCE) ** (1.0 / n_wi)   # Sidak (chisquare.cpp:255)
    wis = CS.random_wi(rng, n_wi)
    if b.type == BR.DIFFTRANS:
        wis[1] = -wis[1]
    for wi in wis:
        u = rng.random((CS.N_SAMPLES, 2), dtype=np.float32)
        wo, w, pdf, eta, flags = BR.sample(b, wi, u, exact=False)
        ok = flags != 0
        p = CS.chi2_pvalue(CS.observed_counts(wo[ok]), expected_counts(b, wi, CS.N_SAMPLES))
        assert p >= alpha, f"{name} wi={wi}: chi-square p-value {p:.3e} < {alpha:.3e}"
        # weight x pdf == eval at the sampled direction, pdf == pdf(wo)
        sel = np.flatnonzero(ok)[:5000]
        val, pdf_e = BR.evaluate(b, wi, wo[sel], exact=False)
        np.testing.assert_allclose(pdf_e, pdf[sel], rtol=1e-5, atol=1e-30)
        np.testing.assert_allclose(w[sel] * pdf[sel][:, None], val, rtol=2e-6, atol=1e-30)
        assert (eta[ok] == 1).all() and (flags[ok] == BR.OK).all()


@pytest.mark.parametrize("cos_i", [0.95, 0.4, -0.08])
def test_thindielectric_split_follows_the_pane_reflectance(cos_i):
    """The pattern of test_dielectric_split_follows_fresnel, with R' = R + T^2 R / (1 - R^2)
    from an independent double-precision Fresnel term."""
    b = BR.thindielectric()
    s = math.sqrt(1 - cos_i ** 2)
    wi = np.array([s, 0.0, cos_i], f32)
    n = 200000
    u = np.random.default_rng(3).random((n, 2), dtype=np.float32)
    wo, w, pdf, eta, flags = BR.sample(b, wi, u)
    R, _ = CS.fresnel_dielectric(abs(cos_i), float(b.ior_eta))
    Rp = R + (1 - R) ** 2 * R / (1 - R * R)
    refl = wo[:, 2] * cos_i > 0
    sigma = math.sqrt(Rp * (1 - Rp) / n)
    assert abs(refl.mean() - Rp) <= 5 * sigma + 1e-6, (refl.mean(), Rp)
    np.testing.assert_allclose(pdf[refl], Rp, rtol=1e-4)
    np.testing.assert_allclose(pdf[~refl], 1 - Rp, rtol=1e-4)
    assert (flags[refl] == (BR.OK | BR.DELTA)).all() and (flags[~refl] == (BR.OK | BR.DELTA | BR.NULL)).all()
    assert (wo[~refl] == -wi).all() and (w == 1).all() and (eta == 1).all()
    assert (wo[refl] == wi * np.array([-1, -1, 1], f32)).all()


# ---------------------------------------------------------------------------
# the scenes from before these plugins keep their descriptors
# ---------------------------------------------------------------------------
def test_existing_scenes_keep_their_descriptors():
    """tests/golden/bsdfs_parent_digests.json: mtsh_scene_digest of the test
    scenes ({descriptor array: [bytes, FNV-1a 64]}), recorded with the host
    library of the commit before the five plugins, in both instancing modes."""
    with open(os.path.join(REPO, "tests", "golden", "bsdfs_parent_digests.json")) as f:
        golden = json.load(f)
    assert len(golden) >= 10
    for key, want in sorted(golden.items()):
        name, instancing = key.split("|")
        got = mtsg.Scene(os.path.join(SCENES, name), instancing=instancing).digest()
        assert sorted(got) == sorted(want), key
        for array, (nbytes, fnv) in want.items():
            assert tuple(got[array]) == (nbytes, fnv), (key, array)
