"""The `ao` integrator on the GPU (csrc/direct.hip; ao.cpp:84-125): the
fraction of N cosine-weighted rays of length rayLength that leave a hit
unoccluded, 1 on a miss.  Film 40 x 24, at most 16 spp.

Per sample, N = 1 and N = 4 equal the restatement from oracle pieces
(direct_ref.ao_reference: the reference's intersection record and
computeShadingFrame in float32 numpy, squareToCosineHemisphere through
oracle_bsdf_sample_n on a diffuse record, oracle.trace_shadow at (Epsilon,
rayLength)) on every non-fragile sample.  The mean is also checked against an
independent estimate: the `field` integrator's
position and shading normal of the same camera samples (the children draw no
random numbers, so the camera rays are those of the `ao` render), cosine-
weighted directions from numpy's own generator in numpy's own tangent frame,
and the oracle's shadow rays.  Ambient occlusion does not depend on the
tangent frame in expectation, so the two estimators agree within their
standard errors."""
import numpy as np
import pytest

import mtsg
from oracle import pyoracle as O
from conftest import SCENES
import direct_ref
from direct_ref import FILM_H, FILM_W, box_geometry, box_props, box_scene, direct_desc, region_masks

pytestmark = pytest.mark.gpu

AO = mtsg.MTSG_INTEGRATOR_AO
LENGTH = 0.45


@pytest.fixture(scope="module")
def box():
    scene = box_scene("ao", [("shadingSamples", "integer", 4), ("rayLength", "float", LENGTH)], spp=16)
    g = mtsg.GPUScene(scene, 0)
    yield scene, g
    g.close()


def ao_samples(g, scene, n, length, **over):
    g.set_direct(direct_desc(ao=n, length=length))
    p = scene.params(**over)
    assert p.integrator == AO
    return g.render_samples(p)


@pytest.mark.parametrize("n", [1, 3, 4])
def test_values_are_multiples_of_one_nth_and_misses_are_one(box, n):
    scene, g = box
    a = ao_samples(g, scene, n, LENGTH)
    rgb, alpha = a[..., :3], a[..., 3]
    assert (rgb[..., 0] == rgb[..., 1]).all() and (rgb[..., 0] == rgb[..., 2]).all()
    recip = np.float32(1) / np.float32(n)   # Spectrum::operator/= multiplies by the reciprocal
    levels = (np.arange(n + 1, dtype=np.float32) * recip).astype(np.float32)
    assert np.isin(rgb[..., 0], levels).all()
    assert set(np.unique(alpha)) == {0.0, 1.0}
    miss = alpha == 0
    assert miss.any() and (rgb[miss] == 1.0).all()
    hit = rgb[~miss][:, 0]
    assert len(np.unique(hit)) == n + 1   # every level occurs on the hits of this box
    # the film: same alpha and weight as any render of the box
    st = g.stats()
    samples = FILM_W * FILM_H * 16
    assert st.launches_trace_closest + st.launches_trace_shadow == 2 and st.launches_finish == 0
    assert st.rays_closest == samples and st.rays_shadow == int((~miss).sum()) * n


@pytest.fixture(scope="module")
def box4():
    """The box at 4 spp, the sample count of the restatement."""
    scene = box_scene("ao", [("shadingSamples", "integer", 4)], spp=4)
    g = mtsg.GPUScene(scene, 0)
    yield scene, g
    g.close()


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("length", ["explicit", "default"])
def test_per_sample_restatement(box4, n, length):
    """Explicit and default rayLength (half the scene's bounding sphere radius, 1.4...)."""
    scene, g = box4
    length = LENGTH if length == "explicit" else scene.direct().ao_ray_length
    assert length > 0 and (length == LENGTH or length > 1.0)
    P = direct_ref.primary(4)
    want, fragile = direct_ref.ao_reference(P, n, length)
    a = ao_samples(g, scene, n, length).reshape(-1, 4)
    assert ((a[:, 3] == 1) == P.hit).all()
    share = fragile.mean()
    wrong = (a[:, 0] != want) & ~fragile
    print(f"ao N={n} rayLength {length:.4f}: fragile {share:.4%}, differing non-fragile samples {int(wrong.sum())} of {len(want)}, "
          f"differing fragile {int(((a[:, 0] != want) & fragile).sum())}")
    assert share <= 0.02
    assert not wrong.any(), (np.nonzero(wrong)[0][:8], a[wrong][:8, 0], want[wrong][:8])


def test_explicit_and_default_lengths_differ(box4):
    scene, g = box4
    assert (ao_samples(g, scene, 4, LENGTH)[..., 0] != ao_samples(g, scene, 4, scene.direct().ao_ray_length)[..., 0]).any()


def test_mean_matches_an_independent_estimate(box):
    scene, g = box
    a = ao_samples(g, scene, 4, LENGTH)[..., 0].astype(np.float64)
    # the same camera samples' hit points and shading normals
    b = mtsg.SceneBuilder(SCENES)
    for f in ("position", "shNormal"):
        b.integrator_child("field", [("field", "string", f), ("undefined", "spectrum", (0.0, 0.0, 0.0))])
    b.multichannel()
    box_props(b, spp=16, pixel_format="rgb, rgb", film_props=[("channelNames", "string", "p, n")])
    box_geometry(b)
    fields = b.finish()
    gf = mtsg.GPUScene(fields, 0)
    try:
        f = gf.render_samples_multi(fields.params())
    finally:
        gf.close()
    pos, nrm, alpha = f[..., 0:3].astype(np.float64), f[..., 3:6].astype(np.float64), f[..., 6]
    hit = alpha == 1
    assert (hit == (ao_samples(g, scene, 4, LENGTH)[..., 3] == 1)).all()
    # own directions: cosine-weighted about the shading normal, own frame, own numbers
    rng = np.random.default_rng(5)
    K = 8
    n = nrm[hit]
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    helper = np.where(np.abs(n[:, :1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    s = np.cross(n, helper)
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    t = np.cross(n, s)
    est = np.zeros((hit.sum(), K))
    for k in range(K):
        u1, u2 = rng.random(len(n)), rng.random(len(n))
        r, phi = np.sqrt(u1), 2 * np.pi * u2
        d = s * (r * np.cos(phi))[:, None] + t * (r * np.sin(phi))[:, None] + n * np.sqrt(1 - u1)[:, None]
        rays = np.concatenate([pos[hit], d, np.full((len(n), 1), 1e-4), np.full((len(n), 1), LENGTH)], axis=1).astype(np.float32)
        est[:, k] = 1.0 - O.trace_shadow(fields.desc, rays)
    ref = np.ones(hit.shape + (K,))
    ref[hit] = est
    # film and six regions, 5 standard errors from the values themselves
    for name, m in [("film", np.ones((FILM_H, FILM_W), bool))] + [(f"region {k}", m) for k, m in enumerate(region_masks(FILM_H, FILM_W))]:
        x, y = a[m].ravel(), ref[m].ravel()
        bound = 5 * np.sqrt(x.var() / x.size + y.var() / y.size)
        print(f"ao {name}: gpu {x.mean():.4f} reference {y.mean():.4f} bound {bound:.4f}")
        assert abs(x.mean() - y.mean()) <= bound, (name, x.mean(), y.mean(), bound)


def test_ray_length_matters_and_the_default_is_the_scenes(box):
    scene, g = box
    short = ao_samples(g, scene, 4, 0.05)[..., 0]
    mid = ao_samples(g, scene, 4, LENGTH)[..., 0]
    assert short.mean() > mid.mean() + 0.02   # shorter rays meet fewer occluders
    # rays a thousand times shorter than the scene are occluded only in creases
    assert ao_samples(g, scene, 4, 1e-3)[..., 0].mean() > 0.97
    # the default length: half the scene's bounding sphere radius, set by the scene route
    dflt = box_scene("ao", [("shadingSamples", "integer", 4)], spp=16)
    d = dflt.direct()
    assert d.ao_ray_length > 1.0
    gd = mtsg.GPUScene(dflt, 0)
    try:
        img = gd.render_samples(dflt.params())[..., 0]
    finally:
        gd.close()
    assert (img.view(np.uint32) == ao_samples(g, scene, 4, d.ao_ray_length)[..., 0].view(np.uint32)).all()
    assert (img != mid).any() and img.mean() < mid.mean()


@pytest.mark.parametrize("sampler", ["sobol", "halton", "ldsampler"])
def test_other_samplers_agree_in_the_mean(box, sampler):
    scene, g = box
    a = ao_samples(g, scene, 4, LENGTH)[..., 0].astype(np.float64)
    other = box_scene("ao", [("shadingSamples", "integer", 4), ("rayLength", "float", LENGTH)], spp=16, sampler=sampler)
    go = mtsg.GPUScene(other, 0)
    try:
        b = go.render_samples(other.params())[..., 0].astype(np.float64)
    finally:
        go.close()
    # (quasi-random samples have less variance than their sample variance says: the bound is conservative)
    for m in [np.ones((FILM_H, FILM_W), bool)] + region_masks(FILM_H, FILM_W):
        x, y = a[m].ravel(), b[m].ravel()
        assert abs(x.mean() - y.mean()) <= 5 * np.sqrt(x.var() / x.size + y.var() / y.size), (sampler, x.mean(), y.mean())


def test_splits(box):
    scene, g = box
    g.set_direct(direct_desc(ao=4, length=LENGTH))
    p, b = scene.params(), scene.border
    whole = g.render(p, b)
    acc = np.zeros_like(whole)
    for off in range(2):
        q = p.copy()
        q.tile_stride, q.tile_offset = 2, off
        acc += g.render(q, b)
    np.testing.assert_allclose(acc, whole, rtol=2e-5, atol=2e-6)
    g.set_batch_paths(512)
    try:
        np.testing.assert_allclose(g.render(p, b), whole, rtol=2e-5, atol=2e-6)
    finally:
        g.set_batch_paths(1 << 20)
