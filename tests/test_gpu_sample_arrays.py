"""Sample arrays of the device samplers (csrc/sampler.h smp_array2D;
Sampler::request2DArray / next2DArray), through mtsg_sampler_draws with
kinds[i] = -n on a handle whose direct descriptor requests the arrays.

halton and sobol: array r is the sequence itself in the reserved dimensions
(5 + 2r, 6 + 2r), element k of sample s the point of index s n + k
(halton.cpp:274-326, sobol.cpp:171-198).  The oracle's plain draws give those
points: its draws 2D, 2D, 1D consume dimensions 0-4, the 2D draws after them
are (5, 6), (7, 8), (9, 10).  (Three 2D draws in a row would land on (4, 5):
the oracle's plain next2D does not skip dimension 4, so the 1D draw in between
is what puts the following pairs on the reserved dimensions.)"""
import numpy as np
import pytest

import mtsg
from oracle import pyoracle as O
from direct_ref import box_scene

pytestmark = pytest.mark.gpu

SPP = 4
CORNER = [(x, y) for y in range(8) for x in range(8)]


def scene_with_arrays(sampler, ne, nb, spp=SPP):
    scene = box_scene("direct", [("emitterSamples", "integer", ne), ("bsdfSamples", "integer", nb)], sampler=sampler, spp=spp)
    return scene, mtsg.GPUScene(scene, 0)


@pytest.mark.parametrize("sampler", ["halton", "sobol"])
def test_qmc_arrays_are_the_sequence_in_the_reserved_dimensions(sampler):
    n0, n1 = 4, 3
    scene, g = scene_with_arrays(sampler, n0, n1)
    try:
        p = scene.params()
        big = scene.params(spp=SPP * n0)   # the oracle's sample indices run to spp * n
        for x, y in CORNER:
            # oracle sample j: [jitter 0-1, 2-3, 4, (5,6), (7,8), (9,10)]
            plain = np.stack([O.sampler_draws(scene.desc, big, x, y, j, [2, 2, 1, 2, 2, 2]) for j in range(SPP * n0)])
            for s in range(SPP):
                got = g.sampler_draws(p, x, y, s, [2, -n0, -n1, 2, 1, 2])
                jitter, a0, a1 = got[0:2], got[2:2 + 2 * n0].reshape(n0, 2), got[2 + 2 * n0:2 + 2 * (n0 + n1)].reshape(n1, 2)
                rest = got[2 + 2 * (n0 + n1):]
                for k in range(n0):
                    assert (a0[k].view(np.uint32) == plain[s * n0 + k, 5:7].view(np.uint32)).all(), (x, y, s, k)
                for k in range(n1):
                    assert (a1[k].view(np.uint32) == plain[s * n1 + k, 7:9].view(np.uint32)).all(), (x, y, s, k)
                # regular draws: dimensions 0-1, 2-3, 4, then past the two reserved pairs: 9-10
                want = np.concatenate([plain[s, 0:5], plain[s, 9:11]])
                assert (np.concatenate([jitter, rest]).view(np.uint32) == want.view(np.uint32)).all(), (x, y, s)
                # a next2D that starts at dimension 4 jumps over the whole reserved range:
                # dimensions 0-1, 2-3, then 9-10 (the BSDF draw of a fan with one BSDF sample)
                got = g.sampler_draws(p, x, y, s, [2, -n0, -n1, 2, 2])
                edge = np.concatenate([got[0:2], got[2 + 2 * (n0 + n1):]])
                want = np.concatenate([plain[s, 0:4], plain[s, 9:11]])
                assert (edge.view(np.uint32) == want.view(np.uint32)).all(), (x, y, s)
    finally:
        g.close()


def test_ldsampler_array_is_a_shuffled_02_net():
    n = 4
    scene, g = scene_with_arrays("ldsampler", n, 1)
    try:
        p = scene.params()
        nets = []
        for x, y in [(3, 5), (4, 5), (39, 23)]:
            pts = np.concatenate([g.sampler_draws(p, x, y, s, [2, -n])[2:].reshape(n, 2) for s in range(SPP)])
            assert pts.shape == (SPP * n, 2) and (pts >= 0).all() and (pts < 1).all()
            # every elementary interval of area 1/16 holds exactly one of the 16 points
            for a in range(5):
                cell = np.floor(pts[:, 0] * (1 << a)).astype(int) * (1 << (4 - a)) + np.floor(pts[:, 1] * (1 << (4 - a))).astype(int)
                assert sorted(cell) == list(range(16)), (x, y, a)
            nets.append(pts)
        assert not np.array_equal(nets[0], nets[1]) and not np.array_equal(nets[0], nets[2])
        # shuffled: the entries are not in the (0,2) sequence's own order in every pixel
        assert any(not np.array_equal(np.argsort(q[:, 0]), np.argsort(nets[0][:, 0])) for q in nets[1:])
    finally:
        g.close()


def test_ldsampler_arrays_of_other_sizes_cover_their_range():
    """n = 3, spp = 4: 12 entries walked out of a 16-cycle, each of the first
    12 points of a (0,2) sequence once: every strip of width 1/4 holds 3."""
    scene, g = scene_with_arrays("ldsampler", 1, 3)
    try:
        p = scene.params()
        pts = np.concatenate([g.sampler_draws(p, 7, 2, s, [2, -3])[2:].reshape(3, 2) for s in range(SPP)])
        assert len(np.unique(pts, axis=0)) == 12
        for c in range(2):
            assert np.bincount(np.floor(pts[:, c] * 4).astype(int), minlength=4).tolist() == [3, 3, 3, 3]
    finally:
        g.close()


def test_independent_arrays_have_their_own_dimensions():
    n0, n1 = 4, 3
    scene, g = scene_with_arrays("independent", n0, n1)
    try:
        p = scene.params()
        kinds = [2, -n0, -n1] + [1] * 64
        seen = []
        for x, y in [(0, 0), (17, 9), (39, 23)]:
            for s in range(SPP):
                got = g.sampler_draws(p, x, y, s, kinds)
                assert (got >= 0).all() and (got < 1).all()
                arrays = got[2:2 + 2 * (n0 + n1)]
                regular = np.concatenate([got[:2], got[2 + 2 * (n0 + n1):]])
                assert len(np.unique(arrays)) == arrays.size
                assert not np.isin(arrays, regular).any()
                # the regular draws are those of a handle without arrays: dimensions 0, 1, 2, ...
                assert (regular.view(np.uint32) == O.sampler_draws(scene.desc, p, x, y, s, [2] + [1] * 64).view(np.uint32)).all()
                again = g.sampler_draws(p, x, y, s, kinds)
                assert (again.view(np.uint32) == got.view(np.uint32)).all()
                seen.append(arrays)
        assert len(np.unique(np.concatenate(seen))) == sum(a.size for a in seen)   # pixels and samples differ
        # (tile splits and batch sizes: test_gpu_direct.py::test_tile_shares_and_batches_and_the_path_job[independent])
    finally:
        g.close()


def test_array_requests_are_checked():
    scene, g = scene_with_arrays("independent", 4, 1)
    try:
        p = scene.params()
        with pytest.raises(RuntimeError, match="next sample array"):
            g.sampler_draws(p, 0, 0, 0, [2, -3])        # the request has 4 elements
        with pytest.raises(RuntimeError, match="next sample array"):
            g.sampler_draws(p, 0, 0, 0, [2, -4, -4])    # one request only
        g.set_direct(None)
        with pytest.raises(RuntimeError, match="next sample array"):
            g.sampler_draws(p, 0, 0, 0, [-4])
    finally:
        g.close()
    scene = box_scene(sampler="hammersley")
    g = mtsg.GPUScene(scene, 0)
    try:
        g.set_direct(mtsg.DirectDesc(2, 1, 0, 0.0))
        q = scene.params()
        q.integrator = mtsg.MTSG_INTEGRATOR_DIRECT
        with pytest.raises(RuntimeError, match="Not supported for the Hammersley QMC sequence"):
            g.render(q, scene.border)
        with pytest.raises(RuntimeError, match="Not supported for the Hammersley QMC sequence"):
            g.sampler_draws(q, 0, 0, 0, [2, -2])
    finally:
        g.close()
