"""Helpers of the `adaptive` tests: the scenes (direct_ref's box around an
`adaptive` parent), the reference's per-pixel rule (adaptive.cpp:197-284)
restated in float32 numpy over the per-sample values of the plain `path`
render, and the film it implies."""
import numpy as np

import mtsg
from conftest import SCENES
import direct_ref as DR
import multichannel_ref as R

f32 = np.float32
N_BASE = 8
PATH_PROPS = (("maxDepth", "integer", 2),)
PREPASS_SAMPLES = 10000   # nSamples (adaptive.cpp:128)


def adaptive_scene(max_error=0.05, factor=32, p_value=0.05, spp=N_BASE, sensor=None, geometry=None, film_props=(),
                   path_props=PATH_PROPS, defaults=False, **kw):
    """direct_ref's box with <integrator type="adaptive"><integrator type="path"/></integrator>."""
    b = mtsg.SceneBuilder(SCENES)
    b.integrator_child("path", list(path_props))
    b.integrator("adaptive", [] if defaults else [("maxError", "float", max_error), ("maxSampleFactor", "integer", factor),
                                                  ("pValue", "float", p_value)])
    DR.box_props(b, spp=spp, film_props=film_props, **kw)
    if sensor is not None:
        b.sensor(*sensor)
    (geometry or DR.box_geometry)(b)
    return b.finish()


def path_scene(spp, sensor=None, geometry=None, film_props=(), path_props=PATH_PROPS, **kw):
    """The same box under the plain `path` integrator at `spp` samples."""
    b = mtsg.SceneBuilder(SCENES)
    b.integrator("path", list(path_props))
    DR.box_props(b, spp=spp, film_props=film_props, **kw)
    if sensor is not None:
        b.sensor(*sensor)
    (geometry or DR.box_geometry)(b)
    return b.finish()


def luminance(rgb):
    """Spectrum::getLuminance of linear RGB (spectrum.h), one float32 rounding per operation."""
    rgb = np.asarray(rgb, f32)
    a = (rgb[..., 0] * f32(0.212671)).astype(f32)
    b = (rgb[..., 1] * f32(0.715160)).astype(f32)
    c = (rgb[..., 2] * f32(0.072169)).astype(f32)
    return ((a + b).astype(f32) + c).astype(f32)


def accepted(samples):
    """ImageBlock::put's test (imageblock.h:147-151): finite and not negative."""
    rgb = samples[..., :3]
    with np.errstate(invalid="ignore"):
        return np.isfinite(rgb).all(-1) & (rgb >= 0).all(-1)


def restate_counts(samples, n_base, factor, max_error, quantile, average_luminance):
    """adaptive.cpp:212-271 for every pixel at once: samples (h, w, cap, 4) in
    sample order -> the count at which each pixel stops (h, w) uint32.  Every
    operation is one float32 operation, in the reference's order."""
    h, w, cap = samples.shape[:3]
    ok = accepted(samples)
    with np.errstate(invalid="ignore", over="ignore"):
        lum = np.where(ok, luminance(np.where(ok[..., None], samples[..., :3], 0)), f32(0)).astype(f32)
    mean = np.zeros((h, w), f32)
    mean_sqr = np.zeros((h, w), f32)
    counts = np.zeros((h, w), np.uint32)
    active = np.ones((h, w), bool)
    quantile, max_error = f32(quantile), f32(max_error)
    floor = (f32(average_luminance) * f32(0.01)).astype(f32)
    limit = factor * n_base
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for s in range(cap):
            count = s + 1
            delta = (lum[:, :, s] - mean).astype(f32)
            mean = np.where(active, (mean + (delta / f32(count)).astype(f32)).astype(f32), mean)
            mean_sqr = np.where(active, (mean_sqr + (delta * (lum[:, :, s] - mean).astype(f32)).astype(f32)).astype(f32), mean_sqr)
            stop = np.zeros((h, w), bool)
            if count >= limit:
                stop[:] = True
            elif count >= n_base:
                variance = (mean_sqr / f32(count - 1)).astype(f32)
                std_error = np.sqrt((variance / f32(count)).astype(f32)).astype(f32)
                ci_width = (std_error * quantile).astype(f32)
                base = np.maximum(mean, floor)
                stop = ci_width <= (max_error * base).astype(f32)
            stop &= active
            counts[stop] = count
            active &= ~stop
            if not active.any():
                break
    assert not active.any(), "the sample range ends before the cap"
    return counts


def jitter_of(width, height, spp, seed=0):
    """The camera's pixel jitter (dimensions 0 and 1 of the counter RNG) of
    every sample of a width x height film at `spp` samples: (h, w, spp, 2)."""
    ys, xs, ss = np.meshgrid(np.arange(height, dtype=np.uint64), np.arange(width, dtype=np.uint64), np.arange(spp, dtype=np.uint64),
                             indexing="ij")
    key = DR.counter_key(seed, (ys * np.uint64(width) + xs) * np.uint64(spp) + ss)
    return np.stack([DR.counter_float(key, 0), DR.counter_float(key, 1)], -1)


def film_reference(D, jitter, samples, counts, width, height):
    """multichannel_ref.film_reference with a per-sample factor: sample s of
    pixel p enters with 1 / n_p (one float32 rounding, adaptive.cpp:275) while
    s < n_p and ImageBlock::put accepts it, else not at all.  Channels: rgb,
    alpha, weight.  Returns the float64 block and the sums of |w v| x factor."""
    cap = samples.shape[2]
    take = (np.arange(cap)[None, None, :] < counts[:, :, None]) & accepted(samples)
    factor = np.where(take, (f32(1) / counts.astype(f32)).astype(f32)[:, :, None], f32(0)).astype(np.float64)
    values = np.concatenate([np.where(take[..., None], samples, 0).astype(np.float64), np.ones(samples.shape[:3] + (1,))], -1)
    return R.film_reference(D, jitter, values * factor[..., None], width, height)


def film_terms(D, cap):
    """Float32 operations behind one texel: (2 border + 1)^2 windows of up to
    `cap` fused terms, one scaling and two additions (LDS, film) each."""
    return (2 * D.border + 1) ** 2 * (cap + 3)


def film_error(block, want, mag, n_terms):
    """max over texels and channels of |block - want| in units of the bound
    n_terms 2^-24 sum|w v| (texels whose sum is zero must be zero)."""
    bound = n_terms * 2.0 ** -24 * mag
    err = np.abs(block.astype(np.float64) - want)
    assert np.all(err[bound == 0] == 0)
    return float((err[bound > 0] / bound[bound > 0]).max())
