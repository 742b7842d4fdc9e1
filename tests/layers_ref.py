"""numpy helpers for the light-path layers of gi.h ("light-path layers"; DESIGN.md "Light-path
layers"). The layers are defined by the device's own reduction, so there is nothing to restate
term by term here; what can be stated independently is what the planes must satisfy:

- plane TOTAL is gi_render_radiance's frame;
- every term is non-negative, so where all other layers of a sample are exactly 0 the total's
  sequential sum and the layer's differ only by additions of +0: the same bits;
- the layers of a sample add up to the total within the rounding of two summation orders;
- a layer's mean, variance and accumulator are radiance_ref's definitions applied to its samples;
- the CLI's -vdenoise sum of the filtered layers.
"""
import numpy as np

import radiance_ref as rr

NAMES = ("surface", "specular", "indirect", "global", "caustic")
SURFACE, SPECULAR, INDIRECT, GLOBAL, CAUSTIC = range(5)
COUNT = TOTAL = 5
# two summation orders of n non-negative terms differ by at most 2 (n - 1) 2^-53 relative; a
# primary sample of the test frames has fewer than 4,096 terms: 9.1e-13
SUM_BOUND = 1e-12
assert 2 * 4095 * 2.0 ** -53 < SUM_BOUND

# flags (added to camera_cases.CORNELL_FLAGS) under which only one layer receives light, and the
# fewest of the frame's 384 pixels that must then hold a qualifying non-zero sample (the oracle,
# run with the same flags, counts 384, 20, 376, 376, 376 such pixels)
ISOLATING = {
    SURFACE: (["-no_transmissive", "-no_specular", "-no_indirect", "-no_caustic"], 300),
    SPECULAR: (["-no_direct", "-no_ambient", "-no_indirect", "-no_caustic"], 16),
    INDIRECT: (["-no_direct", "-no_ambient", "-no_caustic", "-no_transmissive", "-no_specular"], 300),
    GLOBAL: (["-no_direct", "-no_ambient", "-no_indirect", "-no_transmissive", "-no_specular",
              "-no_caustic", "-photon_viz"], 300),
    CAUSTIC: (["-no_direct", "-no_ambient", "-no_indirect", "-no_transmissive", "-no_specular"], 300),
}


def alone(samples, layer):
    """samples [6, H, W, S, 3] -> bool [H, W, S]: the samples where every other layer is exactly
    0 in every channel."""
    others = [l for l in range(COUNT) if l != layer]
    return ~np.any(samples[others] != 0.0, axis=(0, -1))


def alone_pixels(samples, layer):
    """Pixels [H, W] with at least one sample where `layer` is alone and not zero."""
    q = alone(samples, layer) & np.any(samples[layer] != 0.0, axis=-1)
    return q.any(axis=-1)


def sum_ratio(samples):
    """The largest |sum_l samples[l] - samples[TOTAL]| / samples[TOTAL] over the values whose
    total is not 0 (layers added in layer order), and whether the sum is exactly 0 wherever the
    total is."""
    s = np.zeros_like(samples[TOTAL])
    for l in range(COUNT):
        s = s + samples[l]
    tot = samples[TOTAL]
    nz = tot != 0.0
    ratio = float((np.abs(s[nz] - tot[nz]) / tot[nz]).max()) if nz.any() else 0.0
    return ratio, bool((s[~nz] == 0.0).all())


def accum_state(passes):
    """(state [H, W, 6] float64, counts [H, W] int64) of an accumulator that folded the passes
    [(samples [H, W, S, 3], box weight), ...] in order: radiance_ref.Accum's {mu, A} as
    gi_accum_export lays them out."""
    shape = np.shape(passes[0][0])[:2]
    acc = rr.Accum(shape)
    for smp, bw in passes:
        acc.add_samples(smp, bw)
    return np.concatenate([acc.mu, acc.A], axis=-1), np.full(shape, acc.N, dtype=np.int64)


def filtered_sum(parts):
    """The CLI's -layers -vdenoise image before the tone map: per channel the five float32 values
    widened to double, added in layer order, rounded to float32 once."""
    assert len(parts) == COUNT
    s = np.zeros(np.shape(parts[0]), dtype=np.float64)
    for p in parts:
        assert p.dtype == np.float32
        s = s + p.astype(np.float64)
    return s.astype(np.float32)
