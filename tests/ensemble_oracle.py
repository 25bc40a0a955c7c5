"""numpy oracle of `--ensemble`: the members of an ensemble joined per pixel (include/dnnca.h: dnnca_forward_ensemble,
dnnca_ensemble_of; kernels_ensemble.hip: ens_join).

means [n, B, h, w] are the members' mean probabilities, withins (same shape, or None for zeros) their own spreads over their views.
mean_of is what the device must EQUAL: the float32 sum in ascending member order and one float32 division.  between_of, within_of
and total_of are float64; the device may miss each by tests/spread_oracle.py's tolerance, 2^-18 of it plus 2^-23.  shifted32 is
the device's formulation with every operation rounded to float32 (d = mean_m - mean_0, nothing cancels where the members agree),
textbook32 the cancelling E[p^2] - E[p]^2 that the bound must REJECT.  The inputs are those of spread_oracle.family."""

import numpy as np

from spread_oracle import FAMILIES, family, tolerance      # noqa: F401  (the tests take them from here)

f32 = np.float32


def _planes(means, withins):
    means = np.asarray(means, f32)
    withins = np.zeros_like(means) if withins is None else np.asarray(withins, f32)
    assert means.ndim == 4 and withins.shape == means.shape
    return means, withins


def mean_of(means):
    """float32 [B, h, w]: ((m0 + m1) + m2 ...) / n, every operation rounded to float32"""
    means = np.asarray(means, f32)
    s = means[0].copy()
    for q in means[1:]:
        s = (s + q).astype(f32)
    return (s / f32(len(means))).astype(f32)


def between_of(means):
    """float64: the population standard deviation of the members' means"""
    return np.asarray(means, f32).astype(np.float64).std(axis=0)


def within_of(means, withins=None):
    """float64: the root mean square of the members' own spreads"""
    _, withins = _planes(means, withins)
    return np.sqrt((withins.astype(np.float64) ** 2).mean(axis=0))


def total_of(means, withins=None):
    """float64: the law of total variance over the n x V forwards (every member has the same V views)"""
    return np.sqrt(between_of(means) ** 2 + within_of(means, withins) ** 2)


def shifted32(means, withins=None):
    """(between, within, total) float32 as ens_join forms them, every operation rounded to float32"""
    means, withins = _planes(means, withins)
    n = f32(len(means))
    sd, sq = np.zeros_like(means[0]), np.zeros_like(means[0])
    ss = (withins[0] * withins[0]).astype(f32)
    for q, s in zip(means[1:], withins[1:]):
        d = (q - means[0]).astype(f32)
        sd = (sd + d).astype(f32)
        sq = (sq + (d * d).astype(f32)).astype(f32)
        ss = (ss + (s * s).astype(f32)).astype(f32)
    vb = ((sq - ((sd * sd).astype(f32) / n).astype(f32)).astype(f32) / n).astype(f32)
    vb = np.maximum(vb, f32(0))
    vw = (ss / n).astype(f32)
    return np.sqrt(vb).astype(f32), np.sqrt(vw).astype(f32), np.sqrt((vb + vw).astype(f32)).astype(f32)


def textbook32(means):
    """between as sqrt(E[m^2] - E[m]^2) with every operation rounded to float32, sums in ascending member order"""
    means = np.asarray(means, f32)
    n = f32(len(means))
    s, s2 = means[0].copy(), (means[0] * means[0]).astype(f32)
    for q in means[1:]:
        s = (s + q).astype(f32)
        s2 = (s2 + (q * q).astype(f32)).astype(f32)
    mean = (s / n).astype(f32)
    var = ((s2 / n).astype(f32) - (mean * mean).astype(f32)).astype(f32)
    return np.sqrt(np.maximum(var, f32(0))).astype(f32)


def drawn_withins(shape, seed, zero=False):
    """the members' own spreads: uniform in [0, 0.5], or all zero"""
    if zero:
        return np.zeros(shape, f32)
    return (0.5 * np.random.default_rng(seed).random(shape)).astype(f32)
