"""numpy oracle of `--calibration` and `--temperature` (include/dnnca.h: dnnca_calibration, dnnca_prob_temperature).

The definitions the kernels share (csrc/kernels_calib.hip), stated with float32 numpy where the device computes in float32 and with
float64 / integers where it computes in double / integers:
  class  1 when y > 0.5f, else 0
  clamp  p' = fmin(fmax(p, 0), 1) in float32: a NaN becomes 0
  q24    q = rint(p' * 2^24), the product in float32
  bin    k = min(n_bins - 1, floor(p' * float32(n_bins))), the product in float32
  logit  z = log(pc) - log1p(-pc) in float64, pc = p' clamped to [2^-24, 1 - 2^-24]
  nll    a = z * (1 / float64(float32(T))); class 1 adds softplus(-a), class 0 softplus(a); softplus(a) = max(a, 0) + log1p(exp(-|a|))
  scale  p -> float32(1 / (1 + exp(-z / float64(float32(T)))))
tables gives the integer tables (they must EQUAL the device's), nll the float64 sums (math.fsum: no summation error of its own; the
device may differ by relative NLL_RTOL), scale the scaled plane (the device within one float32 ulp).  families draws the inputs."""

import math

import numpy as np

BIN_DTYPE = np.dtype([('n', '<u8', (2,)), ('sum_q24', '<u8', (2,))])
TOTAL_DTYPE = np.dtype([('n', '<u8', (2,)), ('sum_q24', '<u8', (2,)), ('sq_lo', '<u8', (2,)), ('sq_hi', '<u8', (2,))])
Q24 = 16777216
# summing N <= 2^18 non-negative doubles in another order moves the sum by at most N 2^-53 ~ 3e-11 of it; log / exp / log1p of 1 ulp
# add far less
NLL_RTOL = 1e-9
FAMILIES = ('uniform', 'real_like', 'all_0', 'all_1', 'edges')
EDGE_BINS = (1, 10, 15, 256)


def clamp(p):
    return np.fmin(np.fmax(np.asarray(p, np.float32), np.float32(0)), np.float32(1))


def label(y):
    return np.asarray(y, np.float32) > np.float32(0.5)


def q24(p):
    return np.rint(clamp(p) * np.float32(Q24)).astype(np.uint64)


def bin_of(p, n_bins):
    return np.minimum(n_bins - 1, np.floor(clamp(p) * np.float32(n_bins)).astype(np.int64))


def tables(prob, y, n_bins):
    """prob, y [B, h, w] -> (bins BIN_DTYPE [B, n_bins], totals TOTAL_DTYPE [B])"""
    B = len(y)
    prob, y = np.asarray(prob, np.float32).reshape(B, -1), np.asarray(y, np.float32).reshape(B, -1)
    q, k, cls = q24(prob), bin_of(prob, n_bins), label(y)
    q2 = q * q                                   # at most 2^48
    bins, totals = np.zeros((B, n_bins), BIN_DTYPE), np.zeros(B, TOTAL_DTYPE)
    for b in range(B):
        for c in (0, 1):
            m = cls[b] == bool(c)
            bins[b]['n'][:, c] = np.bincount(k[b][m], minlength=n_bins)
            for kk in np.unique(k[b][m]):
                bins[b, kk]['sum_q24'][c] = sum(int(v) for v in q[b][m][k[b][m] == kk])
            totals[b]['n'][c] = int(m.sum())
            totals[b]['sum_q24'][c] = sum(int(v) for v in q[b][m])
            totals[b]['sq_lo'][c] = sum(int(v) & 0xffffffff for v in q2[b][m])
            totals[b]['sq_hi'][c] = sum(int(v) >> 32 for v in q2[b][m])
    return bins, totals


def logit(p):
    pc = np.clip(clamp(p).astype(np.float64), 2.0 ** -24, 1.0 - 2.0 ** -24)
    return np.log(pc) - np.log1p(-pc)


def softplus(a):
    return np.maximum(a, 0.0) + np.log1p(np.exp(-np.abs(a)))


def nll(prob, y, temperatures):
    """float64 [B, T]: the negative log-likelihood summed over every slice at every temperature"""
    B = len(y)
    z = logit(np.asarray(prob, np.float32).reshape(B, -1))
    sign = np.where(label(np.asarray(y, np.float32).reshape(B, -1)), -1.0, 1.0)
    out = np.zeros((B, len(temperatures)), np.float64)
    for t, T in enumerate(np.asarray(temperatures, np.float32)):
        a = z * (1.0 / np.float64(T))
        for b in range(B):
            out[b, t] = math.fsum(softplus(sign[b] * a[b]))
    return out


def scale(prob, temperature):
    """float32, the shape of prob: the probabilities at `temperature`"""
    z = logit(prob)
    return (1.0 / (1.0 + np.exp(-z / np.float64(np.float32(temperature))))).astype(np.float32)


def edge_values():
    """float32(k / n_bins) with its two neighbours for the bin counts of EDGE_BINS, exact 0 and 1, values outside [0, 1] and NaN"""
    v = [0.0, 1.0, -0.25, 1.5, np.nan, 0.5]
    for n in EDGE_BINS:
        for k in range(n + 1):
            e = np.float32(k / n)
            v += [e, np.nextafter(e, np.float32(-1)), np.nextafter(e, np.float32(2))]
    return np.array(v, np.float32)


def family(name, shape, seed):
    """(prob, y) float32 of `shape` [B, h, w] of one of FAMILIES"""
    rng = np.random.default_rng(seed)
    y = (rng.random(shape) < 0.3).astype(np.float32)
    if name == 'uniform':
        p = rng.random(shape)
    elif name == 'real_like':                    # 99 % of the pixels below 0.01 and of class 0
        hot = rng.random(shape) < 0.01
        p = np.where(hot, rng.random(shape), 0.01 * rng.random(shape))
        y = (hot & (rng.random(shape) < 0.7)).astype(np.float32)
    elif name in ('all_0', 'all_1'):
        p = rng.random(shape)
        y = np.full(shape, float(name == 'all_1'), np.float32)
    elif name == 'edges':
        e = edge_values()
        p = e[(np.arange(int(np.prod(shape))) * 7 + seed) % len(e)].reshape(shape)
        y = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), shape)      # 0.5 is class 0
    else:
        raise ValueError(name)
    return np.asarray(p, np.float32), y
