"""numpy oracle of `--uncertainty`: how much the test-time-augmentation views disagree (include/dnnca.h: dnnca_forward_tta_spread,
dnnca_lesion_table_spread, dnnca_spread_by_outcome).

spread_of is the float64 population standard deviation of the float32 planes after they have been mapped back to the original pixels
(tests/tta_oracle.py); the device may miss it by 2^-18 of it plus 2^-23 (tolerance).  textbook32 is what the bound must REJECT: a
float32 emulation of E[p^2] - E[p]^2, which cancels where the views agree.  families draws the five kinds of input at which the
formulations differ.

The tables are integers: a pixel's spread enters every sum as rint(max(s, 0) * 2^24) (float32 product, as the probability enters
sum_prob_q24) and every maximum as the float itself.  lesion_spread walks the components of tests/lesion_oracle.py's pipeline (resize,
threshold, opening, 4-connected components of tests/region_oracle.py, area filter, raster-order numbering) and reads the spread plane
through the same resize; outcome classes a pixel as 2 (y > 0.5) + (prob >= threshold): TN 0, FP 1, FN 2, TP 3.  png_of is the grey
value of uncertainty.png."""

import numpy as np

import lesion_oracle as LO
import region_oracle as O
import tta_oracle as TO

LESION_SPREAD_DTYPE = np.dtype([('slice', '<i4'), ('row', '<i4'), ('area', '<i4'), ('max_spread', '<f4'), ('sum_spread_q24', '<u8')])
SLICE_SPREAD_DTYPE = np.dtype([('pixels', '<i4'), ('max_spread', '<f4'), ('sum_spread_q24', '<u8')])
OUTCOME_DTYPE = np.dtype([('n', '<u8', (4,)), ('sum_q24', '<u8', (4,))])
FAMILIES = ('uniform', 'near_0.9', 'near_1', 'tiny', 'one_ulp')


def back(planes, views):
    """planes [n, B, H, W] in their views' geometry -> float32 [n, B, H, W] at the original pixels"""
    ks = TO.views_of(views)
    planes = np.asarray(planes, np.float32)
    assert len(planes) == len(ks)
    return np.stack([TO.invert_view(p, k) for p, k in zip(planes, ks)])


def spread_of(planes, views):
    """float64 [B, H, W]: the population standard deviation over the views"""
    return back(planes, views).astype(np.float64).std(axis=0)


def tolerance(want):
    return 2.0 ** -18 * np.asarray(want, np.float64) + 2.0 ** -23


def textbook32(planes, views):
    """sqrt(E[p^2] - E[p]^2) with every operation rounded to float32, sums in ascending view order"""
    p = back(planes, views)
    n = np.float32(len(p))
    s, s2 = p[0].copy(), (p[0] * p[0]).astype(np.float32)
    for q in p[1:]:
        s = (s + q).astype(np.float32)
        s2 = (s2 + (q * q).astype(np.float32)).astype(np.float32)
    mean = (s / n).astype(np.float32)
    var = ((s2 / n).astype(np.float32) - (mean * mean).astype(np.float32)).astype(np.float32)
    return np.sqrt(np.maximum(var, np.float32(0))).astype(np.float32)


def family(name, shape, seed):
    """float32 planes of `shape` ([n, B, H, W]) of one of FAMILIES"""
    rng = np.random.default_rng(seed)
    if name == 'uniform':
        v = rng.random(shape)
    elif name == 'near_0.9':
        v = 0.9 + 1e-4 * rng.standard_normal(shape)
    elif name == 'near_1':
        v = np.clip(1.0 - 1e-3 * rng.random(shape) + 1e-6 * rng.standard_normal(shape), 0.0, 1.0)
    elif name == 'tiny':
        v = 1e-6 * rng.random(shape)
    elif name == 'one_ulp':
        v = 0.75 + 2.0 ** -24 * rng.integers(0, 2, shape)
    else:
        raise ValueError(name)
    return v.astype(np.float32)


def q24(s):
    """float32 spread -> uint64 rint(max(s, 0) * 2^24), the product in float32"""
    s = np.maximum(np.asarray(s, np.float32), np.float32(0))
    return np.rint(s * np.float32(LO.Q24)).astype(np.uint64)


def lesion_spread(prob, spread, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256, resize=O.resize):
    """prob, spread [B, H, W] -> (srows LESION_SPREAD_DTYPE [n], one per row of LO.lesion_table in its order; stotals
    SLICE_SPREAD_DTYPE [B] over every pixel of the analysed plane)"""
    prob, spread = np.asarray(prob, np.float32), np.asarray(spread, np.float32)
    B, H, W = prob.shape
    assert spread.shape == prob.shape
    oh, ow = O.out_size(H, W, rf)
    pr = resize(prob, oh, ow)
    sr = np.maximum(resize(spread, oh, ow), np.float32(0)).reshape(B, oh * ow)
    fg = pr >= np.float32(threshold)
    if k > 1:
        fg = O.morph_open(fg, k)
    L = O.ccl(fg).reshape(B, oh * ow)
    q = q24(sr)
    srows, stotals = [], np.zeros(B, SLICE_SPREAD_DTYPE)
    for b in range(B):
        lab = L[b]
        roots, area = np.unique(lab[lab >= 0], return_counts=True)
        for r, root in enumerate(roots[area >= min_area][:max_lesions]):
            px = lab == root
            srows.append((b, r, int(px.sum()), sr[b][px].max(), q[b][px].sum()))
        stotals[b] = (oh * ow, sr[b].max(), q[b].sum())
    return np.array(srows, LESION_SPREAD_DTYPE), stotals


def outcome(prob, spread, y, thresholds):
    """prob, spread, y [B, h, w] -> OUTCOME_DTYPE [T, B]"""
    prob, spread, y = (np.asarray(a, np.float32).reshape(len(y), -1) for a in (prob, spread, y))
    thresholds = np.asarray(thresholds, np.float32).ravel()
    q = q24(spread)
    out = np.zeros((len(thresholds), len(y)), OUTCOME_DTYPE)
    for t, th in enumerate(thresholds):
        cls = 2 * (y > np.float32(0.5)).astype(np.int64) + (prob >= th)
        for b in range(len(y)):
            for c in range(4):
                out[t, b]['n'][c] = int((cls[b] == c).sum())
                out[t, b]['sum_q24'][c] = q[b][cls[b] == c].sum()
    return out


def png_of(spread):
    """uint8 grey value of uncertainty.png: min(255, rint(spread * 510)), so that 0.5 is white (the product is exact in float64)"""
    return np.minimum(255, np.rint(np.asarray(spread, np.float32).astype(np.float64) * 510.0)).astype(np.uint8)


def shifted32(planes, views):
    """the device's formulation with every operation rounded to float32: d_k = p_k - p_first, var = (sum d^2 - (sum d)^2 / n) / n"""
    p = back(planes, views)
    n = np.float32(len(p))
    sd, sq = np.zeros_like(p[0]), np.zeros_like(p[0])
    for q in p[1:]:
        d = (q - p[0]).astype(np.float32)
        sd = (sd + d).astype(np.float32)
        sq = (sq + (d * d).astype(np.float32)).astype(np.float32)
    var = ((sq - ((sd * sd).astype(np.float32) / n).astype(np.float32)).astype(np.float32) / n).astype(np.float32)
    return np.sqrt(np.maximum(var, np.float32(0))).astype(np.float32)
