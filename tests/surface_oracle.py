"""numpy statement of dnnca_surface_distances, brute force.  The two masks are taken from the oracles that
already state them: the prediction mask is the cleaned mask of tests/lesion_oracle.py (every kept component), the label foreground
the pixels that lie in any labelled lesion of tests/match_oracle.py.  Here: the boundary by the four shifts, and the squared distance
of every boundary pixel to the nearest boundary pixel of the other mask by the full pairwise table (the planes are tiny)."""

import numpy as np

import lesion_oracle as LO
import match_oracle as MO

SAMPLE_DTYPE = np.dtype([('slice', '<i4'), ('side', '<i4'), ('pixel', '<i4'), ('d2', '<i4')])


def masks(prob, y, threshold=0.5, rf=1.0, k=5, min_area=0):
    """(prediction mask, label foreground), bool [B, oh, ow] each"""
    prob, y = np.asarray(prob, np.float32), np.asarray(y, np.float32)
    pred = LO.lesion_table(prob, threshold, rf, k, min_area, max_lesions=1)[2] > 0      # the mask does not look at max_lesions
    B, oh, ow = pred.shape
    true = (MO.true_maps(y, rf, max_lesions=oh * ow) >= 0).reshape(B, oh, ow)           # no component is beyond oh * ow rows
    return pred, true


def boundary(mask):
    """a foreground pixel with one of its four neighbours in the background or outside the plane; mask bool [..., h, w]"""
    m = np.asarray(mask, bool)
    p = np.zeros(m.shape[:-2] + (m.shape[-2] + 2, m.shape[-1] + 2), bool)
    p[..., 1:-1, 1:-1] = m
    inside = p[..., :-2, 1:-1] & p[..., 2:, 1:-1] & p[..., 1:-1, :-2] & p[..., 1:-1, 2:]
    return m & ~inside


def nearest_d2(edge, other_edge):
    """int64 [n]: for every pixel of `edge` (bool [h, w], raster order) the smallest squared distance to a pixel of `other_edge`"""
    ay, ax = np.nonzero(edge)
    by, bx = np.nonzero(other_edge)
    table = (ay[:, None] - by[None, :]) ** 2 + (ax[:, None] - bx[None, :]) ** 2
    return table.min(axis=1)


def surface(prob, y, threshold=0.5, rf=1.0, k=5, min_area=0, max_samples=65536):
    """(counts int32 [B, 5], samples SAMPLE_DTYPE sorted by (slice, side, pixel), edges uint8 [B, oh, ow])"""
    pred, true = masks(prob, y, threshold, rf, k, min_area)
    ep, et = boundary(pred), boundary(true)
    B, oh, ow = pred.shape
    counts = np.stack([pred.sum((1, 2)), true.sum((1, 2)), (pred & true).sum((1, 2)), ep.sum((1, 2)), et.sum((1, 2))], 1).astype(np.int32)
    out = []
    for b in range(B):
        if not (0 < counts[b, 3] <= max_samples and 0 < counts[b, 4] <= max_samples):
            continue
        for side, (mine, other) in enumerate(((ep[b], et[b]), (et[b], ep[b]))):
            out += [(b, side, int(p), int(d)) for p, d in zip(np.flatnonzero(mine), nearest_d2(mine, other))]
    return counts, np.array(out, SAMPLE_DTYPE), (ep.astype(np.uint8) | (et.astype(np.uint8) << 1))
