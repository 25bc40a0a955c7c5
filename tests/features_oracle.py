"""numpy oracle of `predict --lesion_features` (include/dnnca.h: dnnca_lesion_table_features), built on tests/lesion_oracle.py: the
rows are LO.lesion_table's and the components come out of the same pipeline (O.resize, threshold, O.morph_open, O.ccl, area filter,
raster-order numbering).  Restated here: the value of a pixel and channel, the shape, body and ring records and the histogram.

A value is x' -- the channel through O.resize, the float32 statement of the resize the probabilities went through -- clamped as
v = min(max(x', 0), 1) with NaN = 0; q = rint(v * 2^16) and the bin min(bins - 1, floor(v * bins)) are float32 products.  Every sum
is made of Python integers (and stored as uint64), every extremum is the float32 itself.  The ring ownership is a direct scan of the
(2R + 1)^2 window of every background pixel."""

import numpy as np

import lesion_oracle as LO
import region_oracle as O

SHAPE_DTYPE = np.dtype([('slice', '<i4'), ('row', '<i4'), ('area', '<i4'), ('boundary', '<i4'), ('edges', '<i4'), ('reserved', '<i4'),
                        ('sum_xx', '<u8'), ('sum_yy', '<u8'), ('sum_xy', '<u8')])
INTENSITY_DTYPE = np.dtype([('slice', '<i4'), ('row', '<i4'), ('channel', '<i4'), ('n', '<i4'), ('min', '<f4'), ('max', '<f4'),
                            ('sum_q16', '<u8'), ('sum_sq_q16', '<u8')])
Q16 = np.float32(65536.0)


def values(x, oh, ow, resize=O.resize):
    """x [B, H, W, C] -> v float32 [B, C, oh, ow]: resized per channel, clamped to [0, 1], NaN = 0"""
    x = np.ascontiguousarray(np.moveaxis(np.asarray(x, np.float32), -1, 1))
    with np.errstate(invalid='ignore'):
        xr = resize(x, oh, ow)
        return np.where(xr > 0, np.minimum(xr, np.float32(1)), np.float32(0)).astype(np.float32)


def q16(v):
    return [int(q) for q in np.rint(np.asarray(v, np.float32) * Q16).astype(np.int64)]


def bin_of(v, bins):
    return np.minimum(bins - 1, np.floor(np.asarray(v, np.float32) * np.float32(bins)).astype(np.int64))


def intensity(b, r, c, v):
    """the record of the float32 values v (one channel of the pixels of a body or a ring; may be empty)"""
    q = q16(v)
    return (b, r, c, len(q), v.min() if len(q) else 0.0, v.max() if len(q) else 0.0, sum(q), sum(i * i for i in q))


def components(prob, threshold, rf, k, min_area, max_lesions, resize=O.resize):
    """-> (oh, ow, rowmap int64 [B, oh, ow]: a numbered lesion's row, -1 on background, -2 on kept components beyond max_lesions)"""
    prob = np.asarray(prob, np.float32)
    B, H, W = prob.shape
    oh, ow = O.out_size(H, W, rf)
    fg = resize(prob, oh, ow) >= np.float32(threshold)
    if k > 1:
        fg = O.morph_open(fg, k)
    L = O.ccl(fg).reshape(B, oh * ow)
    rowmap = np.full((B, oh * ow), -1, np.int64)
    for b in range(B):
        roots, area = np.unique(L[b][L[b] >= 0], return_counts=True)
        for r, root in enumerate(roots[area >= min_area]):
            rowmap[b][L[b] == root] = r if r < max_lesions else -2
    return oh, ow, rowmap.reshape(B, oh, ow)


def lesion_features(prob, x, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256, bins=32, ring=3, resize=O.resize):
    """prob [B, H, W], x [B, H, W, C] -> (shape SHAPE_DTYPE [n], body INTENSITY_DTYPE [n, C], ring INTENSITY_DTYPE [n, C] or None
    (ring == 0), hist uint32 [n, C, bins] or None (bins == 0)), one entry per row of LO.lesion_table in its order"""
    x = np.asarray(x, np.float32)
    C = x.shape[-1]
    oh, ow, rowmap = components(prob, threshold, rf, k, min_area, max_lesions, resize)
    v = values(x, oh, ow, resize)
    B = len(rowmap)
    shape, body, rng, hist = [], [], [], []
    for b in range(B):
        rm = rowmap[b]
        n_rows = int(rm.max()) + 1 if (rm >= 0).any() else 0
        owner = np.full((oh, ow), -1, np.int64)                       # ring ownership: the smallest row in the clipped window
        if ring > 0:
            for y, xx in zip(*np.nonzero(rm == -1)):
                win = rm[max(y - ring, 0):y + ring + 1, max(xx - ring, 0):xx + ring + 1]
                if (win >= 0).any():
                    owner[y, xx] = win[win >= 0].min()
        pad = np.full((oh + 2, ow + 2), -3, np.int64)                 # outside the plane: no lesion
        pad[1:-1, 1:-1] = rm
        for r in range(n_rows):
            px = rm == r
            ys, xs = np.nonzero(px)
            faces = sum((pad[1 + ys + dy, 1 + xs + dx] != r).astype(np.int64) for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)))
            ys, xs = [int(i) for i in ys], [int(i) for i in xs]
            shape.append((b, r, len(ys), int((faces > 0).sum()), int(faces.sum()), 0, sum(i * i for i in xs), sum(i * i for i in ys),
                          sum(i * j for i, j in zip(xs, ys))))
            body.append([intensity(b, r, c, v[b, c][px]) for c in range(C)])
            if ring > 0:
                rng.append([intensity(b, r, c, v[b, c][owner == r]) for c in range(C)])
            if bins > 0:
                hist.append([np.bincount(bin_of(v[b, c][px], bins), minlength=bins) for c in range(C)])
    return (np.array(shape, SHAPE_DTYPE),
            np.array([tuple(t) for row in body for t in row], INTENSITY_DTYPE).reshape(len(shape), C),
            np.array([tuple(t) for row in rng for t in row], INTENSITY_DTYPE).reshape(len(shape), C) if ring > 0 else None,
            np.array(hist, np.uint32).reshape(len(shape), C, bins) if bins > 0 else None)
