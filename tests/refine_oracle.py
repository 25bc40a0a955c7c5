"""numpy oracle of the mask refinement (dnnca_model_set_lesion_refine) on top of tests/region_oracle.py
(resize, morph_open, ccl) and tests/lesion_oracle.py (the table's dtype and q24 rule).  The prediction mask of a slice is, in order:

  hysteresis   M_low = p >= low, M_high = p >= threshold (float32, the same resized p): the 4-connected components of M_low that
               hold a pixel of M_high.  Off: M_high
  opening      region_oracle.morph_open with the filter size, unchanged
  closing      dilation then erosion over [y - c, y + c] x [x - c, x + c], c = (size - 1) / 2, out-of-plane pixels ignored in both
               (OR pads with False, AND pads with True): the dual of morph_open.  Odd sizes only
  fill_holes   a 4-connected component of the background with no pixel in the first or last row or column becomes foreground
then components, area filter, numbering and statistics exactly as tests/lesion_oracle.py states them, over the refined mask.

hysteresis and fill_holes are stated twice: through region_oracle.ccl (what the device does: label, mark roots, keep) and as a plain
breadth-first flood fill from the seeds / from the border (`*_flood`), which shares nothing with ccl."""

from collections import deque

import numpy as np

import lesion_oracle as LO
import region_oracle as O
import surface_oracle as SO

OFF = dict(hysteresis=None, closing=0, fill_holes=False)


def config(refine):
    """a refine spec (None, or a dict with some of hysteresis / closing / fill_holes) with every key"""
    cfg = dict(OFF, **(refine or {}))
    unknown = sorted(set(cfg) - set(OFF))
    if unknown:
        raise ValueError('unknown refine keys %s' % unknown)
    return cfg


def hysteresis(low_mask, high_mask):
    """bool [..., H, W]: the components of low_mask (4-connected, per plane) that contain a pixel of high_mask"""
    low, high = np.asarray(low_mask, bool), np.asarray(high_mask, bool)
    L = O.ccl(low).ravel()
    seeds = high.ravel() & (L >= 0)
    keep = np.zeros(L.size, bool)
    keep[L[seeds]] = True
    return ((L >= 0) & keep[np.maximum(L, 0)]).reshape(low.shape)


def _flood(passable, seeds):
    """one plane: the pixels of `passable` reached from `seeds` (a subset of it) through 4-neighbours, breadth first"""
    H, W = passable.shape
    seen = seeds & passable
    todo = deque(zip(*np.nonzero(seen)))
    while todo:
        y, x = todo.popleft()
        for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= ny < H and 0 <= nx < W and passable[ny, nx] and not seen[ny, nx]:
                seen[ny, nx] = True
                todo.append((ny, nx))
    return seen


def _planes(a):
    a = np.asarray(a, bool)
    return a.reshape((-1,) + a.shape[-2:])


def hysteresis_flood(low_mask, high_mask):
    low = np.asarray(low_mask, bool)
    return np.stack([_flood(l, h.copy()) for l, h in zip(_planes(low), _planes(high_mask))]).reshape(low.shape)


def close(mask, size):
    """closing of bool [..., H, W] by the size x size square (odd); 0 or 1: the mask itself"""
    mask = np.asarray(mask, bool)
    if size in (0, 1):
        return mask
    if size < 0 or size % 2 == 0 or size > 15:
        raise ValueError('closing size %r (odd, 3 .. 15)' % (size,))
    # odd size: region_oracle's window [y - (k - 1) // 2, y + k // 2] is the symmetric one
    return O._window(O._window(mask, size, np.logical_or, False), size, np.logical_and, True)


def fill_holes(mask):
    """bool [..., H, W] plus every background component (4-connected, per plane) that does not touch the plane's outer border"""
    mask = np.asarray(mask, bool)
    bg = ~mask
    L = O.ccl(bg)
    border = np.zeros(mask.shape, bool)
    border[..., 0, :] = border[..., -1, :] = border[..., :, 0] = border[..., :, -1] = True
    open_roots = np.zeros(L.size, bool)
    open_roots[L[border & bg]] = True
    return mask | (bg & ~open_roots[np.maximum(L, 0)].reshape(mask.shape))


def fill_holes_flood(mask):
    mask = np.asarray(mask, bool)
    out = []
    for m in _planes(mask):
        border = np.zeros(m.shape, bool)
        border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
        out.append(~_flood(~m, border & ~m))
    return np.stack(out).reshape(mask.shape)


def refined_mask(prob, threshold, rf, k, refine=None, resize=O.resize):
    """prob [B, H, W] -> (the resized planes float32 [B, oh, ow], the refined mask bool [B, oh, ow]) before the area filter"""
    cfg = config(refine)
    prob = np.asarray(prob, np.float32)
    if prob.ndim == 4:
        prob = prob[..., 0]
    oh, ow = O.out_size(prob.shape[1], prob.shape[2], rf)
    pr = resize(prob, oh, ow)
    with np.errstate(invalid='ignore'):
        fg = pr >= np.float32(threshold)
        if cfg['hysteresis'] is not None:
            low = np.float32(cfg['hysteresis'])
            if not 0 < low < np.float32(threshold):
                raise ValueError('hysteresis %r must lie in (0, threshold %r)' % (cfg['hysteresis'], threshold))
            fg = hysteresis(pr >= low, fg)
    if k > 1:
        fg = O.morph_open(fg, k)
    fg = close(fg, cfg['closing'])
    if cfg['fill_holes']:
        fg = fill_holes(fg)
    return pr, fg


def table_of_mask(pr, fg, min_area=0, max_lesions=256):
    """tests/lesion_oracle.py's components, area filter, numbering and statistics on a given mask: (rows, totals, mask)"""
    B, oh, ow = fg.shape
    L = O.ccl(fg).reshape(B, oh * ow)
    yy, xx = np.divmod(np.arange(oh * ow, dtype=np.int64), ow)
    with np.errstate(invalid='ignore'):          # (a NaN pixel is background unless closing or filling covers it: not a defined input)
        q24 = np.rint(pr.reshape(B, oh * ow).astype(np.float32) * np.float32(LO.Q24)).astype(np.uint64)
    rows, totals = [], np.zeros(B, np.int32)
    mask = np.zeros((B, oh * ow), np.uint8)
    for b in range(B):
        lab = L[b]
        roots, area = np.unique(lab[lab >= 0], return_counts=True)
        keep = area >= min_area
        totals[b] = int(keep.sum())
        mask[b][np.isin(lab, roots[keep])] = 255
        for r, root in enumerate(roots[keep][:max_lesions]):
            px = lab == root
            p = pr[b].reshape(-1)[px]
            rows.append((b, r, int(px.sum()), xx[px].min(), yy[px].min(), xx[px].max(), yy[px].max(), p.max(),
                         xx[px].sum(), yy[px].sum(), q24[b][px].sum()))
    return np.array(rows, LO.ROW_DTYPE), totals, mask.reshape(B, oh, ow)


def lesion_table(prob, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256, resize=O.resize, refine=None):
    """what lesion_oracle.lesion_table returns, on the refined mask"""
    pr, fg = refined_mask(prob, threshold, rf, k, refine, resize)
    return table_of_mask(pr, fg, min_area, max_lesions)


def row_maps(prob, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256, refine=None):
    """tests/link_oracle.py's row_maps on the refined mask: int32 [B, oh * ow], the row of every pixel (-1: none, also beyond
    max_lesions)"""
    pr, fg = refined_mask(prob, threshold, rf, k, refine)
    B, oh, ow = fg.shape
    L = O.ccl(fg).reshape(B, oh * ow)
    maps = np.full((B, oh * ow), -1, np.int32)
    for b in range(B):
        roots, area = np.unique(L[b][L[b] >= 0], return_counts=True)
        for r, root in enumerate(roots[area >= min_area][:max_lesions]):
            maps[b][L[b] == root] = r
    return maps


def surface(prob, y, threshold=0.5, rf=1.0, k=5, min_area=0, max_samples=65536, refine=None):
    """tests/surface_oracle.py's surface with the refined prediction mask (every kept component) and the unrefined label"""
    pred = lesion_table(prob, threshold, rf, k, min_area, 1, refine=refine)[2] > 0
    true = SO.masks(prob, y, threshold, rf, k, min_area)[1]
    ep, et = SO.boundary(pred), SO.boundary(true)
    B = pred.shape[0]
    counts = np.stack([pred.sum((1, 2)), true.sum((1, 2)), (pred & true).sum((1, 2)), ep.sum((1, 2)), et.sum((1, 2))], 1).astype(np.int32)
    out = []
    for b in range(B):
        if not (0 < counts[b, 3] <= max_samples and 0 < counts[b, 4] <= max_samples):
            continue
        for side, (mine, other) in enumerate(((ep[b], et[b]), (et[b], ep[b]))):
            out += [(b, side, int(p), int(d)) for p, d in zip(np.flatnonzero(mine), SO.nearest_d2(mine, other))]
    return counts, np.array(out, SO.SAMPLE_DTYPE), (ep.astype(np.uint8) | (et.astype(np.uint8) << 1))
