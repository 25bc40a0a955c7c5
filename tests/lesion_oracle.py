"""numpy oracle of the lesion table (dnnca_lesion_table), built on tests/region_oracle.py: resize, threshold,
opening and the 4-connected components are that module's; here the area filter, the raster-order numbering, the per-lesion
statistics and the cleaned mask are restated.

A component's root is its smallest pixel index, so "raster order of the root" is the order of the sorted root indices of a slice.
Every statistic is an integer sum or an extremum: area, bounding box (inclusive), sum of x, sum of y, the sum of
rint(p * 2^24) over the component's pixels (p: the resized float32 probability that was thresholded) and the largest p.

`resize` may be replaced (resize64: the same bilinear formula stated in float64 and rounded to float32 once at the end): the test
inputs are drawn so that both statements give the same table, i.e. no result hangs on how a product or a sum was rounded."""

import numpy as np

import region_oracle as O

ROW_DTYPE = np.dtype([('slice', '<i4'), ('row', '<i4'), ('area', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'), ('y1', '<i4'),
                      ('max_prob', '<f4'), ('sum_x', '<u8'), ('sum_y', '<u8'), ('sum_prob_q24', '<u8')])
Q24 = float(1 << 24)


def resize64(img, oh, ow):
    """O.resize with every product and sum in float64 (the scale is still the float32 in / out of TF), rounded to float32 once"""
    img = np.asarray(img, np.float32)
    h, w = img.shape[-2:]
    if (oh, ow) == (h, w):
        return img
    a = img.astype(np.float64)

    def axis(n_in, n_out):
        scale = np.float64(np.float32(np.float32(n_in) / np.float32(n_out)))
        src = (np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5
        fl = np.floor(src)
        return np.maximum(fl.astype(np.int64), 0), np.minimum(np.ceil(src).astype(np.int64), n_in - 1), src - fl

    y0, y1, ly = axis(h, oh)
    x0, x1, lx = axis(w, ow)
    tl, tr = a[..., y0, :][..., x0], a[..., y0, :][..., x1]
    bl, br = a[..., y1, :][..., x0], a[..., y1, :][..., x1]
    top = tl + (tr - tl) * lx
    bot = bl + (br - bl) * lx
    return (top + (bot - top) * ly[:, None]).astype(np.float32)


def lesion_table(prob, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256, resize=O.resize):
    """prob [B, H, W] -> (rows ROW_DTYPE [n], totals int32 [B], mask uint8 [B, oh, ow]).  rows: slice after slice, at most
    max_lesions per slice in raster order of the roots; totals: kept components per slice (may exceed max_lesions); mask: 255 on
    every kept component (also those beyond max_lesions), 0 elsewhere"""
    prob = np.asarray(prob, np.float32)
    if prob.ndim == 4:
        prob = prob[..., 0]
    B, H, W = prob.shape
    oh, ow = O.out_size(H, W, rf)
    pr = resize(prob, oh, ow)
    fg = pr >= np.float32(threshold)
    if k > 1:
        fg = O.morph_open(fg, k)
    L = O.ccl(fg).reshape(B, oh * ow)                                  # roots: flat index over [B, oh, ow]
    yy, xx = np.divmod(np.arange(oh * ow, dtype=np.int64), ow)
    q24 = np.rint(pr.reshape(B, oh * ow).astype(np.float32) * np.float32(Q24)).astype(np.uint64)
    rows, totals = [], np.zeros(B, np.int32)
    mask = np.zeros((B, oh * ow), np.uint8)
    for b in range(B):
        lab = L[b]
        roots, area = np.unique(lab[lab >= 0], return_counts=True)      # sorted: raster order of the roots
        keep = area >= min_area
        totals[b] = int(keep.sum())
        mask[b][np.isin(lab, roots[keep])] = 255
        for r, root in enumerate(roots[keep][:max_lesions]):
            px = lab == root
            p = pr[b].reshape(-1)[px]
            rows.append((b, r, int(px.sum()), xx[px].min(), yy[px].min(), xx[px].max(), yy[px].max(), p.max(),
                         xx[px].sum(), yy[px].sum(), q24[b][px].sum()))
    return np.array(rows, ROW_DTYPE), totals, mask.reshape(B, oh, ow)
