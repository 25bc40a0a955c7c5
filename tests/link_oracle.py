"""numpy statement of the links of dnnca_lesion_table_linked, built on tests/region_oracle.py: resize,
threshold, opening and the 4-connected components are that module's.  Kept components are numbered as tests/lesion_oracle.py
numbers them (raster order of the root, min_area, the first max_lesions); here the per-pixel row map is built from that numbering
and the common pixels of every (row of the slice before, row of the slice) pair are counted for the slices whose flag is set."""

import numpy as np

import region_oracle as O

LINK_DTYPE = np.dtype([('slice', '<i4'), ('row_prev', '<i4'), ('row', '<i4'), ('overlap', '<i4')])


def row_maps(prob, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256):
    """prob [B, H, W] -> int32 [B, oh * ow]: the row number of every pixel's lesion; -1 on background, in a component below
    min_area and in one beyond the first max_lesions of its slice"""
    prob = np.asarray(prob, np.float32)
    B, H, W = prob.shape
    oh, ow = O.out_size(H, W, rf)
    fg = O.resize(prob, oh, ow) >= np.float32(threshold)
    if k > 1:
        fg = O.morph_open(fg, k)
    L = O.ccl(fg).reshape(B, oh * ow)
    maps = np.full((B, oh * ow), -1, np.int32)
    for b in range(B):
        roots, area = np.unique(L[b][L[b] >= 0], return_counts=True)       # sorted: raster order of the roots
        for r, root in enumerate(roots[area >= min_area][:max_lesions]):
            maps[b][L[b] == root] = r
    return maps


def links_of_maps(maps, continues, carry=None):
    """maps int32 [B, hw], continues [B] -> links LINK_DTYPE sorted by (slice, row_prev, row).  Slice 0 links to `carry` (the map
    of the slice before the batch) when its flag is set"""
    out = []
    for b in range(len(maps)):
        if not continues[b]:
            continue
        prev = carry if b == 0 else maps[b - 1]
        assert prev is not None, 'continues[0] without a slice before'
        both = (prev >= 0) & (maps[b] >= 0)
        if not both.any():
            continue
        pairs, n = np.unique(np.stack([prev[both], maps[b][both]], 1), axis=0, return_counts=True)    # sorted by (prev, cur)
        out += [(b, int(p), int(c), int(m)) for (p, c), m in zip(pairs, n)]
    return np.array(out, LINK_DTYPE)


def links(prob, continues, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256, carry=None):
    """the links of one call on prob [B, H, W]; carry: the row map of the last slice of the call before (row_maps(...)[-1])"""
    return links_of_maps(row_maps(prob, threshold, rf, k, min_area, max_lesions), continues, carry)
