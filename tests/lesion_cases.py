"""Drawn inputs of the lesion-table tests (tests/test_lesion_host.py, tests/test_lesion_gpu.py): patterns, never a network's output.

Probabilities are multiples of 1 / 64: foreground 0.5 .. 63 / 64 (graded, so sums, means and maxima tell pixels apart),
background 0 .. 31 / 64.  At resize_factor 1 the plane is analysed as it is; at 0.5 with even sizes every resized pixel is the
exact mean of 2 x 2 such values.  41 x 53 at 0.5 is resized with fractional weights (41 / 20, 53 / 26), where any blend of two
different values is rounded: that drawing is a plateau of exactly the threshold on a background of 0, so every foreground pixel is
a blend of equal values (exact) and every blend with the background lies below the threshold by a weight of 1 / 50 at least.
test_lesion_host.py checks for every case that the float32 and the float64 statement of the resize give the same table."""

import numpy as np


def _grade(mask, seed=0):
    h, w = mask.shape
    yy, xx = np.mgrid[0:h, 0:w]
    fg = (32 + (xx * 5 + yy * 3 + seed) % 32) / 64.0
    bg = ((xx * 7 + yy * 11 + seed) % 32) / 64.0
    return np.where(mask, fg, bg).astype(np.float32)


def tile_borders():
    """72 x 80: a snake through six 32 x 32 tiles, a block wholly inside tile (1, 1), a single pixel at (0, 0); the same drawing
    in both slices.  k = 1.  Hand count: 3 components of 1, 171 and 81 pixels, in this raster order"""
    m = np.zeros((72, 80), bool)
    m[0, 0] = True
    m[10, 5:71] = True               # tiles (0, 0), (0, 1), (0, 2)
    m[10:51, 70] = True              # down into tile (1, 2)
    m[50, 5:71] = True               # back through tiles (1, 1), (1, 0)
    m[36:45, 36:45] = True
    p = _grade(m, 1)
    return np.stack([p, p]), dict(threshold=0.5, rf=1.0, k=1)


def odd_graded():
    """41 x 53 at factor 1, k = 5: a frame 6 pixels wide (touches all four borders), a graded 12 x 14 block, a bar 3 pixels thin
    (vanishes in the opening) and a speck.  Hand count: 2 components: the frame (41 * 53 - 29 * 41 = 984) and the block (168)"""
    m = np.zeros((41, 53), bool)
    m[:6, :] = m[-6:, :] = True
    m[:, :6] = m[:, -6:] = True
    m[14:26, 12:26] = True
    m[10:32, 34:37] = True           # 3 wide: thinner than k
    m[30, 20] = True
    return _grade(m, 2)[None], dict(threshold=0.5, rf=1.0, k=5)


def odd_plateau():
    """41 x 53 at factor 0.5 (20 x 26), k = 5: a frame 12 pixels wide (touches all four borders), a 12 x 15 block and a bar 4
    pixels thin (2 resized pixels: vanishes in the opening), all at exactly the threshold on a background of 0 (see the module
    docstring).  Hand count: 2 components, the frame's box is the plane"""
    p = np.zeros((41, 53), np.float32)
    p[:12, :] = p[-12:, :] = 0.5
    p[:, :12] = p[:, -12:] = 0.5
    p[15:27, 16:31] = 0.5
    p[15:27, 34:38] = 0.5
    return p[None], dict(threshold=0.5, rf=0.5, k=5)


def even_graded_half():
    """40 x 48 at factor 0.5 (20 x 24), k = 3: graded blocks whose 2 x 2 means are exact; the statistics must be those of the
    RESIZED probabilities (the raw ones at the same coordinates differ)"""
    m = np.zeros((40, 48), bool)
    m[4:20, 6:22] = True
    m[24:38, 28:46] = True
    m[30:32, 2:12] = True            # 1 resized row: opened away
    return _grade(m, 3)[None], dict(threshold=0.5, rf=0.5, k=3)


def checkerboard():
    """24 x 40, k = 1: 480 single-pixel components"""
    yy, xx = np.mgrid[0:24, 0:40]
    return _grade((yy + xx) % 2 == 0, 4)[None], dict(threshold=0.5, rf=1.0, k=1)


def areas():
    """components of 1, 4, 9 and 100 pixels (k = 1), in this raster order of their first pixels: 9, 1, 100, 4"""
    m = np.zeros((32, 40), bool)
    m[2:5, 3:6] = True               # 9
    m[3, 20] = True                  # 1
    m[8:18, 10:20] = True            # 100
    m[20:22, 30:32] = True           # 4
    return _grade(m, 5)[None], dict(threshold=0.5, rf=1.0, k=1)


def empty_and_full():
    """40 x 72, two slices of one batch: all zero, all one; k = 5"""
    p = np.zeros((2, 40, 72), np.float32)
    p[1] = 1.0
    return p, dict(threshold=0.5, rf=1.0, k=5)


ALL = dict(tile_borders=tile_borders, odd_graded=odd_graded, odd_plateau=odd_plateau, even_graded_half=even_graded_half,
           checkerboard=checkerboard, areas=areas, empty_and_full=empty_and_full)
