"""Drawn inputs of the slice-link tests (tests/test_link_host.py, tests/test_link_gpu.py): stacks of slices [B, H, W] whose
lesions overlap from slice to slice in known ways.  Probabilities are graded multiples of 1 / 64 as in tests/lesion_cases.py
(foreground 0.5 .. 63 / 64, background below 0.5); drawings analysed at factor 0.5 keep every block edge on even coordinates, so a
resized pixel is the exact mean of four foreground or four background values, or they are plateaus of exactly the threshold."""

import numpy as np

import lesion_cases as LC


def _case(masks, seed, **spec):
    return np.stack([LC._grade(m, seed + i) for i, m in enumerate(masks)]), dict(dict(threshold=0.5, rf=1.0, k=1), **spec)


def checker_on_checker():
    """32 x 32, k = 1: 512 single-pixel lesions on the same 512.  512 = (hw + 1) / 2 links of one pixel: the pair table of
    hw + 1 slots and the link list are at their bounds, and every wave of 64 pixels carries 32 distinct keys"""
    yy, xx = np.mgrid[0:32, 0:32]
    m = (yy + xx) % 2 == 0
    return _case([m, m], 1)


def crossing_stripes():
    """32 x 32, k = 1: the 16 even columns under the 16 even rows: 256 links of one pixel, 16 per lesion of either slice"""
    yy, xx = np.mgrid[0:32, 0:32]
    return _case([xx % 2 == 0, yy % 2 == 0], 2)


def full_planes():
    """72 x 80 (23 blocks of 256 pixels), k = 1: a full plane on a full plane (one link of 5760 pixels, summed over 90 waves),
    then a block of 3 x 4 pixels on the full plane (one link of 12)"""
    full = np.ones((72, 80), bool)
    small = np.zeros((72, 80), bool)
    small[40:43, 50:54] = True
    return _case([full, full, small], 3)


def shifted_snake():
    """72 x 80, k = 1: the drawing of lesion_cases.tile_borders (a snake through six tiles, a block, a pixel) under a copy shifted
    right by 3 columns: the snake's horizontal arms share 63 pixels each (columns 8..70 of rows 10 and 50, through three tiles),
    its vertical arms and the single pixels miss each other, the blocks share 9 x 6"""
    p = LC.tile_borders()[0][0] >= 0.5
    return _case([p, np.roll(p, 3, axis=1)], 4)


def plateau_half():
    """41 x 53 at factor 0.5 (20 x 26), k = 5: the frame of lesion_cases.odd_plateau alone, the whole drawing (frame: row 0, block:
    row 1), the block alone: links (frame, frame) and (block, block), none between frame and block.
    Plateaus of exactly the threshold on 0: the fractional resize weights blend equal values only"""
    a = LC.odd_plateau()[0][0]
    frame, block = a.copy(), np.zeros_like(a)
    frame[15:27, 16:38] = 0.0
    block[15:27, 16:31] = 0.5
    return np.stack([frame, a, block]), dict(threshold=0.5, rf=0.5, k=5)


def graded_half():
    """40 x 48 at factor 0.5 (20 x 24), k = 3.  Resized areas: slice 0 holds A0 (30 pixels) and B0 (150); slice 1 holds A1 (100, on
    A0), C1 (35, on B0) and D1 (77, on B0), in this raster order.  Without an area filter: links (0, 0), (1, 1), (1, 2).  With
    min_area = 40, A0 and C1 are dropped and the rows renumbered: B0 is row 0, A1 row 0, D1 row 1 -- the one link is (0, 1)"""
    m0, m1 = np.zeros((40, 48), bool), np.zeros((40, 48), bool)
    m0[2:12, 2:14] = True            # A0: rows 1..5, columns 1..6 of the resized plane
    m0[16:36, 10:40] = True          # B0: rows 8..17, columns 5..19
    m1[4:14, 4:44] = True            # A1: rows 2..6, columns 2..21
    m1[20:30, 2:16] = True           # C1: rows 10..14, columns 1..7
    m1[24:38, 24:46] = True          # D1: rows 12..18, columns 12..22
    return _case([m0, m1], 5, rf=0.5, k=3)


def three_blocks():
    """32 x 40, k = 1: three slices A, B, C of one exam: lesion_cases.areas shifted right by 0, 2 and 4 pixels plus a bar that is in
    B and C only.  What the flag and the carry tests split and join"""
    a = LC.areas()[0][0] >= 0.5
    bar = np.zeros_like(a)
    bar[26:29, 4:30] = True
    return _case([a, np.roll(a, 2, axis=1) | bar, np.roll(a, 4, axis=1) | bar], 6)


ALL = dict(checker_on_checker=checker_on_checker, crossing_stripes=crossing_stripes, full_planes=full_planes,
           shifted_snake=shifted_snake, plateau_half=plateau_half, graded_half=graded_half, three_blocks=three_blocks)
