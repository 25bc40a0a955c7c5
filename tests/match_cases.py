"""Drawn inputs of the matched-lesion tests (tests/test_match_gpu.py): (prob [B, H, W], y [B, H, W], spec) at the smallest shapes
at which dnnca_lesion_table_matched can still go wrong.  The probabilities are those of tests/link_cases.py and
tests/lesion_cases.py (graded multiples of 1 / 64).  Labels are 0 / 1 unless a case says otherwise; drawings analysed at factor 0.5
keep every edge on even coordinates, so a resized pixel is the exact mean of four equal values or of values whose mean is exact."""

import numpy as np

import lesion_cases as LC
import link_cases as KC

ABOVE_HALF = np.nextafter(np.float32(0.5), np.float32(1))


def _checker(n=32):
    yy, xx = np.mgrid[0:n, 0:n]
    return (yy + xx) % 2 == 0


def checker_on_ones():
    """32 x 32, k = 1: 512 single-pixel predicted lesions on one labelled lesion that fills the plane: 512 = (hw + 1) / 2 pairs of
    one pixel, all with row_true 0: the pair table of hw + 1 slots and the pair list are at their bounds"""
    m = _checker()
    return np.stack([LC._grade(m, 1)] * 2), np.ones((2, 32, 32), np.float32), dict(threshold=0.5, rf=1.0, k=1)


def checker_on_checker():
    """32 x 32, k = 1: 512 labelled single-pixel lesions under the same 512 predicted ones: one pair each; both planes' link
    tables are at their bound as well"""
    m = _checker()
    return np.stack([LC._grade(m, 1)] * 2), np.stack([m, m]).astype(np.float32), dict(threshold=0.5, rf=1.0, k=1)


def complementary_checkers():
    """32 x 32, k = 1: the label is the other colour of the board: 512 lesions on either side and no pair at all"""
    m = _checker()
    return np.stack([LC._grade(m, 2)] * 2), np.stack([~m, ~m]).astype(np.float32), dict(threshold=0.5, rf=1.0, k=1)


def full_planes_shifted():
    """72 x 80 (23 blocks of 256 pixels, six CCL tiles), k = 1: link_cases.full_planes under its own foreground shifted right by 3
    and down by 2 pixels: a pair of 5760 pixels summed over 90 waves, and the 3 x 4 block on its shifted copy (one common pixel)"""
    prob, spec = KC.full_planes()
    return prob, np.roll(prob >= 0.5, (2, 3), axis=(1, 2)).astype(np.float32), spec


def snake_shifted():
    """72 x 80, k = 1: link_cases.shifted_snake (a snake through six tiles, a block, a pixel) under a label that is the
    prediction's foreground shifted right by 2 pixels: the snake's horizontal arms pair across three tiles"""
    prob, spec = KC.shifted_snake()
    return prob, np.roll(prob >= 0.5, 2, axis=2).astype(np.float32), spec


def resized_opened():
    """48 x 40 at factor 0.5 (24 x 20), k = 3, two slices (the second shifted right by 2 pixels).  Prediction: A (resized 5 x 6 =
    30 pixels) and B (12 x 14 = 168).  Label: Ta = 1 over A; Tb = a core of 1 inside rings of 0.75 and 0.25 (the resized label is
    not binary: 0.75 is foreground, 0.25 is not) over B; Tc = a block of nextafter(0.5, 1) (foreground) inside B; a block of
    exactly 0.5 (not foreground) inside B.  Pairs of a slice: (Ta, A), (Tb, B), (Tc, B); with min_area = 40 A is dropped and B
    becomes row 0: (Tb, 0), (Tc, 0)"""
    m = np.zeros((48, 40), bool)
    m[4:14, 4:16] = True             # A
    m[20:44, 8:36] = True            # B
    y = np.zeros((48, 40), np.float32)
    y[2:12, 2:12] = 1.0              # Ta
    y[20:38, 8:28] = 0.25
    y[22:36, 10:26] = 0.75           # Tb: resized rows 11..17, columns 5..12
    y[24:34, 12:24] = 1.0
    y[38:42, 28:34] = ABOVE_HALF     # Tc
    y[38:42, 16:22] = 0.5
    prob = np.stack([LC._grade(m, 7), LC._grade(np.roll(m, 2, axis=1), 8)])
    return prob, np.stack([y, np.roll(y, 2, axis=1)]), dict(threshold=0.5, rf=0.5, k=3)


def three_blocks():
    """32 x 40, k = 1: link_cases.three_blocks (slices A, B, C of one exam) under its foreground shifted down by 1 pixel: what the
    flag and the carry tests split and join"""
    prob, spec = KC.three_blocks()
    return prob, np.roll(prob >= 0.5, 1, axis=1).astype(np.float32), spec


ALL = dict(checker_on_ones=checker_on_ones, checker_on_checker=checker_on_checker, complementary_checkers=complementary_checkers,
           full_planes_shifted=full_planes_shifted, snake_shifted=snake_shifted, resized_opened=resized_opened,
           three_blocks=three_blocks)
