"""The augmentation kernels of csrc/kernels_aug.hip (k_aug_sums, k_aug_apply, k_warp, k_warp_groups<false / true>) against
oracle/augment_oracle.py at the shapes where they can go wrong: more than one block per image and the 64-block cap of the sums,
every position of the label, eight channels, partial and empty contrast masks, windows on two borders, odd margins and widths,
non-square images with a partial last block, control-point counts that need a second pass of the coefficient copy (n = 150) and
that fill the 64 KB of LDS (n = 2046), one and eight channels, both layouts of the groups kernel, and both pinned rings under
back-to-back calls.  Inputs, references and checks live in tests/augment_edges.py; tests/test_augment_edges.py rehearses them on
the CPU and shows which check catches which defect.  NOTES.md ("Augmentation kernels at their edges") maps every arm to its test.

Bounds are those of tests/test_augment.py and tests/test_intrawarp_gpu.py: y bit-exact, x bit-exact where nothing is adjusted and
|dx| <= 2e-6 where it is, sampling positions <= 1e-2 px, smooth channels <= 1e-3, every ramp moved by more than a pixel.  The
float32 restatement of the kernels uses 5.98e-06 px and 2.19e-07 of the two warp bounds on these inputs (measured on the CPU,
tests/test_augment_edges.py), so the bounds leave the oracle three orders of room.

Measured on the MI355X (one run, every test passing): positions at most 5.98e-06 px, smooth channels 2.19e-07, adjusted |dx|
1.19e-07, every bit-exact assertion held, the two layouts of k_warp_groups bit-identical on all five cases.  NOTES.md has the
table per case."""

import ctypes as C

import numpy as np
import pytest

import augment_edges as E

pytestmark = pytest.mark.gpu
LAYOUT_ENV = 'DNNCA_WARP_GROUPS_PIXEL'           # read per call by dnnca_warp_groups_f32: set = one pixel per thread, groups in a loop


def _layouts(monkeypatch):
    """the two layouts of k_warp_groups, block-per-group first"""
    monkeypatch.delenv(LAYOUT_ENV, raising=False)
    yield 'group per block'
    monkeypatch.setenv(LAYOUT_ENV, '1')
    yield 'pixel per thread'
    monkeypatch.delenv(LAYOUT_ENV, raising=False)


# ---------------------------------------------------------------------------------------------------------- crop / flip / contrast
@pytest.mark.parametrize('variant', E.AUG_VARIANTS)
@pytest.mark.parametrize('name', sorted(E.AUG_SHAPES))
def test_augment_edges(gpu, name, variant):
    """k_aug_sums + k_aug_apply against A.augment_batch.  In every batch image 0 sits at top = 0, left + wo = ws, flipped, factor
    1.2; image 1 has factor exactly 1.0; one channel is all 255 (and one all 0) under a factor != 1.  variant 'default': every
    feature channel; 'subset': a proper subset (with one feature channel: that channel and the LABEL's bit, which must have no
    effect); 'none': contrast_channels=() as evaluate passes it -- bit-equal to the oracle at factor 1 and no aug_sums launch."""
    B, hs, ws, cs, label, ho, wo = E.AUG_SHAPES[name]
    dev = E.GpuDevice(gpu, cs - 1, ho, wo, B, profile=True)
    try:
        E.check_augment(dev, name, variant)
    finally:
        dev.close()


def test_augment_ring(gpu):
    """six dnnca_augment_u8 calls back to back, each with draws and outputs of its own and no read or sync in between (the ring
    has four rows), a seventh with batch 5 > max_batch 2 (the ring regrows), ONE sync, then all seven against the oracle"""
    dev = E.GpuDevice(gpu, 2, 16, 12, E.RING_MAX_BATCH)
    try:
        E.check_augment_burst(dev)
    finally:
        dev.close()


def test_warp_groups_ring(gpu, monkeypatch):
    """the same for dnnca_warp_groups_f32: six calls with coefficients of their own, a seventh with four groups instead of two
    (its row outgrows the ring's), one sync; under both layouts"""
    for layout in _layouts(monkeypatch):
        dev = E.GpuDevice(gpu, 3, 12, 20, 1)
        try:
            E.check_warp_groups_burst(dev)
        finally:
            dev.close()


# ------------------------------------------------------------------------------------------------------------------ warp, exact
def test_warp_identity_and_shift(gpu):
    """k_warp on 40 x 72 (2880 = 11 x 256 + 64 pixels), image values multiples of 1/256: zero coefficients give the input back
    bit for bit; constant integer flows (per image; 47 > H in image 1) give img[clip(qy - sy), clip(qx - sx)] bit for bit"""
    dev = E.GpuDevice(gpu, E.EXACT['C'], E.EXACT['H'], E.EXACT['W'], E.EXACT['B'])
    try:
        E.check_warp_identity(dev, 'warp')
        E.check_warp_shift(dev, 'warp')
    finally:
        dev.close()


def test_warp_groups_identity_and_shift(gpu, monkeypatch):
    """the same through k_warp_groups<false> and <true>, with a shift of its own for every group of every image"""
    dev = E.GpuDevice(gpu, E.EXACT['C'], E.EXACT['H'], E.EXACT['W'], E.EXACT['B'])
    try:
        for layout in _layouts(monkeypatch):
            E.check_warp_identity(dev, 'groups')
            E.check_warp_shift(dev, 'groups')
    finally:
        dev.close()


# ----------------------------------------------------------------------------------------------------------- warp, against the oracle
@pytest.mark.parametrize('name', sorted(n for n, c in E.WARP_CASES.items() if c[0] == 'warp'))
def test_warp_matches_oracle(gpu, name):
    """k_warp: non-square both ways (C = 3 and C = 8), max_diff 100 / stddev 20 at 64 x 48 (the border clamps), n = 150 (second
    pass of the coefficient copy), n = 1 and n = 2046 with chosen coefficients (C = 1)"""
    _, B, H, W, kinds, _, _, _ = E.WARP_CASES[name]
    dev = E.GpuDevice(gpu, len(kinds) - 1, H, W, B)
    try:
        E.check_warp_case(dev, name)
    finally:
        dev.close()


@pytest.mark.parametrize('name', sorted(n for n, c in E.WARP_CASES.items() if c[0] == 'groups'))
def test_warp_groups_match_oracle(gpu, monkeypatch, name):
    """k_warp_groups<false> and <true> (at n = 2046 two coefficient sets do not fit 64 KB and the library keeps the group-per-block
    layout): the oracle bounds hold for both; whether the two agree bit for bit is printed, not asserted"""
    _, B, H, W, kinds, _, _, _ = E.WARP_CASES[name]
    dev = E.GpuDevice(gpu, len(kinds) - 1, H, W, B)
    try:
        outs = []
        for layout in _layouts(monkeypatch):
            print(layout)
            outs.append(E.check_warp_case(dev, name)[2])
        same = all(np.array_equal(a, b) for a, b in zip(*outs))
        diff = max(float(np.abs(a - b).max()) for a, b in zip(*outs))
        print('%s: the two layouts %s (largest difference %.3g)' % (name, 'agree bit for bit' if same else 'differ', diff))
    finally:
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- the ABI
def test_cabi_rejects_more_points_than_fit_lds(gpu):
    """n_points 2047 and 2048 ((n * 4 + 6) * 8 bytes > 64 KB): DNNCA_EINVAL from both entry points, the message names the limit,
    nothing is launched.  No test launches above the limit."""
    B, S, c = 1, 16, 2
    dev = E.GpuDevice(gpu, c, S, S, B, profile=True)
    m = dev.m
    try:
        x, xo = (gpu.DeviceBuffer(np.zeros((B, S, S, c), np.float32)) for _ in range(2))
        y, yo = (gpu.DeviceBuffer(np.zeros((B, S, S), np.float32)) for _ in range(2))
        table = np.array([0, 1, 0], np.int32)
        dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731
        m.profile_reset()
        for n in (2047, 2048):
            ctrl, wv = np.zeros((B, 2, n, 2)), np.zeros((B, 2, n + 3, 2))
            rc = m.lib.dnnca_warp_f32(m.handle, x.ptr, y.ptr, B, S, S, c, n, dptr(ctrl), dptr(wv), xo.ptr, yo.ptr)
            msg = m.lib.dnnca_last_error().decode()
            assert rc == -1 and 'dnnca_warp_f32' in msg and '2046' in msg, (rc, msg)
            rc = m.lib.dnnca_warp_groups_f32(m.handle, x.ptr, y.ptr, B, S, S, c, 2, table.ctypes.data_as(C.POINTER(C.c_int)), n,
                                             dptr(ctrl), dptr(wv), xo.ptr, yo.ptr)
            msg = m.lib.dnnca_last_error().decode()
            assert rc == -1 and 'dnnca_warp_groups_f32' in msg and '2046' in msg, (rc, msg)
        m.sync()
        launched = {row[0]: row[1] for row in m.profile()}
        assert not any(k.startswith('aug_warp') for k in launched), launched
    finally:
        dev.close()
