"""-m gpu: the spread of the test-time-augmentation views through the C ABI (kernels_tta.hip: tta_moments; kernels_region.hip:
lesion_spread, spread_outcome; dnnca_forward_tta_spread, dnnca_tta_spread_of, dnnca_get_tta_spread, dnnca_lesion_table_spread,
dnnca_spread_by_outcome) against tests/spread_oracle.py.

The mean must EQUAL dnnca_tta_mean_of / dnnca_forward_tta bit for bit; the spread must lie within 2^-18 of the float64 standard
deviation plus 2^-23 on every pixel and be exactly 0 where the views agree; the tables are integers and extrema and must EQUAL the
oracle.  Host outputs carry guard regions pre-filled with a sentinel.  Shapes are those of tests/test_tta_gpu.py (sides around the
32-pixel LDS tile of the transposed arm; rectangles for the mirrored-run arm) and the drawings of tests/lesion_cases.py."""

import ctypes as C
import os

import numpy as np
import pytest

import lesion_cases as LC
import lesion_oracle as LO
import spread_oracle as SO
import tta_oracle as TO
from test_lesion_gpu import UNET
from test_tta_gpu import CASES, GUARD, LOGIT_TOL, MASKS, PROB_ROUNDING, SENTINEL, SIDES, drawn, guarded, mean_of, random_weights, same, unguard

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dm(gpu):
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    yield m
    m.close()


@pytest.fixture(scope='module')
def wide(gpu):
    m = gpu.DeviceModel('unet', 3, 16, 32, 3, **UNET)
    random_weights(m, 10)
    yield m
    m.close()


def spread_of(dm, planes, views, is_logits=0):
    """dnnca_tta_spread_of with guarded outputs -> (mean, spread) [B, h, w]"""
    from dnncancerannotator_amd._lib import check, fptr
    planes = np.ascontiguousarray(planes, np.float32)
    _, B, h, w = planes.shape
    prob, spread = guarded(B * h * w), guarded(B * h * w)
    check(dm.lib.dnnca_tta_spread_of(dm.handle, fptr(planes), B, h, w, views, is_logits, fptr(prob), fptr(spread)))
    return unguard(prob, B * h * w, (B, h, w)), unguard(spread, B * h * w, (B, h, w))


def within(got, want, what, extra=0.0):
    """every pixel of the float32 spread `got` within the contract of the float64 `want` (plus `extra`)"""
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want)
    tol = SO.tolerance(want) + extra
    worst = int(np.argmax(err - tol))
    print('%s: max |d| %.3e, worst pixel %.3e of %.3e allowed (want %.6e)' % (what, err.max(), err.flat[worst], tol.flat[worst],
                                                                             want.flat[worst]))
    assert (err <= tol).all(), what


def check_planes(dm, planes, views, what, is_logits=0, probs=None):
    mean, spread = spread_of(dm, planes, views, is_logits)
    same(mean, mean_of(dm, planes, views, is_logits))
    within(spread, SO.spread_of(planes if probs is None else probs, views), what)
    return spread


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', SIDES)
def test_spread_of_squares_against_the_oracle(dm, side):
    B = 2 if side == 33 else 1
    for i, views in enumerate(MASKS):
        n = len(TO.views_of(views))
        for f, fam in enumerate(SO.FAMILIES):
            spread = check_planes(dm, SO.family(fam, (n, B, side, side), 100 * i + f), views, '%s %d^2 0x%02X' % (fam, side, views))
            if n == 1:
                assert not spread.any()              # a single view: an all-zero plane


@pytest.mark.parametrize('shape', [(2, 5, 7), (1, 16, 64)], ids=str)
def test_spread_of_flips_on_rectangles_against_the_oracle(dm, shape):
    for i, views in enumerate(m for m in MASKS if m < 16):
        n = len(TO.views_of(views))
        for f, fam in enumerate(SO.FAMILIES):
            check_planes(dm, SO.family(fam, (n,) + shape, 1000 + 100 * i + f), views, '%s %s 0x%02X' % (fam, shape, views))


def test_equal_views_give_exactly_zero(dm):
    base = drawn((2, 33, 33, 1), 21)
    for views in (0x0F, 0xFF, 0xB4):
        planes = np.stack([TO.apply_view(base, k)[..., 0] for k in TO.views_of(views)])     # equal after mapping back
        mean, spread = spread_of(dm, planes, views)
        assert not spread.any() and spread.tobytes() == bytes(spread.nbytes)
        same(mean, mean_of(dm, planes, views))


def test_spread_of_logits_uses_the_devices_sigmoid(dm):
    views = 0xFF
    logits = (8.0 * (drawn((8, 2, 33, 33), 22) - 0.5)).astype(np.float32)
    probs = np.stack([TO.apply_view(mean_of(dm, logits[i:i + 1], 1 << k, is_logits=1)[..., None], k)[..., 0]
                      for i, k in enumerate(TO.views_of(views))])          # p_k in view k's geometry, from the device's own sigmoid
    check_planes(dm, logits, views, 'logits 33^2 d4', is_logits=1, probs=probs)


# ---- 2. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_forward_tta_spread_end_to_end(gpu, name):
    kw, views, batches = CASES[name]
    m = gpu.DeviceModel(**kw)
    try:
        random_weights(m, 8)
        B = batches[0]
        x = drawn((B, kw['height'], kw['width'], kw['in_channels']), 9 + B)
        p0, s0 = m.get_params(), m.get_state()
        first, logits = m.forward(x, training=False, return_logits=True)
        exact = first.tobytes() == m.forward(x, training=False).tobytes()
        singles = np.stack([m.forward_tta(x, 1 << k)[..., 0] for k in TO.views_of(views)])     # already at the original pixels
        want_mean = m.forward_tta(x, views)
        prob, spread = m.forward_tta_spread(x, views)
        same(prob, want_mean)
        extra = 0.0 if exact else LOGIT_TOL * max(1.0, float(np.abs(logits).max())) + PROB_ROUNDING
        within(spread, singles.astype(np.float64).std(axis=0), '%s B=%d (plain forwards repeat: %s)' % (name, B, exact), extra)
        assert spread.any()                          # a random network is not flip-invariant
        same(m.last_spread(B), spread)
        same(m.last_prob(B), prob[..., 0])
        assert m.forward_tta_spread(x, views, return_prob=False, return_spread=False) == (None, None)
        same(m.last_spread(B), spread)               # and from run to run
        same(m.last_prob(B), prob[..., 0])
        assert m.get_params().tobytes() == p0.tobytes() and m.get_state().tobytes() == s0.tobytes()
    finally:
        m.close()


# ---- 3. validity -----------------------------------------------------------------------------------------------------------------
def test_the_models_plane_is_valid_only_behind_forward_tta_spread(gpu):
    from dnncancerannotator_amd import _lib
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    try:
        random_weights(m, 23)
        x = drawn((2, 16, 16, 1), 24)
        y = (x[..., 0] > 0.5).astype(np.float32)

        thr = np.array([0.5], np.float32)

        def refused():
            for call in (lambda: m.lesion_table_spread(batch=2, filter_size=1), lambda: m.spread_by_outcome(y), lambda: m.last_spread(2)):
                with pytest.raises(_lib.DnncaError) as e:
                    call()
                assert e.value.code == -4 and 'dnnca_forward_tta_spread' in str(e.value)     # DNNCA_ESTATE
            # nothing written: the raw calls on sentinel-filled outputs (rows, n_rows, totals, mask, srows, stotals; the plane; out)
            bufs = [np.full(4096, SENTINEL, np.uint8) for _ in range(7)]
            rows, totals, mask, srows, stotals, plane, out = bufs
            n, hw = C.c_int64(-7), (C.c_int32 * 2)()
            assert m.lib.dnnca_lesion_table_spread(
                m.handle, None, 2, 0, 0, 0.5, 1.0, 1, 0, 8, rows.ctypes.data_as(C.POINTER(_lib.LesionRow)), 16, C.byref(n),
                totals.ctypes.data_as(C.POINTER(C.c_int32)), mask.ctypes.data_as(C.c_void_p), 512, hw, None,
                srows.ctypes.data_as(C.POINTER(_lib.LesionSpread)), stotals.ctypes.data_as(C.POINTER(_lib.SliceSpread))) == -4
            assert m.lib.dnnca_get_tta_spread(m.handle, 2, plane.view(np.float32).ctypes.data_as(C.POINTER(C.c_float))) == -4
            assert m.lib.dnnca_spread_by_outcome(m.handle, None, None, _lib.fptr(y), 2, 0, 0, _lib.fptr(thr), 1,
                                                 out.ctypes.data_as(C.POINTER(_lib.SpreadOutcome))) == -4
            assert n.value == -7 and all((b == SENTINEL).all() for b in bufs)
        m.sync()
        m.profile_reset()
        m.profile_enable(1)
        try:
            refused()                                # a fresh model
            assert m.profile() == []
        finally:
            m.profile_enable(0)
            m.profile_reset()
        m.forward(x, training=False, return_prob=False)
        refused()
        m.forward_tta(x, 0x0F, return_prob=False)
        refused()
        prob, spread = m.forward_tta_spread(x, 0x0F)
        thr_p = float(np.median(prob))
        got = m.lesion_table_spread(batch=2, threshold=thr_p, filter_size=1)
        host = m.lesion_table_spread(prob=prob, spread=spread, threshold=thr_p, filter_size=1)
        assert len(got[0]) and all(a.tobytes() == b.tobytes() for a, b in zip(got, host))
        assert m.spread_by_outcome(y, [thr_p]).tobytes() == SO.outcome(prob[..., 0], spread, y, [thr_p]).tobytes()
        same(m.last_spread(2), spread)               # the host-plane call left the model's plane alone
        with pytest.raises(_lib.DnncaError) as e:     # more slices than the plane holds
            m.last_spread(3)
        assert e.value.code == -4
        m.eval_step(x, y, m.loss_cfg())
        refused()
        m.forward_tta_spread(x, 0x0F, return_prob=False, return_spread=False)
        m.pixel_confusion_of(prob, y, [0.5])         # overwrites the probability buffer
        refused()
    finally:
        m.close()


# ---- 4. the lesion table with host planes ----------------------------------------------------------------------------------------
def drawn_spread(shape, seed):
    """multiples of 1 / 128 in [0, 0.5]: a 2 x 2 mean of them is exact"""
    B, h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([((xx * 3 + yy * 5 + seed + 7 * b) % 65) / 128.0 for b in range(B)]).astype(np.float32)


def table_call(dm, prob, spread, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256):
    """dnnca_lesion_table_spread on host planes with guarded buffers -> (rows, totals, masks, srows, stotals)"""
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import check, fptr
    prob, spread = np.ascontiguousarray(prob, np.float32), np.ascontiguousarray(spread, np.float32)
    B, h, w = prob.shape
    oh, ow = LO.O.out_size(h, w, rf)
    cap = B * min(max_lesions, (oh * ow + 1) // 2)
    rows = np.full((cap + 8) * LO.ROW_DTYPE.itemsize, SENTINEL, np.uint8).view(LO.ROW_DTYPE)
    srows = np.full((cap + 8) * SO.LESION_SPREAD_DTYPE.itemsize, SENTINEL, np.uint8).view(SO.LESION_SPREAD_DTYPE)
    stotals = np.full((B + 4) * SO.SLICE_SPREAD_DTYPE.itemsize, SENTINEL, np.uint8).view(SO.SLICE_SPREAD_DTYPE)
    masks = np.full(B * oh * ow + 64, SENTINEL, np.uint8)
    totals = np.full(B + 4, -7, np.int32)
    n, hw = C.c_int64(-1), (C.c_int32 * 2)()
    check(dm.lib.dnnca_lesion_table_spread(dm.handle, fptr(prob), B, h, w, threshold, rf, k, min_area, max_lesions,
                                           rows.ctypes.data_as(C.POINTER(_lib.LesionRow)), cap, C.byref(n),
                                           totals.ctypes.data_as(C.POINTER(C.c_int32)), masks.ctypes.data_as(C.c_void_p), B * oh * ow, hw,
                                           fptr(spread), srows.ctypes.data_as(C.POINTER(_lib.LesionSpread)),
                                           stotals.ctypes.data_as(C.POINTER(_lib.SliceSpread))))
    assert (hw[0], hw[1]) == (oh, ow) and 0 <= n.value <= cap
    for buf, used in ((rows, n.value), (srows, n.value), (stotals, B)):
        assert (buf[used:].view(np.uint8) == SENTINEL).all(), 'written past the end of an output'
    assert (totals[B:] == -7).all() and (masks[B * oh * ow:] == SENTINEL).all()
    return rows[:n.value].copy(), totals[:B].copy(), masks[:B * oh * ow].reshape(B, oh, ow).copy(), srows[:n.value].copy(), stotals[:B].copy()


def check_table(dm, prob, spec, **kw):
    spread = drawn_spread(prob.shape, len(kw) + prob.shape[1])
    got = table_call(dm, prob, spread, spec['threshold'], spec['rf'], spec['k'], **kw)
    plain = dm.lesion_table(prob=prob, threshold=spec['threshold'], resize_factor=spec['rf'], filter_size=spec['k'], **kw)
    assert got[0].tobytes() == plain[0].tobytes() and got[1].tolist() == plain[1].tolist() and np.array_equal(got[2], plain[2])
    srows, stotals = SO.lesion_spread(prob, spread, spec['threshold'], spec['rf'], spec['k'], **kw)
    assert got[3].tolist() == srows.tolist() and got[3].tobytes() == srows.tobytes()
    assert got[4].tolist() == stotals.tolist() and got[4].tobytes() == stotals.tobytes()
    assert got[3]['area'].tolist() == got[0]['area'].tolist() and got[3]['row'].tolist() == got[0]['row'].tolist()
    return got


@pytest.mark.parametrize('name', list(LC.ALL))
def test_lesion_table_spread_equals_the_oracle(dm, name):
    """tile_borders: a lesion of 171 pixels (more than a wave) over two slices; checkerboard: 32 lesions inside every wave;
    even_graded_half / odd_plateau: resize_factor 0.5 with filter sizes 3 and 5; empty_and_full: an all-background slice"""
    prob, spec = LC.ALL[name]()
    got = check_table(dm, prob, spec)
    assert (got[4]['pixels'] == got[2].shape[1] * got[2].shape[2]).all()
    if name == 'empty_and_full':
        assert got[1].tolist() == [0, 1] and got[4]['sum_spread_q24'][0] > 0 and got[3]['sum_spread_q24'][0] == got[4]['sum_spread_q24'][1]
    if name in ('odd_plateau', 'even_graded_half', 'areas'):       # batch 3; 20 x 26 and 20 x 24 planes end inside a block's first runs
        three = np.concatenate([prob, np.zeros_like(prob), prob[:, ::-1].copy()])
        check_table(dm, three, spec)


def test_lesion_table_spread_truncation_and_area_filter(dm):
    prob, spec = LC.checkerboard()
    got = check_table(dm, prob, spec, max_lesions=16)             # 480 components, 16 rows
    assert got[1].tolist() == [480] and len(got[3]) == 16
    prob, spec = LC.areas()
    got = check_table(dm, prob, spec, min_area=5)
    assert got[3]['area'].tolist() == [9, 100]
    prob, spec = LC.even_graded_half()
    check_table(dm, prob, dict(spec, k=1))                        # resize_factor 0.5 without an opening


def test_lesion_table_spread_on_planes_smaller_than_a_wave(dm):
    """3 slices of 3 x 5: one block per slice, most of its lanes and all but its first run behind the plane"""
    prob = np.zeros((3, 3, 5), np.float32)
    prob[0, 0, :2] = prob[1, 1, 1:4] = prob[2] = 0.75
    check_table(dm, prob, dict(threshold=0.5, rf=1.0, k=1))


# ---- 5. spread by outcome --------------------------------------------------------------------------------------------------------
def outcome_call(dm, prob, spread, y, thr):
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import check, fptr
    prob, spread, y = (np.ascontiguousarray(a, np.float32) for a in (prob, spread, y))
    thr = np.ascontiguousarray(thr, np.float32)
    B, h, w = y.shape
    n = len(thr) * B
    out = np.full((n + 2) * SO.OUTCOME_DTYPE.itemsize, SENTINEL, np.uint8).view(SO.OUTCOME_DTYPE)
    check(dm.lib.dnnca_spread_by_outcome(dm.handle, fptr(prob), fptr(spread), fptr(y), B, h, w, fptr(thr), len(thr),
                                         out.ctypes.data_as(C.POINTER(_lib.SpreadOutcome))))
    assert (out[n:].view(np.uint8) == SENTINEL).all()
    return out[:n].reshape(len(thr), B).copy()


@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 5, 7), (3, 16, 32), (1, 33, 65), (1, 96, 96)], ids=str)
def test_spread_by_outcome_equals_the_oracle(dm, shape):
    """probabilities and thresholds are multiples of 1 / 64, so many pixels sit exactly at a threshold; labels are 0, 0.5 (background:
    not > 0.5) and 1.  96 x 96 takes more than one block per slice (4096 pixels each)"""
    rng = np.random.default_rng(sum(shape))
    prob = (rng.integers(0, 65, shape) / 64.0).astype(np.float32)
    y = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), shape)
    spread = (rng.integers(0, 65, shape) / 128.0).astype(np.float32)
    for thr in ([0.5], [0.25, 0.5, 1.0], list(np.arange(64) / 64.0 + 1 / 64.0)):
        got = outcome_call(dm, prob, spread, y, thr)
        want = SO.outcome(prob, spread, y, thr)
        assert np.array_equal(got['n'], want['n']) and np.array_equal(got['sum_q24'], want['sum_q24']) and got.tobytes() == want.tobytes()
        assert (got['n'].sum(axis=-1) == shape[1] * shape[2]).all()


def test_spread_by_outcome_on_slices_of_one_class(dm):
    shape = (3, 16, 32)
    spread = drawn_spread(shape, 3)
    prob = np.stack([np.zeros(shape[1:]), np.ones(shape[1:]), np.ones(shape[1:])]).astype(np.float32)
    y = np.stack([np.zeros(shape[1:]), np.zeros(shape[1:]), np.ones(shape[1:])]).astype(np.float32)
    got = outcome_call(dm, prob, spread, y, [0.5])
    assert got.tobytes() == SO.outcome(prob, spread, y, [0.5]).tobytes()
    assert [int(np.argmax(g['n'])) for g in got[0]] == [0, 1, 3] and [int((g['n'] > 0).sum()) for g in got[0]] == [1, 1, 1]


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(dm, wide):
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import fptr
    sq, rect = drawn((4, 16, 16, 1), 12), drawn((4, 16, 32, 3), 13)
    planes = drawn((8, 4, 16, 32), 14)
    thr, nan = np.array([0.5] * 65, np.float32), np.array([0.5, np.nan], np.float32)
    for m in (dm, wide):
        m.sync()
        m.profile_reset()
        m.profile_enable(1)
    try:
        out, out2 = guarded(0), guarded(0)        # too small for anything: a refused call must not touch them
        lib = dm.lib
        rows, srows, stot = (out.ctypes.data_as(C.POINTER(t)) for t in (_lib.LesionRow, _lib.LesionSpread, _lib.SliceSpread))
        oc = out.ctypes.data_as(C.POINTER(_lib.SpreadOutcome))
        n, hw, totals = C.c_int64(-1), (C.c_int32 * 2)(), out2.ctypes.data_as(C.POINTER(C.c_int32))
        p = planes[0]

        def table(prob, batch, spread, k=1, cap=1 << 20, h=16, w=32):
            return lib.dnnca_lesion_table_spread(dm.handle, prob, batch, h, w, 0.5, 1.0, k, 0, 256, rows, cap, C.byref(n), totals, None, 0,
                                                 hw, spread, srows, stot)
        cases = [('views 0', lambda: lib.dnnca_forward_tta_spread(dm.handle, fptr(sq), 2, 0, fptr(out), fptr(out2))),
                 ('views 256', lambda: lib.dnnca_forward_tta_spread(dm.handle, fptr(sq), 2, 256, fptr(out), fptr(out2))),
                 ('view 4 at 16 x 32', lambda: lib.dnnca_forward_tta_spread(wide.handle, fptr(rect), 2, 1 << 4, fptr(out), fptr(out2))),
                 ('d4 at 16 x 32', lambda: lib.dnnca_forward_tta_spread(wide.handle, fptr(rect), 2, 0xFF, fptr(out), fptr(out2))),
                 ('batch 0', lambda: lib.dnnca_forward_tta_spread(dm.handle, fptr(sq), 0, 0x0F, fptr(out), fptr(out2))),
                 ('batch max_batch + 1', lambda: lib.dnnca_forward_tta_spread(dm.handle, fptr(sq), 4, 0x0F, fptr(out), fptr(out2))),
                 ('spread_of views 0', lambda: lib.dnnca_tta_spread_of(dm.handle, fptr(planes), 2, 16, 32, 0, 0, fptr(out), fptr(out2))),
                 ('spread_of views 256', lambda: lib.dnnca_tta_spread_of(dm.handle, fptr(planes), 2, 16, 32, 256, 0, fptr(out), fptr(out2))),
                 ('spread_of view 5 at 16 x 32',
                  lambda: lib.dnnca_tta_spread_of(dm.handle, fptr(planes), 2, 16, 32, 1 << 5, 0, fptr(out), fptr(out2))),
                 ('spread_of batch 0', lambda: lib.dnnca_tta_spread_of(dm.handle, fptr(planes), 0, 16, 32, 1, 0, fptr(out), fptr(out2))),
                 ('spread_of batch max_batch + 1',
                  lambda: lib.dnnca_tta_spread_of(dm.handle, fptr(planes), 4, 16, 32, 1, 0, fptr(out), fptr(out2))),
                 ('spread_of null spread', lambda: lib.dnnca_tta_spread_of(dm.handle, fptr(planes), 2, 16, 32, 1, 0, fptr(out), None)),
                 ('get_tta_spread batch 0', lambda: lib.dnnca_get_tta_spread(dm.handle, 0, fptr(out))),
                 ('table: spread without prob', lambda: table(None, 2, fptr(p), h=0, w=0)),
                 ('table: prob without spread', lambda: table(fptr(p), 2, None)),
                 ('table: batch 0', lambda: table(fptr(p), 0, fptr(p))),
                 ('table: batch max_batch + 1', lambda: table(fptr(p), 4, fptr(p))),
                 ('table: filter_size 16', lambda: table(fptr(p), 2, fptr(p), k=16)),
                 ('table: rows too short', lambda: table(fptr(p), 2, fptr(p), cap=1)),
                 ('outcome: 0 thresholds', lambda: lib.dnnca_spread_by_outcome(dm.handle, fptr(p), fptr(p), fptr(p), 2, 16, 32, fptr(thr), 0, oc)),
                 ('outcome: 65 thresholds', lambda: lib.dnnca_spread_by_outcome(dm.handle, fptr(p), fptr(p), fptr(p), 2, 16, 32, fptr(thr), 65, oc)),
                 ('outcome: NaN threshold', lambda: lib.dnnca_spread_by_outcome(dm.handle, fptr(p), fptr(p), fptr(p), 2, 16, 32, fptr(nan), 2, oc)),
                 ('outcome: spread without prob', lambda: lib.dnnca_spread_by_outcome(dm.handle, None, fptr(p), fptr(p), 2, 16, 32, fptr(thr), 1, oc)),
                 ('outcome: prob without spread', lambda: lib.dnnca_spread_by_outcome(dm.handle, fptr(p), None, fptr(p), 2, 16, 32, fptr(thr), 1, oc)),
                 ('outcome: null y', lambda: lib.dnnca_spread_by_outcome(dm.handle, fptr(p), fptr(p), None, 2, 16, 32, fptr(thr), 1, oc)),
                 ('outcome: batch max_batch + 1', lambda: lib.dnnca_spread_by_outcome(dm.handle, fptr(p), fptr(p), fptr(p), 4, 16, 32, fptr(thr), 1, oc)),
                 ('outcome: empty plane', lambda: lib.dnnca_spread_by_outcome(dm.handle, fptr(p), fptr(p), fptr(p), 2, 0, 32, fptr(thr), 1, oc))]
        for what, call in cases:
            assert call() == -1, what             # DNNCA_EINVAL
            assert lib.dnnca_last_error()
            assert (out.view(np.uint8) == SENTINEL).all() and (out2.view(np.uint8) == SENTINEL).all(), what
        assert n.value == -1
        assert dm.profile() == [] and wide.profile() == []
    finally:
        for m in (dm, wide):
            m.profile_enable(0)
            m.profile_reset()


# ---- 7. launches -----------------------------------------------------------------------------------------------------------------
def test_launches_and_untouched_plans(wide):
    m = wide
    before = {mode: m.plan(variants=True, mode=mode) for mode in ('train', 'eval', 'forward')}
    x = drawn((3, 16, 32, 3), 15)

    def profiled(call):
        m.sync()
        m.profile_reset()
        m.profile_enable(1)
        try:
            call()
            return {name: (n, by) for name, n, _, by, _ in m.profile()}
        finally:
            m.profile_enable(0)
            m.profile_reset()
    rows = profiled(lambda: m.forward_tta_spread(x, 0x0F))
    assert rows['tta_moments'][0] == 4 and rows['tta_view_in'][0] == 3 and 'tta_accumulate' not in rows and 'g_sigmoid' not in rows
    forward = [r[0] for r in m.plan(mode='forward') if r[0] != 'g_sigmoid']
    assert all(rows[k][0] == 4 * forward.count(k) for k in set(forward))   # one forward per view
    table = profiled(lambda: m.lesion_table_spread(batch=3, filter_size=1))
    plain = profiled(lambda: m.lesion_table(batch=3, filter_size=1))          # reads the same probabilities
    assert table['lesion_spread'][0] == 1 and 'lesion_spread' not in plain
    assert {k: v[0] for k, v in table.items() if k != 'lesion_spread'} == {k: v[0] for k, v in plain.items()}
    y = (x[..., 0] > 0.5).astype(np.float32)
    m.forward_tta_spread(x, 0x0F, return_prob=False, return_spread=False)
    assert {k: v[0] for k, v in profiled(lambda: m.spread_by_outcome(y, [0.25, 0.5])).items()} == {'spread_outcome': 1}
    # forward_tta launches what tests/test_tta_gpu.py asserts
    rows = profiled(lambda: m.forward_tta(x, 0x0F))
    assert rows['tta_accumulate'][0] == 4 and rows['tta_view_in'][0] == 3 and 'g_sigmoid' not in rows and 'tta_moments' not in rows
    assert rows['tta_view_in'][1] == 8.0 * x.size
    assert rows['tta_accumulate'][1] == (8.0 + 3 * 12.0) / 4 * x[..., 0].size
    assert all(rows[k][0] == 4 * forward.count(k) for k in set(forward))
    for mode, plan in before.items():
        assert m.plan(variants=True, mode=mode) == plan
        assert not [r[0] for r in plan if r[0].startswith('tta') or 'spread' in r[0]]


# ---- 8. the command line ---------------------------------------------------------------------------------------------------------
def _files(root):
    out = {}
    for d, _, fs in os.walk(root):
        for fn in fs:
            with open(os.path.join(d, fn), 'rb') as f:
                out[os.path.relpath(os.path.join(d, fn), root)] = f.read()
    return out


def _run_with_checkpoint(tmp_path, labels):
    import yaml
    from dnncancerannotator_amd import engine
    from dnncancerannotator_amd.runs.train import make_dataset
    cfg = {'model': 'UNetAnnotator', 'model_options': UNET, 'deploy_options': {'optimizer': 'adam', 'enable_multigpu': False},
           'data_options': {'eval': {'batch_size': 2}}}
    run, data = str(tmp_path / 'run'), 'synthetic:16x16x2'
    e = engine.TFKerasModel(cfg)
    ds = make_dataset([data], cfg['data_options']['eval'], training=False, include_meta=True, labels=labels)
    e._build(ds)
    random_weights(e.device_model, 16)
    e.current_step = 1
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    with open(os.path.join(run, 'options.yaml'), 'w') as f:
        yaml.safe_dump({'config': cfg}, f)
    return e.device_model, list(ds), run, data


def test_cli_predict_uncertainty(gpu, tmp_path):
    from dnncancerannotator_amd import __main__ as cli, casewise as CW
    m, batches, run, data = _run_with_checkpoint(tmp_path, labels=False)
    thr = float(np.median(m.forward_tta(batches[0][0], 0x0F)))
    texts = {}
    for name, flags in (('bare', []), ('flips', ['--tta', 'flips']), ('spread', ['--tta', 'flips', '--uncertainty'])):
        out = str(tmp_path / name)
        assert cli.main(['predict', '--save_path', run, '--data_path', data, '--output', out, '--export_images', '--threshold', repr(thr),
                         '--filter_size', '1'] + flags) == 0
        texts[name] = _files(out)
    new = sorted(set(texts['spread']) - set(texts['flips']))
    n_slices = sum(len(b[0]) for b in batches)
    assert sorted(f for f in new if f.endswith('.csv')) == ['lesion_uncertainty.csv', 'slice_uncertainty.csv'] and len(new) == 2 + n_slices
    assert all(texts['spread'][k] == v for k, v in texts['flips'].items()) and texts['flips'] != texts['bare']
    lesion_lines, slice_lines, pngs = [], [], {}
    for x, paths, ids in batches:
        prob, spread = m.forward_tta_spread(x, 0x0F)
        rows, totals, _, srows, stotals = m.lesion_table_spread(prob=prob, spread=spread, threshold=thr, filter_size=1)
        for b in range(len(x)):
            mine = rows['slice'] == b
            lesion_lines += [CW.lesion_uncertainty_values(paths[b], ids[b], r, s) for r, s in zip(rows[mine], srows[mine])]
            slice_lines.append(CW.slice_uncertainty_values(paths[b], ids[b], rows[mine], srows[mine], totals[b], stotals[b]))
            pngs[os.path.relpath(CW.uncertainty_path(str(tmp_path), CW.tag_of(paths[b], ids[b])), str(tmp_path))] = \
                CW.encode_png(SO.png_of(spread[b]))
    assert lesion_lines and texts['spread']['lesion_uncertainty.csv'].decode() == CW.plain_csv(CW.LESION_UNCERTAINTY_COLUMNS, lesion_lines)
    assert texts['spread']['slice_uncertainty.csv'].decode() == CW.plain_csv(CW.SLICE_UNCERTAINTY_COLUMNS, slice_lines)
    assert {k: texts['spread'][k] for k in pngs} == pngs and any(SO.png_of(s).any() for s in [spread])
    m.close()


def test_cli_evaluate_uncertainty(gpu, tmp_path):
    from dnncancerannotator_amd import __main__ as cli, casewise as CW
    m, batches, run, data = _run_with_checkpoint(tmp_path, labels=True)
    thrs = [0.5, float(np.median(m.forward_tta(batches[0][0], 0x0F)))]
    base = ['evaluate', '--save_path', run, '--data_path', data, '--export_csv', '--skip_visualization', '--tta', 'flips']
    flags = ['--uncertainty', '--uncertainty_threshold'] + [repr(t) for t in thrs]
    assert cli.main(base + ['--tag', 'plain', '--export_path', str(tmp_path / 'a')]) == 0
    assert cli.main(base + ['--tag', 'plain', '--export_path', str(tmp_path / 'b')] + flags) == 0
    a, b = _files(str(tmp_path / 'a')), _files(str(tmp_path / 'b'))
    new = sorted(set(b) - set(a))
    assert new == ['plain/uncertainty_results.csv', 'plain/uncertainty_slices.csv'] and all(b[k] == v for k, v in a.items()) and a
    per = [[] for _ in thrs]
    for x, y, paths, ids in batches:
        prob, spread = m.forward_tta_spread(x, 0x0F)
        want = SO.outcome(prob[..., 0], spread, np.asarray(y, np.float32).reshape(spread.shape), thrs)
        for t in range(len(thrs)):
            per[t] += [(paths[i], int(ids[i]), want[t, i]) for i in range(len(x))]
    results, slices = [], []
    for t, thr in enumerate(thrs):
        lead = [1, repr(thr)]
        slices += [lead + CW.outcome_slice_values(p, k, o) for p, k, o in per[t]]
        results.append(lead + CW.outcome_summary([o for _, _, o in per[t]]))
    assert b['plain/uncertainty_results.csv'].decode() == CW.plain_csv(['step', 'threshold'] + CW.UNCERTAINTY_RESULT_COLUMNS, results)
    assert b['plain/uncertainty_slices.csv'].decode() == CW.plain_csv(['step', 'threshold'] + CW.UNCERTAINTY_SLICE_COLUMNS, slices)
    m.close()
