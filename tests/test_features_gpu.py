"""-m gpu: per-lesion intensity, shape and ring records through the C ABI (kernels_region.hip: lesion_features, lesion_ring;
dnnca_lesion_table_features) against tests/features_oracle.py.

Everything is an integer sum or an extremum: every field must EQUAL the oracle, there is no tolerance.  Host outputs carry guard
regions pre-filled with a sentinel; outputs the call must not touch (ring records with ring = 0, histograms with bins = 0) are such
regions as a whole.  The drawings are those of tests/lesion_cases.py plus planes made for the ring rule."""

import ctypes as C
import os

import numpy as np
import pytest

import features_oracle as FO
import lesion_cases as LC
import lesion_oracle as LO
from test_lesion_gpu import UNET
from test_spread_gpu import _files, _run_with_checkpoint
from test_tta_gpu import SENTINEL, drawn, random_weights

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


def _sentinel(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, SENTINEL, np.uint8).view(dtype)


def features_call(dm, prob, x, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256, bins=32, ring=3):
    """dnnca_lesion_table_features on host planes (x None: the model's own, prob is then only the batch size) with guarded buffers
    -> (rows, totals, masks, shape, body, ring or None, hist or None)"""
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import check, fptr
    if x is None:
        B, (h, w, ch) = int(prob), dm.in_shape
        pp, xp, ah, aw = None, None, 0, 0
    else:
        prob, x = np.ascontiguousarray(prob, np.float32), np.ascontiguousarray(x, np.float32)
        (B, h, w), ch = prob.shape, x.shape[-1]
        pp, xp, ah, aw = fptr(prob), fptr(x), h, w
    oh, ow = LO.O.out_size(h, w, rf)
    cap = B * min(max_lesions, (oh * ow + 1) // 2)
    rows, shape = _sentinel(cap + 8, LO.ROW_DTYPE), _sentinel(cap + 8, FO.SHAPE_DTYPE)
    body, rng = _sentinel((cap + 8) * ch, FO.INTENSITY_DTYPE), _sentinel((cap + 8) * ch, FO.INTENSITY_DTYPE)
    hist = _sentinel((cap + 8) * ch * max(bins, 1), np.uint32)
    masks = np.full(B * oh * ow + 64, SENTINEL, np.uint8)
    totals = np.full(B + 4, -7, np.int32)
    n, hw = C.c_int64(-1), (C.c_int32 * 2)()
    rec = C.POINTER(_lib.LesionIntensity)
    check(dm.lib.dnnca_lesion_table_features(dm.handle, pp, B, ah, aw, threshold, rf, k, min_area, max_lesions,
                                             rows.ctypes.data_as(C.POINTER(_lib.LesionRow)), cap, C.byref(n),
                                             totals.ctypes.data_as(C.POINTER(C.c_int32)), masks.ctypes.data_as(C.c_void_p), B * oh * ow, hw,
                                             xp, 0 if x is None else ch, bins, ring, shape.ctypes.data_as(C.POINTER(_lib.LesionShape)),
                                             body.ctypes.data_as(rec), rng.ctypes.data_as(rec), hist.ctypes.data_as(C.POINTER(C.c_uint32))))
    assert (hw[0], hw[1]) == (oh, ow) and 0 <= n.value <= cap
    n = n.value
    for buf, used in ((rows, n), (shape, n), (body, n * ch), (rng, n * ch if ring else 0), (hist, n * ch * bins)):
        assert (buf[used:].view(np.uint8) == SENTINEL).all(), 'written past the end of an output, or into one that is off'
    assert (totals[B:] == -7).all() and (masks[B * oh * ow:] == SENTINEL).all()
    return (rows[:n].copy(), totals[:B].copy(), masks[:B * oh * ow].reshape(B, oh, ow).copy(), shape[:n].copy(),
            body[:n * ch].reshape(n, ch).copy(), rng[:n * ch].reshape(n, ch).copy() if ring else None,
            hist[:n * ch * bins].reshape(n, ch, bins).copy() if bins else None)


def equal(got, want, what):
    if want is None:
        assert got is None, what
        return
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype.names:
        for f in got.dtype.names:
            assert got[f].tolist() == want[f].tolist(), '%s: field %s' % (what, f)
    assert got.tobytes() == want.tobytes(), what


def check_features(dm, prob, x, spec, **kw):
    """the call against the oracle, the table against lesion_table; returns the call's outputs"""
    got = features_call(dm, prob, x, spec['threshold'], spec['rf'], spec['k'], **kw)
    table = {a: v for a, v in kw.items() if a in ('min_area', 'max_lesions')}
    plain = dm.lesion_table(prob=prob, threshold=spec['threshold'], resize_factor=spec['rf'], filter_size=spec['k'], **table)
    assert got[0].tobytes() == plain[0].tobytes() and got[1].tolist() == plain[1].tolist() and np.array_equal(got[2], plain[2])
    want = FO.lesion_features(prob, x, spec['threshold'], spec['rf'], spec['k'], **kw)
    for g, w, what in zip(got[3:], want, ('shape', 'body', 'ring', 'hist')):
        equal(g, w, what)
    assert got[3]['area'].tolist() == got[0]['area'].tolist() and got[3]['row'].tolist() == got[0]['row'].tolist()
    assert got[3]['slice'].tolist() == got[0]['slice'].tolist() and (got[4]['n'] == got[3]['area'][:, None]).all()
    if got[6] is not None:
        assert (got[6].sum(axis=-1) == got[3]['area'][:, None]).all()
    return got


# ---- 1. the drawings of the lesion table -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels', [1, 3, 5])
@pytest.mark.parametrize('name', list(LC.ALL))
def test_features_equal_the_oracle(dm, name, channels):
    """tile_borders: a lesion of 171 pixels over two slices; checkerboard: 32 lesions inside every wave, every ring pixel contested;
    even_graded_half / odd_plateau: resize_factor 0.5 (odd_plateau with fractional weights); empty_and_full: no lesion, and one
    that is the plane"""
    prob, spec = LC.ALL[name]()
    x = drawn(prob.shape + (channels,), 7 * channels + len(name))
    got = check_features(dm, prob, x, spec)
    if name == 'empty_and_full':
        assert got[1].tolist() == [0, 1] and got[5]['n'].tolist() == [[0] * channels] and not got[5]['max'].any()


def test_values_outside_the_unit_interval_and_nan(dm):
    prob, spec = LC.areas()
    x = (3.0 * drawn(prob.shape + (3,), 31) - 1.0).astype(np.float32)        # a third below 0, a third above 1
    x[0, 9, 11, 1] = x[0, 3, 20, 0] = x[0, 7, 12, 2] = np.nan                 # in a body, a one-pixel body, a ring
    x[0, 10, 12, 0], x[0, 10, 13, 0] = -0.0, np.inf
    got = check_features(dm, prob, x, spec)
    assert got[4]['min'].min() == 0.0 and got[4]['max'].max() == 1.0 and np.isfinite(got[4]['max']).all()


@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 5, 7), (1, 33, 65)], ids=str)
def test_small_and_odd_planes(dm, shape):
    """1 x 1 x 1 and 2 x 5 x 7: less than a wave, most of the ring tile outside the plane; 33 x 65: a tile of one row / column"""
    rng = np.random.default_rng(sum(shape))
    prob = (rng.random(shape) < 0.35).astype(np.float32)
    if shape == (1, 1, 1):
        prob[:] = 1.0
    for ring in (1, 3, 8):
        check_features(dm, prob, drawn(shape + (3,), ring), dict(threshold=0.5, rf=1.0, k=1), ring=ring)


def test_one_lesion_that_is_the_plane(dm):
    """96 x 96 = 9216 pixels: three blocks of lesion_features add to one record, 144 waves each; the outline is the plane's border"""
    prob = np.ones((1, 96, 96), np.float32)
    got = check_features(dm, prob, drawn((1, 96, 96, 3), 5), dict(threshold=0.5, rf=1.0, k=5), ring=8, bins=256)
    assert got[3]['area'].tolist() == [9216] and got[3]['boundary'].tolist() == [4 * 95] and got[3]['edges'].tolist() == [4 * 96]
    assert got[5]['n'].tolist() == [[0, 0, 0]] and got[5]['sum_q16'].tolist() == [[0, 0, 0]]


@pytest.mark.parametrize('ring', [1, 3, 8])
def test_shared_ring_pixels_go_to_the_lower_row(dm, ring):
    """two blocks two pixels apart (closer than every R but 1) and a third in the corner, its window clipped by the plane; 40 x 72
    crosses the 32-pixel tiles of lesion_ring"""
    prob = np.zeros((1, 40, 72), np.float32)
    prob[0, 12:20, 28:31] = prob[0, 14:18, 33:40] = prob[0, 36:, 68:] = 1.0
    x = drawn((1, 40, 72, 2), ring)
    x[..., 0] = 0.0
    x[0, 14:18, 31:33, 0] = 1.0                                                # channel 0 marks the gap between the two blocks
    got = check_features(dm, prob, x, dict(threshold=0.5, rf=1.0, k=1), ring=ring)
    assert got[3]['area'].tolist() == [24, 28, 16]
    # R = 1: column 31 sees row 0 alone, column 32 row 1 alone; a larger window sees both and gives all 8 pixels to row 0
    assert got[5]['sum_q16'][:, 0].tolist() == ([4 << 16, 4 << 16, 0] if ring == 1 else [8 << 16, 0, 0])
    grown = (4 + ring) ** 2 - 16                                               # the corner block's window is clipped on two sides
    assert got[5]['n'][2].tolist() == [grown, grown]


def test_truncated_and_filtered_components(dm):
    """max_lesions 2 of 4 components: the others get no record and no ring, and their pixels are no ring pixels either; min_area:
    a filtered component is background, so its pixels are ring pixels"""
    prob, spec = LC.areas()
    x = drawn(prob.shape + (3,), 11)
    got = check_features(dm, prob, x, spec, max_lesions=2, ring=8)
    assert got[1].tolist() == [4] and got[3]['area'].tolist() == [9, 1]
    got = check_features(dm, prob, x, spec, min_area=5, ring=8)
    assert got[3]['area'].tolist() == [9, 100]
    all_kept = check_features(dm, prob, x, spec, ring=8)
    # the one-pixel component at (3, 20) and the pixels it owned fell to the ring of the block of 100 (row 1 here, row 2 there)
    assert got[5]['n'][1, 0] > all_kept[5]['n'][2, 0]
    prob, spec = LC.checkerboard()
    got = check_features(dm, prob, drawn(prob.shape + (1,), 12), spec, max_lesions=16, ring=2)
    assert got[1].tolist() == [480] and len(got[3]) == 16


def test_resize_factor_half(dm):
    prob, spec = LC.even_graded_half()
    for k in (1, 3):
        check_features(dm, prob, drawn(prob.shape + (3,), 13 + k), dict(spec, k=k), ring=2)
    three = np.concatenate([prob, np.zeros_like(prob), prob[:, ::-1].copy()])
    check_features(dm, three, drawn(three.shape + (2,), 14), spec)


@pytest.mark.parametrize('bins,ring', [(1, 3), (32, 0), (256, 1), (0, 3), (0, 0)])
def test_bins_and_ring_switched_off_leave_their_outputs_alone(dm, bins, ring):
    prob, spec = LC.tile_borders()
    x = drawn(prob.shape + (3,), bins + ring)
    x[0, 36:45, 36:45, 0] = 1.0                                                # v = 1 lands in the last bin, not behind it
    got = check_features(dm, prob, x, spec, bins=bins, ring=ring)              # features_call holds the sentinels
    assert (got[5] is None) == (ring == 0) and (got[6] is None) == (bins == 0)
    if bins == 256:
        assert got[6][2, 0, 255] == 81


def test_twice_the_same_and_the_python_method(dm):
    prob, spec = LC.odd_graded()
    x = drawn(prob.shape + (3,), 17)
    a = features_call(dm, prob, x, spec['threshold'], spec['rf'], spec['k'])
    b = features_call(dm, prob, x, spec['threshold'], spec['rf'], spec['k'])
    m = dm.lesion_table_features(prob=prob, x=x, threshold=spec['threshold'], resize_factor=spec['rf'], filter_size=spec['k'])
    assert len(m) == 7
    for i in range(7):
        assert a[i].tobytes() == b[i].tobytes() == m[i].tobytes()
    m = dm.lesion_table_features(prob=prob, x=x, threshold=spec['threshold'], filter_size=spec['k'], bins=0, ring=0)
    assert m[5] is None and m[6] is None and m[4].tobytes() == a[4].tobytes()
    with pytest.raises(ValueError):
        dm.lesion_table_features(prob=prob)
    with pytest.raises(ValueError):
        dm.lesion_table_features(batch=1, x=x)


# ---- 2. the model's own planes ---------------------------------------------------------------------------------------------------
def test_the_staged_batch_is_read_untransformed(wide):
    """after forward and after forward_tta (whose views run on transformed copies) the features read the x that was given"""
    m = wide
    x = drawn((3, 16, 32, 3), 21)
    for run in (lambda: m.forward(x, training=False), lambda: m.forward_tta(x, 0x0F)):
        prob = run()
        thr = float(np.median(prob))
        own = features_call(m, 3, None, thr, 1.0, 1, ring=2)
        host = features_call(m, prob[..., 0], x, thr, 1.0, 1, ring=2)
        assert len(own[0]) > 0
        for a, b in zip(own, host):
            assert a.tobytes() == b.tobytes()
        want = FO.lesion_features(prob[..., 0], x, thr, 1.0, 1, ring=2)
        for g, w, what in zip(own[3:], want, ('shape', 'body', 'ring', 'hist')):
            equal(g, w, what)
        py = m.lesion_table_features(batch=3, threshold=thr, filter_size=1, ring=2)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(own, py))


def test_fewer_staged_slices_are_a_state_error(wide):
    from dnncancerannotator_amd import _lib
    m = wide
    m.forward(drawn((2, 16, 32, 3), 22), training=False)
    features_call(m, 2, None, 0.5, 1.0, 1)
    with pytest.raises(Exception):
        m.lesion_table_features(batch=3, filter_size=1)
    rows = _sentinel(4096, LO.ROW_DTYPE)
    hw, n = (C.c_int32 * 2)(), C.c_int64(-1)
    rc = m.lib.dnnca_lesion_table_features(m.handle, None, 3, 0, 0, 0.5, 1.0, 1, 0, 256, rows.ctypes.data_as(C.POINTER(_lib.LesionRow)), 4096,
                                           C.byref(n), rows.ctypes.data_as(C.POINTER(C.c_int32)), None, 0, hw, None, 0, 32, 3,
                                           rows.ctypes.data_as(C.POINTER(_lib.LesionShape)), rows.ctypes.data_as(C.POINTER(_lib.LesionIntensity)),
                                           rows.ctypes.data_as(C.POINTER(_lib.LesionIntensity)), rows.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == -4 and n.value == -1 and (rows.view(np.uint8) == SENTINEL).all()           # DNNCA_ESTATE


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(dm):
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import fptr
    p, x = drawn((2, 16, 32), 23), drawn((2, 16, 32, 17), 24)
    tall = np.zeros((1, 65536, 1), np.float32)
    dm.sync()
    dm.profile_reset()
    dm.profile_enable(1)
    try:
        out, out2 = _sentinel(64, np.uint8), _sentinel(64, np.uint8)      # too small for anything: a refused call must not touch them
        lib = dm.lib
        rows, shape, rec, hist = (out.ctypes.data_as(C.POINTER(t)) for t in (_lib.LesionRow, _lib.LesionShape, _lib.LesionIntensity, C.c_uint32))
        n, totals = C.c_int64(-1), out2.ctypes.data_as(C.POINTER(C.c_int32))
        hw = (C.c_int32 * 2)()

        def call(prob=fptr(p), xs=fptr(x), batch=2, h=16, w=32, k=1, cap=1 << 20, ch=3, bins=32, ring=3, thr=0.5, rf=1.0, min_area=0,
                 max_lesions=256, sh=shape, body=rec, rg=rec, hs=hist, tot=totals):
            return lib.dnnca_lesion_table_features(dm.handle, prob, batch, h, w, thr, rf, k, min_area, max_lesions, rows, cap, C.byref(n), tot,
                                                   None, 0, hw, xs, ch, bins, ring, sh, body, rg, hs)
        cases = [('x without prob', lambda: call(prob=None, h=0, w=0)), ('prob without x', lambda: call(xs=None)),
                 ('channels 0', lambda: call(ch=0)), ('channels 17', lambda: call(ch=17)),
                 ('bins -1', lambda: call(bins=-1)), ('bins 257', lambda: call(bins=257)),
                 ('ring -1', lambda: call(ring=-1)), ('ring 9', lambda: call(ring=9)),
                 ('null shape', lambda: call(sh=None)), ('null body', lambda: call(body=None)),
                 ('null ring_out', lambda: call(rg=None)), ('null hist', lambda: call(hs=None)),
                 ('a side of 65536', lambda: call(prob=fptr(tall), xs=fptr(tall), batch=1, h=65536, w=1, ch=1)),
                 ('batch 0', lambda: call(batch=0)), ('batch max_batch + 1', lambda: call(batch=4)),
                 ('filter_size 16', lambda: call(k=16)), ('filter_size 0', lambda: call(k=0)),
                 ('threshold NaN', lambda: call(thr=float('nan'))), ('resize factor 0', lambda: call(rf=0.0)),
                 ('min_area -1', lambda: call(min_area=-1)), ('max_lesions 0', lambda: call(max_lesions=0)),
                 ('null totals', lambda: call(tot=None)), ('rows too short', lambda: call(cap=1)),
                 ('an empty plane', lambda: call(h=0, w=32))]
        for what, c in cases:
            assert c() == -1, what                # DNNCA_EINVAL
            assert lib.dnnca_last_error()
            assert (out == SENTINEL).all() and (out2 == SENTINEL).all(), what
        assert n.value == -1
        assert dm.profile() == []
        assert call(rg=None, ring=0, hs=None, bins=0, cap=0, sh=None, body=None) == -1     # rows without room, even with everything off
        assert dm.profile() == []
    finally:
        dm.profile_enable(0)
        dm.profile_reset()


# ---- 4. launches and plans -------------------------------------------------------------------------------------------------------
def test_launches_and_plans(wide):
    m = wide
    modes = ('train', 'eval', 'forward', 'lesion', 'lesion_linked', 'lesion_matched')
    x = drawn((3, 16, 32, 3), 25)
    m.forward(x, training=False)
    m.lesion_table(batch=3, filter_size=3)
    before = {mode: m.plan(variants=True, mode=mode) for mode in modes}

    def profiled(call):
        m.sync()
        m.profile_reset()
        m.profile_enable(1)
        try:
            call()
            return {name: n for name, n, _, _, _ in m.profile()}
        finally:
            m.profile_enable(0)
            m.profile_reset()
    plain = profiled(lambda: m.lesion_table(batch=3, filter_size=3))
    with_ring = profiled(lambda: m.lesion_table_features(batch=3, filter_size=3, ring=2, bins=8))
    assert with_ring.pop('lesion_features') == 1 and with_ring.pop('lesion_ring') == 1 and with_ring == plain
    names = [r[0] for r in m.plan(mode='lesion_features', batch=3)]
    assert names.count('lesion_features') == 1 and names.count('lesion_ring') == 1
    assert sorted(n for n in names if n not in ('lesion_features', 'lesion_ring')) == sorted(r[0] for r in before['lesion'])
    without = profiled(lambda: m.lesion_table_features(batch=3, filter_size=1, ring=0, mask=False))
    assert without.pop('lesion_features') == 1 and 'lesion_ring' not in without and 'region_open' not in without
    names = [r[0] for r in m.plan(mode='lesion_features', batch=3)]       # replays filter size 1, no mask, no ring
    assert names.count('lesion_features') == 1 and not {'lesion_ring', 'region_open', 'lesion_mask'} & set(names)
    for mode, plan in before.items():
        assert m.plan(variants=True, mode=mode) == plan
        assert not [r[0] for r in plan if r[0] in ('lesion_features', 'lesion_ring')]
    with pytest.raises(ValueError):
        m.plan(mode='lesion_feature')


# ---- 5. the command line ---------------------------------------------------------------------------------------------------------
def test_cli_predict_lesion_features(gpu, tmp_path):
    from dnncancerannotator_amd import __main__ as cli, casewise as CW
    m, batches, run, data = _run_with_checkpoint(tmp_path, labels=False)
    thr = float(np.median(m.forward(batches[0][0], training=False)))
    texts = {}
    for name, flags in (('bare', []), ('feat', ['--lesion_features', '--feature_bins', '16', '--feature_ring', '2'])):
        out = str(tmp_path / name)
        assert cli.main(['predict', '--save_path', run, '--data_path', data, '--output', out, '--export_images', '--link_slices',
                         '--threshold', repr(thr), '--filter_size', '1'] + flags) == 0
        texts[name] = _files(out)
    assert sorted(set(texts['feat']) - set(texts['bare'])) == ['exam_lesion_features.csv', 'lesion_features.csv']
    assert all(texts['feat'][k] == v for k, v in texts['bare'].items())
    assert {'lesions.csv', 'slices.csv', 'exam_lesions.csv', 'exam_lesion_parts.csv'} <= set(texts['bare'])
    lines, records = [], {}
    for x, paths, ids in batches:
        prob = m.forward(x, training=False)[..., 0]
        rows, _, _ = LO.lesion_table(prob, thr, 1.0, 1)
        sh, bd, rg, hs = FO.lesion_features(prob, x, thr, 1.0, 1, bins=16, ring=2)
        for j, r in enumerate(rows):
            p, k = paths[r['slice']], ids[r['slice']]
            lines.append(CW.lesion_feature_values(p, k, r, sh[j], bd[j], rg[j], hs[j]))
            records[(str(p), int(k), int(r['row']))] = (sh[j], bd[j], rg[j], hs[j])
    names = CW.modality_names(None, batches[0][0].shape[-1])
    assert lines and texts['feat']['lesion_features.csv'].decode() == CW.plain_csv(CW.lesion_feature_columns(names), lines)
    members = {}                                 # the membership is that of exam_lesion_parts.csv, which the flag leaves as it is
    for line in texts['feat']['exam_lesion_parts.csv'].decode().splitlines()[1:]:
        exam, k, lesion, e = line.rsplit(',', 3)
        members.setdefault((exam, int(e)), []).append(records[(exam, int(k), int(lesion))])
    exam_lines = [CW.exam_lesion_feature_values(exam, e, parts) for (exam, e), parts in members.items()]
    assert texts['feat']['exam_lesion_features.csv'].decode() == CW.plain_csv(CW.exam_lesion_feature_columns(names), exam_lines)
    m.close()
