"""-m gpu: the reliability table, the NLL at a set of temperatures and the temperature scaling through the C ABI (kernels_calib.hip:
calib_bins, calib_nll, calib_nll_sum, prob_temperature; dnnca_calibration, dnnca_prob_temperature) against tests/calib_oracle.py.

The tables are integers and must EQUAL the oracle byte for byte; the NLL must lie within relative 1e-9 of the float64 oracle (a bound
derived in the oracle, not measured); both must be byte-identical from run to run.  A scaled probability must lie within one float32
ulp of the float64 oracle rounded to float32.  Host outputs carry guard regions pre-filled with a sentinel.

Shapes: the rectangles and the 33 x 33 of the TTA tests; 64 x 65 = 4160 pixels is 64 more than the 4096 one calib_bins block walks (two
blocks add to one slice, the second one ragged) and takes five calib_nll blocks of 1024; batch 3 on a model of max_batch 3."""

import ctypes as C

import numpy as np
import pytest

import calib_oracle as CO
from test_lesion_gpu import UNET
from test_tta_gpu import SENTINEL, drawn, guarded, random_weights, same, unguard

pytestmark = pytest.mark.gpu

SHAPES = [(2, 5, 7), (1, 16, 64), (2, 33, 33), (1, 64, 65), (3, 16, 32)]
TEMPS = (0.05, 0.5, 1.0, 1.7, 20.0)
ELEVEN = (0.05, 0.25, 0.5, 0.8, 1.0, 1.25, 1.7, 2.5, 4.0, 10.0, 20.0)      # more than one chunk of eight, the second one ragged
GRID41 = tuple(2.0 ** ((j - 20) / 10.0) for j in range(41))


@pytest.fixture(scope='module')
def dm(gpu):
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    random_weights(m, 31)
    yield m
    m.close()


def raw(n_items, dtype, extra=4):
    return np.full((n_items + extra) * dtype.itemsize, SENTINEL, np.uint8).view(dtype)


def calib_call(dm, prob, y, n_bins, temps):
    """dnnca_calibration on host planes with guarded outputs -> (bins [B, n_bins], totals [B], nll [B, T])"""
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import check, fptr
    prob, y = np.ascontiguousarray(prob, np.float32), np.ascontiguousarray(y, np.float32)
    temps = np.ascontiguousarray(temps, np.float32)
    B, h, w = y.shape
    T = len(temps)
    bins, totals, nll = raw(B * n_bins, CO.BIN_DTYPE), raw(B, CO.TOTAL_DTYPE), raw(B * T, np.dtype('<f8'))
    check(dm.lib.dnnca_calibration(dm.handle, fptr(prob), fptr(y), B, h, w, n_bins, fptr(temps) if T else None, T,
                                   bins.ctypes.data_as(C.POINTER(_lib.CalibBin)), totals.ctypes.data_as(C.POINTER(_lib.CalibTotal)),
                                   nll.ctypes.data_as(C.POINTER(C.c_double))))
    for buf, used in ((bins, B * n_bins), (totals, B), (nll, B * T)):
        assert (buf[used:].view(np.uint8) == SENTINEL).all(), 'written past the end of an output'
    return bins[:B * n_bins].reshape(B, n_bins).copy(), totals[:B].copy(), nll[:B * T].reshape(B, T).copy()


def check_case(dm, prob, y, n_bins, temps, what):
    bins, totals, nll = calib_call(dm, prob, y, n_bins, temps)
    wb, wt = CO.tables(prob, y, n_bins)
    for got, want in ((bins, wb), (totals, wt)):
        for field in want.dtype.names:
            assert np.array_equal(got[field], want[field]), '%s: %s' % (what, field)
        assert got.tobytes() == want.tobytes(), what
    hw = y.shape[1] * y.shape[2]
    assert (totals['n'].sum(axis=-1) == hw).all() and (bins['n'].sum(axis=(1, 2)) == hw).all()
    want = CO.nll(prob, y, temps)
    rel = np.abs(nll - want) / want
    print('%s: NLL max relative error %.3e of %.1e allowed' % (what, rel.max() if rel.size else 0.0, CO.NLL_RTOL))
    assert np.isfinite(nll).all() and (want > 0).all() and (rel <= CO.NLL_RTOL).all(), what
    again = calib_call(dm, prob, y, n_bins, temps)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((bins, totals, nll), again)), what + ': differs from run to run'
    return bins, totals, nll


# ---- 1. tables and NLL -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_tables_and_nll_against_the_oracle(dm, shape):
    for f, fam in enumerate(CO.FAMILIES):
        prob, y = CO.family(fam, shape, 10 * sum(shape) + f)
        for n_bins in (CO.EDGE_BINS if fam == 'edges' else (15,)):
            temps = ELEVEN if n_bins == 15 else TEMPS
            _, totals, _ = check_case(dm, prob, y, n_bins, temps, '%s %s %d bins' % (fam, shape, n_bins))
        if fam == 'all_0':
            assert not totals['n'][:, 1].any() and not totals['sq_lo'][:, 1].any()
        if fam == 'all_1':
            assert not totals['n'][:, 0].any() and not totals['sum_q24'][:, 0].any()


def test_edge_values_fall_into_the_oracles_bins(dm):
    """every edge value in one plane: k / n_bins and its float32 neighbours, 0, 1, -0.25, 1.5 and NaN"""
    e = CO.edge_values()
    prob = np.resize(e, (2, 24, 36)).astype(np.float32)            # 864 values per slice: each of them once
    assert prob[0].size == e.size
    y = np.stack([np.zeros((24, 36)), np.ones((24, 36))]).astype(np.float32)
    for n_bins in CO.EDGE_BINS:
        bins, totals, _ = check_case(dm, prob, y, n_bins, TEMPS, 'edge plane, %d bins' % n_bins)
        assert bins[0]['n'][:, 0].tolist() == bins[1]['n'][:, 1].tolist()
    assert int(bins[0]['n'][0, 0]) >= 3                             # 256 bins: -0.25, NaN and 0 share bin 0


def test_the_41_point_grid_and_64_temperatures(dm):
    prob, y = CO.family('uniform', (2, 33, 33), 5)
    check_case(dm, prob, y, 15, GRID41, '41 temperatures')
    check_case(dm, prob, y, 15, np.linspace(0.05, 20.0, 64), '64 temperatures')


def test_without_temperatures_nll_is_not_touched(dm):
    prob, y = CO.family('real_like', (3, 16, 32), 6)
    bins, totals, nll = calib_call(dm, prob, y, 10, ())
    assert nll.size == 0
    wb, wt = CO.tables(prob, y, 10)
    assert bins.tobytes() == wb.tobytes() and totals.tobytes() == wt.tobytes()


# ---- 2. temperature scaling ------------------------------------------------------------------------------------------------------
def scale_call(dm, prob, T):
    from dnncancerannotator_amd._lib import check, fptr
    prob = np.ascontiguousarray(prob, np.float32)
    B, h, w = prob.shape
    out = guarded(prob.size)
    check(dm.lib.dnnca_prob_temperature(dm.handle, fptr(prob), B, h, w, T, fptr(out)))
    return unguard(out, prob.size, prob.shape)


@pytest.mark.parametrize('shape', [(2, 5, 7), (2, 33, 33), (1, 64, 65), (3, 16, 32)], ids=str)
def test_scaled_probabilities_within_one_ulp(dm, shape):
    for fam in ('uniform', 'real_like', 'edges'):
        prob, _ = CO.family(fam, shape, sum(shape))
        prob.flat[0] = 0.5
        for T in TEMPS:
            got, want = scale_call(dm, prob, T), CO.scale(prob, T)
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            print('%s %s T=%g: %d of %d pixels differ, by at most %.3g ulp' % (fam, shape, T, int((err > 0).sum()), err.size,
                                                                              float((err / np.spacing(want)).max())))
            assert np.isfinite(got).all() and (err <= np.spacing(want)).all(), (fam, T)
            assert got.flat[0] == np.float32(0.5)
            assert got.tobytes() == scale_call(dm, prob, T).tobytes()


def test_scaling_is_monotone_and_keeps_one_half(dm):
    prob = np.sort(np.concatenate([CO.edge_values()[:4], CO.edge_values()[5:], drawn(4096 - 863 + 64, 7)]))[:4160].reshape(1, 64, 65)
    assert not np.isnan(prob).any() and (prob == 0.5).any()
    for T in TEMPS:
        got = scale_call(dm, prob, T).reshape(-1)
        assert (np.diff(got) >= 0).all(), T
        assert (got[prob.reshape(-1) == 0.5] == 0.5).all()


def test_in_place_scaling_equals_the_host_plane_call(dm):
    x = drawn((3, 16, 16, 1), 8)
    dm.forward(x, training=False, return_prob=False)
    before = dm.last_prob(3)
    host = dm.scale_temperature(1.7, 3, prob=before)
    same(dm.last_prob(3), before)                                            # the host-plane call left the model's plane alone
    assert dm.scale_temperature(1.7, 3) is None
    same(dm.last_prob(3), host)
    assert host.tobytes() != before.tobytes()
    # out_hw beside the in-place call: a copy of the scaled plane; two slices of three: the third one stays
    from dnncancerannotator_amd._lib import check, fptr
    dm.forward(x, training=False, return_prob=False)
    out = guarded(2 * 256)
    check(dm.lib.dnnca_prob_temperature(dm.handle, None, 2, 16, 16, 0.5, fptr(out)))
    got = unguard(out, 2 * 256, (2, 16, 16))
    same(got, dm.scale_temperature(0.5, 2, prob=before[:2]))
    same(dm.last_prob(3)[:2], got)
    same(dm.last_prob(3)[2:], before[2:])


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------
def test_the_models_plane_after_forward_and_forward_tta(dm):
    x = drawn((3, 16, 16, 1), 9)
    y = (drawn((3, 16, 16), 10) < 0.3).astype(np.float32)
    p0, s0 = dm.get_params(), dm.get_state()
    first = dm.forward(x, training=False)
    for call in (lambda: dm.forward(x, training=False, return_prob=False), lambda: dm.forward_tta(x, 0x0F, return_prob=False)):
        call()
        prob = dm.last_prob(3)
        mine = dm.calibration(y, 15, GRID41, batch=3)
        host = dm.calibration(y, 15, GRID41, prob=prob)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(mine, host))
        wb, wt = CO.tables(prob, y, 15)
        assert mine[0].tobytes() == wb.tobytes() and mine[1].tobytes() == wt.tobytes() and mine[2].shape == (3, 41)
        same(dm.last_prob(3), prob)
        two = dm.calibration(y[:2], 15, TEMPS)                               # fewer slices than the forward had
        assert two[0].tobytes() == mine[0][:2].tobytes() and two[1].tobytes() == mine[1][:2].tobytes()
    assert dm.get_params().tobytes() == p0.tobytes() and dm.get_state().tobytes() == s0.tobytes()
    same(dm.forward(x, training=False), first)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_touch_nothing(gpu):
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import fptr
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    try:
        random_weights(m, 11)
        lib = m.lib
        p = drawn((4, 16, 32), 12)
        x = drawn((2, 16, 16, 1), 13)
        ok, many = np.array([1.0, 2.0], np.float32), np.ones(65, np.float32)
        bufs = [np.full(1 << 16, SENTINEL, np.uint8) for _ in range(4)]
        bins, totals = bufs[0].ctypes.data_as(C.POINTER(_lib.CalibBin)), bufs[1].ctypes.data_as(C.POINTER(_lib.CalibTotal))
        nll, out = bufs[2].ctypes.data_as(C.POINTER(C.c_double)), bufs[3].view(np.float32)

        def cal(prob=fptr(p), y=fptr(p), batch=2, h=16, w=32, n_bins=15, temps=fptr(ok), nt=2, bins=bins, totals=totals, nll=nll):
            return lib.dnnca_calibration(m.handle, prob, y, batch, h, w, n_bins, temps, nt, bins, totals, nll)

        def bad_t(v):
            return fptr(np.array([1.0, v], np.float32))
        einval = [('batch 0', lambda: cal(batch=0)), ('batch max_batch + 1', lambda: cal(batch=4)),
                  ('0 bins', lambda: cal(n_bins=0)), ('257 bins', lambda: cal(n_bins=257)),
                  ('-1 temperatures', lambda: cal(nt=-1)), ('65 temperatures', lambda: cal(temps=fptr(many), nt=65)),
                  ('null temperatures', lambda: cal(temps=None)), ('null nll', lambda: cal(nll=None)),
                  ('NaN temperature', lambda: cal(temps=bad_t(np.nan))), ('temperature 0.04', lambda: cal(temps=bad_t(0.04))),
                  ('temperature 20.5', lambda: cal(temps=bad_t(20.5))), ('temperature 0', lambda: cal(temps=bad_t(0.0))),
                  ('temperature -1', lambda: cal(temps=bad_t(-1.0))), ('temperature inf', lambda: cal(temps=bad_t(np.inf))),
                  ('null y', lambda: cal(y=None)), ('null bins', lambda: cal(bins=None)), ('null totals', lambda: cal(totals=None)),
                  ('empty plane', lambda: cal(h=0)), ('2^31 pixels', lambda: cal(h=65536, w=32768)),
                  ('the model\'s plane at another size', lambda: cal(prob=None, h=16, w=32)),
                  ('scale: batch 0', lambda: lib.dnnca_prob_temperature(m.handle, fptr(p), 0, 16, 32, 1.5, fptr(out))),
                  ('scale: batch max_batch + 1', lambda: lib.dnnca_prob_temperature(m.handle, fptr(p), 4, 16, 32, 1.5, fptr(out))),
                  ('scale: temperature 0.04', lambda: lib.dnnca_prob_temperature(m.handle, fptr(p), 2, 16, 32, 0.04, fptr(out))),
                  ('scale: temperature 21', lambda: lib.dnnca_prob_temperature(m.handle, fptr(p), 2, 16, 32, 21.0, fptr(out))),
                  ('scale: NaN', lambda: lib.dnnca_prob_temperature(m.handle, fptr(p), 2, 16, 32, float('nan'), fptr(out))),
                  ('scale: host plane without out', lambda: lib.dnnca_prob_temperature(m.handle, fptr(p), 2, 16, 32, 1.5, None)),
                  ('scale: empty plane', lambda: lib.dnnca_prob_temperature(m.handle, fptr(p), 2, 16, 0, 1.5, fptr(out))),
                  ('scale: the model\'s plane at another size', lambda: lib.dnnca_prob_temperature(m.handle, None, 2, 16, 32, 1.5, fptr(out)))]
        estate = [('calibration', lambda b: cal(prob=None, batch=b, h=0, w=0)),
                  ('calibration, size given', lambda b: cal(prob=None, batch=b, h=16, w=16)),
                  ('scale', lambda b: lib.dnnca_prob_temperature(m.handle, None, b, 0, 0, 1.5, fptr(out)))]

        def refused(cases, code, *a):
            m.sync()
            m.profile_reset()
            m.profile_enable(1)
            try:
                for what, call in cases:
                    assert call(*a) == code, what
                    assert lib.dnnca_last_error()
                    assert all((b == SENTINEL).all() for b in bufs), what
                assert m.profile() == []
            finally:
                m.profile_enable(0)
                m.profile_reset()
        refused(einval, -1)                          # DNNCA_EINVAL
        refused(estate, -4, 1)                       # DNNCA_ESTATE: a fresh model has no probabilities
        m.forward(x, training=False, return_prob=False)
        before = m.last_prob(2)
        refused(estate, -4, 3)                       # the last forward had two slices
        refused(einval, -1)
        same(m.last_prob(2), before)
    finally:
        m.close()


# ---- 5. launches -----------------------------------------------------------------------------------------------------------------
def test_launches_and_untouched_plans(dm):
    before = {mode: dm.plan(variants=True, mode=mode) for mode in ('train', 'eval', 'forward')}
    x = drawn((3, 16, 16, 1), 14)
    y = (drawn((3, 16, 16), 15) < 0.3).astype(np.float32)
    dm.forward(x, training=False, return_prob=False)

    def profiled(call):
        dm.sync()
        dm.profile_reset()
        dm.profile_enable(1)
        try:
            call()
            return {name: n for name, n, _, _, _ in dm.profile()}
        finally:
            dm.profile_enable(0)
            dm.profile_reset()
    assert profiled(lambda: dm.calibration(y, 15, GRID41)) == {'calib_bins': 1, 'calib_nll': 1, 'calib_nll_sum': 1}
    assert profiled(lambda: dm.calibration(y, 15)) == {'calib_bins': 1}
    assert profiled(lambda: dm.calibration(y, 15, (1.0,), prob=dm.last_prob(3))) == {'calib_bins': 1, 'calib_nll': 1, 'calib_nll_sum': 1}
    assert profiled(lambda: dm.scale_temperature(1.5, 3)) == {'prob_temperature': 1}
    assert profiled(lambda: dm.scale_temperature(1.5, 3, prob=dm.last_prob(3))) == {'prob_temperature': 1}
    for mode, plan in before.items():
        assert dm.plan(variants=True, mode=mode) == plan
        assert not [r[0] for r in plan if r[0].startswith('calib') or r[0] == 'prob_temperature']


# ---- 6. the command line ---------------------------------------------------------------------------------------------------------
def test_cli_evaluate_calibration_and_temperature(gpu, tmp_path):
    from dnncancerannotator_amd import __main__ as cli, casewise as CW
    from test_spread_gpu import _files, _run_with_checkpoint
    m, batches, run, data = _run_with_checkpoint(tmp_path, labels=True)
    base = ['evaluate', '--save_path', run, '--data_path', data, '--export_csv', '--skip_visualization', '--tag', 't']
    runs = {'plain': [], 'one': ['--temperature', '1'], 'cal': ['--calibration', '--calibration_bins', '10'],
            'scaled': ['--calibration', '--calibration_bins', '10', '--temperature', '1.7'],
            'views': ['--calibration', '--calibration_bins', '10', '--temperature', '1.7', '--tta', 'flips']}
    files = {}
    for name, flags in runs.items():
        assert cli.main(base + ['--export_path', str(tmp_path / name)] + flags) == 0
        files[name] = _files(str(tmp_path / name))
    new = ['t/calibration_bins.csv', 't/calibration_results.csv', 't/calibration_slices.csv']
    assert files['one'] == files['plain'] and sorted(set(files['cal']) - set(files['plain'])) == new
    assert all(files['cal'][k] == v for k, v in files['plain'].items()) and files['plain']
    grid = CW.calibration_grid()
    for name, forward, T in (('cal', lambda x: m.forward(x, training=False), None), ('scaled', lambda x: m.forward(x, training=False), 1.7),
                             ('views', lambda x: m.forward_tta(x, 0x0F), 1.7)):
        bins, totals, nll, slices = [], [], [], []
        for x, y, paths, ids in batches:
            prob = forward(x)[..., 0]
            prob = prob if T is None else m.scale_temperature(T, len(x), prob=prob)
            y = np.asarray(y, np.float32).reshape(prob.shape)
            b, t = CO.tables(prob, y, 10)
            n = m.calibration(y, 10, grid, prob=prob)[2]
            assert np.abs(n - CO.nll(prob, y, grid)).max() <= CO.NLL_RTOL * n.max()
            bins.append(b), totals.append(t), nll.append(n)
            slices += [[1] + CW.calibration_slice_values(paths[i], ids[i], b[i], t[i], n[i, grid.index(1.0)]) for i in range(len(x))]
        result, lines = CW.calibration_summary(np.concatenate(bins), np.concatenate(totals), grid, np.concatenate(nll))
        got = files[name]
        assert got['t/calibration_results.csv'].decode() == CW.plain_csv(['step'] + CW.CALIBRATION_RESULT_COLUMNS, [[1] + result]), name
        assert got['t/calibration_bins.csv'].decode() == CW.plain_csv(['step'] + CW.CALIBRATION_BIN_COLUMNS, [[1] + l for l in lines]), name
        assert got['t/calibration_slices.csv'].decode() == CW.plain_csv(['step'] + CW.CALIBRATION_SLICE_COLUMNS, slices), name
    assert files['scaled']['t/calibration_results.csv'] != files['cal']['t/calibration_results.csv']
    loss = lambda f: [l.split(',')[:2] for l in f['t/results.csv'].decode().splitlines()]
    assert loss(files['scaled']) == loss(files['plain'])                      # the unscaled test step's loss
    m.close()


def test_cli_predict_temperature(gpu, tmp_path):
    from dnncancerannotator_amd import __main__ as cli, casewise as CW
    from test_spread_gpu import _files, _run_with_checkpoint
    m, batches, run, data = _run_with_checkpoint(tmp_path, labels=False)
    thr = float(np.median(m.scale_temperature(0.5, None, prob=m.forward(batches[0][0], training=False)[..., 0])))
    texts = {}
    for name, flags in (('bare', []), ('one', ['--temperature', '1.0']), ('half', ['--temperature', '0.5'])):
        out = str(tmp_path / name)
        assert cli.main(['predict', '--save_path', run, '--data_path', data, '--output', out, '--threshold', repr(thr), '--filter_size', '1'] +
                        flags) == 0
        texts[name] = _files(out)
    assert texts['one'] == texts['bare'] and texts['half'] != texts['bare'] and sorted(texts['half']) == sorted(texts['bare'])
    lesions, slices = [], []
    for x, paths, ids in batches:
        prob = m.scale_temperature(0.5, len(x), prob=m.forward(x, training=False)[..., 0])
        rows, totals, _ = m.lesion_table(prob=prob, threshold=thr, filter_size=1, mask=False)
        for b in range(len(x)):
            mine = rows[rows['slice'] == b]
            lesions += [CW.lesion_values(paths[b], ids[b], r) for r in mine]
            slices.append(CW.slice_values(paths[b], ids[b], mine, totals[b]))
    assert lesions and texts['half']['lesions.csv'].decode() == CW.plain_csv(CW.LESION_COLUMNS, lesions)
    assert texts['half']['slices.csv'].decode() == CW.plain_csv(CW.SLICE_COLUMNS, slices)
    m.close()
