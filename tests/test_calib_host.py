"""CPU: the host side of `--calibration` and `--temperature`.  casewise's arithmetic on hand-computed tables, the temperature fit against
a fine search of the same curve, engine.eval and engine.annotate on a fake device served by the oracle (tests/fake_calib_device.py)
-- the files, the order of the calls, what runs without the flags -- and the command line."""

import inspect
import math
import os

import numpy as np
import pytest

import calib_oracle as CO
from dnncancerannotator_amd import casewise as CW
from dnncancerannotator_amd.__main__ import build_parser
from fake_calib_device import fake_engine
from fake_link_device import Slices
from fake_match_device import LabelledSlices
from test_spread_host import EXAMS, IDS, KW, _Pairs, _drawn, _texts

GRID = CW.calibration_grid()


# ---- casewise: hand-computed -----------------------------------------------------------------------------------------------------
def _two_slices():
    """slice 0: two pixels each at 0, 0.25, 0.5 and 1; slice 1: eight pixels at 0.75.  With four bins 0.75 and 1 share the last one:
    slice 0 is over-confident there (1 against 1 of 2), slice 1 under-confident (0.75 against 7 of 8), pooled they cancel"""
    prob = np.array([[0, 0, 0.25, 0.25, 0.5, 0.5, 1, 1], [0.75] * 8], np.float32).reshape(2, 2, 4)
    y = np.array([[0, 0, 0, 1, 0, 1, 1, 0], [1, 1, 1, 1, 1, 1, 1, 0]], np.float32).reshape(2, 2, 4)
    return prob, y


def test_table_errors_and_brier_from_the_integers():
    prob, y = _two_slices()
    bins, totals = CO.tables(prob, y, 4)
    assert bins['n'].tolist() == [[[2, 0], [1, 1], [1, 1], [1, 1]], [[0, 0], [0, 0], [0, 0], [1, 7]]]
    pooled = CW.calibration_table(bins)
    assert [r[:5] for r in pooled] == [[0, 0.0, 0.25, 2, 0], [1, 0.25, 0.5, 2, 1], [2, 0.5, 0.75, 2, 1], [3, 0.75, 1.0, 10, 8]]
    assert [r[5:] for r in pooled] == [[0.0, 0.0, 0.0], [0.25, 0.5, 0.25], [0.5, 0.5, 0.0], [0.8, 0.8, 0.0]]
    assert CW.calibration_errors(pooled) == (0.03125, 0.25)
    # per slice: 2/8 * 0.25 + 2/8 * 0.5, and 8/8 * 0.125 -- their mean is not the pooled value
    assert CW.calibration_errors(CW.calibration_table(bins[0])) == (0.1875, 0.5)
    assert CW.calibration_errors(CW.calibration_table(bins[1])) == (0.125, 0.125)
    assert CW.calibration_table(bins[1])[0][5:] == [None, None, None]              # an empty bin has no mean
    assert [CW.brier_score(t) for t in totals] == [0.265625, 0.125] and CW.brier_score(totals) == 0.1953125
    assert CW.calibration_errors(CW.calibration_table(np.zeros(4, CO.BIN_DTYPE))) == (None, None)
    assert CW.brier_score(np.zeros(1, CO.TOTAL_DTYPE)) is None


def test_brier_needs_both_words_of_the_squares():
    """512 x 512 pixels at p = 1 and class 0: sum q^2 = 2^66 does not fit one uint64; the two words give exactly 1"""
    t = np.zeros(1, CO.TOTAL_DTYPE)
    n = 512 * 512
    t['n'][0, 0], t['sum_q24'][0, 0] = n, n << 24
    t['sq_lo'][0, 0], t['sq_hi'][0, 0] = 0, n << 16                              # q^2 = 2^48: low word 0, high word 2^16
    assert CW.brier_score(t) == 1.0
    t['n'][0], t['sum_q24'][0], t['sq_lo'][0], t['sq_hi'][0] = [0, n], [0, n << 24], [0, 0], [0, n << 16]
    assert CW.brier_score(t) == 0.0                                              # the same pixels of class 1: n 2^48 - 2^25 n 2^24 + n 2^48


def test_the_default_grid_and_what_the_grid_refuses():
    assert len(GRID) == 41 and GRID[0] == 0.25 and GRID[20] == 1.0 and GRID[-1] == 4.0 and GRID == sorted(GRID)
    assert CW.calibration_grid([2.0, 0.5]) == [0.5, 1.0, 2.0] and CW.calibration_grid([1.0, 1.0, 3.0]) == [1.0, 3.0]
    assert all(np.float32(t) == t for t in GRID)                                  # what the device receives is what the fit sees
    for bad in ([0.04], [21.0], [float('nan')], list(np.linspace(1.5, 2.5, 64))):
        with pytest.raises(ValueError, match='calibration_temperatures'):
            CW.calibration_grid(bad)
    assert len(CW.calibration_grid([1.0] + list(np.linspace(1.5, 2.5, 63)))) == 64


# ---- the temperature fit ---------------------------------------------------------------------------------------------------------
def _synthetic(n, sharpen, seed):
    """n pixels whose labels are drawn from sigmoid(z) and whose probability is sigmoid(z * sharpen): the NLL is smallest near
    T = sharpen (> 1: over-confident, < 1: under-confident)"""
    rng = np.random.default_rng(seed)
    z = rng.normal(0.0, 2.0, n)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    return (1.0 / (1.0 + np.exp(-z * sharpen))).astype(np.float32).reshape(1, 1, n), y.reshape(1, 1, n)


def _curve(prob, y, temperatures):
    """CO.nll with numpy's pairwise sum: 400 temperatures x 32768 pixels in a fraction of a second"""
    z = CO.logit(prob.reshape(-1)) * np.where(CO.label(y.reshape(-1)), -1.0, 1.0)
    return [float(CO.softplus(z * (1.0 / np.float64(np.float32(t)))).sum()) for t in temperatures]


@pytest.mark.parametrize('n', [512, 2178, 32768])
def test_fit_temperature_against_a_fine_search(n):
    for s, sharpen in enumerate((1.9, 0.6)):
        prob, y = _synthetic(n, sharpen, n + s)
        nll = CO.nll(prob, y, GRID)[0]
        t, v, edge = CW.fit_temperature(GRID, nll)
        i = int(np.argmin(nll))
        assert edge == 0 and 0 < i < 40 and GRID[i - 1] <= t <= GRID[i + 1]
        # the NLL is convex in 1 / T, so the curve's minimum lies between the neighbours of the grid's: the 4001-point search of
        # [0.25, 4] (log steps of ln 16 / 4000) restricted to that interval
        fine = [f for f in np.exp(np.log(0.25) + np.arange(4001) * math.log(16.0) / 4000) if GRID[i - 1] <= f <= GRID[i + 1]]
        curve = _curve(prob, y, fine)
        best = float(np.float32(fine[int(np.argmin(curve))]))
        print('n = %d, sharpened by %g: fitted %.6f, fine search %.6f (%.4f %% apart), NLL %.6f against %.6f' % (
            n, sharpen, t, best, 100 * abs(t / best - 1), v, min(curve)))
        assert abs(t / best - 1) <= 0.005
        assert abs(v - min(curve)) <= 1e-4 * min(curve) and v <= nll[i]


def test_fit_temperature_at_the_ends_of_the_grid_and_on_odd_grids():
    prob, y = _synthetic(2178, 1.9, 3)
    low = [t for t in GRID if t <= 1.0]                 # the minimum lies beyond the last point
    t, v, edge = CW.fit_temperature(low, CO.nll(prob, y, low)[0])
    assert (t, edge) == (1.0, 1) and v == CO.nll(prob, y, [1.0])[0, 0]
    high = [t for t in GRID if t >= 3.0]
    assert CW.fit_temperature(high, CO.nll(prob, y, high)[0])[::2] == (high[0], 1) and 3.0 < high[0] < 3.1
    assert CW.fit_temperature([2.0], [5.0]) == (2.0, 5.0, 1)
    # an exact parabola in log T on an uneven grid, given out of order: the vertex and its value
    ts = [4.0, 1.0, 2.0, 8.0]
    assert CW.fit_temperature(ts, [(math.log(t) - 1.0) ** 2 + 3.0 for t in ts]) == pytest.approx((math.e, 3.0, 0), rel=1e-12)
    assert CW.fit_temperature([1.0, 2.0, 4.0], [7.0, 7.0, 7.0])[1:] == (7.0, 1)      # flat: the first point, an end
    with pytest.raises(ValueError):
        CW.fit_temperature([], [])


# ---- evaluate on the fake device -------------------------------------------------------------------------------------------------
def _engine(tmp_path, monkeypatch, prob, y, exams, ids, batch, max_batch):
    e = fake_engine(monkeypatch, max_batch)
    ds = LabelledSlices(prob, y, exams, ids, batch) if y is not None else Slices(prob, exams, ids, batch)
    e._build(ds)
    e.current_step = 1
    run = str(tmp_path / 'run')
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    e.metrics = []
    return e, ds, run


def test_evaluate_calibration_files_hold_the_hand_computed_values(tmp_path, monkeypatch):
    prob, y = _two_slices()
    e, ds, run = _engine(tmp_path, monkeypatch, prob, y, ['a', 'a'], [0, 1], 2, 1)
    e.eval(_Pairs(ds), run, tag='p', export_csv=True)
    e.device_model.calls.clear()
    e.eval(_Pairs(ds), run, tag='c', export_csv=True, calibration_ds=ds, calibration=True, calibration_bins=4)
    calls = e.device_model.calls
    # one slice per call: forward and one calibration for the whole grid each, behind the evaluation
    assert [c for c in calls if c[0] != 'eval'] == [('forward', 1), ('calibration', 1, 4, GRID)] * 2
    plain, with_flag = _texts(os.path.join(run, 'tfevents', 'p')), _texts(os.path.join(run, 'tfevents', 'c'))
    assert sorted(set(with_flag) - set(plain)) == ['calibration_bins.csv', 'calibration_results.csv', 'calibration_slices.csv']
    assert all(with_flag[k] == v for k, v in plain.items()) and 'results.csv' in plain
    nll = CO.nll(prob, y, GRID)
    pooled = [float(v) / 16 for v in nll.sum(axis=0)]
    t_fit, v_fit, edge = CW.fit_temperature(GRID, pooled)
    assert with_flag['calibration_results.csv'].decode().splitlines() == [
        'step,' + ','.join(CW.CALIBRATION_RESULT_COLUMNS),
        '1,16,10,0.59375,0.625,0.03125,0.25,0.1953125,%r,%r,%r,%d' % (pooled[20], t_fit, v_fit, edge)]
    assert with_flag['calibration_bins.csv'].decode().splitlines() == [
        'step,bin,lower,upper,pixels,positives,mean_prob,frequency,gap', '1,0,0.0,0.25,2,0,0.0,0.0,0.0', '1,1,0.25,0.5,2,1,0.25,0.5,0.25',
        '1,2,0.5,0.75,2,1,0.5,0.5,0.0', '1,3,0.75,1.0,10,8,0.8,0.8,0.0']
    assert with_flag['calibration_slices.csv'].decode().splitlines() == [
        'step,exam,slice,pixels,positives,ece,brier,nll', '1,a,0,8,3,0.1875,0.265625,%r' % (float(nll[0, 20]) / 8),
        '1,a,1,8,7,0.125,0.125,%r' % (float(nll[1, 20]) / 8)]
    # a pixel at exactly 1 of class 0 costs 16.6 / T: the NLL keeps falling to the end of the grid
    assert v_fit < pooled[20] and (t_fit, edge) == (4.0, 1)


def test_evaluate_calibration_pools_over_calls_and_takes_a_grid_of_its_own(tmp_path, monkeypatch):
    prob, y = _drawn()
    e, ds, run = _engine(tmp_path, monkeypatch, prob, y, EXAMS, IDS, 4, 3)
    e.eval(_Pairs(ds), run, tag='c', calibration_ds=ds, calibration=True, calibration_bins=10, calibration_temperatures=(0.5, 2.0, 4.0),
           tta='flips')
    calls = [c for c in e.device_model.calls if c[0] != 'eval']
    own = [c for c in calls if c[0] in ('forward_tta', 'calibration')][-6:]
    assert own == sum([[('forward_tta', n, 0x0F), ('calibration', n, 10, [0.5, 1.0, 2.0, 4.0])] for n in (3, 1, 3)], [])
    text = _texts(os.path.join(run, 'tfevents', 'c'))
    lines = text['calibration_results.csv'].decode().splitlines()
    assert len(lines) == 2 and lines[1].split(',')[1] == str(7 * 144)
    assert len(text['calibration_slices.csv'].decode().splitlines()) == 1 + 7
    assert len(text['calibration_bins.csv'].decode().splitlines()) == 1 + 10
    # the flag without a data set of its own (or off) runs no pass; other ranks run none either
    e.device_model.calls.clear()
    e.eval(_Pairs(ds), run, tag='d', calibration=False, calibration_ds=ds)
    e.eval(_Pairs(ds), run, tag='e', calibration=True)
    assert not [c for c in e.device_model.calls if c[0] == 'calibration']


def test_the_fitted_temperature_calibrates_round_trip(tmp_path, monkeypatch):
    """over-confident slices: evaluate --calibration fits T; evaluate --calibration --temperature T measures the scaled
    probabilities and must fit a temperature within 1 % of 1"""
    p, y = _synthetic(6 * 400, 1.9, 11)
    prob, y = p.reshape(6, 20, 20), y.reshape(6, 20, 20)
    e, ds, run = _engine(tmp_path, monkeypatch, prob, y, ['a'] * 6, range(6), 3, 2)

    def fitted(tag, **kw):
        e.eval(_Pairs(ds), run, tag=tag, calibration_ds=ds, calibration=True, **kw)
        row = dict(zip(['step'] + CW.CALIBRATION_RESULT_COLUMNS,
                       _texts(os.path.join(run, 'tfevents', tag))['calibration_results.csv'].decode().splitlines()[1].split(',')))
        return {k: float(v) for k, v in row.items()}
    first = fitted('a')
    assert 1.5 < first['temperature'] < 2.4 and first['nll_at_temperature'] < first['nll'] and first['at_grid_edge'] == 0
    e.device_model.calls.clear()
    second = fitted('b', temperature=first['temperature'])
    assert abs(second['temperature'] - 1.0) <= 0.01
    assert second['nll'] == pytest.approx(first['nll_at_temperature'], rel=1e-3) and second['ece'] < first['ece']
    assert second['brier'] < first['brier']
    names = [c[0] for c in e.device_model.calls]
    assert names == ['eval', 'scale_temperature'] * 4 + ['forward', 'scale_temperature', 'calibration'] * 4      # chunks of 2, 1, 2, 1


# ---- --temperature: what runs, and in which order --------------------------------------------------------------------------------
class _SeenProb:
    """a pixel metric that keeps the probabilities it was given"""
    name = 'seen'

    def __init__(self):
        self.thresholds, self.planes = [0.5], []

    def reset_state(self):
        self.planes = []

    def update_state(self, dm, y):
        self.planes.append(np.asarray(dm.prob, np.float32).copy())

    def result(self):
        return float(len(self.planes))

    def merge(self, rank_sum):
        pass


def _order(calls, forwards=('forward', 'forward_tta', 'forward_tta_spread', 'eval')):
    """the names of the calls, chunk by chunk: every chunk starts at a forward"""
    chunks = []
    for c in calls:
        if c[0] in forwards and not (c[0].startswith('forward') and chunks and chunks[-1] == ['eval']):
            chunks.append([])
        chunks[-1].append(c[0])
    return chunks


def test_evaluate_temperature_scales_once_behind_every_forward(tmp_path, monkeypatch):
    prob, y = _drawn()
    e, ds, run = _engine(tmp_path, monkeypatch, prob, y, EXAMS, IDS, 4, 3)
    kw = dict(exam_ds=ds, exam_lesions=True, exam_filter_size=1, surface_ds=ds, surface_distances=True, surface_filter_size=1,
              calibration_ds=ds, calibration=True, export_csv=True)
    seen = _SeenProb()
    e.metrics = [seen]
    plain = e.eval(_Pairs(ds), run, tag='p', **kw)
    unscaled = list(seen.planes)
    assert not [c for c in e.device_model.calls if c[0] == 'scale_temperature']
    e.device_model.calls.clear()
    one = e.eval(_Pairs(ds), run, tag='one', temperature=1.0, **kw)                     # T = 1 is no flag at all
    assert not [c for c in e.device_model.calls if c[0] == 'scale_temperature'] and one == plain
    a, b = _texts(os.path.join(run, 'tfevents', 'p')), _texts(os.path.join(run, 'tfevents', 'one'))
    assert a == b and 'calibration_results.csv' in a
    e.device_model.calls.clear()
    scaled = e.eval(_Pairs(ds), run, tag='s', temperature=2.0, **kw)
    calls = e.device_model.calls
    # batch by batch: the test step, one scaling, then the metrics; every extra pass: the forward, one scaling, its consumers
    assert _order(calls) == ([['eval', 'scale_temperature']] * 3 + [['forward', 'scale_temperature', 'lesion_table_matched']] * 3 +
                             [['forward', 'scale_temperature', 'surface_distances']] * 3 +
                             [['forward', 'scale_temperature', 'calibration']] * 3)
    assert all(c[2] == 2.0 for c in calls if c[0] == 'scale_temperature')
    assert scaled[1]['loss'] == plain[1]['loss']                                        # the unscaled test step's
    assert len(seen.planes) == 3 and all(np.array_equal(s, CO.scale(u, 2.0)) for s, u in zip(seen.planes, unscaled))
    c = _texts(os.path.join(run, 'tfevents', 's'))
    assert c['calibration_results.csv'] != a['calibration_results.csv'] and c['surface_slices.csv'] == a['surface_slices.csv']
    # with views: the scaling comes behind forward_tta, and the spread of --uncertainty is that of the unscaled views
    e.device_model.calls.clear()
    e.eval(_Pairs(ds), run, tag='u', tta='flips', uncertainty_ds=ds, uncertainty=True, temperature=2.0)
    e.eval(_Pairs(ds), run, tag='v', tta='flips', uncertainty_ds=ds, uncertainty=True)
    assert _order(e.device_model.calls)[:6] == ([['eval', 'forward_tta', 'scale_temperature']] * 3 +
                                                [['forward_tta_spread', 'scale_temperature', 'spread_by_outcome']] * 3)
    u, v = (_texts(os.path.join(run, 'tfevents', t))['uncertainty_results.csv'].decode().splitlines()[1].split(',') for t in 'uv')
    assert u[2:7] == v[2:7] and float(u[-3]) + float(u[-2]) == pytest.approx(float(v[-3]) + float(v[-2]), rel=0.5)


def test_the_visualizer_scales_behind_its_forward(tmp_path, monkeypatch):
    prob, y = _drawn()
    e, ds, run = _engine(tmp_path, monkeypatch, prob, y, EXAMS, IDS, 4, 3)
    writer = CW.Writer()
    try:
        e._visualize(ds, 1, str(tmp_path / 'viz'), False, True, False, [], writer, temperature=0.5)
        e._visualize(ds, 1, str(tmp_path / 'viz2'), False, True, False, [], writer, tta_mask=0x0F, temperature=0.5)
    finally:
        writer.close()
    assert _order(e.device_model.calls) == [['forward', 'scale_temperature', 'render_composite']] * 3 + \
        [['forward_tta', 'scale_temperature', 'render_composite']] * 3


@pytest.mark.parametrize('flags', [{}, dict(link_slices=True), dict(tta='flips', uncertainty=True),
                                   dict(tta='d4', uncertainty=True, link_slices=True)], ids=str)
def test_annotate_temperature_scales_once_behind_every_forward(tmp_path, monkeypatch, flags):
    prob, _ = _drawn()
    e, ds, run = _engine(tmp_path, monkeypatch, prob, None, EXAMS, IDS, 4, 3)
    e.annotate(ds, run, str(tmp_path / 'p'), **KW, **flags)
    plain_calls = list(e.device_model.calls)
    e.device_model.calls.clear()
    e.annotate(ds, run, str(tmp_path / 'one'), temperature=1.0, **KW, **flags)
    assert e.device_model.calls == plain_calls and _texts(str(tmp_path / 'one')) == _texts(str(tmp_path / 'p'))
    e.device_model.calls.clear()
    e.annotate(ds, run, str(tmp_path / 's'), temperature=0.5, **KW, **flags)
    calls = e.device_model.calls
    want = []
    for c in plain_calls:                            # the same calls, with one scaling behind every forward
        want.append(c)
        if c[0].startswith('forward'):
            want.append(('scale_temperature', c[1], 0.5))
    assert calls == want and len([c for c in calls if c[0] == 'scale_temperature']) == 3
    a, b = _texts(str(tmp_path / 'p')), _texts(str(tmp_path / 's'))
    assert sorted(a) == sorted(b) and a['lesions.csv'] != b['lesions.csv']               # mean_prob and max_prob moved
    key = lambda text: [l.split(',')[:10] for l in text.decode().splitlines()]
    assert key(a['lesions.csv']) == key(b['lesions.csv'])                                # the lesions themselves did not (threshold 0.5)
    if 'uncertainty' in flags:                                                           # the spread is that of the unscaled views
        assert a['lesion_uncertainty.csv'] == b['lesion_uncertainty.csv'] and a['slice_uncertainty.csv'] == b['slice_uncertainty.csv']


def test_temperature_out_of_range_is_refused_before_anything_is_read(tmp_path, monkeypatch):
    from dnncancerannotator_amd import engine
    prob, y = _drawn()
    e, ds, run = _engine(tmp_path, monkeypatch, prob, y, EXAMS, IDS, 4, 3)
    touched = []
    monkeypatch.setattr(engine.TFKerasModel, 'load', lambda self, path: touched.append(path))
    monkeypatch.setattr(engine.TFKerasModel, 'get_ckpts', lambda self, path: touched.append(path) or {})
    for bad in (0.04, 20.5, 0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='--temperature'):
            e.annotate(ds, run, str(tmp_path / 'o'), temperature=bad)
        with pytest.raises(ValueError, match='--temperature'):
            e.eval(_Pairs(ds), run, tag='t', temperature=bad)
    for kw in (dict(calibration_bins=0), dict(calibration_bins=257), dict(calibration_temperatures=[0.01]),
               dict(calibration_temperatures=list(np.linspace(1.5, 2.5, 64)))):
        with pytest.raises(ValueError, match='--calibration'):
            e.eval(_Pairs(ds), run, tag='t', calibration=True, calibration_ds=ds, **kw)
    assert touched == [] and not os.path.exists(str(tmp_path / 'o')) and e.device_model.calls == []
    assert engine.check_temperature(None) is None and engine.check_temperature(1) is None and engine.check_temperature('0.05') == 0.05


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_and_signatures():
    from dnncancerannotator_amd import engine
    from dnncancerannotator_amd.runs.evaluate import evaluate
    from dnncancerannotator_amd.runs.predict import predict
    p = build_parser()
    ev, pr = ['evaluate', '--save_path', 's', '--data_path', 'd', '--tag', 't'], ['predict', '--save_path', 's', '--data_path', 'd', '--output', 'o']
    for base, fn, method in ((pr, predict, engine.TFKerasModel.annotate), (ev, evaluate, engine.TFKerasModel.eval)):
        assert 'temperature' not in vars(p.parse_args(base))                # the default is that of the run function
        assert inspect.signature(fn).parameters['temperature'].default is None
        assert inspect.signature(method).parameters['temperature'].default is None
        assert vars(p.parse_args(base + ['--temperature', '1.7']))['temperature'] == 1.7
    got = vars(p.parse_args(ev + ['--calibration', '--calibration_bins', '10', '--calibration_temperatures', '0.5', '2']))
    assert got['calibration'] is True and got['calibration_bins'] == 10 and got['calibration_temperatures'] == [0.5, 2.0]
    assert 'calibration' not in vars(p.parse_args(ev))
    sig = inspect.signature(evaluate).parameters
    assert sig['calibration'].default is False and sig['calibration_bins'].default == 15 and sig['calibration_temperatures'].default is None
    sig = inspect.signature(engine.TFKerasModel.eval).parameters
    assert sig['calibration'].default is False and sig['calibration_bins'].default == CW.CALIBRATION_BINS == 15
    with pytest.raises(SystemExit):
        p.parse_args(pr + ['--calibration'])


def test_cli_checks_the_flags_before_anything_is_read(monkeypatch, tmp_path):
    import yaml
    from dnncancerannotator_amd import __main__ as cli, engine
    touched, seen = [], []
    monkeypatch.setattr(engine.TFKerasModel, '__init__', lambda self, config: touched.append('init'))
    monkeypatch.setattr(engine.TFKerasModel, 'load', lambda self, path: touched.append('load'))
    monkeypatch.setattr(engine.TFKerasModel, 'eval', lambda self, dataset, **kw: seen.append(kw) or {})
    monkeypatch.setattr(engine.TFKerasModel, 'annotate', lambda self, dataset, **kw: seen.append(kw) or {})
    save = tmp_path / 'run'
    save.mkdir()                                     # no options.yaml yet: reading it first would raise another error
    ev = ['evaluate', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--tag', 't', '--skip_visualization']
    pr = ['predict', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--output', str(tmp_path / 'o')]
    for base in (ev, pr):
        for t in ('0.01', '25', 'nan'):
            with pytest.raises(ValueError, match='--temperature'):
                cli.main(base + ['--temperature', t])
    with pytest.raises(ValueError, match='--calibration_bins'):
        cli.main(ev + ['--calibration', '--calibration_bins', '300'])
    with pytest.raises(ValueError, match='--calibration_temperatures'):
        cli.main(ev + ['--calibration', '--calibration_temperatures', '30'])
    assert touched == [] and seen == []
    monkeypatch.undo()
    monkeypatch.setattr(engine.TFKerasModel, '__init__', lambda self, config: None)
    monkeypatch.setattr(engine.TFKerasModel, 'eval', lambda self, dataset, **kw: seen.append(kw) or {})
    monkeypatch.setattr(engine.TFKerasModel, 'annotate', lambda self, dataset, **kw: seen.append(kw) or {})
    (save / 'options.yaml').write_text(yaml.safe_dump({'config': {'data_options': {'eval': {'batch_size': 2}}}}))
    assert cli.main(ev + ['--calibration', '--temperature', '1.7']) == 0 and cli.main(ev + ['--temperature', '1']) == 0
    assert cli.main(pr + ['--temperature', '0.5']) == 0 and cli.main(pr + ['--temperature', '1.0']) == 0 and cli.main(ev) == 0
    assert seen[0]['calibration'] is True and seen[0]['calibration_ds'] is not None and seen[0]['temperature'] == 1.7
    assert seen[0]['calibration_bins'] == 15 and seen[0]['calibration_temperatures'] is None
    assert 'temperature' not in seen[1] and 'calibration' not in seen[1] and seen[2]['temperature'] == 0.5
    assert 'temperature' not in seen[3] and sorted(seen[1]) == sorted(seen[4])           # --temperature 1 is no flag at all
