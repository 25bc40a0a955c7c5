"""CPU: `annotator evaluate --bootstrap` above the device -- the oracle of the resampling (tests/bootstrap_oracle.py) held to the
existing detection functions on the resample written out, casewise's pool, replicate values and interval, engine.check_bootstrap,
the command line, and the two passes on a fake device (tests/fake_bootstrap_device.py)."""

import csv
import io
import math
import os
from collections import OrderedDict

import numpy as np
import pytest

import bootstrap_cases as BC
import bootstrap_oracle as BO
from dnncancerannotator_amd import casewise as CW
from dnncancerannotator_amd.__main__ import build_parser
from fake_bootstrap_device import LabelledSlices, fake_engine
from test_detection_host import EXAMS, IDS, _drawn

F32 = np.float32


# ---- (a) the oracle against the existing functions ---------------------------------------------------------------------------
def test_oracle_equals_the_existing_functions_on_the_resample_written_out():
    exams, cands = CW.detection_bootstrap_inputs(BC.CASES)
    E, L = len(BC.CASES), BO.levels_of(cands)
    assert exams.dtype == BO.EXAM_DTYPE and cands.dtype == BO.CANDIDATE_DTYPE
    assert exams['tumours'].tolist() == [c['tumours'] for c in BC.CASES]
    # scores 0.96875 0.75 0.75 0 0 0.5 0.875 0.875 0.625 0.25 0.3125 0: dense ranks, 0 the lowest
    assert exams['score_rank'].tolist() == [7, 5, 5, 0, 0, 3, 6, 6, 4, 1, 2, 0]
    # descending confidence, ties by (exam, number); a level per distinct confidence
    assert cands['exam'].tolist() == [0, 6, 7, 1, 2, 2, 8, 0, 5, 8, 8, 5, 10, 2, 8, 9, 7]
    assert cands['level'].tolist() == [0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 5, 6, 7, 8, 8, 8, 9] and L == 10
    assert cands['hit'].tolist() == [1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    pool, strata = BO.plain(E)
    mult = BO.multiplicities(E, pool, strata, BC.REPLICATES, BC.SEED)
    assert (mult.sum(1) == E).all()
    rows, exact = BO.detection(exams, cands, mult)
    left_out = undefined = 0
    for row, m, x in zip(rows, mult, exact):
        curves, auroc = BC.reference_values(BC.CASES, m)
        assert int(row['positive_exams']) == sum(1 for c in BC.written_out(BC.CASES, m) if c['tumours'] > 0)
        assert float(x) == row['ap']
        BC.hold_to_reference(CW.detection_replicate_values(row, E), row, curves, auroc, L)
        left_out += int(m[0] == 0)
        undefined += int(auroc is None)
    assert 0 < left_out < BC.REPLICATES          # the top-ranked candidate's exam is left out by some replicates
    # the whole sample once (every multiplicity 1) is the estimate itself
    row, x = BO.detection(exams, cands, np.ones((1, E), np.int64))
    curves, auroc = BC.reference_values(BC.CASES, [1] * E)
    BC.hold_to_reference(CW.detection_replicate_values(row[0], E), row[0], curves, auroc, L)


def test_oracle_draws_by_hand():
    """E = 1: every draw picks the one exam; two strata of one: each exam exactly once; a stratum's draws stay inside it"""
    assert BO.multiplicities(1, [0], [1], 3, 9).tolist() == [[1]] * 3
    assert BO.multiplicities(2, [1, 0], [1, 1], 5, 9).tolist() == [[1, 1]] * 5
    m = BO.multiplicities(7, [6, 5, 4, 3, 2, 1, 0], [2, 5], 40, (1 << 63) + 5)
    assert (m[:, [6, 5]].sum(1) == 2).all() and (m[:, :5].sum(1) == 5).all() and len(set(map(tuple, m.tolist()))) > 20
    # the draw of (replicate 0, draw 0) is word 0 of Philox on the counter (0, 0, 0, 0): pool[(x * n) >> 32]
    from intensity_oracle import philox4x32_10
    x = int(philox4x32_10(np.zeros((1, 4), np.uint32), (5, 0))[0, 0])
    assert BO.draws(10, np.arange(10), [10], 1, 5)[0, 0] == (x * 10) >> 32
    # the same (seed, E, strata) resample identically whatever is resampled; another seed does not
    assert BO.multiplicities(9, *BO.plain(9), 4, 1).tolist() != BO.multiplicities(9, *BO.plain(9), 4, 2).tolist()


def test_exam_match_values_use_the_summary_arithmetic():
    cases = [['a', 2, 3, 1, 1, 2, 1, 0], ['b', 0, 1, 0, 0, 0, 1, 0], ['c', 1, 0, 0, 1, 0, 0, 0]]
    summary = CW.exam_match_summary(cases)
    assert summary[:7] == [3, 3, 4, 1, 2, 2, 2]
    assert summary[7:] == [repr(v) for v in CW.exam_match_replicate_values([3, 4, 1, 2, 2, 2], 3)]
    assert summary[7:] == [repr(float(F32(1) / (F32(3) + F32(1e-07)))), repr(float(F32(2) / (F32(4) + F32(1e-07)))),
                           repr(float(F32(2) * (F32(2) / (F32(4) + F32(1e-07))) * (F32(1) / (F32(3) + F32(1e-07))) /
                                      (F32(2) / (F32(4) + F32(1e-07)) + F32(1) / (F32(3) + F32(1e-07)) + F32(1e-07)))), repr(2 / 3)]
    assert CW.exam_match_summary([])[7:] == ['0.0', '0.0', '0.0', '0.0']
    # a resample: sums of m * counts
    cols = np.array([c[1:7] for c in cases], np.int32)
    m = np.array([[2, 0, 1]])
    assert CW.exam_match_replicate_values(BO.sums(cols, m)[0], 3) == CW.exam_match_replicate_values([5, 6, 2, 3, 4, 2], 3)


# ---- (b) the pool and the interval -------------------------------------------------------------------------------------------
def test_bootstrap_pool():
    pool, strata = CW.bootstrap_pool([1, 0, 1, 0, 0], False)
    assert pool.tolist() == [0, 1, 2, 3, 4] and strata.tolist() == [5] and pool.dtype == strata.dtype == np.int32
    pool, strata = CW.bootstrap_pool([True, False, True, False, False], True)
    assert pool.tolist() == [0, 2, 1, 3, 4] and strata.tolist() == [2, 3]
    for flags in ([1, 1, 1], [0, 0, 0]):         # an empty stratum is left out
        pool, strata = CW.bootstrap_pool(flags, True)
        assert pool.tolist() == [0, 1, 2] and strata.tolist() == [3]


def test_bootstrap_interval_by_hand():
    for values in ([], [None, None]):
        b = CW.bootstrap_interval(values, 0.95)
        assert (b['mean'], b['std'], b['lo'], b['hi'], b['n'], b['undefined']) == (None, None, None, None, 0, len(values))
    b = CW.bootstrap_interval([3.0], 0.95)
    assert (b['mean'], b['std'], b['lo'], b['hi'], b['n'], b['undefined']) == (3.0, 0.0, 3.0, 3.0, 1, 0)
    b = CW.bootstrap_interval([3.0, 1.0], 0.9)   # h = 0.05 and 0.95
    assert b['lo'] == pytest.approx(1.1, abs=1e-14) and b['hi'] == pytest.approx(2.9, abs=1e-14)
    assert (b['mean'], b['std'], b['n']) == (2.0, 1.0, 2)
    b = CW.bootstrap_interval([5.0, None, 1.0, 4.0, None, 2.0, 3.0], 0.8)     # h = 0.4 and 3.6 over 1 2 3 4 5
    assert b['lo'] == pytest.approx(1.4, abs=1e-14) and b['hi'] == pytest.approx(4.6, abs=1e-14)
    assert (b['mean'], b['n'], b['undefined']) == (3.0, 5, 2) and b['std'] == math.sqrt(2.0)
    b = CW.bootstrap_interval([0.0, 1.0, 2.0, 3.0, 4.0], 0.5000001)
    assert b['lo'] == pytest.approx(1.0, abs=1e-6) and b['hi'] == pytest.approx(3.0, abs=1e-6)


def test_bootstrap_interval_against_numpy():
    rng = np.random.default_rng(4)
    for n in (2, 3, 10, 101, 2000):
        v = rng.random(n) * rng.choice([1e-3, 1.0, 1e3])
        for level in (0.6, 0.9, 0.95, 0.99):
            b = CW.bootstrap_interval(v.tolist(), level)
            for got, q in ((b['lo'], (1 - level) / 2), (b['hi'], 1 - (1 - level) / 2)):
                want = float(np.quantile(v, q, method='linear'))
                assert abs(got - want) <= 2 * np.spacing(max(abs(got), abs(want))), (n, level, got, want)
            assert b['mean'] == pytest.approx(v.mean(), rel=1e-14) and b['std'] == pytest.approx(v.std(), rel=1e-12)


# ---- (c) check_bootstrap and the command line --------------------------------------------------------------------------------
REFUSED = [
    (dict(bootstrap=99), 'must be an integer in'), (dict(bootstrap=(1 << 20) + 1), 'must be an integer in'),
    (dict(bootstrap=200.0), 'must be an integer in'), (dict(bootstrap=True), 'must be an integer in'),
    (dict(bootstrap=200, detection=False), 'add one of them'),
    (dict(bootstrap=200, seed=-1), 'bootstrap_seed'), (dict(bootstrap=200, seed=1 << 64), 'bootstrap_seed'),
    (dict(bootstrap=200, seed=1.5), 'bootstrap_seed'),
    (dict(bootstrap=200, level=0.5), 'bootstrap_level'), (dict(bootstrap=200, level=1.0), 'bootstrap_level'),
    (dict(bootstrap=200, level=float('nan')), 'bootstrap_level'), (dict(bootstrap=200, level=0.3), 'bootstrap_level'),
    (dict(bootstrap=200, level='0.9'), 'bootstrap_level'),
    (dict(bootstrap=200, stratified=True, detection=False, exam_lesions=True), 'bootstrap_stratified'),
    (dict(seed=1), 'add --bootstrap'), (dict(level=0.9), 'add --bootstrap'), (dict(stratified=True), 'add --bootstrap'),
    (dict(seed=0), 'add --bootstrap'),
]


def test_check_bootstrap_values():
    from dnncancerannotator_amd.engine import check_bootstrap
    assert check_bootstrap() is None and check_bootstrap(None, None, None, False, True, True) is None
    assert check_bootstrap(100, detection=True) == dict(replicates=100, seed=0, level=0.95, stratified=False)
    assert check_bootstrap(1 << 20, (1 << 64) - 1, 0.9, True, True, False) == dict(replicates=1 << 20, seed=(1 << 64) - 1, level=0.9,
                                                                                  stratified=True)
    assert check_bootstrap(2000, exam_lesions=True)['replicates'] == 2000
    assert check_bootstrap(2000, stratified=True, detection=True, exam_lesions=True)['stratified'] is True
    for kw, message in REFUSED:
        with pytest.raises(ValueError, match=message):
            check_bootstrap(**dict(dict(detection=True), **kw))


def test_refusals_come_before_anything_is_read(tmp_path):
    """a save_path that does not exist: a bad value must be the error, not the missing options.yaml"""
    from dnncancerannotator_amd.runs.evaluate import evaluate
    nowhere = str(tmp_path / 'nowhere')
    names = dict(seed='bootstrap_seed', level='bootstrap_level', stratified='bootstrap_stratified')
    for kw, message in REFUSED:
        kw = dict(dict(detection=True), **{names.get(k, k): v for k, v in kw.items()})
        with pytest.raises(ValueError, match=message):
            evaluate(nowhere, ['synthetic:16x16x2'], 't', **kw)
    with pytest.raises(FileNotFoundError):
        evaluate(nowhere, ['synthetic:16x16x2'], 't', detection=True, bootstrap=200)
    assert not os.path.exists(nowhere)


def test_parser_bootstrap_flags():
    base = ['evaluate', '--save_path', 's', '--data_path', 'd', '--tag', 't']
    args = vars(build_parser('x').parse_args(base))
    assert not [k for k in args if k.startswith('bootstrap')]
    args = vars(build_parser('x').parse_args(base + ['--detection', '--bootstrap', '2000', '--bootstrap_seed', str((1 << 64) - 1),
                                                     '--bootstrap_level', '0.9', '--bootstrap_stratified']))
    assert (args['bootstrap'], args['bootstrap_seed'], args['bootstrap_level'], args['bootstrap_stratified']) == (
        2000, (1 << 64) - 1, 0.9, True)


def test_cli_flags_reach_engine_eval(monkeypatch, tmp_path):
    from dnncancerannotator_amd import engine, load
    from dnncancerannotator_amd.runs import evaluate as ev
    seen = []
    monkeypatch.setattr(engine.TFKerasModel, 'eval', lambda self, dataset, **kw: seen.append(kw) or {})
    monkeypatch.setattr(engine.TFKerasModel, '__init__', lambda self, config: None)
    monkeypatch.setattr(load, 'load_config', lambda path: dict(config={}))
    monkeypatch.setattr(ev, 'make_dataset', lambda *a, **k: object())
    ev.evaluate(str(tmp_path), ['d'], 't', detection=True)
    assert not [k for k in seen[-1] if k.startswith('bootstrap')]
    ev.evaluate(str(tmp_path), ['d'], 't', detection=True, bootstrap=300, bootstrap_stratified=True)
    assert {k: v for k, v in seen[-1].items() if k.startswith('bootstrap')} == dict(bootstrap=300, bootstrap_seed=0, bootstrap_level=0.95,
                                                                                    bootstrap_stratified=True)


# ---- (d) the passes on a fake device -----------------------------------------------------------------------------------------
# tests/test_detection_host.py's slices: exam a (a tumour found at 0.9, a false block at 0.3), b (no tumour, a false block at 0.6),
# c (a tumour, nothing found), d (a tumour found at 0.3)
HAND = [dict(exam='a', tumours=1, confidences=[float(F32(0.9)), float(F32(0.3))], hits=[1, 0]),
        dict(exam='b', tumours=0, confidences=[float(F32(0.6))], hits=[0]),
        dict(exam='c', tumours=1, confidences=[], hits=[]),
        dict(exam='d', tumours=1, confidences=[float(F32(0.3))], hits=[1])]
BOOT = ('bootstrap_sums', 'bootstrap_detection')


def _eval(tmp_path, monkeypatch, rank=0, **kw):
    from dnncancerannotator_amd import engine
    prob, y = _drawn()
    e = fake_engine(monkeypatch, 3)
    ds = LabelledSlices(prob, y, EXAMS, IDS, 4)
    monkeypatch.setattr(engine.TFKerasModel, '_evaluate', lambda self, dataset, staged=False: OrderedDict(loss=0.25))
    e._build(ds)
    e.current_step = 1
    run = str(tmp_path / ('run%d' % len(os.listdir(str(tmp_path)))))
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    e.ctx = e.ctx._replace(rank=rank)
    for name in ('detection_ds', 'exam_ds'):
        if kw.get(name):
            kw[name] = ds
    e.eval(ds, run, tag='t', export_csv=True, **kw)
    out = os.path.join(run, 'tfevents', 't')
    texts = {}
    for name in sorted(os.listdir(out)) if os.path.isdir(out) else []:
        with open(os.path.join(out, name), newline='') as f:
            texts[name] = f.read()
    return texts, [c for c in e.device_model.calls if c[0] in BOOT]


def test_detection_pass_with_bootstrap_on_the_fake_device(tmp_path, monkeypatch):
    flags = dict(detection_ds=True, detection=True, detection_min_area=4)
    R, seed = 100, 3
    plain, calls = _eval(tmp_path, monkeypatch, **flags)
    assert calls == [] and not [k for k in plain if 'bootstrap' in k]
    texts, calls = _eval(tmp_path, monkeypatch, bootstrap=R, bootstrap_seed=seed, **flags)
    assert calls == [('bootstrap_detection', 4, 4, R, seed, [0, 1, 2, 3], [4])]          # once per checkpoint, after the summary
    assert sorted(set(texts) - set(plain)) == ['detection_bootstrap.csv', 'detection_bootstrap_replicates.csv']
    assert all(texts[k] == v for k, v in plain.items())                                 # the old files byte for byte
    # the expected files from the hand-made cases and the oracle
    assert [str(v) for v in CW.detection_summary(HAND)[0]] == plain['detection_results.csv'].splitlines()[1].split(',')[1:]
    exams, cands = CW.detection_bootstrap_inputs(HAND)
    assert cands.tolist() == [(0, 1, 0), (1, 0, 1), (0, 0, 2), (3, 1, 2)] and exams.tolist() == [(1, 3), (0, 2), (1, 0), (1, 1)]
    mult = BO.multiplicities(4, *BO.plain(4), R, seed)
    rows, _ = BO.detection(exams, cands, mult)
    values = [CW.detection_replicate_values(r, 4) for r in rows]
    cfg = dict(replicates=R, seed=seed, level=0.95, stratified=False)
    estimates = plain['detection_results.csv'].splitlines()[1].split(',')[8:19]
    want = CW.plain_csv(['step'] + CW.BOOTSTRAP_COLUMNS, [[1] + l for l in CW.bootstrap_lines(CW.DETECTION_BOOTSTRAP_METRICS, estimates, values, cfg)])
    assert texts['detection_bootstrap.csv'] == want
    lines = list(csv.DictReader(io.StringIO(texts['detection_bootstrap.csv'])))
    assert [l['metric'] for l in lines] == ['ap', 'auroc', 'score', 'sensitivity_at_0.125', 'sensitivity_at_0.25', 'sensitivity_at_0.5',
                                            'sensitivity_at_1', 'sensitivity_at_2', 'sensitivity_at_4', 'sensitivity_at_8', 'cpm']
    assert list(lines[0]) == ['step', 'metric', 'estimate', 'mean', 'std', 'lo', 'hi', 'level', 'replicates', 'undefined', 'seed', 'stratified']
    ap = lines[0]
    assert float(ap['estimate']) == 1 / 3 + (2 / 3 - 1 / 3) * 0.5                       # test_detection_host.py's value by hand
    assert (ap['step'], ap['level'], ap['replicates'], ap['seed'], ap['stratified']) == ('1', '0.95', str(R), str(seed), '0')
    # a replicate without a tumour (only b drawn: (1/4)^4) is rare; one without a negative exam (b not drawn: (3/4)^4) is common
    no_tumour, no_pairs = int((rows['tumours'] == 0).sum()), int((rows['auroc_pairs'] == 0).sum())
    assert int(ap['undefined']) == no_tumour and int(lines[1]['undefined']) == no_pairs and 15 <= no_pairs <= 50
    assert int(lines[2]['undefined']) == int(((rows['tumours'] == 0) | (rows['auroc_pairs'] == 0)).sum())
    for l in lines:
        assert float(l['lo']) <= float(l['mean']) <= float(l['hi']) and float(l['std']) >= 0
    reps = list(csv.DictReader(io.StringIO(texts['detection_bootstrap_replicates.csv'])))
    assert list(reps[0]) == ['step'] + CW.DETECTION_REPLICATE_COLUMNS and len(reps) == R
    assert [int(r['replicate']) for r in reps] == list(range(R))
    for r, row, m, v in zip(reps, rows, mult, values):
        assert int(r['tumours']) == int(m[0] + m[2] + m[3]) == int(row['tumours']) and int(r['positive_exams']) == int(r['tumours'])
        assert int(r['candidates']) == int(2 * m[0] + m[1] + m[3]) and int(r['tp']) == int(m[0] + m[3]) and int(r['fp']) == int(m[0] + m[1])
        assert int(r['auroc_pairs']) == int((m[0] + m[2] + m[3]) * m[1])
        # b (0.6) lies below a (0.9) and above c (0) and d (0.3)
        assert int(r['auroc_twice']) == int(2 * m[0] * m[1])
        assert [r[k] for k in CW.DETECTION_BOOTSTRAP_METRICS] == ['' if x is None else repr(x) for x in v]
        assert [int(r['tp_at_%g' % x]) for x in CW.DETECTION_FP_RATES] == [int(t) for t in row['tp_at']]
    # stratified: the positive exams a, c, d first, then b; the old files stay, the new ones change
    strat, calls = _eval(tmp_path, monkeypatch, bootstrap=R, bootstrap_seed=seed, bootstrap_stratified=True, bootstrap_level=0.8, **flags)
    assert calls == [('bootstrap_detection', 4, 4, R, seed, [0, 2, 3, 1], [3, 1])]
    assert all(strat[k] == v for k, v in plain.items()) and strat['detection_bootstrap.csv'] != texts['detection_bootstrap.csv']
    lines = list(csv.DictReader(io.StringIO(strat['detection_bootstrap.csv'])))
    assert all((l['stratified'], l['level'], l['undefined']) == ('1', '0.8', '0') for l in lines)       # b and a tumour in every replicate
    # another rank writes nothing and calls nothing
    other, calls = _eval(tmp_path, monkeypatch, rank=1, bootstrap=R, **flags)
    assert calls == [] and other == {}


def test_exam_lesion_pass_with_bootstrap_on_the_fake_device(tmp_path, monkeypatch):
    flags = dict(exam_ds=True, exam_lesions=True, exam_filter_size=1, exam_threshold=(0.25, 0.55))
    R, seed = 100, 11
    plain, calls = _eval(tmp_path, monkeypatch, **flags)
    assert calls == []
    texts, calls = _eval(tmp_path, monkeypatch, bootstrap=R, bootstrap_seed=seed, **flags)
    assert sorted(set(texts) - set(plain)) == ['exam_lesion_bootstrap.csv'] and all(texts[k] == v for k, v in plain.items())
    per_thr = OrderedDict()
    for l in csv.DictReader(io.StringIO(plain['exam_lesion_cases.csv'])):
        per_thr.setdefault(l['threshold'], []).append([int(l[k]) for k in ('true', 'predicted', 'detected', 'missed', 'matched', 'false')])
    assert len(per_thr) == 2 and all(len(v) == 4 for v in per_thr.values())
    assert calls == [('bootstrap_sums', cols, R, seed, [4]) for cols in per_thr.values()]     # once per threshold
    results = list(csv.DictReader(io.StringIO(plain['exam_lesion_results.csv'])))
    lines = list(csv.DictReader(io.StringIO(texts['exam_lesion_bootstrap.csv'])))
    assert list(lines[0]) == ['step', 'threshold'] + CW.BOOTSTRAP_COLUMNS and len(lines) == 8
    mult = BO.multiplicities(4, *BO.plain(4), R, seed)
    for i, (thr, cols) in enumerate(per_thr.items()):
        sums = BO.sums(np.array(cols), mult)
        for k, name in enumerate(CW.EXAM_BOOTSTRAP_METRICS):
            l = lines[4 * i + k]
            b = CW.bootstrap_interval([CW.exam_match_replicate_values(s, 4)[k] for s in sums], 0.95)
            assert (l['threshold'], l['metric'], l['estimate']) == (thr, name, results[i][name])
            assert [l[c] for c in ('mean', 'std', 'lo', 'hi')] == [repr(b[c]) for c in ('mean', 'std', 'lo', 'hi')]
            assert (l['replicates'], l['undefined'], l['seed'], l['stratified'], l['level']) == (str(R), '0', str(seed), '0', '0.95')
    # false_per_exam by hand: the mean over replicates of sum m * false / 4
    false = np.array(per_thr[list(per_thr)[0]])[:, 5]
    assert float(lines[3]['mean']) == pytest.approx(float((mult @ false).mean()) / 4, rel=1e-12)
    # both passes at once, stratified: the exam-lesion pass stays plain and says so
    both, calls = _eval(tmp_path, monkeypatch, bootstrap=R, bootstrap_seed=seed, bootstrap_stratified=True, detection_ds=True, detection=True,
                        detection_min_area=4, **flags)
    assert [c[0] for c in calls] == ['bootstrap_sums', 'bootstrap_sums', 'bootstrap_detection'] and calls[-1][-1] == [3, 1]
    assert both['exam_lesion_bootstrap.csv'] == texts['exam_lesion_bootstrap.csv']
    assert {l['stratified'] for l in csv.DictReader(io.StringIO(both['detection_bootstrap.csv']))} == {'1'}
