"""CPU tests of `--ensemble`: the oracle's own properties (tests/ensemble_oracle.py), engine.check_ensemble / parse_member /
check_uncertainty on temporary directories, the command line, and eval / annotate on a fake device
(tests/fake_ensemble_device.py): the keyword travels only with the flag and forward_ensemble runs once per batch."""

import inspect
import json
import os

import numpy as np
import pytest

import ensemble_oracle as EO
from dnncancerannotator_amd import casewise as CW
from dnncancerannotator_amd.__main__ import build_parser
from fake_ensemble_device import fake_engine, member_planes
from fake_link_device import Slices
from fake_match_device import LabelledSlices
from test_spread_host import EXAMS, IDS, KW, _Pairs, _drawn, _texts

COUNTS = (1, 2, 3, 5, 8, 16)
PLANE = (2, 33, 35)


def _worst(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want) / EO.tolerance(want)))


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def test_one_member_and_equal_members_have_nothing_between_them():
    for family in EO.FAMILIES:
        one = EO.family(family, (1,) + PLANE, 1)
        assert not EO.between_of(one).any() and not EO.shifted32(one)[0].any()
        for n in (2, 3, 16):
            same = np.repeat(one, n, axis=0)
            between, within, total = EO.shifted32(same)
            assert not EO.between_of(same).any() and not between.any() and not within.any() and not total.any()
        assert EO.mean_of(one).tobytes() == one[0].tobytes()
        assert EO.mean_of(np.repeat(one, 2, axis=0)).tobytes() == one[0].tobytes()


def test_the_total_is_the_sum_of_the_two_variances():
    means = EO.family('uniform', (5,) + PLANE, 2)
    withins = EO.drawn_withins(means.shape, 3)
    b, w, t = EO.between_of(means), EO.within_of(means, withins), EO.total_of(means, withins)
    assert np.allclose(t ** 2, b ** 2 + w ** 2, rtol=1e-14, atol=0) and (t >= np.maximum(b, w)).all()
    assert not EO.within_of(means).any() and np.array_equal(EO.total_of(means), b)
    # the law of total variance: V = 4 views per member drawn around each member's mean with the member's own spread
    rng = np.random.default_rng(4)
    views = rng.random((5, 4) + PLANE)
    total = views.reshape((20,) + PLANE).std(axis=0)
    assert np.allclose(total, EO.total_of(views.mean(axis=1), views.std(axis=1)), rtol=1e-6)


def test_the_inputs_catch_the_textbook_formula_and_admit_the_shifted_one():
    worst = {'between': 0.0, 'within': 0.0, 'total': 0.0}
    for family in EO.FAMILIES:
        for n in COUNTS:
            means = EO.family(family, (n,) + PLANE, 10 + n)
            for zero in (False, True):
                withins = EO.drawn_withins(means.shape, 20 + n, zero=zero)
                got = EO.shifted32(means, withins)
                want = (EO.between_of(means), EO.within_of(means, withins), EO.total_of(means, withins))
                for name, g, w in zip(worst, got, want):
                    worst[name] = max(worst[name], _worst(g, w))
    print('float32 emulation of ens_join, worst error in units of the tolerance: %s' % worst)
    assert worst['between'] < 0.5 and worst['within'] < 0.5 and worst['total'] < 0.5       # the bound leaves the device room
    for family in ('near_1', 'one_ulp'):
        means = EO.family(family, (5,) + PLANE, 30)
        assert _worst(EO.textbook32(means), EO.between_of(means)) > 1.0, family
        assert _worst(EO.shifted32(means)[0], EO.between_of(means)) < 1.0, family


def test_casewise_values():
    assert CW.ENSEMBLE_UNCERTAINTY_RESULT_COLUMNS[:5] == ['slices', 'tn_px', 'fp_px', 'fn_px', 'tp_px']
    assert len(CW.ENSEMBLE_UNCERTAINTY_RESULT_COLUMNS) == 5 + 3 * 7 and 'mean_between_wrong' in CW.ENSEMBLE_UNCERTAINTY_RESULT_COLUMNS
    import spread_oracle as SO
    prob = np.array([[[0.25, 0.75], [0.75, 0.25]]], np.float32)
    y = np.array([[[0.0, 1.0], [0.0, 1.0]]], np.float32)
    planes = [np.full((1, 2, 2), v, np.float32) for v in (0.125, 0.25, 0.5)]
    outs = [list(SO.outcome(prob, p, y, [0.5])[0]) for p in planes]
    line = CW.ensemble_outcome_summary(*outs)
    assert len(line) == len(CW.ENSEMBLE_UNCERTAINTY_RESULT_COLUMNS) and line[:5] == [1, 1, 1, 1, 1]
    assert line[5:12] == ['0.125'] * 6 + ['1.0'] and line[12:19] == ['0.25'] * 6 + ['1.0'] and line[19:] == ['0.5'] * 6 + ['1.0']
    other = list(SO.outcome(1 - prob, planes[0], y, [0.5])[0])
    other[0]['n'][0] += 1
    with pytest.raises(ValueError, match='classed differently'):
        CW.ensemble_outcome_summary(other, outs[1], outs[2])
    b = np.array([[0.0, 0.5], [0.25, 0.25]], np.float32)
    assert CW.slice_ensemble_uncertainty_values('e', 3, b, np.zeros_like(b)) == ['e', 3, '0.25', '0.5', '0.0', '0']


# ---- check_ensemble --------------------------------------------------------------------------------------------------------------
VARS = [dict(name='conv.kernel', shape=[3, 3, 1, 2], trainable=True, offset=0), dict(name='bn.moving_mean', shape=[2], trainable=False, offset=0)]
INFOS = [('conv.kernel', (3, 3, 1, 2), True, 0), ('bn.moving_mean', (2,), False, 0)]


def _run(root, name, steps, variables=VARS, ema=()):
    base = os.path.join(str(root), name, 'checkpoints')
    os.makedirs(base)
    for step in steps:
        index = dict(format='dnnca-ckpt-1', step=step, iterations=step, learning_rate=1e-3, variables=variables)
        if step in ema:
            index['ema'] = dict(decay=0.9, warmup=True, num_updates=step)
        with open(os.path.join(base, 'ckpt-%d.index' % step), 'w') as f:
            json.dump(index, f)
    return os.path.join(str(root), name)


def test_parse_member():
    from dnncancerannotator_amd import engine
    assert engine.parse_member('runs/fold1') == ('runs/fold1', None)
    assert engine.parse_member('runs/fold1:800') == ('runs/fold1', 800)
    assert engine.parse_member('host:/data/run') == ('host:/data/run', None)        # a colon that leads no step
    assert engine.parse_member('c:/x:12') == ('c:/x', 12)
    assert engine.parse_member(('r', 5)) == ('r', 5) and engine.parse_member(('r', None)) == ('r', None)


def test_check_ensemble(tmp_path):
    from dnncancerannotator_amd import engine
    own = _run(tmp_path, 'fold0', (800, 900), ema=(800, 900))
    f1 = _run(tmp_path, 'fold1', (800, 900), ema=(800, 900))
    f2 = _run(tmp_path, 'fold2', (800,), ema=())
    odd = _run(tmp_path, 'odd', (800, 900), variables=VARS[:1])
    ck = lambda run, step: os.path.join(run, 'checkpoints', 'ckpt-%d' % step)      # noqa: E731
    # a member without a step follows the step being read; a pinned one stays
    got = engine.check_ensemble(own, [f1, f1 + ':800'], [800, 900], param_infos=INFOS)
    assert got == {800: [ck(f1, 800), ck(f1, 800)], 900: [ck(f1, 900), ck(f1, 800)]}
    assert engine.check_ensemble(own, [(own, 800), (own, 900)], [900]) == {900: [ck(own, 800), ck(own, 900)]}       # snapshots of one run
    # predict without --step: every unpinned member's own latest checkpoint
    assert engine.check_ensemble(own, [f1, f2], [None]) == {None: [ck(f1, 900), ck(f2, 800)]}
    # a missing step: one error that names the first
    with pytest.raises(ValueError, match=r'no checkpoint of step 900 under .*fold2/checkpoints \(have \[800\]\)'):
        engine.check_ensemble(own, [f1, f2, odd], [800, 900])
    with pytest.raises(ValueError, match=r'no checkpoint of step 700 under .*fold1/checkpoints'):
        engine.check_ensemble(own, [f1 + ':700'], [800])
    with pytest.raises(ValueError, match=r'no checkpoint of step 800 under .*nowhere/checkpoints \(have \[\]\)'):
        engine.check_ensemble(own, [str(tmp_path / 'nowhere')], [800])
    # a member of another architecture: against the model, and before a model exists against save_path's own checkpoint
    for infos in (INFOS, None):
        with pytest.raises(ValueError, match=r'odd/checkpoints/ckpt-800 does not match the model'):
            engine.check_ensemble(own, [f1, odd], [800], param_infos=infos)
    # at most 15
    with pytest.raises(ValueError, match='at most 15 members'):
        engine.check_ensemble(own, [f1] * 16, [800])
    assert len(engine.check_ensemble(own, [f1] * 15, [800])[800]) == 15
    with pytest.raises(ValueError, match='at least one member'):
        engine.check_ensemble(own, [], [800])
    # --weights ema: every member needs an average
    assert engine.check_ensemble(own, [f1], [800], weights='ema') == {800: [ck(f1, 800)]}
    with pytest.raises(ValueError, match=r'--weights ema: checkpoint .*fold2/checkpoints/ckpt-800 holds no weight average'):
        engine.check_ensemble(own, [f1, f2], [800], weights='ema')


def test_check_uncertainty():
    from dnncancerannotator_amd import engine
    for tta in ('none',):
        with pytest.raises(ValueError, match='--tta flips'):
            engine.check_uncertainty(True, tta)
        with pytest.raises(ValueError, match='--tta flips'):
            engine.check_uncertainty(True, tta, None)
        with pytest.raises(ValueError, match='--tta flips'):
            engine.check_uncertainty(True, tta, [])
        engine.check_uncertainty(True, tta, [('run', None)])            # the spread between the members alone
        engine.check_uncertainty(False, tta)
    engine.check_uncertainty(True, 'flips')
    engine.check_uncertainty(True, 'd4', [('run', 3)])


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_and_signatures():
    from dnncancerannotator_amd import engine
    from dnncancerannotator_amd.runs.evaluate import evaluate
    from dnncancerannotator_amd.runs.predict import predict
    p = build_parser()
    for base, fn, method in ((['predict', '--save_path', 's', '--data_path', 'd', '--output', 'o'], predict, engine.TFKerasModel.annotate),
                             (['evaluate', '--save_path', 's', '--data_path', 'd', '--tag', 't'], evaluate, engine.TFKerasModel.eval)):
        assert 'ensemble' not in vars(p.parse_args(base))                   # the default is that of the run function
        assert inspect.signature(fn).parameters['ensemble'].default is None
        assert inspect.signature(method).parameters['ensemble'].default is None
        assert vars(p.parse_args(base + ['--ensemble', 'r1', 'r2:800', '--uncertainty']))['ensemble'] == ['r1', 'r2:800']
        with pytest.raises(SystemExit):
            p.parse_args(base + ['--ensemble'])
    for name in ('_forward_on_device',):
        assert inspect.signature(getattr(engine, name)).parameters['ensemble'].default is None
    for name in ('_evaluate', '_visualize', '_forwarded_splits', '_exam_lesion_pass', '_detection_pass', '_surface_pass', '_uncertainty_pass',
                 '_calibration_pass'):
        assert inspect.signature(getattr(engine.TFKerasModel, name)).parameters['ensemble'].default is None


def test_cli_resolves_the_members_before_anything_is_read(monkeypatch, tmp_path):
    import yaml
    from dnncancerannotator_amd import __main__ as cli, engine
    touched, seen = [], []
    monkeypatch.setattr(engine.TFKerasModel, '__init__', lambda self, config: touched.append('init'))
    monkeypatch.setattr(engine.TFKerasModel, 'eval', lambda self, dataset, **kw: seen.append(kw) or {})
    monkeypatch.setattr(engine.TFKerasModel, 'annotate', lambda self, dataset, **kw: seen.append(kw) or {})
    save = _run(tmp_path, 'fold0', (800, 900))
    f1 = _run(tmp_path, 'fold1', (800,))
    with open(os.path.join(save, 'options.yaml'), 'w') as f:
        yaml.safe_dump({'config': {'data_options': {'eval': {'batch_size': 2}}}}, f)
    ev = ['evaluate', '--save_path', save, '--data_path', 'synthetic:16x16x2', '--tag', 't', '--skip_visualization']
    pr = ['predict', '--save_path', save, '--data_path', 'synthetic:16x16x2', '--output', str(tmp_path / 'o')]
    with pytest.raises(ValueError, match='no checkpoint of step 900 under .*fold1'):
        cli.main(ev + ['--ensemble', f1])
    with pytest.raises(ValueError, match='no checkpoint of step 900 under .*fold1'):
        cli.main(pr + ['--ensemble', f1, '--step', '900'])
    with pytest.raises(ValueError, match='at most 15'):
        cli.main(pr + ['--ensemble'] + [f1] * 16)
    assert touched == [] and seen == []
    assert cli.main(ev + ['--ensemble', f1, '--step_range', '800', '800', '--uncertainty']) == 0
    assert cli.main(pr + ['--ensemble', f1, save + ':800', '--uncertainty']) == 0 and cli.main(pr) == 0 and cli.main(ev) == 0
    assert seen[0]['ensemble'] == [(f1, None)] and seen[0]['uncertainty'] is True and 'tta' not in seen[0]
    assert seen[1]['ensemble'] == [(f1, None), (save, 800)]
    assert 'ensemble' not in seen[2] and 'ensemble' not in seen[3]


# ---- eval and annotate on the fake device ----------------------------------------------------------------------------------------
def _runs(tmp_path, e, n=2):
    """the run of the engine itself and n further ones, each with a checkpoint of step 1"""
    e.current_step = 1
    runs = [str(tmp_path / ('run%d' % i)) for i in range(n + 1)]
    for i, run in enumerate(runs):
        e.device_model.init_glorot(seed=i + 1)
        e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    e.device_model.init_glorot(seed=1)
    return runs


def test_annotate_passes_the_keyword_only_with_the_flag(tmp_path, monkeypatch):
    from dnncancerannotator_amd import engine
    prob, _ = _drawn()
    e = fake_engine(monkeypatch, 3)
    ds = Slices(prob, EXAMS, IDS, 4)
    e._build(ds)
    runs = _runs(tmp_path, e)
    seen = []
    real = engine._forward_on_device
    monkeypatch.setattr(engine, '_forward_on_device', lambda *a, **kw: seen.append(kw) or real(*a, **kw))
    e.annotate(ds, runs[0], str(tmp_path / 'plain'), **KW)
    assert seen and all('ensemble' not in kw for kw in seen) and not [c for c in e.device_model.calls if c[0] in ('set_members', 'forward_ensemble')]
    del seen[:]
    e.device_model.calls.clear()
    res = e.annotate(ds, runs[0], str(tmp_path / 'ens'), ensemble=[(runs[1], None), (runs[2], 1)], uncertainty=True, **KW)
    dm = e.device_model
    assert all(kw.get('ensemble') is True for kw in seen) and len(seen) == 3
    # batches of 4 and 3 on a device of 3 slices per call: chunks of 3, 1, 3, ONE call each for all three members
    assert [c for c in dm.calls if c[0].startswith('forward')] == [('forward_ensemble', n, 1, True) for n in (3, 1, 3)]
    assert [c for c in dm.calls if c[0] == 'set_members'] == [('set_members', 3)]
    stored = [engine.read_member(os.path.join(r, 'checkpoints', 'ckpt-1')) for r in runs]
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(dm.members, stored))
    assert not np.array_equal(stored[0][0], stored[1][0])
    plain, ens = _texts(str(tmp_path / 'plain')), _texts(str(tmp_path / 'ens'))
    assert sorted(set(ens) - set(plain)) == ['lesion_uncertainty.csv', 'slice_ensemble_uncertainty.csv', 'slice_uncertainty.csv']
    assert ens['lesions.csv'] != plain['lesions.csv'] and res['slices'] == 7
    # the new file from the oracle alone: without views the spread is purely between the members
    lines = []
    for i, (exam, k) in enumerate(zip(EXAMS, IDS)):
        means, withins = member_planes(prob[i:i + 1, ..., None], 1, 3)
        assert not withins.any()
        lines.append(CW.slice_ensemble_uncertainty_values(exam, k, EO.between_of(means).astype(np.float32)[0],
                                                          EO.within_of(means, withins).astype(np.float32)[0]))
    assert ens['slice_ensemble_uncertainty.csv'].decode() == CW.plain_csv(CW.SLICE_ENSEMBLE_UNCERTAINTY_COLUMNS, lines)
    assert any(float(l[2]) > 0 for l in lines) and all(l[4] == '0.0' for l in lines)
    # with views the members run under them, and without --uncertainty no plane leaves the device
    dm.calls.clear()
    e.annotate(ds, runs[0], str(tmp_path / 'tta'), ensemble=[(runs[1], None)], tta='flips', **KW)
    assert [c for c in dm.calls if c[0].startswith('forward')] == [('forward_ensemble', n, 0x0F, False) for n in (3, 1, 3)]
    assert not [c for c in dm.calls if c[0] in ('last_ensemble_spread', 'last_spread')]
    assert sorted(_texts(str(tmp_path / 'tta'))) == ['lesions.csv', 'slices.csv']
    # a member that is missing is refused before the model is touched
    dm.calls.clear()
    with pytest.raises(ValueError, match='no checkpoint under .*nowhere'):
        e.annotate(ds, runs[0], str(tmp_path / 'no'), ensemble=[(str(tmp_path / 'nowhere'), None)], **KW)
    assert dm.calls == [] and not os.path.exists(str(tmp_path / 'no'))


def test_eval_passes_the_keyword_only_with_the_flag(tmp_path, monkeypatch):
    from dnncancerannotator_amd import engine
    import spread_oracle as SO
    prob, y = _drawn()
    e = fake_engine(monkeypatch, 3)
    ds = LabelledSlices(prob, y, EXAMS, IDS, 4)
    e._build(ds)
    runs = _runs(tmp_path, e, n=1)
    e.metrics = []
    seen = []
    real = engine._forward_on_device
    monkeypatch.setattr(engine, '_forward_on_device', lambda *a, **kw: seen.append(kw) or real(*a, **kw))
    kw = dict(exam_ds=ds, exam_lesions=True, exam_filter_size=1, surface_ds=ds, surface_distances=True, surface_filter_size=1)
    e.eval(_Pairs(ds), runs[0], tag='plain', export_csv=True, **kw)
    assert seen and all('ensemble' not in k for k in seen)
    assert not [c for c in e.device_model.calls if c[0] in ('set_members', 'forward_ensemble')]
    del seen[:]
    e.device_model.calls.clear()
    thrs = (0.5, 0.7)
    e.eval(_Pairs(ds), runs[0], tag='ens', export_csv=True, ensemble=[(runs[1], None)], uncertainty_ds=ds, uncertainty=True,
           uncertainty_thresholds=thrs, **kw)
    calls = e.device_model.calls
    assert all(k.get('ensemble') is True for k in seen) and len(seen) == 3 * 3           # three passes of three chunks
    # the evaluation itself: batches of 4 and 3 in chunks of 3, 1, 3, each a test step and then ONE ensemble call
    head = [c for c in calls if c[0] in ('eval', 'forward_ensemble')][:6]
    assert head == sum([[('eval', n), ('forward_ensemble', n, 1, False)] for n in (3, 1, 3)], [])
    assert [c for c in calls if c[0] == 'forward_ensemble'][3:] == [('forward_ensemble', n, 1, False) for n in (3, 1, 3)] * 2 + \
        [('forward_ensemble', n, 1, True) for n in (3, 1, 3)]
    assert not [c for c in calls if c[0] in ('forward', 'forward_tta', 'forward_tta_spread')]
    assert [c for c in calls if c[0] == 'set_members'] == [('set_members', 2)]
    plain, ens = _texts(os.path.join(runs[0], 'tfevents', 'plain')), _texts(os.path.join(runs[0], 'tfevents', 'ens'))
    assert sorted(set(ens) - set(plain)) == ['ensemble_uncertainty_results.csv', 'uncertainty_results.csv', 'uncertainty_slices.csv']
    # the three components from the oracle alone
    means, withins = member_planes(prob[..., None], 1, 2)
    mean = EO.mean_of(means)
    planes = [f(means, withins).astype(np.float32) for f in (lambda m, w: EO.between_of(m), EO.within_of, EO.total_of)]
    lines, results = [], []
    for t, thr in enumerate(thrs):
        outs = [list(SO.outcome(mean, p, y, [thr])[0]) for p in planes]
        lines.append([1, repr(thr)] + CW.ensemble_outcome_summary(*outs))
        results.append([1, repr(thr)] + CW.outcome_summary(outs[2]))
    assert ens['ensemble_uncertainty_results.csv'].decode() == CW.plain_csv(['step', 'threshold'] + CW.ENSEMBLE_UNCERTAINTY_RESULT_COLUMNS, lines)
    assert ens['uncertainty_results.csv'].decode() == CW.plain_csv(['step', 'threshold'] + CW.UNCERTAINTY_RESULT_COLUMNS, results)
    # a bigger batch than the model holds elsewhere: _ensure_capacity carries the members to the model that replaces this one
    e2 = fake_engine(monkeypatch)
    small = LabelledSlices(prob[:2], y[:2], EXAMS[:2], IDS[:2], 2)
    e2._build(small)
    e2.metrics = []
    e2.eval(_Pairs(ds), runs[0], tag='grown', export_csv=True, ensemble=[(runs[1], None)])
    assert e2.device_model.max_batch == 4 and len(e2.device_model.members) == 2
    assert [c for c in e2.device_model.calls if c[0] == 'forward_ensemble'] == [('forward_ensemble', 4, 1, False), ('forward_ensemble', 3, 1, False)]
