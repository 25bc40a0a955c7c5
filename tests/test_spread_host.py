"""CPU: the host side of `--uncertainty`.  The numpy oracle of the views' spread (tests/spread_oracle.py) checked against itself --
above all that its inputs can tell an admissible formulation from the textbook one --, casewise's values, engine.annotate and
engine.eval on a fake device whose views disagree (tests/fake_spread_device.py), and the command line."""

import inspect
import os

import numpy as np
import pytest

import spread_oracle as SO
import tta_oracle as TO
from dnncancerannotator_amd import casewise as CW
from dnncancerannotator_amd.__main__ import build_parser
from fake_link_device import Slices
from fake_match_device import LabelledSlices
from fake_spread_device import fake_engine

MASKS = [1 << k for k in range(8)] + [0x0F, 0xFF, 0x07, 0xB4]


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def test_the_inputs_catch_the_textbook_formula_and_admit_the_shifted_one():
    caught = {}
    for f, fam in enumerate(SO.FAMILIES):
        for views in MASKS:
            n = len(TO.views_of(views))
            planes = SO.family(fam, (n, 2, 33, 33), 10 * views + f)
            want = SO.spread_of(planes, views)
            assert want.dtype == np.float64 and (want <= 0.5 + 2.0 ** -23).all() and (want >= 0).all()
            good = np.abs(SO.shifted32(planes, views).astype(np.float64) - want)
            assert (good <= SO.tolerance(want)).all(), (fam, views, good.max())
            if n == 1:
                assert not want.any() and not SO.shifted32(planes, views).any()
            bad = np.abs(SO.textbook32(planes, views).astype(np.float64) - want)
            caught[fam] = caught.get(fam, 0) + int((bad > SO.tolerance(want)).sum())
    # where the views agree to 1e-4 .. 1e-3 around a large p the textbook form loses everything: the bound must reject it there
    assert caught['near_0.9'] > 1000 and caught['near_1'] > 1000 and caught['one_ulp'] > 0, caught


def test_equal_views_have_no_spread_and_the_classes_partition_the_pixels():
    base = np.random.default_rng(1).random((2, 8, 8, 1)).astype(np.float32)
    planes = np.stack([TO.apply_view(base, k)[..., 0] for k in range(8)])
    assert not SO.spread_of(planes, 0xFF).any() and not SO.shifted32(planes, 0xFF).any()
    two = np.stack([np.zeros((1, 4, 4)), np.ones((1, 4, 4))]).astype(np.float32)
    assert (SO.spread_of(two, 0x03) == 0.5).all()                           # the largest spread there is
    rng = np.random.default_rng(2)
    prob, y = (rng.integers(0, 5, (3, 5, 7)) / 4.0).astype(np.float32), rng.choice(np.array([0, 0.5, 1], np.float32), (3, 5, 7))
    spread = (rng.integers(0, 65, (3, 5, 7)) / 128.0).astype(np.float32)
    out = SO.outcome(prob, spread, y, [0.0, 0.5, 1.0, 1.5])
    assert out.shape == (4, 3) and (out['n'].sum(axis=-1) == 35).all()
    assert (out['sum_q24'].sum(axis=-1) == SO.q24(spread).reshape(3, -1).sum(axis=1)[None]).all()
    assert (out[0]['n'][:, [0, 2]] == 0).all() and (out[3]['n'][:, [1, 3]] == 0).all()     # everything / nothing predicted
    assert int(out[1, 0]['n'][3]) == int(((y[0] > 0.5) & (prob[0] >= 0.5)).sum())           # 0.5 itself is predicted, a label of 0.5 is not
    assert SO.png_of(np.array([0.0, 0.001, 0.25, 0.5, 0.6], np.float32)).tolist() == [0, 1, 128, 255, 255]
    assert np.array_equal(CW.uncertainty_image(spread[0]), SO.png_of(spread[0]))


def test_lesion_spread_follows_the_lesion_table():
    prob = np.zeros((2, 6, 8), np.float32)
    prob[0, 1:3, 1:4] = 0.75
    prob[0, 4, 6] = 0.5
    spread = np.zeros_like(prob)
    spread[0, 1:3, 1:4] = 0.25
    spread[0, 0, 0] = 0.5
    spread[1, 5, 7] = 0.125
    rows, totals, _ = SO.LO.lesion_table(prob, 0.5, 1.0, 1)
    srows, stotals = SO.lesion_spread(prob, spread, 0.5, 1.0, 1)
    assert totals.tolist() == [2, 0] and srows['area'].tolist() == rows['area'].tolist() == [6, 1]
    assert srows['sum_spread_q24'].tolist() == [6 << 22, 0] and srows['max_spread'].tolist() == [0.25, 0.0]
    assert stotals['pixels'].tolist() == [48, 48] and stotals['sum_spread_q24'].tolist() == [(6 << 22) + (1 << 23), 1 << 21]
    assert stotals['max_spread'].tolist() == [0.5, 0.125]
    assert len(SO.lesion_spread(prob, spread, 0.5, 1.0, 1, max_lesions=1)[0]) == 1
    assert len(SO.lesion_spread(prob, spread, 0.5, 1.0, 1, min_area=2)[0]) == 1


# ---- casewise --------------------------------------------------------------------------------------------------------------------
def test_casewise_values():
    row = np.array([(0, 2, 6, 1, 1, 3, 2, 0.75, 12, 9, 6 * 3 << 22)], SO.LO.ROW_DTYPE)[0]
    srow = np.array([(0, 2, 6, 0.25, 6 << 22)], SO.LESION_SPREAD_DTYPE)[0]
    assert CW.lesion_uncertainty_values('e', 3, row, srow) == ['e', 3, 2, '0.25', '0.25']
    with pytest.raises(ValueError, match='spread record'):
        CW.lesion_uncertainty_values('e', 3, row, np.array([(0, 1, 6, 0.25, 0)], SO.LESION_SPREAD_DTYPE)[0])
    stotal = np.array([(48, 0.5, (6 << 22) + (1 << 23))], SO.SLICE_SPREAD_DTYPE)[0]
    assert CW.slice_uncertainty_values('e', 3, [row], [srow], 1, stotal) == ['e', 3, repr(2.0 / 48), '0.5', '0.25', 0]
    assert CW.slice_uncertainty_values('e', 3, [], [], 2, stotal)[-2:] == ['', 1]
    o = np.zeros((), SO.OUTCOME_DTYPE)
    o['n'], o['sum_q24'] = [40, 2, 0, 6], [40 << 20, 2 << 22, 0, 6 << 21]
    assert CW.outcome_slice_values('e', 3, o) == ['e', 3, 40, 2, 0, 6, '0.0625', '0.25', '', '0.125', '0.25', repr(52 / 46 / 16), repr(0.25 / (52 / 46 / 16))]
    assert CW.outcome_summary([o, o]) == [2, 80, 4, 0, 12] + CW.outcome_slice_values('e', 3, o)[6:]
    o['n'][1], o['sum_q24'][1] = 0, 0
    assert CW.outcome_slice_values('e', 3, o)[-3:] == ['', repr(52 / 46 / 16), '']     # nothing wrong: no ratio


# ---- annotate on the fake device -------------------------------------------------------------------------------------------------
def _drawn():
    """7 slices of 12 x 12 of exams a (4 slices) and b (3), as tests/test_tta_host.py draws them; slice 6 has no lesion, slice 5 is
    a checkerboard of 72 single-pixel lesions"""
    prob, y = np.zeros((7, 12, 12), np.float32), np.zeros((7, 12, 12), np.float32)
    y[0:6, 2:6, 2:6] = 1.0
    prob[0:5, 3:7, 2:6] = 0.75
    prob[2:4, 9:11, 1:4] = 0.625
    yy, xx = np.mgrid[0:12, 0:12]
    prob[5] = np.where((yy + xx) % 2 == 0, 0.875, 0.0)
    return prob, y


def _texts(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            with open(os.path.join(d, f), 'rb') as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


EXAMS, IDS = ['a'] * 4 + ['b'] * 3, [0, 1, 2, 3, 0, 1, 2]
KW = dict(threshold=0.5, filter_size=1, max_lesions=8)


def _annotate_setup(tmp_path, monkeypatch):
    prob, _ = _drawn()
    e = fake_engine(monkeypatch, 3)
    ds = Slices(prob, EXAMS, IDS, 4)
    e._build(ds)
    e.current_step = 1
    run = str(tmp_path / 'run')
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    return e, ds, run


def _expected_predict(views):
    """the two CSV texts and the PNGs from the oracles alone, slice by slice"""
    prob, _ = _drawn()
    planes = np.stack([(TO.apply_view(prob[..., None], k)[..., 0] * np.float32(1 - k / 32)).astype(np.float32) for k in TO.views_of(views)])
    mean, spread = TO.mean_of(planes, views), SO.spread_of(planes, views).astype(np.float32)
    s = (KW['threshold'], 1.0, KW['filter_size'], 0, KW['max_lesions'])
    lesions, slices, pngs = [], [], {}
    for i, (exam, k) in enumerate(zip(EXAMS, IDS)):
        rows, totals, _ = SO.LO.lesion_table(mean[i:i + 1], *s)
        srows, stotals = SO.lesion_spread(mean[i:i + 1], spread[i:i + 1], *s)
        lesions += [CW.lesion_uncertainty_values(exam, k, r, q) for r, q in zip(rows, srows)]
        slices.append(CW.slice_uncertainty_values(exam, k, rows, srows, totals[0], stotals[0]))
        pngs[os.path.relpath(CW.uncertainty_path('.', CW.tag_of(exam, k)), '.')] = CW.encode_png(SO.png_of(spread[i]))
    return CW.plain_csv(CW.LESION_UNCERTAINTY_COLUMNS, lesions), CW.plain_csv(CW.SLICE_UNCERTAINTY_COLUMNS, slices), pngs, slices


@pytest.mark.parametrize('link', [False, True])
def test_annotate_uncertainty_files(tmp_path, monkeypatch, link):
    e, ds, run = _annotate_setup(tmp_path, monkeypatch)
    e.annotate(ds, run, str(tmp_path / 'tta'), export_images=True, tta='flips', link_slices=link, **KW)
    plain_calls = list(e.device_model.calls)
    e.device_model.calls.clear()
    res = e.annotate(ds, run, str(tmp_path / 'unc'), export_images=True, tta='flips', uncertainty=True, link_slices=link, **KW)
    calls = e.device_model.calls
    # data set batches of 4 and 3 on a device of 3 slices per call: chunks of 3, 1, 3, each one forward with the spread
    assert [c for c in calls if c[0].startswith('forward')] == [('forward_tta_spread', n, 0x0F) for n in (3, 1, 3)]
    assert [c[0] for c in plain_calls if c[0].startswith('forward')] == ['forward_tta'] * 3
    assert [c[:2] for c in calls if c[0] == 'lesion_table_spread'] == [('lesion_table_spread', n) for n in (3, 1, 3)]
    assert [c for c in calls if c[0] == 'last_spread'] == [('last_spread', n) for n in (3, 1, 3)]
    if link:                         # the linked table runs exactly as without the flag; the spread records come from a second call
        assert [c for c in calls if c[0] == 'lesion_table_linked'] == [c for c in plain_calls if c[0] == 'lesion_table_linked']
        assert all(c[2] is False for c in calls if c[0] == 'lesion_table_spread')
    else:
        assert not [c for c in calls if c[0] == 'lesion_table']
    with_flag, without = _texts(str(tmp_path / 'unc')), _texts(str(tmp_path / 'tta'))
    lesions, slices, pngs, slice_values = _expected_predict(0x0F)
    assert sorted(set(with_flag) - set(without)) == sorted(['lesion_uncertainty.csv', 'slice_uncertainty.csv'] + list(pngs))
    assert all(with_flag[k] == v for k, v in without.items()) and 'lesions.csv' in without
    assert with_flag['lesion_uncertainty.csv'].decode() == lesions and with_flag['slice_uncertainty.csv'].decode() == slices
    assert {k: with_flag[k] for k in pngs} == pngs
    # one line per line of lesions.csv, in its order
    key = lambda text: [l.split(',')[:3] for l in text.decode().splitlines()[1:]]
    assert key(with_flag['lesion_uncertainty.csv']) == key(with_flag['lesions.csv']) and res['lesions'] == len(key(with_flag['lesions.csv']))
    # slice 5 has 72 components, 8 of them listed: truncated; slice 6 has no lesion: no mean over lesions
    assert [v[-1] for v in slice_values] == [0, 0, 0, 0, 0, 1, 0] and slice_values[6][-2] == '' and slice_values[0][-2] != ''
    assert float(slice_values[0][2]) > 0 and res['slices'] == 7


def test_annotate_uncertainty_without_images_keeps_the_plane_on_the_device(tmp_path, monkeypatch):
    e, ds, run = _annotate_setup(tmp_path, monkeypatch)
    e.annotate(ds, run, str(tmp_path / 'unc'), tta='d4', uncertainty=True, **KW)
    assert not [c for c in e.device_model.calls if c[0] == 'last_spread']
    assert [c for c in e.device_model.calls if c[0].startswith('forward')] == [('forward_tta_spread', n, 0xFF) for n in (3, 1, 3)]
    texts = _texts(str(tmp_path / 'unc'))
    assert sorted(texts) == ['lesion_uncertainty.csv', 'lesions.csv', 'slice_uncertainty.csv', 'slices.csv']
    assert texts['lesion_uncertainty.csv'].decode() == _expected_predict(0xFF)[0]


def test_uncertainty_without_views_is_refused_before_load(tmp_path, monkeypatch):
    from dnncancerannotator_amd import engine
    e, ds, run = _annotate_setup(tmp_path, monkeypatch)
    touched = []
    monkeypatch.setattr(engine.TFKerasModel, 'load', lambda self, path: touched.append(path))
    monkeypatch.setattr(engine.TFKerasModel, 'get_ckpts', lambda self, path: touched.append(path) or {})
    for kw in (dict(), dict(tta='none')):
        with pytest.raises(ValueError, match='--tta flips'):
            e.annotate(ds, run, str(tmp_path / 'o'), uncertainty=True, **kw)
        with pytest.raises(ValueError, match='--tta flips'):
            e.eval(ds, run, tag='t', uncertainty=True, uncertainty_ds=ds, **kw)
    assert touched == [] and not os.path.exists(str(tmp_path / 'o'))


# ---- eval on the fake device -----------------------------------------------------------------------------------------------------
class _Pairs:
    """the (x, y) batches of a LabelledSlices: what the evaluation itself reads"""

    def __init__(self, ds):
        self.ds, self.element_spec = ds, ds.element_spec

    def __iter__(self):
        for x, y, _, _ in self.ds:
            yield x, y


def test_eval_uncertainty_files(tmp_path, monkeypatch):
    prob, y = _drawn()
    e = fake_engine(monkeypatch, 3)
    ds = LabelledSlices(prob, y, EXAMS, IDS, 4)
    e._build(ds)
    e.current_step = 1
    run = str(tmp_path / 'run')
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    e.metrics = []
    kw = dict(exam_ds=ds, exam_lesions=True, exam_filter_size=1, surface_ds=ds, surface_distances=True, surface_filter_size=1)
    e.eval(_Pairs(ds), run, tag='t', export_csv=True, tta='flips', **kw)
    e.device_model.calls.clear()
    thrs = (0.5, 0.7)
    e.eval(_Pairs(ds), run, tag='u', export_csv=True, tta='flips', uncertainty_ds=ds, uncertainty=True, uncertainty_thresholds=thrs, **kw)
    calls = e.device_model.calls
    # one more pass, behind the others: chunks of 3, 1, 3, one forward with the spread and one outcome call for both thresholds each
    assert [c for c in calls if c[0] in ('forward_tta_spread', 'spread_by_outcome')] == sum(
        [[('forward_tta_spread', n, 0x0F), ('spread_by_outcome', n, [0.5, 0.7])] for n in (3, 1, 3)], [])
    assert calls[-1][0] == 'spread_by_outcome' and not [c for c in calls if c[0] == 'last_spread']
    plain, with_flag = _texts(os.path.join(run, 'tfevents', 't')), _texts(os.path.join(run, 'tfevents', 'u'))
    assert sorted(set(with_flag) - set(plain)) == ['uncertainty_results.csv', 'uncertainty_slices.csv']
    assert all(with_flag[k] == v for k, v in plain.items()) and 'surface_slices.csv' in plain
    planes = np.stack([(TO.apply_view(prob[..., None], k)[..., 0] * np.float32(1 - k / 32)).astype(np.float32) for k in range(4)])
    want = SO.outcome(TO.mean_of(planes, 0x0F), SO.spread_of(planes, 0x0F).astype(np.float32), y, thrs)
    results, slices = [], []
    for t, thr in enumerate(thrs):
        slices += [[1, repr(thr)] + CW.outcome_slice_values(p, k, o) for p, k, o in zip(EXAMS, IDS, want[t])]
        results.append([1, repr(thr)] + CW.outcome_summary(list(want[t])))
    assert with_flag['uncertainty_results.csv'].decode() == CW.plain_csv(['step', 'threshold'] + CW.UNCERTAINTY_RESULT_COLUMNS, results)
    assert with_flag['uncertainty_slices.csv'].decode() == CW.plain_csv(['step', 'threshold'] + CW.UNCERTAINTY_SLICE_COLUMNS, slices)
    assert results[0][2 + 1 + 3] > 0 and results[0][-1] != ''          # true positives, and a ratio of wrong to right
    # the flag without a data set of its own (or off) runs no pass
    e.device_model.calls.clear()
    e.eval(_Pairs(ds), run, tag='v', export_csv=True, tta='flips', uncertainty=False, uncertainty_ds=ds)
    assert not [c for c in e.device_model.calls if c[0] == 'forward_tta_spread']


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_and_signatures():
    from dnncancerannotator_amd import engine
    from dnncancerannotator_amd.runs.evaluate import evaluate
    from dnncancerannotator_amd.runs.predict import predict
    p = build_parser()
    for base, fn, method in ((['predict', '--save_path', 's', '--data_path', 'd', '--output', 'o'], predict, engine.TFKerasModel.annotate),
                             (['evaluate', '--save_path', 's', '--data_path', 'd', '--tag', 't'], evaluate, engine.TFKerasModel.eval)):
        assert 'uncertainty' not in vars(p.parse_args(base))                # the default is that of the run function
        assert inspect.signature(fn).parameters['uncertainty'].default is False
        assert inspect.signature(method).parameters['uncertainty'].default is False
        assert vars(p.parse_args(base + ['--tta', 'flips', '--uncertainty']))['uncertainty'] is True
    ev = p.parse_args(['evaluate', '--save_path', 's', '--data_path', 'd', '--tag', 't', '--uncertainty_threshold', '0.25', '0.5'])
    assert ev.uncertainty_threshold == [0.25, 0.5]
    assert inspect.signature(evaluate).parameters['uncertainty_threshold'].default == (0.5,)
    assert inspect.signature(engine.TFKerasModel.eval).parameters['uncertainty_thresholds'].default == (0.5,)
    with pytest.raises(SystemExit):
        p.parse_args(['predict', '--save_path', 's', '--data_path', 'd', '--output', 'o', '--uncertainty_threshold', '0.5'])


def test_cli_refuses_uncertainty_without_views_before_anything_is_read(monkeypatch, tmp_path):
    import yaml
    from dnncancerannotator_amd import __main__ as cli, engine
    touched = []
    monkeypatch.setattr(engine.TFKerasModel, '__init__', lambda self, config: touched.append('init'))
    monkeypatch.setattr(engine.TFKerasModel, 'load', lambda self, path: touched.append('load'))
    seen = []
    monkeypatch.setattr(engine.TFKerasModel, 'eval', lambda self, dataset, **kw: seen.append(kw) or {})
    monkeypatch.setattr(engine.TFKerasModel, 'annotate', lambda self, dataset, **kw: seen.append(kw) or {})
    save = tmp_path / 'run'
    save.mkdir()
    (save / 'options.yaml').write_text(yaml.safe_dump({'config': {'data_options': {'eval': {'batch_size': 2}}}}))
    ev = ['evaluate', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--tag', 't', '--skip_visualization']
    pr = ['predict', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--output', str(tmp_path / 'o')]
    for base in (ev, pr):
        for flags in (['--uncertainty'], ['--uncertainty', '--tta', 'none']):
            with pytest.raises(ValueError, match='--tta flips'):
                cli.main(base + flags)
    assert touched == [] and seen == []
    assert cli.main(ev + ['--tta', 'flips', '--uncertainty', '--uncertainty_threshold', '0.25', '0.5']) == 0
    assert cli.main(pr + ['--tta', 'd4', '--uncertainty']) == 0 and cli.main(pr + ['--tta', 'd4']) == 0
    assert seen[0]['uncertainty'] is True and seen[0]['uncertainty_thresholds'] == (0.25, 0.5) and seen[0]['uncertainty_ds'] is not None
    assert seen[1]['uncertainty'] is True and 'uncertainty' not in seen[2]
