"""CPU: the host side of `annotator evaluate --surface_distances`.  The brute-force oracle of the device call
(tests/surface_oracle.py) is held to scipy where scipy imports; casewise.surface_* on hand-written samples; engine._surface_pass on a
fake device that the oracle serves (tests/fake_surface_device.py); the flags of the command line.

Floats compare at 1e-12 relative: every value is a sqrt of an integer below 2^25 and sums of fewer than 2^20 float64 terms."""

import csv
import inspect
import io
import os
from collections import OrderedDict

import numpy as np
import pytest

import surface_oracle as SO
from dnncancerannotator_amd import casewise as CW
from dnncancerannotator_amd.__main__ import build_parser
from fake_surface_device import LabelledSlices, fake_engine

REL = 1e-12


def close(got, want):
    return abs(float(got) - float(want)) <= REL * abs(float(want))


# ---- the oracle against scipy ----------------------------------------------------------------------------------------------------
def test_oracle_against_scipy():
    ndi = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(11)
    checked = 0
    for i in range(200):
        density = (0.05, 0.3, 0.6, 0.9)[i % 4], (0.9, 0.5, 0.1, 0.4)[(i // 4) % 4]
        a, b = rng.random((12, 14)) < density[0], rng.random((12, 14)) < density[1]
        ea, eb = SO.boundary(a), SO.boundary(b)
        for m, e in ((a, ea), (b, eb)):
            assert np.array_equal(e, m & ~ndi.binary_erosion(m))              # 4-connected cross, border value 0
        if not (ea.any() and eb.any()):
            continue
        for mine, other in ((ea, eb), (eb, ea)):
            want = np.rint(ndi.distance_transform_edt(~other)[mine] ** 2).astype(np.int64)
            assert SO.nearest_d2(mine, other).tolist() == want.tolist()
        checked += 1
    assert checked > 150
    assert SO.boundary(np.ones((3, 4), bool)).sum() == 10 and not SO.boundary(np.zeros((3, 4), bool)).any()


def test_oracle_masks_are_the_other_oracles():
    import lesion_oracle as LO
    import match_cases as MC
    import match_oracle as MO
    prob, y, spec = MC.resized_opened()
    s = (spec['threshold'], spec['rf'], spec['k'])
    pred, true = SO.masks(prob, y, *s, min_area=40)
    assert np.array_equal(pred, LO.lesion_table(prob, *s, min_area=40)[2] > 0) and pred.sum((1, 2)).tolist() == [168, 168]
    assert np.array_equal(true.reshape(2, -1), MO.true_maps(y, spec['rf']) >= 0) and true.sum((1, 2)).tolist() == [87, 87]
    counts, samples, edges = SO.surface(prob, y, *s, min_area=40, max_samples=47)     # B alone: 2 (12 + 14) - 4
    assert counts[:, 3].tolist() == [48, 48] and len(samples) == 0 and int((edges & 1).sum()) == 96       # cut, never a subset
    assert 'LO.lesion_table' in inspect.getsource(SO.masks) and 'MO.true_maps' in inspect.getsource(SO.masks)


# ---- casewise.surface_* on hand-written samples ------------------------------------------------------------------------------------
def test_distance_values_and_the_interpolated_percentile():
    hd, p95, assd = CW.surface_distance_values([0, 1, 4], [9, 16])
    # d: 0 1 2 | 3 4.  The 95th percentile of 5 sorted values lies at index 0.95 * 4 = 3.8: 3 + 0.8 * (4 - 3)
    assert hd == 4.0 and close(p95, 3.8) and close(assd, (1.0 + 3.5) / 2)
    assert close(CW.surface_distance_values([0, 1, 4], [9, 16], percentile=50)[1], 2.0)
    assert close(CW.surface_distance_values([2], [2, 2, 8], percentile=100)[1], np.sqrt(8.0))
    hd, p95, assd = CW.surface_distance_values([2, 2], [8])
    assert close(hd, np.sqrt(8.0)) and close(assd, (np.sqrt(2.0) + np.sqrt(8.0)) / 2)
    assert close(p95, np.sqrt(2.0) + 0.9 * (np.sqrt(8.0) - np.sqrt(2.0)))       # index 0.95 * 2 = 1.9
    assert p95 == float(np.percentile(np.sqrt(np.array([2.0, 2.0, 8.0])), 95.0))
    with pytest.raises(ValueError):
        CW.surface_distance_values([], [1])


def test_every_status_of_a_slice():
    v = CW.surface_slice_values('e', 3, [36, 64, 36, 20, 28], [1] * 20, [1] * 24 + [2] * 4)
    assert v[:9] == ['e', 3, 'both', 36, 64, 36, 20, 28, repr(0.72)]
    assert close(v[9], np.sqrt(2.0)) and close(v[10], np.sqrt(2.0)) and close(v[11], (1.0 + (24 + 4 * np.sqrt(2.0)) / 28) / 2)
    # 44 ones, then 4 roots of 2: index 0.95 * 47 = 44.65 lies among the roots, 0.9 * 47 = 42.3 among the ones
    assert CW.surface_slice_values('e', 3, [36, 64, 36, 20, 28], [1] * 20, [1] * 24 + [2] * 4, percentile=90.0)[10] == repr(1.0)
    assert CW.surface_slice_values('e', 0, [9, 0, 0, 8, 0], [], []) == ['e', 0, 'pred_only', 9, 0, 0, 8, 0, repr(0.0), '', '', '']
    assert CW.surface_slice_values('e', 0, [0, 4, 0, 0, 4], [], [])[2:] == ['label_only', 0, 4, 0, 0, 4, repr(0.0), '', '', '']
    assert CW.surface_slice_values('e', 0, [0, 0, 0, 0, 0], [], [])[2:] == ['neither', 0, 0, 0, 0, 0, '', '', '', '']
    assert CW.surface_slice_values('e', 0, [600, 600, 300, 512, 512], [], [])[2:] == ['truncated', 600, 600, 300, 512, 512, repr(0.5), '', '', '']
    for counts, p, t in (([9, 9, 0, 8, 8], [1] * 8, [1] * 7), ([9, 0, 0, 8, 0], [1] * 8, []), ([9, 9, 0, 8, 8], [1] * 8, [])):
        with pytest.raises(ValueError):
            CW.surface_slice_values('e', 0, counts, p, t)
    assert CW.SURFACE_SLICE_COLUMNS[2] == 'status' and CW.SURFACE_SLICE_COLUMNS[8:] == ['dice', 'hd', 'hd_percentile', 'assd']
    assert len(v) == len(CW.SURFACE_SLICE_COLUMNS)


def test_exam_pools_the_samples_of_its_both_slices():
    a = ([4, 4, 1, 4, 4], [1, 4, 9, 16], [0, 0, 25, 36])
    b = ([2, 3, 0, 2, 3], [49, 64], [1, 1, 100])
    slices = [a, ([9, 0, 0, 8, 0], [], []), b, ([0, 0, 0, 0, 0], [], []), ([600, 600, 0, 512, 512], [], []), ([0, 4, 0, 0, 4], [], [])]
    v = CW.surface_exam_values('e', slices, percentile=90.0)
    assert v[:7] == ['e', 6, 2, 1, 1, 1, 1] and len(v) == len(CW.SURFACE_CASE_COLUMNS)
    dp, dt = np.sqrt(np.array([1, 4, 9, 16, 49, 64.0])), np.sqrt(np.array([0, 0, 25, 36, 1, 1, 100.0]))      # concatenated by hand
    assert close(v[7], 10.0) and close(v[8], np.percentile(np.concatenate([dp, dt]), 90.0)) and close(v[9], (dp.mean() + dt.mean()) / 2)
    assert close(v[9], (25 / 6 + 23 / 7) / 2)
    # not the mean of the slices' values
    assert not close(v[9], (float(CW.surface_slice_values('e', 0, *a)[11]) + float(CW.surface_slice_values('e', 2, *b)[11])) / 2)
    assert CW.surface_exam_values('f', slices[1:2] + slices[3:]) == ['f', 4, 0, 1, 1, 1, 1, '', '', '']
    assert CW.surface_exam_values('g', []) == ['g', 0, 0, 0, 0, 0, 0, '', '', '']


def test_summary_means_over_both_slices_and_exams_with_any():
    sv = [CW.surface_slice_values('e', 0, [4, 4, 1, 4, 4], [1, 4, 9, 16], [0, 0, 25, 36]),
          CW.surface_slice_values('e', 1, [9, 0, 0, 8, 0], [], []),
          CW.surface_slice_values('f', 0, [2, 3, 1, 2, 3], [49, 64], [1, 1, 100]),
          CW.surface_slice_values('g', 0, [0, 0, 0, 0, 0], [], []),
          CW.surface_slice_values('g', 1, [600, 600, 0, 512, 512], [], [])]
    ev = [CW.surface_exam_values('e', [([4, 4, 1, 4, 4], [1, 4, 9, 16], [0, 0, 25, 36]), ([9, 0, 0, 8, 0], [], [])]),
          CW.surface_exam_values('f', [([2, 3, 1, 2, 3], [49, 64], [1, 1, 100])]),
          CW.surface_exam_values('g', [([0, 0, 0, 0, 0], [], []), ([600, 600, 0, 512, 512], [], [])])]
    got = CW.surface_summary(sv, ev)
    assert got[:7] == [5, 2, 1, 0, 1, 1, 2] and len(got) == len(CW.SURFACE_RESULT_COLUMNS)
    assert close(got[7], (2 / 8 + 2 / 5) / 2) and close(got[8], (6.0 + 10.0) / 2)
    for i, j in ((9, 10), (10, 11)):
        assert close(got[i], (float(sv[0][j]) + float(sv[2][j])) / 2)
    for i, j in ((11, 7), (12, 8), (13, 9)):
        assert close(got[i], (float(ev[0][j]) + float(ev[1][j])) / 2)
    assert CW.surface_summary(sv[1:2], ev[2:]) == [1, 0, 1, 0, 0, 0, 0, '', '', '', '', '', '', '']
    assert CW.surface_summary([], []) == [0, 0, 0, 0, 0, 0, 0, '', '', '', '', '', '', '']


# ---- engine.eval on a fake device ------------------------------------------------------------------------------------------------
def _drawn():
    """7 slices of 12 x 12 of exams a (4 slices) and b (3): a labelled block under a prediction shifted by a pixel at 0.75, a second
    predicted block at 0.55 (below the second threshold) in slices 2..3, slice 5 without a prediction, slice 6 empty"""
    prob, y = np.zeros((7, 12, 12), np.float32), np.zeros((7, 12, 12), np.float32)
    y[0:6, 2:6, 2:6] = 1.0
    prob[0:5, 3:7, 2:6] = 0.75
    prob[2:4, 9:11, 1:4] = 0.55
    return prob, y


def _eval(tmp_path, monkeypatch, max_batch=3, rank=0, exam=False, **kw):
    from dnncancerannotator_amd import engine
    prob, y = _drawn()
    e = fake_engine(monkeypatch, max_batch)
    ds = LabelledSlices(prob, y, ['a'] * 4 + ['b'] * 3, [0, 1, 2, 3, 0, 1, 2], 4)
    monkeypatch.setattr(engine.TFKerasModel, '_evaluate', lambda self, dataset, staged=False: OrderedDict(loss=0.25))
    e._build(ds)
    e.current_step = 1
    run = str(tmp_path / ('run%d' % len(os.listdir(str(tmp_path)))))
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    e.ctx = e.ctx._replace(rank=rank)
    if exam:
        kw = dict(kw, exam_ds=ds, exam_lesions=True, exam_filter_size=1)
    rows = e.eval(ds, run, tag='t', export_csv=True, **kw)
    out = os.path.join(run, 'tfevents', 't')
    texts = {}
    for name in sorted(os.listdir(out)) if os.path.isdir(out) else []:
        with open(os.path.join(out, name), newline='') as f:
            texts[name] = f.read()
    return rows, texts, [c for c in e.device_model.calls if c[0] in ('forward', 'surface_distances', 'lesion_table_matched')], ds


def test_surface_pass_one_forward_per_split_one_call_per_threshold(tmp_path, monkeypatch):
    prob, y = _drawn()
    rows, texts, calls, ds = _eval(tmp_path, monkeypatch, surface_ds=None, surface_distances=True)
    assert calls == [] and sorted(texts) == ['results.csv']                    # no data set, no pass
    plain = texts
    kw = dict(surface_distances=True, surface_threshold=[0.5, 0.7], surface_filter_size=1, surface_percentile=90.0, surface_max_samples=18)
    ds = LabelledSlices(prob, y, ['a'] * 4 + ['b'] * 3, [0, 1, 2, 3, 0, 1, 2], 4)
    rows, texts, calls, _ = _eval(tmp_path, monkeypatch, surface_ds=ds, **kw)
    assert rows == OrderedDict([(1, OrderedDict(loss=0.25))])
    s = lambda n, thr: ('surface_distances', n, thr, 18)
    # data set batches of 4 and 3 on a device of 3 slices per call: splits of 3, 1, 3
    assert calls == [('forward', 3), s(3, 0.5), s(3, 0.7), ('forward', 1), s(1, 0.5), s(1, 0.7), ('forward', 3), s(3, 0.5), s(3, 0.7)]
    assert sorted(texts) == ['results.csv', 'surface_cases.csv', 'surface_results.csv', 'surface_slices.csv']
    assert texts['results.csv'] == plain['results.csv']
    results, cases, slices = [], [], []
    exams, ids = ['a'] * 4 + ['b'] * 3, [0, 1, 2, 3, 0, 1, 2]
    for thr in (0.5, 0.7):
        counts, samples, _ = SO.surface(prob, y, thr, 1.0, 1, 0, 18)
        d2 = lambda b, side: samples['d2'][(samples['slice'] == b) & (samples['side'] == side)]
        sv = [CW.surface_slice_values(exams[b], ids[b], counts[b], d2(b, 0), d2(b, 1), percentile=90.0) for b in range(7)]
        ev = [CW.surface_exam_values(n, [(counts[b], d2(b, 0), d2(b, 1)) for b in range(7) if exams[b] == n], percentile=90.0) for n in 'ab']
        slices += [[1, repr(thr)] + v for v in sv]
        cases += [[1, repr(thr)] + v for v in ev]
        results.append([1, repr(thr)] + CW.surface_summary(sv, ev))
    assert texts['surface_slices.csv'] == CW.plain_csv(['step', 'threshold'] + CW.SURFACE_SLICE_COLUMNS, slices)
    assert texts['surface_cases.csv'] == CW.plain_csv(['step', 'threshold'] + CW.SURFACE_CASE_COLUMNS, cases)
    assert texts['surface_results.csv'] == CW.plain_csv(['step', 'threshold'] + CW.SURFACE_RESULT_COLUMNS, results)
    lines = list(csv.DictReader(io.StringIO(texts['surface_slices.csv'])))
    assert [l['status'] for l in lines[:7]] == ['both', 'both', 'both', 'both', 'both', 'label_only', 'neither']
    assert [l['status'] for l in lines[7:]] == [l['status'] for l in lines[:7]]
    assert [l['edge_pred'] for l in lines[:7]] == ['12', '12', '18', '18', '12', '0', '0']     # 0.55 counts at 0.5 ...
    assert [l['edge_pred'] for l in lines[7:]] == ['12', '12', '12', '12', '12', '0', '0']     # ... and not at 0.7
    assert lines[0]['hd'] == repr(1.0) and lines[0]['dice'] == repr(0.75)
    res = list(csv.DictReader(io.StringIO(texts['surface_results.csv'])))
    assert [(r['slices'], r['both'], r['label_only'], r['neither'], r['exams']) for r in res] == [('7', '5', '1', '1', '2')] * 2
    # the bound: the 18 boundary pixels of slices 2 and 3 at 0.5 just fit; with one less these two slices are cut
    _, cut, _, _ = _eval(tmp_path, monkeypatch, surface_ds=ds, **dict(kw, surface_max_samples=17))
    status = [l['status'] for l in csv.DictReader(io.StringIO(cut['surface_slices.csv']))]
    assert status[:5] == ['both', 'both', 'truncated', 'truncated', 'both'] and status[7:12] == ['both'] * 5


def test_other_ranks_nothing_and_beside_the_exam_pass(tmp_path, monkeypatch):
    prob, y = _drawn()
    ds = LabelledSlices(prob, y, ['a'] * 4 + ['b'] * 3, [0, 1, 2, 3, 0, 1, 2], 4)
    _, texts, calls, _ = _eval(tmp_path, monkeypatch, rank=1, surface_ds=ds, surface_distances=True)
    assert texts == {} and calls == []
    _, alone, _, _ = _eval(tmp_path, monkeypatch, surface_ds=ds, surface_distances=True, surface_filter_size=1)
    _, exam, calls, _ = _eval(tmp_path, monkeypatch, exam=True)
    assert not [c for c in calls if c[0] == 'surface_distances'] and not [k for k in exam if k.startswith('surface')]
    _, both, calls, _ = _eval(tmp_path, monkeypatch, exam=True, surface_ds=ds, surface_distances=True, surface_filter_size=1)
    assert sorted(both) == sorted(set(alone) | set(exam))
    assert all(both[k] == v for k, v in alone.items()) and all(both[k] == v for k, v in exam.items())
    assert [c[0] for c in calls].count('forward') == 6                         # a pass of its own: three splits each


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_surface_flags(capsys):
    from dnncancerannotator_amd.runs.evaluate import evaluate
    p = build_parser()
    base = ['evaluate', '--save_path', 's', '--data_path', 'd', '--tag', 't']
    a = vars(p.parse_args(base))
    assert not [k for k in a if k.startswith('surface_')]                    # the defaults are those of runs.evaluate.evaluate
    sig = inspect.signature(evaluate).parameters
    assert {k: sig[k].default for k in sig if k.startswith('surface_')} == dict(
        surface_distances=False, surface_threshold=(0.5,), surface_percentile=95.0, surface_min_area=0, surface_filter_size=5,
        surface_resize_factor=1.0, surface_max_samples=65536)
    from dnncancerannotator_amd import engine
    esig = inspect.signature(engine.TFKerasModel.eval).parameters
    assert all(esig[k].default == sig[k].default for k in sig if k.startswith('surface_')) and esig['surface_ds'].default is None
    a = vars(p.parse_args(base + ['--surface_distances', '--surface_threshold', '0.3', '0.5', '--surface_percentile', '90',
                                  '--surface_min_area', '4', '--surface_filter_size', '3', '--surface_resize_factor', '0.5',
                                  '--surface_max_samples', '1000']))
    assert {k: v for k, v in a.items() if k.startswith('surface_')} == dict(
        surface_distances=True, surface_threshold=[0.3, 0.5], surface_percentile=90.0, surface_min_area=4, surface_filter_size=3,
        surface_resize_factor=0.5, surface_max_samples=1000)
    for flag, bad in (('--surface_threshold', 'x'), ('--surface_percentile', 'high'), ('--surface_max_samples', '0'),
                      ('--surface_filter_size', '2.5'), ('--surface_min_area', 'x'), ('--surface_resize_factor', 'half')):
        with pytest.raises(SystemExit) as e:
            p.parse_args(base + ['--surface_distances', flag, bad])
        assert e.value.code == 2 and flag[2:] in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--surface_samples', '3'])                        # no such flag


def test_evaluate_forwards_nothing_new_without_the_flag(monkeypatch, tmp_path):
    import yaml
    from dnncancerannotator_amd import __main__ as cli, engine
    from dnncancerannotator_amd.runs import evaluate as ev
    seen, built = [], []
    monkeypatch.setattr(engine.TFKerasModel, 'eval', lambda self, dataset, **kw: seen.append(kw) or {})
    monkeypatch.setattr(engine.TFKerasModel, '__init__', lambda self, config: None)
    make = ev.make_dataset
    monkeypatch.setattr(ev, 'make_dataset', lambda *a, **k: built.append(k.get('include_meta', False)) or make(*a, **k))
    save = tmp_path / 'run'
    save.mkdir()
    (save / 'options.yaml').write_text(yaml.safe_dump({'config': {'data_options': {'eval': {'batch_size': 2}}}}))
    base = ['evaluate', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--tag', 't', '--skip_visualization']
    flags = ['--surface_distances', '--surface_threshold', '0.3', '0.5']
    assert cli.main(base) == 0 and cli.main(base + ['--exam_lesions']) == 0
    assert not [k for kw in seen for k in kw if k.startswith('surface')]       # what model.eval saw before this flag existed
    assert built == [False, False, True]
    del built[:]
    assert cli.main(base + flags) == 0 and cli.main(base + flags + ['--exam_lesions']) == 0
    assert built == [False, True, False, True]                                 # one data set with meta, shared by the two flags
    assert seen[2]['surface_distances'] is True and seen[2]['surface_threshold'] == [0.3, 0.5] and seen[2]['surface_max_samples'] == 65536
    assert len(next(iter(seen[2]['surface_ds']))) == 4 and seen[2]['exam_ds'] is None and seen[2]['exam_lesions'] is False
    assert seen[3]['surface_ds'] is seen[3]['exam_ds'] and seen[3]['exam_lesions'] is True
    assert {k for k in seen[2] if k.startswith('surface')} == {
        'surface_ds', 'surface_distances', 'surface_threshold', 'surface_percentile', 'surface_min_area', 'surface_filter_size',
        'surface_resize_factor', 'surface_max_samples'}
