"""CPU: the host side of `annotator evaluate --exam_lesions`: casewise.match_exam_lesions and exam_match_summary on hand-written
tables, engine.eval's exam pass on a fake device (tests/fake_match_device.py: the numpy oracles in the place of
dnnca_lesion_table_matched), and the command line."""

import csv
import inspect
import io
import os
from collections import OrderedDict

import numpy as np
import pytest

import lesion_oracle as LO
import match_oracle as MO
from dnncancerannotator_amd import casewise as CW
from dnncancerannotator_amd.__main__ import build_parser
from fake_match_device import LabelledSlices, fake_engine


def rows_of(*areas):
    """lesion rows of one slice with these areas (every other field plausible: link_lesions divides sums by the volume)"""
    r = np.zeros(len(areas), LO.ROW_DTYPE)
    r['row'], r['area'] = np.arange(len(areas)), areas
    r['x1'], r['y1'], r['max_prob'] = 3, 3, 0.75
    return r


def exam(true_areas, true_links, pred_areas, pred_links, pairs, totals=None, iou=0.3):
    """slices of hand-written areas -> match_exam_lesions' (case, lines); totals: (true, predicted) kept components per slice"""
    n = len(true_areas)
    tt, pt = totals or ([len(a) for a in true_areas], [len(a) for a in pred_areas])
    ts = [(10 + i, rows_of(*true_areas[i]), tt[i]) for i in range(n)]
    ps = [(10 + i, rows_of(*pred_areas[i]), pt[i]) for i in range(n)]
    return CW.match_exam_lesions('/d/e', ts, ps, CW.link_lesions('/d/e', ts, true_links), CW.link_lesions('/d/e', ps, pred_links), pairs,
                                 iou=iou)


def test_one_tumour_under_two_predictions_and_a_false_one():
    """T runs through three slices (volume 30).  P0 covers it in slices 10 and 11 (16 voxels, all common: IoU 16 / 30), P1 in
    slice 12 (12 voxels, all common: 12 / 30); P2 (slice 11) touches nothing: two hits, one detected, two matched, one false"""
    case, lines = exam([[10], [10], [10]], [[], [(0, 0, 10)], [(0, 0, 10)]],
                       [[8], [8, 5], [12]], [[], [(0, 0, 8)], []],
                       [[(0, 0, 8)], [(0, 0, 8)], [(0, 0, 12)]])
    assert case == ['/d/e', 1, 3, 1, 0, 2, 1, 0]
    assert [l[:7] for l in lines] == [['true', '/d/e', 0, 10, 12, 3, 30], ['predicted', '/d/e', 0, 10, 11, 2, 16],
                                      ['predicted', '/d/e', 1, 11, 11, 1, 5], ['predicted', '/d/e', 2, 12, 12, 1, 12]]
    assert lines[0][7:] == [0, 16, repr(16 / 30), repr(32 / 46), 1]            # the best partner of T is P0
    assert lines[1][7:] == [0, 16, repr(16 / 30), repr(32 / 46), 1]
    assert lines[2][7:] == [-1, 0, '0.0', '0.0', 0]                            # false: no partner
    assert lines[3][7:] == [0, 12, repr(12 / 30), repr(24 / 42), 1]
    text = CW.plain_csv(['step', 'threshold'] + CW.EXAM_MATCH_COLUMNS, [[7, repr(0.5)] + l for l in lines])
    assert text.splitlines()[0] == 'step,threshold,kind,exam,exam_lesion,first_slice,last_slice,n_slices,volume_px,partner,overlap_px,iou,dice,hit'
    back = list(csv.DictReader(io.StringIO(text)))
    assert float(back[0]['iou']) == 16 / 30 and back[2]['partner'] == '-1'


def test_the_equality_case_is_a_hit_and_no_overlap_is_none():
    """overlap / union == iou exactly hits (>=, plain float division); overlap 0 never hits, not even with iou 0"""
    one = lambda pairs, iou, pa=9: exam([[30]], [[]], [[pa]], [[]], [pairs], iou=iou)[0]
    assert 9 / 30 == 0.3
    assert one([(0, 0, 9)], 0.3)[3:7] == [1, 0, 1, 0]                          # 9 / (30 + 9 - 9) == 0.3
    assert one([(0, 0, 9)], np.nextafter(0.3, 1))[3:7] == [0, 1, 0, 1]
    assert one([(0, 0, 10)], 0.5, pa=10)[3:7] == [0, 1, 0, 1]              # 10 / 30 < 0.5
    assert exam([[20]], [[]], [[10]], [[]], [[(0, 0, 10)]], iou=0.5)[0][3:7] == [1, 0, 1, 0]      # 10 / 20 == 0.5
    case, lines = exam([[30]], [[]], [[9]], [[]], [[(0, 0, 0)]], iou=0.0)
    assert case[3:7] == [0, 1, 0, 1] and [l[7:] for l in lines] == [[-1, 0, '0.0', '0.0', 0]] * 2
    assert one([], 0.0)[3:7] == [0, 1, 0, 1]
    assert one([(0, 0, 1)], 0.0)[3:7] == [1, 0, 1, 0]


def test_overlaps_sum_over_parts_and_the_best_partner_breaks_ties_by_number():
    """T0 (two slices, 20) and T1 (one slice, 10) under one P through both slices (volume 24): overlap(T0, P) = 6 + 6 over its
    parts; two predictions with the same IoU on one tumour: the smaller number is the partner"""
    case, lines = exam([[10, 10], [10]], [[], [(0, 0, 5)]], [[12], [12]], [[], [(0, 0, 12)]],
                       [[(0, 0, 6), (1, 0, 4)], [(0, 0, 6)]], iou=0.3)
    assert case == ['/d/e', 2, 1, 1, 1, 1, 0, 0]
    assert [l[7:] for l in lines] == [[0, 12, repr(12 / 32), repr(24 / 44), 1], [0, 4, repr(4 / 30), repr(8 / 34), 0],
                                      [0, 12, repr(12 / 32), repr(24 / 44), 1]]
    _, lines = exam([[20]], [[]], [[5, 5]], [[]], [[(0, 0, 5), (0, 1, 5)]], iou=0.3)
    assert lines[0][7:9] == [0, 5] and lines[0][-1] == 0


def test_empty_exam_truncated_slice_and_refusals():
    assert exam([], [], [], [], []) == (['/d/e', 0, 0, 0, 0, 0, 0, 0], [])
    assert exam([[], []], [[], []], [[], []], [[], []], [[], []]) == (['/d/e', 0, 0, 0, 0, 0, 0, 0], [])
    assert exam([[4]], [[]], [[4]], [[]], [[(0, 0, 4)]], totals=([1], [3]))[0] == ['/d/e', 1, 1, 1, 0, 1, 0, 1]
    assert exam([[4]], [[]], [[4]], [[]], [[(0, 0, 4)]], totals=([2], [1]))[0][-1] == 1
    with pytest.raises(ValueError):
        exam([[4]], [[]], [[4]], [[]], [[(0, 1, 4)]])                           # a row the slice does not have
    with pytest.raises(ValueError):
        exam([[4]], [[]], [[4]], [[]], [])


def test_summary_uses_the_region_metrics_expression():
    from dnncancerannotator_amd import region_metrics as RM
    cases = [['a', 3, 4, 2, 1, 3, 1, 0], ['b', 1, 0, 0, 1, 0, 0, 1]]
    got = CW.exam_match_summary(cases)
    assert got[:7] == [2, 4, 4, 2, 2, 3, 1]
    m = RM.RegionBasedConfusionMatrix([0.5])
    eps = np.float32(m.epsilon)
    r, p = np.float32(2) / (np.float32(4) + eps), np.float32(3) / (np.float32(4) + eps)
    assert got[7:] == [repr(float(r)), repr(float(p)), repr(float(np.float32(2) * p * r / (p + r + eps))), repr(0.5)]
    assert CW.exam_match_summary([]) == [0, 0, 0, 0, 0, 0, 0, '0.0', '0.0', '0.0', '0.0']
    assert 'EXAM_EPSILON' in inspect.getsource(CW.exam_match_summary) and CW.EXAM_EPSILON == m.epsilon and CW.EXAM_IOU == 0.30


# ---- engine.eval on a fake device ------------------------------------------------------------------------------------------------
KW = dict(exam_filter_size=1)


def _drawn():
    """7 slices of 12 x 12: a labelled tumour through slices 0..4 and one in slice 5 alone; the prediction finds the first one
    shifted by a pixel at 0.75 (slices 0..5) and draws a false block at 0.55 (below the second threshold) in slices 2..3"""
    prob, y = np.zeros((7, 12, 12), np.float32), np.zeros((7, 12, 12), np.float32)
    y[0:5, 2:6, 2:6] = 1.0
    y[5, 8:10, 8:10] = 1.0
    prob[0:6, 3:7, 2:6] = 0.75
    prob[2:4, 9:11, 1:4] = 0.55
    return prob, y


def _eval(tmp_path, monkeypatch, prob, y, exams, ids, batch, max_batch=None, rank=0, viz=False, **kw):
    from dnncancerannotator_amd import engine
    e = fake_engine(monkeypatch, max_batch)
    ds = LabelledSlices(prob, y, exams, ids, batch)
    seen = []
    monkeypatch.setattr(engine.TFKerasModel, '_evaluate', lambda self, dataset, staged=False: OrderedDict(loss=0.25))
    monkeypatch.setattr(engine.TFKerasModel, '_visualize', lambda self, *a, **k: seen.append('visualize'))
    e._build(ds)
    e.current_step = 1
    run = str(tmp_path / ('run%d' % len(os.listdir(str(tmp_path)))))
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    e.ctx = e.ctx._replace(rank=rank)
    rows = e.eval(ds, run, viz_ds=ds if viz else None, tag='t', export_csv=True, exam_ds=ds, **dict(KW, **kw))
    out = os.path.join(run, 'tfevents', 't')
    texts = {}
    for name in sorted(os.listdir(out)) if os.path.isdir(out) else []:
        with open(os.path.join(out, name), newline='') as f:
            texts[name] = f.read()
    return rows, texts, [c for c in e.device_model.calls if c[0] in ('forward', 'lesion_table_matched', 'last_prob')], seen


def _expected(prob, y, exams_ids, thresholds, step=1, iou=0.3, **okw):
    """the three tables from one oracle call per exam and threshold"""
    results, cases, matches = [], [], []
    for thr in thresholds:
        mine = []
        for name, (lo, hi, ids) in exams_ids.items():
            flags = [b > 0 and ids[b] == ids[b - 1] + 1 for b in range(hi - lo)]
            r, t, _, l, tr, tt, tl, pr = MO.matched(prob[lo:hi], y[lo:hi], flags, thr, 1.0, 1, **okw)
            sl = lambda rows, tot: [(ids[b], rows[rows['slice'] == b], tot[b]) for b in range(hi - lo)]
            of = lambda a: [[tuple(v)[1:] for v in a[a['slice'] == b].tolist()] for b in range(hi - lo)]
            ts, ps = sl(tr, tt), sl(r, t)
            case, lines = CW.match_exam_lesions(name, ts, ps, CW.link_lesions(name, ts, of(tl)), CW.link_lesions(name, ps, of(l)), of(pr), iou=iou)
            mine.append(case)
            matches += [[step, repr(thr)] + v for v in lines]
        cases += [[step, repr(thr)] + c for c in mine]
        results.append([step, repr(thr)] + CW.exam_match_summary(mine))
    return {'exam_lesion_results.csv': CW.plain_csv(['step', 'threshold'] + CW.EXAM_RESULT_COLUMNS, results),
            'exam_lesion_cases.csv': CW.plain_csv(['step', 'threshold'] + CW.EXAM_CASE_COLUMNS, cases),
            'exam_lesion_matches.csv': CW.plain_csv(['step', 'threshold'] + CW.EXAM_MATCH_COLUMNS, matches)}


def test_eval_links_across_splits_and_batches_with_one_forward_per_split(tmp_path, monkeypatch):
    """one exam of 7 slices, data set batches of 4 on a device of 3 slices per call: splits of 3, 1, 3.  Two thresholds share
    every forward; with two thresholds the slice before a split is put back for each of them by a one-slice call on the host copy"""
    prob, y = _drawn()
    rows, texts, calls, seen = _eval(tmp_path, monkeypatch, prob, y, ['a'] * 7, range(7), 4, max_batch=3, exam_lesions=True,
                                     exam_threshold=[0.5, 0.7])
    T, F = True, False
    assert rows == OrderedDict([(1, OrderedDict(loss=0.25))]) and seen == []
    assert [c[:2] for c in calls if c[0] == 'forward'] == [('forward', 3), ('forward', 1), ('forward', 3)]
    m = lambda n, src, thr, flags: ('lesion_table_matched', n, src, thr, flags)
    assert calls == [('forward', 3), m(3, 'last', 0.5, [F, T, T]), m(3, 'last', 0.7, [F, T, T]), ('last_prob', 3),
                     ('forward', 1), m(1, 'host', 0.5, [F]), m(1, 'last', 0.5, [T]), m(1, 'host', 0.7, [F]), m(1, 'last', 0.7, [T]),
                     ('last_prob', 1),
                     ('forward', 3), m(1, 'host', 0.5, [F]), m(3, 'last', 0.5, [T, T, T]), m(1, 'host', 0.7, [F]),
                     m(3, 'last', 0.7, [T, T, T]), ('last_prob', 3)]
    want = _expected(prob, y, {'a': (0, 7, list(range(7)))}, [0.5, 0.7])
    assert sorted(texts) == ['exam_lesion_cases.csv', 'exam_lesion_matches.csv', 'exam_lesion_results.csv', 'results.csv']
    assert all(texts[k] == want[k] for k in want)
    res = list(csv.DictReader(io.StringIO(texts['exam_lesion_results.csv'])))
    # 0.5: the found tumour, the missed one, and the false block; 0.7: the false block is gone
    assert [(r['threshold'], r['true'], r['predicted'], r['detected'], r['missed'], r['matched'], r['false'], r['false_per_exam']) for r in res] == [
        ('0.5', '2', '2', '1', '1', '1', '1', '1.0'), ('0.7', '2', '1', '1', '1', '1', '0', '0.0')]
    lines = list(csv.DictReader(io.StringIO(texts['exam_lesion_matches.csv'])))
    true = [[l[k] for k in CW.EXAM_MATCH_COLUMNS[:7]] for l in lines if l['kind'] == 'true']
    assert true[:2] == true[2:] and [t[3:6] for t in true[:2]] == [['0', '4', '5'], ['5', '5', '1']]
    # one threshold: no host copy, no call in between
    _, one, calls, _ = _eval(tmp_path, monkeypatch, prob, y, ['a'] * 7, range(7), 4, max_batch=3, exam_lesions=True)
    assert [c[2:] for c in calls if c[0] == 'lesion_table_matched'] == [('last', 0.5, [F, T, T]), ('last', 0.5, [T]), ('last', 0.5, [T, T, T])]
    assert not [c for c in calls if c[0] == 'last_prob']
    assert all(one[k] == v for k, v in _expected(prob, y, {'a': (0, 7, list(range(7)))}, [0.5]).items())


def test_eval_flags_follow_exams_and_gaps(tmp_path, monkeypatch):
    """exam a slices 0 1 2 (3 is missing) 4, exam b slices 0 1, then another exam: the rule of annotate"""
    prob, y = _drawn()
    exams, ids = ['a', 'a', 'a', 'a', 'b', 'b', 'c'], [0, 1, 2, 4, 0, 1, 2]
    _, texts, calls, _ = _eval(tmp_path, monkeypatch, prob, y, exams, ids, 4, max_batch=3, exam_lesions=True, exam_iou=0.2,
                               exam_link_min_overlap=2)
    assert [c[4] for c in calls if c[0] == 'lesion_table_matched'] == [[False, True, True], [False], [False, True, False]]
    want = _expected(prob, y, {'a': (0, 4, [0, 1, 2, 4]), 'b': (4, 6, [0, 1]), 'c': (6, 7, [2])}, [0.5], iou=0.2)
    assert all(texts[k] == want[k] for k in want)
    assert [r['exam'] for r in csv.DictReader(io.StringIO(texts['exam_lesion_cases.csv']))] == ['a', 'b', 'c']


def test_other_ranks_write_nothing_and_the_visualizer_is_not_needed(tmp_path, monkeypatch):
    prob, y = _drawn()
    _, texts, calls, seen = _eval(tmp_path, monkeypatch, prob, y, ['a'] * 7, range(7), 4, rank=1, exam_lesions=True)
    assert texts == {} and calls == [] and seen == []
    # --skip_visualization --exam_lesions: no Visualizer data set, the pass runs
    _, texts, calls, seen = _eval(tmp_path, monkeypatch, prob, y, ['a'] * 7, range(7), 4, exam_lesions=True)
    assert seen == [] and 'exam_lesion_results.csv' in texts and 'casewise_results.csv' not in texts and calls
    # with the Visualizer: it runs as before, its files beside the new ones
    _, with_viz, _, seen = _eval(tmp_path, monkeypatch, prob, y, ['a'] * 7, range(7), 4, viz=True, exam_lesions=True)
    assert seen == ['visualize'] and 'casewise_results.csv' in with_viz
    assert all(with_viz[k] == texts[k] for k in texts)
    # without the flag: none of the new files, no call, the old files byte for byte
    _, plain, calls, _ = _eval(tmp_path, monkeypatch, prob, y, ['a'] * 7, range(7), 4, viz=True)
    assert calls == [] and sorted(plain) == ['casewise_results.csv', 'results.csv'] and all(plain[k] == with_viz[k] for k in plain)


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_exam_flags(capsys):
    from dnncancerannotator_amd.runs.evaluate import evaluate
    p = build_parser()
    base = ['evaluate', '--save_path', 's', '--data_path', 'd', '--tag', 't']
    a = vars(p.parse_args(base))
    assert not [k for k in a if k.startswith('exam_')]                       # the defaults are those of runs.evaluate.evaluate
    sig = inspect.signature(evaluate).parameters
    assert {k: sig[k].default for k in sig if k.startswith('exam_')} == dict(
        exam_lesions=False, exam_threshold=(0.5,), exam_iou=0.30, exam_min_area=0, exam_filter_size=5, exam_resize_factor=1.0,
        exam_max_lesions=256, exam_link_min_overlap=1)
    a = vars(p.parse_args(base + ['--exam_lesions', '--exam_threshold', '0.3', '0.5', '--exam_iou', '0.1', '--exam_min_area', '4',
                                  '--exam_filter_size', '3', '--exam_resize_factor', '0.5', '--exam_max_lesions', '32',
                                  '--exam_link_min_overlap', '2']))
    assert {k: v for k, v in a.items() if k.startswith('exam_')} == dict(
        exam_lesions=True, exam_threshold=[0.3, 0.5], exam_iou=0.1, exam_min_area=4, exam_filter_size=3, exam_resize_factor=0.5,
        exam_max_lesions=32, exam_link_min_overlap=2)
    for flag, bad in (('--exam_threshold', 'x'), ('--exam_iou', 'high'), ('--exam_max_lesions', '0'), ('--exam_link_min_overlap', '-1'),
                      ('--exam_filter_size', '2.5'), ('--exam_min_area', 'x')):
        with pytest.raises(SystemExit) as e:
            p.parse_args(base + ['--exam_lesions', flag, bad])
        assert e.value.code == 2 and flag[2:] in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--exam_lesion_size', '3'])                      # no such flag


def test_cli_flags_reach_engine_eval(monkeypatch, tmp_path):
    import yaml
    from dnncancerannotator_amd import __main__ as cli, engine
    seen = []
    monkeypatch.setattr(engine.TFKerasModel, 'eval', lambda self, dataset, **kw: seen.append(kw) or {})
    monkeypatch.setattr(engine.TFKerasModel, '__init__', lambda self, config: None)
    save = tmp_path / 'run'
    save.mkdir()
    (save / 'options.yaml').write_text(yaml.safe_dump({'config': {'data_options': {'eval': {'batch_size': 2}}}}))
    base = ['evaluate', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--tag', 't', '--skip_visualization']
    assert cli.main(base + ['--exam_lesions', '--exam_threshold', '0.3', '0.5']) == 0 and cli.main(base) == 0
    assert seen[0]['exam_lesions'] is True and seen[0]['exam_threshold'] == [0.3, 0.5] and seen[0]['viz_ds'] is None
    assert len(next(iter(seen[0]['exam_ds']))) == 4                           # (x, y, paths, sliceIDs): a data set of its own
    assert seen[1]['exam_lesions'] is False and seen[1]['exam_ds'] is None
