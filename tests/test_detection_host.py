"""CPU: the host side of `annotator evaluate --detection` and `annotator predict --detection_map`: the oracle of the detection map
(tests/detection_oracle.py) on hand-drawn planes, casewise.detection_match / detection_curves / detection_auroc on hand-computed
cases, engine.check_detection, the two passes on a fake device (tests/fake_detection_device.py: the numpy oracles in the place of
dnnca_detection_map and dnnca_lesion_table_matched), and the command line."""

import csv
import io
import os
from collections import OrderedDict

import numpy as np
import pytest

import detection_oracle as DO
import lesion_oracle as LO
import match_oracle as MO
from dnncancerannotator_amd import casewise as CW
from dnncancerannotator_amd.__main__ import build_parser
from fake_detection_device import LabelledSlices, fake_engine
from fake_link_device import Slices

F32 = np.float32


# ---- the oracle on hand-drawn planes ---------------------------------------------------------------------------------------------
def test_oracle_peak_with_shoulder_gives_two_touching_candidates():
    p = np.zeros((1, 8, 8), F32)
    p[0, 2:6, 2:6] = 0.3
    p[0, 3:5, 3:5] = 0.9
    D, rows, slices = DO.detection_map(p, min_area=1)
    assert slices.tolist() == [(2, 2, 0, 0)]
    assert rows.tolist() == [(0, 0, 3 * 8 + 3, 4, F32(0.9)), (0, 1, 2 * 8 + 2, 12, F32(0.3))]
    want = np.zeros((8, 8), F32)
    want[2:6, 2:6], want[3:5, 3:5] = 0.3, 0.9
    assert D[0].tobytes() == want.tobytes()


def test_oracle_lowest_index_wins_a_tie_and_small_regions_spend_a_round():
    p = np.zeros((1, 6, 10), F32)
    p[0, 4, 6:9] = 0.7
    p[0, 1, 1:3] = 0.7
    p[0, 0, 9] = 0.8                                                 # one pixel: below min_area 2
    D, rows, slices = DO.detection_map(p, min_area=2, max_candidates=2, rounds=3)
    assert slices.tolist() == [(2, 3, 1, 0)] and rows['seed'].tolist() == [11, 46] and rows['area'].tolist() == [2, 3]
    assert D[0, 0, 9] == 0 and (D[0, 1, 1:3] == F32(0.7)).all()
    _, rows, slices = DO.detection_map(p, min_area=2, max_candidates=2, rounds=2)
    assert slices.tolist() == [(1, 2, 1, 1)] and rows['seed'].tolist() == [11]      # the rounds are used up, a peak is left
    _, rows, slices = DO.detection_map(p, min_area=4, max_candidates=3, rounds=3)
    assert slices.tolist() == [(0, 3, 3, 0)] and not len(rows)                      # exactly used up, nothing left


def test_oracle_clamps_and_the_threshold_is_one_float32_product():
    p = np.array([[[np.nan, -1.0, 2.0, 1.0, 0.05]]], F32)
    D, rows, slices = DO.detection_map(p, min_area=1)
    assert D.tolist() == [[[0.0, 0.0, 1.0, 1.0, 0.0]]] and rows.tolist() == [(0, 0, 2, 2, F32(1))] and slices.tolist() == [(1, 1, 0, 0)]
    m, f = F32(0.7), F32(0.4)
    t = F32(m * f)
    below = np.nextafter(t, F32(0))
    p = np.array([[[m, t, below, t]]], F32)
    _, rows, _ = DO.detection_map(p, min_area=1, max_candidates=1)
    assert rows['area'].tolist() == [2]                              # t itself is in (>=), its lower neighbour is not
    assert DO.detection_map(np.full((2, 3, 3), 0.0999, F32))[2].tolist() == [(0, 0, 0, 0)] * 2


# ---- casewise.detection_match on hand-written tables -----------------------------------------------------------------------------
def rows_of(areas, confs=None):
    r = np.zeros(len(areas), LO.ROW_DTYPE)
    r['row'], r['area'] = np.arange(len(areas)), areas
    r['x1'], r['y1'] = 3, 3
    r['max_prob'] = 1.0 if confs is None else confs
    return r


def match(true_areas, true_links, pred_areas, pred_confs, pred_links, pairs, iou=0.1):
    n = len(true_areas)
    ts = [(10 + i, rows_of(true_areas[i]), len(true_areas[i])) for i in range(n)]
    ps = [(10 + i, rows_of(pred_areas[i], pred_confs[i]), len(pred_areas[i])) for i in range(n)]
    return CW.detection_match('/d/e', ts, ps, CW.link_lesions('/d/e', ts, true_links), CW.link_lesions('/d/e', ps, pred_links), pairs, iou=iou)


def test_match_a_candidate_that_only_reaches_a_taken_tumour_is_false():
    """T0 runs through three slices (volume 30), T1 (slice 12, 6 voxels) is never touched.  P0 (0.9, slices 10 and 11, 16 voxels, all
    common) takes T0; P1 (0.6, slice 12, 12 voxels, all common with T0) reaches only the taken T0: FP; P2 (0.5) touches nothing"""
    case, lines = match([[10], [10], [10, 6]], [[], [(0, 0, 10)], [(0, 0, 10)]],
                        [[8], [8, 5], [12]], [[0.9], [0.7, 0.5], [0.6]], [[], [(0, 0, 8)], []],
                        [[(0, 0, 8)], [(0, 0, 8)], [(0, 0, 12)]])
    assert case == dict(exam='/d/e', tumours=2, confidences=[float(F32(0.9)), float(F32(0.5)), float(F32(0.6))], hits=[1, 0, 0])
    assert lines == [['/d/e', 0, 10, 11, 16, '%.9g' % F32(0.9), 0, repr(16 / 30), 'tp'],
                     ['/d/e', 1, 11, 11, 5, '%.9g' % F32(0.5), -1, '0.0', 'fp'],
                     ['/d/e', 2, 12, 12, 12, '%.9g' % F32(0.6), 0, repr(12 / 30), 'fp']]
    assert CW.detection_case_values(case) == ['/d/e', 1, '%.9g' % F32(0.9), 3, 1, 2, 1]


def test_match_ties_go_to_the_lower_numbers_and_iou_is_inclusive():
    # two candidates of one confidence on one tumour: the lower number takes it
    case, lines = match([[20]], [[]], [[5, 5]], [[0.8, 0.8]], [[]], [[(0, 0, 5), (0, 1, 5)]])
    assert case['hits'] == [1, 0] and [l[6:] for l in lines] == [[0, repr(0.25), 'tp'], [0, repr(0.25), 'fp']]
    # the stronger one goes first whatever its number
    case, _ = match([[20]], [[]], [[5, 5]], [[0.7, 0.8]], [[]], [[(0, 0, 5), (0, 1, 5)]])
    assert case['hits'] == [0, 1]
    # one candidate on two tumours at one IoU: the lower tumour; the next candidate takes the other
    case, lines = match([[10, 10]], [[]], [[10, 4]], [[0.9, 0.5]], [[]], [[(0, 0, 4), (1, 0, 4), (0, 1, 4)]])
    assert case['hits'] == [1, 0] and lines[0][6:8] == [0, repr(4 / 16)] and lines[1][6:] == [0, repr(0.4), 'fp']
    case, lines = match([[10, 10]], [[]], [[10, 4]], [[0.9, 0.5]], [[]], [[(0, 0, 4), (1, 0, 4), (1, 1, 4)]])
    assert case['hits'] == [1, 1] and lines[1][6:] == [1, repr(0.4), 'tp']
    # overlap / union == iou exactly hits; just above it does not
    assert match([[30]], [[]], [[10]], [[0.9]], [[]], [[(0, 0, 10)]], iou=10 / 30)[0]['hits'] == [1]
    assert match([[30]], [[]], [[10]], [[0.9]], [[]], [[(0, 0, 10)]], iou=np.nextafter(10 / 30, 1))[0]['hits'] == [0]
    # an exam without candidates, one without anything
    assert match([[7]], [[]], [[]], [[]], [[]], [[]])[0] == dict(exam='/d/e', tumours=1, confidences=[], hits=[])
    assert CW.detection_case_values(match([[]], [[]], [[]], [[]], [[]], [[]])[0]) == ['/d/e', 0, '0', 0, 0, 0, 0]


def test_match_exam_lesions_is_what_it_was():
    """the overlap computation moved into exam_overlaps: the hand-computed case of test_match_host, unchanged"""
    ts = [(10 + i, rows_of(a), len(a)) for i, a in enumerate([[10], [10], [10]])]
    ps = [(10 + i, rows_of(a), len(a)) for i, a in enumerate([[8], [8, 5], [12]])]
    tl, pl = CW.link_lesions('/d/e', ts, [[], [(0, 0, 10)], [(0, 0, 10)]]), CW.link_lesions('/d/e', ps, [[], [(0, 0, 8)], []])
    case, lines = CW.match_exam_lesions('/d/e', ts, ps, tl, pl, [[(0, 0, 8)], [(0, 0, 8)], [(0, 0, 12)]])
    assert case == ['/d/e', 1, 3, 1, 0, 2, 1, 0] and lines[0][7:] == [0, 16, repr(16 / 30), repr(32 / 46), 1]
    with pytest.raises(ValueError, match='match_exam_lesions: 3 / 3 slices and 2 pair lists'):
        CW.match_exam_lesions('/d/e', ts, ps, tl, pl, [[], []])
    with pytest.raises(ValueError, match='detection_match: 3 / 3 slices and 2 pair lists'):
        CW.detection_match('/d/e', ts, ps, tl, pl, [[], []])


# ---- casewise.detection_curves / detection_auroc on hand-computed cases ----------------------------------------------------------
def case(tumours, confidences=(), hits=(), exam='e'):
    return dict(exam=exam, tumours=tumours, confidences=list(confidences), hits=list(hits))


CASES = [case(2, [0.9, 0.7, 0.7], [1, 1, 0]), case(0, [0.7, 0.3], [0, 0]), case(1), case(1, [0.3], [1])]


def test_curves_with_ties_in_confidence():
    """4 exams, 4 tumours.  Levels: 0.9 -> TP 1 FP 0; 0.7 (three candidates of two exams enter together) -> TP 2 FP 2; 0.3 -> TP 3
    FP 3.  AP = 1/4 * 1 + 1/4 * 1/2 + 1/4 * 1/2 = 1/2.  FP per exam 0, 1/2, 3/4: the sensitivity at 1/8 and 1/4 is that of the first
    level, at 1/2 that of the second, from 1 on that of the third; CPM = (1/4 + 1/4 + 1/2 + 4 * 3/4) / 7"""
    c = CW.detection_curves(CASES)
    assert c['levels'] == [(0.9, 1, 0, 0.25, 0.0, 1.0), (0.7, 2, 2, 0.5, 0.5, 0.5), (0.3, 3, 3, 0.75, 0.75, 0.5)]
    assert (c['exams'], c['tumours'], c['candidates'], c['tp'], c['fp'], c['fn']) == (4, 4, 6, 3, 3, 1)
    assert c['ap'] == 0.5 and c['sensitivities'] == [0.25, 0.25, 0.5, 0.75, 0.75, 0.75, 0.75] and c['cpm'] == 4.0 / 7
    # the order of the exams and of the candidates inside a level does not matter
    again = CW.detection_curves([dict(k, confidences=k['confidences'][::-1], hits=k['hits'][::-1]) for k in CASES[::-1]])
    assert again == c
    # no level within the budget: 0 -- one exam, its strongest candidate false
    c = CW.detection_curves([case(1, [0.9, 0.8], [0, 1])])
    assert c['sensitivities'] == [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0] and c['ap'] == 0.5


def test_auroc_counts_pairs_and_ties_exactly():
    """positive exams score 0.9, 0 (no candidate) and 0.3; the negative one 0.7: one pair of three is ordered"""
    assert CW.detection_auroc(CASES) == 1 / 3
    more = CASES + [case(0, [0.3], [0]), case(0)]                    # negatives 0.7, 0.3, 0: 3 + (1/2 + 1) + 1/2 of 9
    assert CW.detection_auroc(more) == 5 / 9
    assert CW.detection_auroc([case(1, [0.5], [1]), case(0, [0.5], [0])]) == 0.5


def test_summary_blank_cells_where_a_value_is_undefined():
    result, froc = CW.detection_summary(CASES, slices_exhausted=2)
    assert dict(zip(CW.DETECTION_RESULT_COLUMNS, result)) == dict(
        exams=4, positive_exams=3, tumours=4, candidates=6, tp=3, fp=3, fn=1, ap='0.5', auroc=repr(1 / 3), score=repr((0.5 + 1 / 3) / 2),
        **{'sensitivity_at_0.125': '0.25', 'sensitivity_at_0.25': '0.25', 'sensitivity_at_0.5': '0.5', 'sensitivity_at_1': '0.75',
           'sensitivity_at_2': '0.75', 'sensitivity_at_4': '0.75', 'sensitivity_at_8': '0.75'}, cpm=repr(4.0 / 7), slices_exhausted=2)
    assert froc == [['0.9', 1, 0, '0.25', '0.0', '1.0'], ['0.7', 2, 2, '0.5', '0.5', '0.5'], ['0.3', 3, 3, '0.75', '0.75', '0.5']]
    # no tumours at all: AP, the sensitivities, CPM, AUROC and the score are undefined
    result, froc = CW.detection_summary([case(0, [0.4], [0]), case(0)])
    assert result == [2, 0, 0, 1, 0, 1, 0] + [''] * 11 + [0] and froc == [['0.4', 0, 1, '', '0.5', '0.0']]
    # every exam positive: AP is defined, AUROC and the score are not
    result, _ = CW.detection_summary([case(1, [0.4], [1]), case(2)])
    assert result[:7] == [2, 2, 3, 1, 1, 0, 2] and result[7:10] == [repr(1 / 3), '', ''] and result[10] == repr(1 / 3)
    # tumours but no candidate: AP 0
    assert CW.detection_summary([case(1), case(0)])[0][7:10] == ['0.0', '0.5', '0.25']
    assert CW.detection_summary([])[0] == [0] * 7 + [''] * 11 + [0]


# ---- check_detection --------------------------------------------------------------------------------------------------------------
BAD = [dict(min_confidence=0.0009), dict(min_confidence=1.5), dict(min_confidence=float('nan')), dict(factor=0.009), dict(factor=1.01),
       dict(factor=float('nan')), dict(max_candidates=0), dict(max_candidates=65), dict(min_area=0), dict(min_area=(1 << 30) + 1),
       dict(rounds=257), dict(rounds=4), dict(max_candidates=17), dict(max_candidates=2.5), dict(iou=0.0), dict(iou=1.5),
       dict(iou=float('nan')), dict(link_min_overlap=0), dict(max_lesions=0)]


def test_check_detection_values():
    from dnncancerannotator_amd.engine import check_detection
    assert check_detection(False) is None
    assert check_detection(True) == dict(cfg=CW.DETECTION_DEFAULTS, iou=0.10, link_min_overlap=1, max_lesions=256)
    got = check_detection(True, 0.001, 1, 64, 1 << 30, 256, 1.0, 3, 7)
    assert got == dict(cfg=dict(min_confidence=0.001, factor=1.0, max_candidates=64, min_area=1 << 30, rounds=256), iou=1.0,
                       link_min_overlap=3, max_lesions=7)
    assert isinstance(got['cfg']['factor'], float) and isinstance(got['cfg']['rounds'], int)
    for bad in BAD:
        with pytest.raises(ValueError):
            check_detection(True, **bad)
    for key in ('min_confidence', 'factor', 'max_candidates', 'min_area', 'rounds', 'iou', 'link_min_overlap', 'max_lesions'):
        with pytest.raises(ValueError, match='add --detection'):
            check_detection(False, **{key: 1})


def test_refusals_come_before_anything_is_read(tmp_path):
    """a save_path that does not exist: a bad value must be the error, not the missing options.yaml"""
    from dnncancerannotator_amd.runs.evaluate import evaluate
    from dnncancerannotator_amd.runs.predict import predict
    nowhere = str(tmp_path / 'nowhere')
    for bad in BAD:
        with pytest.raises(ValueError, match='detection'):
            evaluate(nowhere, ['synthetic:16x16x2'], 't', detection=True, **{'detection_' + k: v for k, v in bad.items()})
        if 'iou' not in bad:
            with pytest.raises(ValueError, match='detection'):
                predict(nowhere, ['synthetic:16x16x2'], str(tmp_path / 'out'), detection_map=True,
                        **{'detection_' + k: v for k, v in bad.items()})
    with pytest.raises(ValueError, match='add --detection'):
        evaluate(nowhere, ['synthetic:16x16x2'], 't', detection_rounds=20)
    with pytest.raises(ValueError, match='add --detection_map'):
        predict(nowhere, ['synthetic:16x16x2'], str(tmp_path / 'out'), detection_factor=0.5)
    with pytest.raises(FileNotFoundError):
        evaluate(nowhere, ['synthetic:16x16x2'], 't', detection=True)
    assert not os.path.exists(nowhere)


# ---- the two passes on a fake device -----------------------------------------------------------------------------------------------
CFG = dict(min_confidence=0.1, factor=0.4, max_candidates=5, min_area=4, rounds=16)


def _drawn():
    """8 slices of 12 x 12.  Exam a (slices 0..3): a labelled tumour through all of them; the model sees it shifted by a pixel with a
    0.9 core inside a 0.5 body (one candidate: 0.5 >= 0.4 * 0.9) and draws a faint false block (0.3) in slices 1..2.  Exam b (slices
    0..1): no tumour, a false block at 0.6.  Exam c (slice 0): a tumour and nothing found.  Exam d (slice 0): a tumour under a 0.3"""
    prob, y = np.zeros((8, 12, 12), F32), np.zeros((8, 12, 12), F32)
    y[0:4, 2:6, 2:6] = 1.0
    prob[0:4, 3:7, 2:6] = 0.5
    prob[0:4, 4:6, 3:5] = 0.9
    prob[1:3, 9:11, 1:4] = 0.3
    prob[4:6, 6:9, 6:9] = 0.6
    y[6, 8:10, 8:10] = 1.0
    prob[6, 0, 0] = 0.95                                             # one pixel: dropped (min_area 4)
    y[7, 1:4, 1:4] = 1.0
    prob[7, 1:4, 2:5] = 0.3
    return prob, y


EXAMS, IDS = ['a', 'a', 'a', 'a', 'b', 'b', 'c', 'd'], [0, 1, 2, 3, 0, 1, 0, 0]
SPANS = {'a': (0, 4), 'b': (4, 6), 'c': (6, 7), 'd': (7, 8)}


def _eval(tmp_path, monkeypatch, prob, y, batch, max_batch=None, rank=0, **kw):
    from dnncancerannotator_amd import engine
    e = fake_engine(monkeypatch, max_batch)
    ds = LabelledSlices(prob, y, EXAMS, IDS, batch)
    monkeypatch.setattr(engine.TFKerasModel, '_evaluate', lambda self, dataset, staged=False: OrderedDict(loss=0.25))
    e._build(ds)
    e.current_step = 1
    run = str(tmp_path / ('run%d' % len(os.listdir(str(tmp_path)))))
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    e.ctx = e.ctx._replace(rank=rank)
    e.eval(ds, run, tag='t', export_csv=True, **kw)
    out = os.path.join(run, 'tfevents', 't')
    texts = {}
    for name in sorted(os.listdir(out)) if os.path.isdir(out) else []:
        with open(os.path.join(out, name), newline='') as f:
            texts[name] = f.read()
    return texts, [c for c in e.device_model.calls if c[0] in ('forward', 'detection_map', 'lesion_table_matched', 'last_prob')]


def _expected(prob, y, cfg, iou=0.1, step=1):
    """the four tables from the oracles: the map of every slice, one matched call per exam on it, casewise on top"""
    D, _, recs = DO.detection_map(prob, **cfg)
    cases, lines = [], []
    for name, (lo, hi) in SPANS.items():
        n = hi - lo
        r, t, _, l, tr, tt, tl, pr = MO.matched(D[lo:hi], y[lo:hi], [b > 0 for b in range(n)], cfg['min_confidence'], 1.0, 1, 0, 256)
        sl = lambda rows, tot: [(IDS[lo + b], rows[rows['slice'] == b], tot[b]) for b in range(n)]
        of = lambda a: [[tuple(v)[1:] for v in a[a['slice'] == b].tolist()] for b in range(n)]
        ts, ps = sl(tr, tt), sl(r, t)
        c, ls = CW.detection_match(name, ts, ps, CW.link_lesions(name, ts, of(tl)), CW.link_lesions(name, ps, of(l)), of(pr), iou=iou)
        cases.append(c)
        lines += [[step] + v for v in ls]
    result, froc = CW.detection_summary(cases, int(recs['exhausted'].sum()))
    return {'detection_results.csv': CW.plain_csv(['step'] + CW.DETECTION_RESULT_COLUMNS, [[step] + result]),
            'detection_froc.csv': CW.plain_csv(['step'] + CW.DETECTION_FROC_COLUMNS, [[step] + v for v in froc]),
            'detection_cases.csv': CW.plain_csv(['step'] + CW.DETECTION_CASE_COLUMNS, [[step] + CW.detection_case_values(c) for c in cases]),
            'detection_candidates.csv': CW.plain_csv(['step'] + CW.DETECTION_CANDIDATE_COLUMNS, lines)}


def test_eval_detection_pass_on_the_fake_device(tmp_path, monkeypatch):
    """data set batches of 4 on a device of 3 slices per call: splits of 3, 1, 3, 1; one forward, one in-place map and one matched
    call per split, in that order"""
    prob, y = _drawn()
    flags = dict(detection=True, detection_min_area=4)
    texts, calls = _eval(tmp_path, monkeypatch, prob, y, 4, max_batch=3, detection_ds=LabelledSlices(prob, y, EXAMS, IDS, 4), **flags)
    T, F = True, False
    want_calls = []
    for n, cont in ((3, [F, T, T]), (1, [T]), (3, [F, T, F]), (1, [F])):
        want_calls += [('forward', n), ('detection_map', n, CFG), ('lesion_table_matched', n, 'last', 0.1, cont)]
    assert calls == want_calls
    new = ['detection_candidates.csv', 'detection_cases.csv', 'detection_froc.csv', 'detection_results.csv']
    assert sorted(texts) == new + ['results.csv']
    want = _expected(prob, y, CFG)
    for k in want:
        assert texts[k] == want[k], k
    head = lambda k: texts[k].splitlines()[0].split(',')
    assert head('detection_results.csv') == ['step', 'exams', 'positive_exams', 'tumours', 'candidates', 'tp', 'fp', 'fn', 'ap', 'auroc',
                                             'score', 'sensitivity_at_0.125', 'sensitivity_at_0.25', 'sensitivity_at_0.5',
                                             'sensitivity_at_1', 'sensitivity_at_2', 'sensitivity_at_4', 'sensitivity_at_8', 'cpm',
                                             'slices_exhausted']
    assert head('detection_froc.csv') == ['step', 'confidence', 'tp', 'fp', 'sensitivity', 'fp_per_exam', 'precision']
    assert head('detection_cases.csv') == ['step', 'exam', 'positive', 'score', 'candidates', 'tp', 'fp', 'fn']
    assert head('detection_candidates.csv') == ['step', 'exam', 'candidate', 'first_slice', 'last_slice', 'volume_px', 'confidence',
                                                'tumour', 'iou', 'outcome']
    # by hand: a's tumour found at 0.9 (IoU 48 / 80), its false block at 0.3, b's false block at 0.6, c's pixel dropped, d found at 0.3
    res = next(csv.DictReader(io.StringIO(texts['detection_results.csv'])))
    assert [res[k] for k in ('exams', 'positive_exams', 'tumours', 'candidates', 'tp', 'fp', 'fn')] == ['4', '3', '3', '4', '2', '2', '1']
    # levels 0.9 (TP 1), 0.6 (FP 1), 0.3 (TP 2, FP 2): AP = 1/3 * 1 + 1/3 * 1/2; AUROC: 0.9 > 0.6, 0 < 0.6, 0.3 < 0.6
    assert float(res['ap']) == 1 / 3 + (2 / 3 - 1 / 3) * 0.5 and float(res['auroc']) == 1 / 3
    cands = list(csv.DictReader(io.StringIO(texts['detection_candidates.csv'])))
    assert [(c['exam'], c['first_slice'], c['last_slice'], c['volume_px'], c['tumour'], c['outcome']) for c in cands] == [
        ('a', '0', '3', '64', '0', 'tp'), ('a', '1', '2', '12', '-1', 'fp'), ('b', '0', '1', '18', '-1', 'fp'), ('d', '0', '0', '9', '0', 'tp')]
    assert float(cands[0]['iou']) == 48 / 80 and F32(cands[0]['confidence']) == F32(0.9)
    # other values of the flags reach the device call and the matching
    texts2, calls2 = _eval(tmp_path, monkeypatch, prob, y, 8, detection_ds=LabelledSlices(prob, y, EXAMS, IDS, 8), detection=True,
                           detection_min_area=1, detection_factor=1.0, detection_iou=0.7, detection_rounds=5, detection_max_candidates=2)
    cfg2 = dict(CFG, min_area=1, factor=1.0, rounds=5, max_candidates=2)
    assert [c[2] for c in calls2 if c[0] == 'detection_map'] == [cfg2]
    want2 = _expected(prob, y, cfg2, iou=0.7)
    assert all(texts2[k] == want2[k] for k in want2) and texts2['detection_results.csv'] != texts['detection_results.csv']
    # without the flag: none of the new files, no new call, the old files byte for byte; another rank writes nothing
    plain, calls = _eval(tmp_path, monkeypatch, prob, y, 4, max_batch=3)
    assert calls == [] and sorted(plain) == ['results.csv'] and plain['results.csv'] == texts['results.csv']
    other, calls = _eval(tmp_path, monkeypatch, prob, y, 4, rank=1, detection_ds=LabelledSlices(prob, y, EXAMS, IDS, 4), **flags)
    assert calls == [] and other == {}


def test_eval_detection_beside_exam_lesions_leaves_their_files_alone(tmp_path, monkeypatch):
    prob, y = _drawn()
    ds = LabelledSlices(prob, y, EXAMS, IDS, 4)
    exam = dict(exam_ds=ds, exam_lesions=True, exam_filter_size=1)
    both, _ = _eval(tmp_path, monkeypatch, prob, y, 4, max_batch=3, detection_ds=ds, detection=True, detection_min_area=4, **exam)
    alone, _ = _eval(tmp_path, monkeypatch, prob, y, 4, max_batch=3, **exam)
    assert len(both) == len(alone) + 4 and all(both[k] == v for k, v in alone.items())
    assert all(both[k] == v for k, v in _expected(prob, y, CFG).items())


def _predict(tmp_path, monkeypatch, prob, batch, max_batch=None, **kw):
    e = fake_engine(monkeypatch, max_batch)
    ds = Slices(prob, EXAMS, IDS, batch)
    e._build(ds)
    e.current_step = 1
    if not os.path.isdir(str(tmp_path / 'run')):
        e.save(str(tmp_path / 'run' / 'checkpoints' / 'ckpt-1'))
    out = str(tmp_path / ('out%d' % len(os.listdir(str(tmp_path)))))
    res = e.annotate(ds, str(tmp_path / 'run'), out, threshold=0.5, filter_size=1, **kw)
    files = {}
    for d, _, fs in os.walk(out):
        for fn in fs:
            with open(os.path.join(d, fn), 'rb') as f:
                files[os.path.relpath(os.path.join(d, fn), out)] = f.read()
    return res, files, [c for c in e.device_model.calls if c[0].startswith(('lesion', 'detection', 'forward', 'last_prob'))]


def test_predict_detection_map_on_the_fake_device(tmp_path, monkeypatch):
    prob, _ = _drawn()
    D, drows, drecs = DO.detection_map(prob, **CFG)
    table = LO.lesion_table(D, 0.1, 1.0, 1, 0, 256)
    flags = dict(detection_map=True, detection_min_area=4)
    plain_res, plain, _ = _predict(tmp_path, monkeypatch, prob, 4, max_batch=3)
    res, files, calls = _predict(tmp_path, monkeypatch, prob, 4, max_batch=3, **flags)
    # per split: the forward, the table of the lesions, then -- last -- the map and the table read from it
    assert [c[0] for c in calls] == ['forward', 'lesion_table', 'detection_map', 'lesion_table'] * 4
    assert [c[2] for c in calls if c[0] == 'detection_map'] == [CFG] * 4
    assert sorted(set(files) - set(plain)) == ['candidates.csv', 'slice_candidates.csv'] and all(files[k] == v for k, v in plain.items())
    assert res == dict(plain_res, candidates=len(table[0])) and len(table[0]) == 9
    want = [CW.candidate_values(EXAMS[r['slice']], IDS[r['slice']], r) for r in table[0]]
    assert files['candidates.csv'].decode() == CW.plain_csv(CW.LESION_COLUMNS + ['confidence'], want)
    lines = list(csv.DictReader(io.StringIO(files['candidates.csv'].decode())))
    assert [l['confidence'] for l in lines] == [l['max_prob'] for l in lines] and lines[0]['confidence'] == '%.9g' % F32(0.9)
    assert files['slice_candidates.csv'].decode() == CW.plain_csv(
        ['exam', 'slice', 'candidates', 'rounds', 'dropped', 'exhausted'], [[EXAMS[i], IDS[i]] + list(drecs[i].tolist()) for i in range(8)])
    assert drecs[6].tolist() == (0, 1, 1, 0)
    # --link_slices: the candidates' chain is the matched call's, the lesions' chain stays the linked call's
    linked_res, linked, _ = _predict(tmp_path, monkeypatch, prob, 4, max_batch=3, link_slices=True)
    res, files, calls = _predict(tmp_path, monkeypatch, prob, 4, max_batch=3, link_slices=True, **flags)
    assert [c[0] for c in calls] == ['forward', 'lesion_table_linked', 'detection_map', 'lesion_table_matched'] * 4
    assert [c[4] for c in calls if c[0] == 'lesion_table_matched'] == [c[3] for c in calls if c[0] == 'lesion_table_linked']
    assert sorted(set(files) - set(linked)) == ['candidates.csv', 'exam_candidates.csv', 'slice_candidates.csv']
    assert all(files[k] == v for k, v in linked.items())
    exam_lines = list(csv.DictReader(io.StringIO(files['exam_candidates.csv'].decode())))
    assert list(exam_lines[0]) == CW.EXAM_LESION_COLUMNS + ['confidence']
    assert [(l['exam'], l['first_slice'], l['last_slice'], l['volume_px'], l['confidence']) for l in exam_lines] == [
        ('a', '0', '3', '64', '%.9g' % F32(0.9)), ('a', '1', '2', '12', '%.9g' % F32(0.3)), ('b', '0', '1', '18', '%.9g' % F32(0.6)),
        ('d', '0', '0', '9', '%.9g' % F32(0.3))]
    # --export_images: one detection.png per slice, rint(D * 255); only then is the map fetched
    res, files, calls = _predict(tmp_path, monkeypatch, prob, 8, export_images=True, **flags)
    assert [c[0] for c in calls] == ['forward', 'lesion_table', 'detection_map', 'lesion_table', 'last_prob']
    pngs = sorted(k for k in files if k.endswith('detection.png'))
    assert len(pngs) == 8 and len([k for k in files if k.endswith('mask.png')]) == 8
    by_tag = {CW.detection_path('', CW.tag_of(EXAMS[i], IDS[i])).lstrip(os.sep): i for i in range(8)}
    for k in pngs:
        assert files[k] == CW.encode_png(np.rint(D[by_tag[k]].astype(np.float64) * 255).astype(np.uint8))
    # 0.5 * 255 = 127.5 rounds to even; the float32 below 0.9 gives 229.4999939
    assert CW.detection_image(np.array([[0.0, 0.5, 1.0, F32(0.9)]])).tolist() == [[0, 128, 255, 229]]


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_detection_flags(capsys):
    p = build_parser()
    base = ['evaluate', '--save_path', 's', '--data_path', 'd', '--tag', 't']
    assert not [k for k in vars(p.parse_args(base)) if k.startswith('detection')]
    a = vars(p.parse_args(base + ['--detection', '--detection_min_confidence', '0.2', '--detection_factor', '0.5',
                                  '--detection_max_candidates', '3', '--detection_min_area', '4', '--detection_rounds', '8',
                                  '--detection_iou', '0.25', '--detection_link_min_overlap', '2', '--detection_max_lesions', '32']))
    assert {k: v for k, v in a.items() if k.startswith('detection')} == dict(
        detection=True, detection_min_confidence=0.2, detection_factor=0.5, detection_max_candidates=3, detection_min_area=4,
        detection_rounds=8, detection_iou=0.25, detection_link_min_overlap=2, detection_max_lesions=32)
    base = ['predict', '--save_path', 's', '--data_path', 'd', '--output', 'o']
    assert not [k for k in vars(p.parse_args(base)) if k.startswith('detection')]
    a = vars(p.parse_args(base + ['--detection_map', '--detection_factor', '0.5', '--detection_rounds', '8']))
    assert {k: v for k, v in a.items() if k.startswith('detection')} == dict(detection_map=True, detection_factor=0.5, detection_rounds=8)
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--detection_map', '--detection_iou', '0.2'])      # evaluate's alone
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--detection_map', '--detection_rounds', 'many'])
    capsys.readouterr()


def test_cli_flags_reach_engine_eval_and_annotate(monkeypatch, tmp_path):
    import yaml
    from dnncancerannotator_amd import __main__ as cli, engine
    seen = []
    monkeypatch.setattr(engine.TFKerasModel, 'eval', lambda self, dataset, **kw: seen.append(kw) or {})
    monkeypatch.setattr(engine.TFKerasModel, 'annotate', lambda self, dataset, **kw: seen.append(kw) or {})
    monkeypatch.setattr(engine.TFKerasModel, '__init__', lambda self, config: None)
    save = tmp_path / 'run'
    save.mkdir()
    (save / 'options.yaml').write_text(yaml.safe_dump({'config': {'data_options': {'eval': {'batch_size': 2}}}}))
    base = ['evaluate', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--tag', 't', '--skip_visualization']
    assert cli.main(base + ['--detection', '--detection_rounds', '9']) == 0 and cli.main(base) == 0
    assert seen[0]['detection'] is True and seen[0]['detection_rounds'] == 9 and seen[0]['detection_factor'] is None
    assert len(next(iter(seen[0]['detection_ds']))) == 4              # (x, y, paths, sliceIDs): the shared data set with meta
    assert not [k for k in seen[1] if k.startswith('detection')]     # the keywords reach model.eval only with the flag
    with pytest.raises(ValueError, match='add --detection'):
        cli.main(base + ['--detection_rounds', '9'])
    base = ['predict', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--output', str(tmp_path / 'o')]
    assert cli.main(base + ['--detection_map', '--detection_min_area', '3']) == 0 and cli.main(base) == 0
    assert seen[2]['detection_map'] is True and seen[2]['detection_min_area'] == 3
    assert not [k for k in seen[3] if k.startswith('detection')]
    with pytest.raises(ValueError, match='add --detection_map'):
        cli.main(base + ['--detection_min_area', '3'])
