"""CPU: the mask refinement (`--refine_hysteresis`, `--refine_closing`, `--refine_fill_holes`) without a device.  The numpy oracle
(tests/refine_oracle.py) against its own second statements and its stated properties, engine.check_refine and the command line's
refusals before anything is read, and the engine on a fake device that records when the setting is made (tests/fake_refine_device.py)."""

import os
from collections import OrderedDict

import numpy as np
import pytest

import lesion_oracle as LO
import refine_oracle as RO
from dnncancerannotator_amd.__main__ import build_parser
from dnncancerannotator_amd.engine import check_refine
from fake_link_device import Slices
from fake_refine_device import LabelledSlices, fake_engine

F32 = np.float32


def small_planes(n=300, seed=0):
    """n random boolean planes of 2 .. 12 pixels a side at densities from sparse to almost full"""
    rs = np.random.RandomState(seed)
    for _ in range(n):
        h, w = rs.randint(2, 13, 2)
        yield rs.rand(h, w) < rs.choice([0.2, 0.45, 0.6, 0.8, 0.95])


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def test_fill_holes_and_hysteresis_agree_with_the_flood_fill():
    rs = np.random.RandomState(1)
    filled = seeded = 0
    for m in small_planes():
        got = RO.fill_holes(m)
        assert np.array_equal(got, RO.fill_holes_flood(m))
        filled += int(got.sum() - m.sum())
        high = m & (rs.rand(*m.shape) < 0.15)
        kept = RO.hysteresis(m, high)
        assert np.array_equal(kept, RO.hysteresis_flood(m, high))
        assert not (kept & ~m).any() and not (high & ~kept).any()
        seeded += int(kept.sum())
    assert filled > 100 and seeded > 1000
    # a stack of planes is its planes one by one: nothing crosses from a slice into the next
    stack = np.stack([np.pad(m, ((0, 12 - m.shape[0]), (0, 12 - m.shape[1])), constant_values=True) for m in small_planes(8, seed=2)])
    assert np.array_equal(RO.fill_holes(stack), np.stack([RO.fill_holes(p) for p in stack]))
    assert np.array_equal(RO.fill_holes(stack), RO.fill_holes_flood(stack))


def test_close_contains_its_input_and_is_idempotent():
    for i, m in enumerate(small_planes(200, seed=3)):
        size = (3, 5, 7, 15)[i % 4]
        c = RO.close(m, size)
        assert not (m & ~c).any()
        assert np.array_equal(RO.close(c, size), c)
    assert RO.close(m, 0) is not None and np.array_equal(RO.close(m, 1), m) and np.array_equal(RO.close(m, 0), m)
    for bad in (2, 4, 14, 16, 17, -1):
        with pytest.raises(ValueError):
            RO.close(m, bad)
    # two bars: a gap of size - 1 closes, a gap of size stays
    for size in (3, 5, 15):
        for gap, parts in ((size - 1, 1), (size, 2)):
            m = np.zeros((20, 60), bool)
            m[8:12, 10:14] = m[8:12, 14 + gap:18 + gap] = True
            roots = LO.O.ccl(RO.close(m, size))
            assert len(np.unique(roots[roots >= 0])) == parts, (size, gap)


def test_fill_holes_is_idempotent_and_leaves_the_border_components():
    for m in small_planes(200, seed=4):
        f = RO.fill_holes(m)
        assert np.array_equal(RO.fill_holes(f), f) and not (m & ~f).any()
        border = np.zeros(m.shape, bool)
        border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
        bg = LO.O.ccl(~m)
        touching = np.isin(bg, np.unique(bg[border & ~m]))
        assert not (f & touching).any()                  # no component of the background that touches the border was filled
        assert (f | touching).all()                      # and everything else is foreground now
    ring = np.ones((5, 5), bool)
    ring[2, 2] = False
    assert RO.fill_holes(ring).all()
    ring[2, 3] = ring[2, 4] = False                      # a channel to the border
    assert np.array_equal(RO.fill_holes(ring), ring)
    diag = np.zeros((5, 5), bool)
    diag[1, 2] = diag[3, 2] = diag[2, 1] = diag[2, 3] = True      # closed only diagonally: the background inside is its own component
    assert RO.fill_holes(diag)[2, 2] and RO.fill_holes(diag).sum() == 5


def test_everything_off_is_the_lesion_oracle():
    rs = np.random.RandomState(5)
    prob = rs.rand(3, 21, 17).astype(F32)
    for kw in (dict(threshold=0.5, rf=1.0, k=3), dict(threshold=0.7, rf=0.5, k=1, min_area=2, max_lesions=3)):
        want = LO.lesion_table(prob, **kw)
        for refine in (None, {}, dict(closing=1), dict(hysteresis=None, closing=0, fill_holes=False)):
            got = RO.lesion_table(prob, refine=refine, **kw)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist() and np.array_equal(got[2], want[2])
    # the stated order: hysteresis, opening, closing, filling
    p = np.full((1, 20, 30), 0.1, F32)
    p[0, 5:13, 3:11] = p[0, 5:13, 18:26] = p[0, 8, 11:18] = 0.4
    p[0, 9, 22] = 0.8
    _, fg = RO.refined_mask(p, 0.5, 1.0, 3, dict(hysteresis=0.3))
    assert fg.sum() == 128                               # both blocks: the one without a high pixel was joined when it counted
    with pytest.raises(ValueError):
        RO.refined_mask(p, 0.5, 1.0, 3, dict(hysteresis=0.5))


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def test_check_refine_values():
    assert check_refine() is None and check_refine(None, None, False, [0.5]) is None
    assert check_refine(closing=0) is None and check_refine(closing=1, thresholds=[0.5]) is None
    assert check_refine(0.3, 5, True, [0.5]) == dict(hysteresis=0.3, closing=5, fill_holes=True)
    assert check_refine(fill_holes=True) == dict(hysteresis=None, closing=0, fill_holes=True)
    assert check_refine(closing=15) == dict(hysteresis=None, closing=15, fill_holes=False)
    just = float(np.nextafter(F32(0.5), F32(0)))
    assert check_refine(just, thresholds=[0.5])['hysteresis'] == just
    for low in (0.0, 1.0, -0.2, 1.5, float('nan')):
        with pytest.raises(ValueError, match='--refine_hysteresis'):
            check_refine(low, thresholds=[0.5])
    for low, thresholds in ((0.5, [0.5]), (0.6, [0.5]), (0.3, [0.5, 0.3, 0.7]), (0.25, [0.7, 0.2]), (0.5 + 1e-12, [0.5])):
        with pytest.raises(ValueError, match='--refine_hysteresis .* below every threshold'):
            check_refine(low, thresholds=thresholds)
    for k in (2, 4, 14, 16, 17, -1, -3, 2.5, True):
        with pytest.raises(ValueError, match='--refine_closing'):
            check_refine(closing=k, thresholds=[0.5])
    for flags in (dict(hysteresis=0.3), dict(closing=3), dict(fill_holes=True), dict(closing=1)):
        with pytest.raises(ValueError, match='add one of them'):
            check_refine(thresholds=[0.5], consumers=False, **flags)
    assert check_refine(consumers=False) is None


def test_refusals_come_before_anything_is_read(tmp_path):
    """a save_path that does not exist: a bad value must be the error, not the missing options.yaml"""
    from dnncancerannotator_amd.runs.evaluate import evaluate
    from dnncancerannotator_amd.runs.predict import predict
    nowhere, data = str(tmp_path / 'nowhere'), ['synthetic:16x16x2']
    bad = [dict(refine_hysteresis=0.5), dict(refine_hysteresis=0.0), dict(refine_hysteresis=1.0), dict(refine_closing=4),
           dict(refine_closing=17), dict(refine_closing=-1)]
    for kw in bad:
        with pytest.raises(ValueError, match='--refine_'):
            predict(nowhere, data, str(tmp_path / 'out'), **kw)
        with pytest.raises(ValueError, match='--refine_'):
            evaluate(nowhere, data, 't', exam_lesions=True, **kw)
        with pytest.raises(ValueError, match='--refine_'):
            evaluate(nowhere, data, 't', surface_distances=True, **kw)
    with pytest.raises(ValueError, match='below every threshold'):
        predict(nowhere, data, str(tmp_path / 'out'), threshold=0.3, refine_hysteresis=0.4)
    with pytest.raises(ValueError, match='below every threshold'):       # the smallest of several
        evaluate(nowhere, data, 't', exam_lesions=True, exam_threshold=(0.5, 0.2, 0.7), refine_hysteresis=0.25)
    with pytest.raises(ValueError, match='below every threshold'):       # either pass's
        evaluate(nowhere, data, 't', exam_lesions=True, exam_threshold=(0.5,), surface_distances=True, surface_threshold=(0.2,),
                 refine_hysteresis=0.25)
    for kw in (dict(refine_hysteresis=0.3), dict(refine_closing=3), dict(refine_fill_holes=True)):
        with pytest.raises(ValueError, match='add one of them'):
            evaluate(nowhere, data, 't', **kw)
        with pytest.raises(ValueError, match='add one of them'):
            evaluate(nowhere, data, 't', detection=True, **kw)
    with pytest.raises(FileNotFoundError):               # a threshold of a pass that does not run is not looked at
        evaluate(nowhere, data, 't', exam_lesions=True, surface_threshold=(0.1,), refine_hysteresis=0.25)
    with pytest.raises(FileNotFoundError):
        predict(nowhere, data, str(tmp_path / 'out'), refine_hysteresis=0.25, refine_closing=5, refine_fill_holes=True)
    assert not os.path.exists(nowhere)


def test_parser_refine_flags(capsys):
    p = build_parser()
    for base in (['evaluate', '--save_path', 's', '--data_path', 'd', '--tag', 't'],
                 ['predict', '--save_path', 's', '--data_path', 'd', '--output', 'o']):
        assert not [k for k in vars(p.parse_args(base)) if k.startswith('refine')]
        a = vars(p.parse_args(base + ['--refine_hysteresis', '0.3', '--refine_closing', '5', '--refine_fill_holes']))
        assert {k: v for k, v in a.items() if k.startswith('refine')} == dict(refine_hysteresis=0.3, refine_closing=5,
                                                                               refine_fill_holes=True)
        with pytest.raises(SystemExit):
            p.parse_args(base + ['--refine_closing', 'wide'])
    with pytest.raises(SystemExit):
        p.parse_args(['train', '--config', 'c', '--save_path', 's', '--data_path', 'd', '--max_steps', '1', '--refine_fill_holes'])
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
    refine = lambda kw: {k: v for k, v in kw.items() if k.startswith('refine')}
    base = ['evaluate', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--tag', 't', '--skip_visualization']
    assert cli.main(base + ['--exam_lesions', '--refine_hysteresis', '0.3', '--refine_fill_holes']) == 0
    assert cli.main(base + ['--exam_lesions']) == 0 and cli.main(base + ['--surface_distances', '--refine_closing', '1']) == 0
    assert refine(seen[0]) == dict(refine_hysteresis=0.3, refine_closing=None, refine_fill_holes=True)
    assert not refine(seen[1]) and not refine(seen[2])   # the keywords travel only when they ask for something
    with pytest.raises(ValueError, match='add one of them'):
        cli.main(base + ['--refine_fill_holes'])
    with pytest.raises(ValueError, match='below every threshold'):
        cli.main(base + ['--surface_distances', '--surface_threshold', '0.6', '0.3', '--refine_hysteresis', '0.3'])
    base = ['predict', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--output', str(tmp_path / 'o')]
    assert cli.main(base + ['--refine_closing', '7']) == 0 and cli.main(base) == 0
    assert refine(seen[3]) == dict(refine_hysteresis=None, refine_closing=7, refine_fill_holes=False) and not refine(seen[4])
    with pytest.raises(ValueError, match='--refine_closing'):
        cli.main(base + ['--refine_closing', '6'])
    with pytest.raises(ValueError, match='below every threshold'):
        cli.main(base + ['--threshold', '0.4', '--refine_hysteresis', '0.4'])
    assert len(seen) == 5


# ---- the engine on a fake device ---------------------------------------------------------------------------------------------------
EXAMS, IDS = ['a', 'a', 'a', 'a', 'b', 'b', 'c', 'd'], [0, 1, 2, 3, 0, 1, 0, 0]
REFINE = dict(refine_hysteresis=0.25, refine_closing=3, refine_fill_holes=True)
SET = ('set_lesion_refine', 0.25, 3, True)
CLEAR = ('set_lesion_refine', None, 0, False)


def _drawn():
    """8 slices of 14 x 14.  Exam a: a labelled tumour through four slices that the model sees as a ring (0.8) round a core below
    the threshold (0.1) with a halo at 0.3; exam b: a false block in two parts one pixel apart; c: nothing found; d: a faint 0.3"""
    prob, y = np.zeros((8, 14, 14), F32), np.zeros((8, 14, 14), F32)
    y[0:4, 3:10, 3:10] = 1.0
    prob[0:4, 2:11, 2:11] = 0.3
    prob[0:4, 3:10, 3:10] = 0.8
    prob[0:4, 5:8, 5:8] = 0.1
    prob[4:6, 4:8, 2:5] = prob[4:6, 4:8, 6:9] = 0.7
    y[6, 8:10, 8:10] = 1.0
    y[7, 1:4, 1:4] = 1.0
    prob[7, 1:4, 2:5] = 0.3
    return prob, y


def _eval(tmp_path, monkeypatch, prob, y, batch, max_batch=None, **kw):
    from dnncancerannotator_amd import engine
    e = fake_engine(monkeypatch, max_batch)
    ds = LabelledSlices(prob, y, EXAMS, IDS, batch)
    monkeypatch.setattr(engine.TFKerasModel, '_evaluate', lambda self, dataset, staged=False: OrderedDict(loss=0.25))
    e._build(ds)
    e.current_step = 1
    run = str(tmp_path / ('run%d' % len(os.listdir(str(tmp_path)))))
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    e.eval(ds, run, tag='t', export_csv=True, **{k: (ds if v == 'ds' else v) for k, v in kw.items()})
    out = os.path.join(run, 'tfevents', 't')
    texts = {}
    for name in sorted(os.listdir(out)):
        with open(os.path.join(out, name), newline='') as f:
            texts[name] = f.read()
    kinds = ('set_lesion_refine', 'detection_map', 'lesion_table_matched', 'surface_distances')
    return texts, [c for c in e.device_model.calls if c[0] in kinds]


def test_eval_sets_the_refinement_once_and_clears_it_around_detection(tmp_path, monkeypatch):
    prob, y = _drawn()
    passes = dict(exam_ds='ds', exam_lesions=True, exam_filter_size=1, surface_ds='ds', surface_distances=True, surface_filter_size=1,
                  detection_ds='ds', detection=True, detection_min_area=4)
    texts, calls = _eval(tmp_path, monkeypatch, prob, y, 4, max_batch=3, **passes, **REFINE)
    plain, plain_calls = _eval(tmp_path, monkeypatch, prob, y, 4, max_batch=3, **passes)
    # once, before the first table call; around every table call on a detection map: off, the call, back on
    assert calls[0] == SET and [c for c in calls[1:9] if c[0] == 'set_lesion_refine'] == []
    assert not [c for c in plain_calls if c[0] == 'set_lesion_refine']
    assert [c for c in calls if c[0] != 'set_lesion_refine'] == plain_calls
    first = [c[0] for c in calls].index('detection_map')         # the detection pass runs last
    assert [c for c in calls[:first] if c[0] == 'set_lesion_refine'] == [SET]
    assert [c[0] for c in calls[first:]] == ['detection_map', 'set_lesion_refine', 'lesion_table_matched', 'set_lesion_refine'] * 4
    assert [c for c in calls[first:] if c[0] == 'set_lesion_refine'] == [CLEAR, SET] * 4
    # the detection files are byte for byte what they are without the flags; the refined passes moved: the ring was filled
    assert sorted(texts) == sorted(plain)
    for name in texts:
        assert (texts[name] == plain[name]) == name.startswith(('detection', 'results')), name
    import csv
    import io
    rows = lambda t, name: list(csv.DictReader(io.StringIO(t[name])))
    assert list(rows(texts, 'surface_results.csv')[0]) == list(rows(plain, 'surface_results.csv')[0])
    dice = lambda t: float(rows(t, 'surface_results.csv')[0]['dice'])
    assert dice(texts) != dice(plain)
    # no pass that reads the refined mask: the refusal, before the data set is looked at
    with pytest.raises(ValueError, match='add one of them'):
        fake_engine(monkeypatch).eval(None, str(tmp_path / 'nowhere'), tag='t', detection=True, **REFINE)
    with pytest.raises(ValueError, match='below every threshold'):
        fake_engine(monkeypatch).eval(None, str(tmp_path / 'nowhere'), tag='t', exam_lesions=True, exam_threshold=(0.5, 0.25), **REFINE)


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
    return res, files, [c for c in e.device_model.calls if c[0].startswith(('lesion', 'detection', 'set_lesion'))]


def test_annotate_sets_the_refinement_once_and_clears_it_around_the_candidates(tmp_path, monkeypatch):
    prob, _ = _drawn()
    plain_res, plain, plain_calls = _predict(tmp_path, monkeypatch, prob, 4, max_batch=3, export_images=True)
    assert not [c for c in plain_calls if c[0] == 'set_lesion_refine']
    res, files, calls = _predict(tmp_path, monkeypatch, prob, 4, max_batch=3, export_images=True, **REFINE)
    assert calls[0] == SET and calls.count(SET) == 1 and CLEAR not in calls and calls[1:] == plain_calls
    want = RO.lesion_table(prob, 0.5, 1.0, 1, refine=dict(hysteresis=0.25, closing=3, fill_holes=True))
    assert res['lesions'] == len(want[0]) == 6 and plain_res['lesions'] == 8      # b's two parts are one lesion now
    assert sorted(files) == sorted(plain) and files['lesions.csv'] != plain['lesions.csv']
    assert files['lesions.csv'].splitlines()[0] == plain['lesions.csv'].splitlines()[0]      # no column gained or lost
    from test_casewise_host import decode_png
    from dnncancerannotator_amd import casewise as CW
    for i in range(8):
        with_png = files[CW.mask_path('', CW.tag_of(EXAMS[i], IDS[i])).lstrip(os.sep)]
        assert np.array_equal(decode_png(with_png)[..., 0], want[2][i])
    assert int((want[2][0] > 0).sum()) == 81             # the ring, its halo and its core
    # --link_slices --detection_map: per split the linked call refined, the candidates' calls unrefined, and the lesions' chain holds
    flags = dict(link_slices=True, detection_map=True, detection_min_area=4)
    base_res, base, _ = _predict(tmp_path, monkeypatch, prob, 4, max_batch=3, **flags)
    res, files, calls = _predict(tmp_path, monkeypatch, prob, 4, max_batch=3, **flags, **REFINE)
    names = [c[0] for c in calls]
    assert names == ['set_lesion_refine'] + ['lesion_table_linked', 'set_lesion_refine', 'detection_map', 'lesion_table_matched',
                                             'set_lesion_refine'] * 4
    assert [c for c in calls if c[0] == 'set_lesion_refine'] == [SET] + [CLEAR, SET] * 4
    for name in ('candidates.csv', 'slice_candidates.csv', 'exam_candidates.csv'):
        assert files[name] == base[name], name           # the candidates are what they are without the flags
    assert files['exam_lesions.csv'] != base['exam_lesions.csv'] and res['exam_lesions'] == 2 and base_res['exam_lesions'] == 3
