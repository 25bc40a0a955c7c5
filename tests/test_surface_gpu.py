"""-m gpu: dnnca_surface_distances through the C ABI: the prediction mask of the lesion table and the label foreground of the matched
call, their boundary pixels (surface_edges), the vertical distances to them (surface_cols) and per boundary pixel the exact squared
distance to the other side's boundary (surface_sample).  Everything is an integer: counts, samples and edges must EQUAL the brute-force
numpy oracle (tests/surface_oracle.py) on the drawn cases of tests/match_cases.py and tests/lesion_cases.py and on hand-written
planes whose expected values stand in the tests.  The host buffers carry guard regions behind them, pre-filled with a sentinel:
nothing may be written past the counted entries."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lesion_cases as LC
import link_oracle as KO
import match_cases as MC
import surface_oracle as SO
from test_lesion_gpu import ROOT, SENTINEL, UNET, call as plain_call
from test_link_gpu import LESION_PLAN, _model, call as linked_call, same_links
from test_match_gpu import call as matched_call, same_all

pytestmark = pytest.mark.gpu

GUARD = 8
SURFACE_PLAN = ['surface_edges', 'surface_cols', 'surface_sample']
REUSED_PLAN = LESION_PLAN[:6] + ['region_prep']      # prep, open, ccl x 3, sizes of the prediction; prep of the label


@pytest.fixture(scope='module')
def dm(gpu):
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    yield m
    m.close()


def call(dm, prob, y, threshold=0.5, rf=1.0, k=5, min_area=0, max_samples=65536, edges=True, batch=None, short=None, null=None):
    """dnnca_surface_distances on host probabilities and labels [B, h, w] with guarded buffers -> (counts, samples, edges).
    short: 'samples' or 'edges': that capacity is one too small; null: 'y', 'samples' or 'n_samples'"""
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import check, fptr
    prob, y = np.ascontiguousarray(prob, np.float32), np.ascontiguousarray(y, np.float32)
    B, h, w = prob.shape
    B = B if batch is None else batch
    oh, ow = SO.LO.O.out_size(h, w, rf)
    cap, nedge = B * 2 * min(max(max_samples, 0), oh * ow), B * oh * ow
    counts = np.full((B + 1) * 5, -7, np.int32)
    samples = np.full(max(cap, 0) + GUARD, SENTINEL, np.uint8).repeat(SO.SAMPLE_DTYPE.itemsize).view(SO.SAMPLE_DTYPE)
    planes = np.full(max(nedge, 0) + 64, SENTINEL, np.uint8)
    n, hw = C.c_int64(-1), (C.c_int32 * 2)()
    check(dm.lib.dnnca_surface_distances(
        dm.handle, fptr(prob), None if null == 'y' else fptr(y), B, h, w, threshold, rf, k, min_area, max_samples,
        counts.ctypes.data_as(C.POINTER(C.c_int32)), None if null == 'samples' else samples.ctypes.data_as(C.POINTER(_lib.SurfaceSample)),
        cap - (short == 'samples'), None if null == 'n_samples' else C.byref(n), planes.ctypes.data_as(C.c_void_p) if edges else None,
        (nedge - (short == 'edges')) if edges else 0, hw))
    assert (hw[0], hw[1]) == (oh, ow) and 0 <= n.value <= cap
    assert (samples[n.value:].view(np.uint8) == SENTINEL).all(), 'samples written past the list'
    assert (counts[B * 5:] == -7).all()
    assert (planes[nedge:] == SENTINEL).all() and (edges or (planes == SENTINEL).all())
    return counts[:B * 5].reshape(B, 5).copy(), samples[:n.value].copy(), (planes[:nedge].reshape(B, oh, ow).copy() if edges else None)


def same(got, want):
    assert got[0].tolist() == want[0].tolist(), (got[0], want[0])
    assert got[1].dtype == SO.SAMPLE_DTYPE and got[1].tolist() == want[1].tolist()
    if got[2] is not None:
        assert np.array_equal(got[2], want[2])


def check_drawn(dm, prob, y, spec, **kw):
    """the call against the oracle; the prediction's area against the mask dnnca_lesion_table writes for the same arguments"""
    s = (spec['threshold'], spec['rf'], spec['k'])
    got = call(dm, prob, y, *s, **kw)
    same(got, SO.surface(prob, y, *s, **{k: v for k, v in kw.items() if k in ('min_area', 'max_samples')}))
    mask = plain_call(dm, prob, *s, min_area=kw.get('min_area', 0), max_lesions=1)[2]
    assert got[0][:, 0].tolist() == (mask > 0).sum((1, 2)).tolist()
    assert got[2] is None or np.array_equal((got[2] & 1) > 0, SO.boundary(mask > 0))
    return got


def _squares(n=1):
    """16 x 16: the label is the square 4..11, the prediction the square 5..10"""
    prob, y = np.zeros((n, 16, 16), np.float32), np.zeros((n, 16, 16), np.float32)
    y[:, 4:12, 4:12] = 1.0
    prob[:, 5:11, 5:11] = 0.75
    return prob, y


def _hand_samples(b):
    """the expected samples of slice b of _squares: written out, not the oracle's"""
    ring = lambda lo, hi: [y * 16 + x for y in range(lo, hi + 1) for x in range(lo, hi + 1) if y in (lo, hi) or x in (lo, hi)]
    corners = {4 * 16 + 4, 4 * 16 + 11, 11 * 16 + 4, 11 * 16 + 11}
    return [(b, 0, p, 1) for p in ring(5, 10)] + [(b, 1, p, 2 if p in corners else 1) for p in ring(4, 11)]


def test_hand_case_nested_squares(dm):
    prob, y = _squares()
    counts, samples, edges = call(dm, prob, y, k=1)
    assert counts.tolist() == [[36, 64, 36, 20, 28]]
    assert samples.tolist() == _hand_samples(0)
    pred, true = samples[samples['side'] == 0], samples[samples['side'] == 1]
    assert pred['d2'].tolist() == [1] * 20 and sorted(true['d2'].tolist()) == [1] * 24 + [2] * 4
    assert np.sqrt(float(samples['d2'].max())) == np.sqrt(2.0)                  # hd
    assert int((edges & 1).sum()) == 20 and int((edges >> 1).sum()) == 28 and edges[0, 5, 5] == 1 and edges[0, 4, 4] == 2
    same((counts, samples, edges), SO.surface(prob, y, k=1))
    from dnncancerannotator_amd import casewise as CW
    assert CW.surface_slice_values('e', 0, counts[0], pred['d2'], true['d2'])[8:10] == [repr(72 / 100), repr(float(np.sqrt(2.0)))]


@pytest.mark.parametrize('name', sorted(MC.ALL))
def test_match_cases_equal_the_oracle(dm, name):
    prob, y, spec = MC.ALL[name]()
    got = check_drawn(dm, prob, y, spec)
    assert len(got[0]) in (2, 3)
    if name == 'resized_opened':                                                # the area filter drops A: the outline of B alone
        cut = check_drawn(dm, prob, y, spec, min_area=40)
        assert cut[0][:, 0].tolist() == [168, 168] and got[0][:, 0].tolist() == [198, 198]
        check_drawn(dm, prob, y, spec, edges=False)
    if name == 'full_planes_shifted':                                           # 72 x 80 full: the boundary is the image frame
        assert got[0][0].tolist()[3:] == [2 * 72 + 2 * 80 - 4] * 2


@pytest.mark.parametrize('name', sorted(LC.ALL))
def test_lesion_cases_against_their_shifted_copy(dm, name):
    """the label is the prediction's foreground shifted down by 2 and left by 3 pixels"""
    prob, spec = LC.ALL[name]()
    y = np.roll(prob >= np.float32(spec['threshold']), (2, -3), axis=(1, 2)).astype(np.float32)
    got = check_drawn(dm, prob, y, spec)
    if name == 'areas':                                                         # components of 9, 1, 100 and 4 pixels
        assert got[0][0, 0] == 114 and check_drawn(dm, prob, y, spec, min_area=5)[0][0, 0] == 109
    if name == 'empty_and_full':
        assert got[0].tolist() == [[0, 0, 0, 0, 0], [2880, 2880, 2880, 220, 220]]
        assert set(got[1]['slice'].tolist()) == {1} and got[1]['d2'].tolist() == [0] * 440


def test_far_corners(dm):
    """24 x 40: one pixel in either corner, every other column without a boundary pixel: the sentinel's square never wins"""
    prob, y = np.zeros((1, 24, 40), np.float32), np.zeros((1, 24, 40), np.float32)
    prob[0, 0, 0] = 1.0
    y[0, 23, 39] = 1.0
    counts, samples, _ = call(dm, prob, y, k=1)
    assert counts.tolist() == [[1, 1, 0, 1, 1]]
    assert samples.tolist() == [(0, 0, 0, 23 ** 2 + 39 ** 2), (0, 1, 23 * 40 + 39, 2050)]
    same(call(dm, y, prob, k=1), SO.surface(y, prob, k=1))                       # mirrored: the walk to the left


def test_tall_plane_more_pieces_than_lanes(dm):
    """545 x 20: a column is 18 pieces of 32 rows, more than the 16 a block's threads take in one round; the nearest boundary row
    lies up to 16 pieces away"""
    prob, y = np.zeros((2, 545, 20), np.float32), np.zeros((2, 545, 20), np.float32)
    prob[0, 0, 3] = prob[0, 544, 17] = 1.0
    y[0, 300, 10] = 1.0
    prob[1, 520:545, 0:5] = 1.0
    y[1, 0:3, 12:20] = 1.0
    counts, samples, _ = call(dm, prob, y, k=1)
    assert counts[0].tolist() == [2, 1, 0, 2, 1]
    assert samples[samples['slice'] == 0].tolist() == [(0, 0, 3, 300 ** 2 + 7 ** 2), (0, 0, 544 * 20 + 17, 244 ** 2 + 7 ** 2),
                                                       (0, 1, 300 * 20 + 10, 244 ** 2 + 7 ** 2)]
    assert int(samples[samples['slice'] == 1]['d2'].min()) == 518 ** 2 + 8 ** 2   # (520, 4) to (2, 12)
    same((counts, samples, None), SO.surface(prob, y, k=1))


def test_statuses_in_one_batch(dm):
    prob, y = _squares(3)
    prob[0], y[0], y[1], prob[2] = 0, 0, 0, 0
    counts, samples, edges = call(dm, prob, y, k=1)
    assert counts.tolist() == [[0, 0, 0, 0, 0], [36, 0, 0, 20, 0], [0, 64, 0, 0, 28]] and len(samples) == 0
    assert [int((e & 1).sum()) for e in edges] == [0, 20, 0] and [int((e >> 1).sum()) for e in edges] == [0, 0, 28]


def test_the_sample_bound(dm):
    """a 32 x 32 checkerboard on its complement: 512 boundary pixels on either side, every one next to the other side"""
    board = MC._checker()
    prob, y = board.astype(np.float32)[None], (~board).astype(np.float32)[None]
    counts, samples, edges = call(dm, prob, y, k=1, max_samples=512)
    assert counts.tolist() == [[512, 512, 0, 512, 512]] and len(samples) == 1024 and samples['d2'].tolist() == [1] * 1024
    same((counts, samples, edges), SO.surface(prob, y, k=1, max_samples=512))
    cut = call(dm, prob, y, k=1, max_samples=511)
    assert cut[0].tolist() == counts.tolist() and len(cut[1]) == 0 and np.array_equal(cut[2], edges)
    # between two hand-case slices: the neighbours' samples are intact, the board gives none
    sq_p, sq_y = _squares()
    big_p, big_y = np.zeros((3, 32, 32), np.float32), np.zeros((3, 32, 32), np.float32)
    big_p[0, :16, :16] = big_p[2, :16, :16] = sq_p[0]
    big_y[0, :16, :16] = big_y[2, :16, :16] = sq_y[0]
    big_p[1], big_y[1] = prob[0], y[0]
    got = call(dm, big_p, big_y, k=1, max_samples=511)
    assert got[0].tolist() == [[36, 64, 36, 20, 28], [512, 512, 0, 512, 512], [36, 64, 36, 20, 28]]
    widen = lambda rows: [(b, s, (p // 16) * 32 + p % 16, d) for b, s, p, d in rows]
    assert got[1].tolist() == widen(_hand_samples(0)) + widen(_hand_samples(2))
    same(got, SO.surface(big_p, big_y, k=1, max_samples=511))


def test_batches_and_two_runs(dm):
    prob, y, spec = MC.three_blocks()
    s = (spec['threshold'], spec['rf'], spec['k'])
    whole = call(dm, prob, y, *s)
    again = call(dm, prob, y, *s)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again)) and len(whole[1]) > 0
    for b in range(3):                                                          # batch 1: every slice alone is its part of batch 3
        one = call(dm, prob[b:b + 1], y[b:b + 1], *s)
        part = whole[1][whole[1]['slice'] == b].copy()
        part['slice'] = 0
        assert one[0].tolist() == whole[0][b:b + 1].tolist() and one[1].tolist() == part.tolist()
        assert np.array_equal(one[2][0], whole[2][b])


def test_refusals_launch_nothing(gpu):
    from dnncancerannotator_amd._lib import DnncaError
    prob, y = _squares(3)
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    try:
        m.sync()
        m.profile_reset()
        m.profile_enable(1)
        for word, kw in [('batch', dict(batch=0)), ('batch', dict(batch=4)), ('filter_size', dict(k=16)), ('max_samples', dict(max_samples=0)),
                         ('y_hw', dict(null='y')), ('samples', dict(short='samples')), ('edges', dict(short='edges')),
                         ('samples', dict(null='samples')), ('n_samples', dict(null='n_samples')), ('threshold', dict(threshold=-0.5)),
                         ('resize factor', dict(rf=0.0)), ('min_area', dict(min_area=-1))]:
            with pytest.raises(DnncaError) as e:
                call(m, prob, y, **dict(dict(k=1), **kw))
            assert e.value.code == -1 and word in str(e.value), str(e.value)
            assert m.profile() == []
        m.profile_enable(0)
        assert call(m, prob, y, k=1)[0].tolist() == [[36, 64, 36, 20, 28]] * 3
    finally:
        m.profile_enable(0)
        m.profile_reset()
        m.close()


def test_chains_of_the_linked_and_the_matched_call_do_not_notice(dm):
    prob, y, spec = MC.three_blocks()
    s = (spec['threshold'], spec['rf'], spec['k'])
    surface = lambda: call(dm, prob[1:], y[1:], *s)                            # the same plane size, other slices
    linked_call(dm, prob[:2], [0, 1], *s)
    want = linked_call(dm, prob[2:], [1], *s)
    linked_call(dm, prob[:2], [0, 1], *s)
    surface()
    got = linked_call(dm, prob[2:], [1], *s)
    same_links(got[3], want[3])
    same_links(got[3], KO.links(prob[2:], [1], *s, carry=KO.row_maps(prob[:2], *s)[-1]))
    assert len(got[3]) > 0
    matched_call(dm, prob[:2], y[:2], [0, 1], *s)
    want = matched_call(dm, prob[2:], y[2:], [1], *s)
    matched_call(dm, prob[:2], y[:2], [0, 1], *s)
    surface()
    got = matched_call(dm, prob[2:], y[2:], [1], *s)
    same_all(got, want)
    assert len(got[3]) > 0 and len(got[6]) > 0


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_last_forward_plan_and_nothing_else_changes(gpu, dtype):
    """surface_distances on the last forward's probabilities (DeviceModel): equal to the call on last_prob and to the oracle; the
    dry plan is the live profile: the reused launches, then the three new ones; no other plan holds them; parameters, state,
    optimizer slots and last_prob are untouched"""
    m, x = _model(gpu, dtype)
    try:
        prob = m.forward(x, training=False)[..., 0]
        thr = float(np.median(prob))
        y = np.roll(prob >= np.float32(np.quantile(prob, 0.4)), 2, axis=2).astype(np.float32)
        p0, s0, o0 = m.get_params(), m.get_state(), m.get_opt_state()
        kw = dict(threshold=thr, resize_factor=0.5, filter_size=3, min_area=2)
        before = {mode: m.plan(mode=mode) for mode in ('train', 'eval', 'forward', 'lesion', 'lesion_linked', 'lesion_matched')}
        m.profile_reset()
        m.profile_enable(1)
        dev = m.surface_distances(y, batch=3, edges=True, **kw)
        live = {name: n for name, n, _, _, _ in m.profile()}
        m.profile_enable(0)
        m.profile_reset()
        plan = [r[0] for r in m.plan(mode='surface', batch=3)]
        assert plan == REUSED_PLAN + SURFACE_PLAN and {k: plan.count(k) for k in plan} == live
        for mode, rows in before.items():
            assert m.plan(mode=mode) == rows and not [r for r in rows if r[0] in SURFACE_PLAN]
        want = SO.surface(prob, y, thr, 0.5, 3, 2)
        same(dev, want)
        assert dev[1].dtype == SO.SAMPLE_DTYPE and len(dev[1]) > 0 and dev[2].shape == (3, 16, 24)
        host = m.surface_distances(y, prob=m.last_prob(3), **kw)
        assert host[2] is None and host[0].tobytes() == dev[0].tobytes() and host[1].tobytes() == dev[1].tobytes()
        m.surface_distances(y, batch=3, filter_size=1)                          # no opening: the plan follows the last call
        assert [r[0] for r in m.plan(mode='surface')] == [k for k in REUSED_PLAN if k != 'region_open'] + SURFACE_PLAN
        assert m.last_prob(3).tobytes() == prob.tobytes()
        assert m.get_params().tobytes() == p0.tobytes() and m.get_state().tobytes() == s0.tobytes()
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(m.get_opt_state(), o0))
        with pytest.raises(ValueError):
            m.surface_distances(y[:2], batch=3, **kw)
        with pytest.raises(ValueError):
            m.plan(mode='surfaces')
    finally:
        m.close()


def test_cli_evaluate_surface_distances_end_to_end(gpu, tmp_path):
    """six slices of one exam from an .npz; train 4 steps with a checkpoint every 2, then `evaluate --export_csv` with and without
    --surface_distances under two tags: the three new files exist only under the first, with one line per step x threshold, per
    exam and per slice; every other file is the same; the new files are DeviceModel.surface_distances + casewise.surface_* on
    the checkpoints' probabilities"""
    import yaml
    from dnncancerannotator_amd import casewise as CW, engine
    from dnncancerannotator_amd.runs.train import make_dataset
    rng = np.random.default_rng(3)
    y = np.zeros((6, 32, 32), np.float32)
    for b in range(4):
        y[b, 6 + b:16 + b, 8:20] = 1.0
    y[4, 22:27, 3:9] = 1.0
    x = np.stack([np.clip(y + rng.normal(0, 0.2, y.shape), 0, 1), rng.random(y.shape)], -1).astype(np.float32)
    npz = str(tmp_path / 'exam.npz')
    np.savez(npz, x=x, y=y)
    cfg = {'model': 'UNetAnnotator', 'model_options': UNET,
           'deploy_options': {'optimizer': 'adam', 'enable_multigpu': False},
           'data_options': {'train': {'batch_size': 2}, 'eval': {'batch_size': 2}}}
    cfg_path, run = str(tmp_path / 'cfg.yaml'), str(tmp_path / 'run')
    with open(cfg_path, 'w') as f:
        yaml.safe_dump(cfg, f)
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, '-m', 'dnncancerannotator_amd']
    r = subprocess.run(base + ['train', '--config', cfg_path, '--save_path', run, '--data_path', npz, '--max_steps', '4',
                               '--save_freq', '2'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    thresholds, texts = [0.3, 0.5], {}
    flags = ['--surface_distances', '--surface_threshold', '0.3', '0.5', '--surface_filter_size', '3', '--surface_percentile', '90']
    for tag, extra in (('surface', flags), ('plain', [])):
        r = subprocess.run(base + ['evaluate', '--save_path', run, '--data_path', npz, '--tag', tag, '--export_csv'] + extra,
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        root, texts[tag] = os.path.join(run, 'tfevents', tag), {}
        for d, _, files in os.walk(root):
            for fn in files:
                with open(os.path.join(d, fn), 'rb') as f:
                    texts[tag][os.path.relpath(os.path.join(d, fn), root)] = f.read()
    new = ['surface_cases.csv', 'surface_results.csv', 'surface_slices.csv']
    assert sorted(set(texts['surface']) - set(texts['plain'])) == new and set(texts['plain']) <= set(texts['surface'])
    assert 'results.csv' in texts['plain'] and 'casewise_results.csv' in texts['plain'] and len(texts['plain']) > 2
    assert all(texts['surface'][k] == texts['plain'][k] for k in texts['plain'])
    e = engine.TFKerasModel(cfg)
    ds = make_dataset([npz], cfg['data_options']['eval'], training=False, include_meta=True)
    e._build(ds)
    batches = list(ds)
    exams = [p for b in batches for p in b[2]]
    ids = [int(k) for b in batches for k in b[3]]
    big = gpu.DeviceModel('unet', 1, 16, 16, 6, **UNET)
    results, cases, slices = [], [], []
    try:
        steps = e.get_ckpts(os.path.join(run, 'checkpoints'))
        assert len(steps) == 2
        for step, path in steps.items():
            e.load(path)
            prob = np.concatenate([e.device_model.forward(b[0], training=False)[..., 0] for b in batches])
            for thr in thresholds:
                counts, samples, _ = big.surface_distances(y, prob=prob, threshold=thr, filter_size=3)
                d2 = lambda b, side: samples['d2'][(samples['slice'] == b) & (samples['side'] == side)]
                lead = [step, repr(thr)]
                sv = [CW.surface_slice_values(exams[b], ids[b], counts[b], d2(b, 0), d2(b, 1), percentile=90.0) for b in range(6)]
                ev = [CW.surface_exam_values(name, [(counts[b], d2(b, 0), d2(b, 1)) for b in range(6) if exams[b] == name], percentile=90.0)
                      for name in dict.fromkeys(exams)]
                slices += [lead + v for v in sv]
                cases += [lead + v for v in ev]
                results.append(lead + CW.surface_summary(sv, ev))
    finally:
        big.close()
        e.device_model.close()
    lead = ['step', 'threshold']
    assert len(results) == 4 and len(slices) == 24 and len(cases) == 4 * len(set(exams))
    assert texts['surface']['surface_results.csv'].decode() == CW.plain_csv(lead + CW.SURFACE_RESULT_COLUMNS, results)
    assert texts['surface']['surface_cases.csv'].decode() == CW.plain_csv(lead + CW.SURFACE_CASE_COLUMNS, cases)
    assert texts['surface']['surface_slices.csv'].decode() == CW.plain_csv(lead + CW.SURFACE_SLICE_COLUMNS, slices)
