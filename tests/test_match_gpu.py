"""-m gpu: dnnca_lesion_table_matched through the C ABI: the linked call on the probabilities, the same on the labels, and the
common pixels of labelled and predicted lesions, per chunk the launches of the lesion table for either plane, then lesion_match,
lesion_link_emit and lesion_match_carry.  Everything is an integer: all eight outputs must EQUAL the numpy oracles
(tests/match_oracle.py) on the drawn cases of tests/match_cases.py, the first four must equal what dnnca_lesion_table_linked
returns, and the label's three what that call returns for the labels.  The host buffers carry guard regions behind them,
pre-filled with a sentinel: nothing may be written past the counted entries."""

import csv
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lesion_oracle as LO
import link_oracle as KO
import match_cases as MC
import match_oracle as MO
from test_lesion_gpu import ROOT, SENTINEL, UNET, same
from test_link_gpu import LESION_PLAN, LINK_PLAN, _model, call as linked_call, same_links

pytestmark = pytest.mark.gpu

GUARD = 8
TABLE_PLAN = LESION_PLAN[2:8]            # ccl x 3, sizes, scan, stats: what the label plane adds behind its own region_prep
MATCH_PLAN = ['lesion_match', 'lesion_link_emit', 'lesion_match_carry']


@pytest.fixture(scope='module')
def dm(gpu):
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    yield m
    m.close()


def _guarded(n, dtype):
    return np.full(max(n, 0) + GUARD, SENTINEL, np.uint8).repeat(dtype.itemsize).view(dtype)


def call(dm, prob, y, continues, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256, mask=True, batch=None, short=None,
         null=None):
    """dnnca_lesion_table_matched on host probabilities and labels [B, h, w] with guarded buffers -> the eight outputs.
    short: one of 'rows', 'links', 'true_rows', 'true_links', 'pairs', 'mask': that capacity is one too small; null: 'y' or
    'continues'"""
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import check, fptr
    prob, y = np.ascontiguousarray(prob, np.float32), np.ascontiguousarray(y, np.float32)
    B, h, w = prob.shape
    B = B if batch is None else batch
    oh, ow = LO.O.out_size(h, w, rf)
    per = min(max_lesions, (oh * ow + 1) // 2)
    cap, lcap, nmask = B * per, B * min(per * per, (oh * ow + 1) // 2), B * oh * ow
    less = lambda name: 1 if short == name else 0
    flags = np.ascontiguousarray(continues, np.uint8)
    masks = np.full(max(nmask, 0) + 64, SENTINEL, np.uint8)
    bufs, outs = {}, {}
    for side in ('', 'true_'):
        rows, links, totals = _guarded(cap, LO.ROW_DTYPE), _guarded(lcap, KO.LINK_DTYPE), np.full(B + 4, -7, np.int32)
        bufs[side] = rows, links, totals
        outs[side] = _lib.LesionPlaneOut(rows.ctypes.data_as(C.POINTER(_lib.LesionRow)), cap - less(side + 'rows'), -1,
                                         totals.ctypes.data_as(C.POINTER(C.c_int32)), links.ctypes.data_as(C.POINTER(_lib.LesionLink)),
                                         lcap - less(side + 'links'), -1)
    pairs = _guarded(lcap, MO.PAIR_DTYPE)
    po = _lib.LesionPairsOut(pairs.ctypes.data_as(C.POINTER(_lib.LesionPair)), lcap - less('pairs'), -1)
    hw = (C.c_int32 * 2)()
    check(dm.lib.dnnca_lesion_table_matched(dm.handle, fptr(prob), None if null == 'y' else fptr(y), B, h, w, threshold, rf, k, min_area,
                                            max_lesions, None if null == 'continues' else flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            C.byref(outs['']), masks.ctypes.data_as(C.c_void_p) if mask else None,
                                            (nmask - less('mask')) if mask else 0, C.byref(outs['true_']), C.byref(po), hw))
    assert (hw[0], hw[1]) == (oh, ow)
    res = []
    for side in ('', 'true_'):
        (rows, links, totals), o = bufs[side], outs[side]
        assert 0 <= o.n_rows <= cap and 0 <= o.n_links <= lcap
        assert (rows[o.n_rows:].view(np.uint8) == SENTINEL).all(), side + 'rows written past the table'
        assert (links[o.n_links:].view(np.uint8) == SENTINEL).all(), side + 'links written past the list'
        assert (totals[B:] == -7).all()
        res.append((rows[:o.n_rows].copy(), totals[:B].copy(), links[:o.n_links].copy()))
    assert 0 <= po.n_pairs <= lcap and (pairs[po.n_pairs:].view(np.uint8) == SENTINEL).all(), 'pairs written past the list'
    assert (masks[nmask:] == SENTINEL).all() and (mask or (masks == SENTINEL).all())
    (r, t, l), (tr, tt, tl) = res
    return r, t, (masks[:nmask].reshape(B, oh, ow).copy() if mask else None), l, tr, tt, tl, pairs[:po.n_pairs].copy()


def same_all(got, want):
    """the eight outputs against eight expected ones (a mask of None on either side is not compared)"""
    same(got[:3], want[:3] if got[2] is not None and want[2] is not None else (want[0], want[1], None))
    same_links(got[3], want[3])
    same((got[4], got[5], None), (want[4], want[5], None))
    same_links(got[6], want[6])
    assert got[7].dtype == MO.PAIR_DTYPE and got[7].tolist() == want[7].tolist()


def check_case(dm, name, continues=None, **kw):
    """the matched call on a drawn case against the oracle, against the linked call on the probabilities and the linked call on
    the labels -> the eight outputs"""
    prob, y, spec = MC.ALL[name]()
    continues = [b > 0 for b in range(len(prob))] if continues is None else continues
    s = (spec['threshold'], spec['rf'], spec['k'])
    got = call(dm, prob, y, continues, *s, **kw)
    okw = {k: v for k, v in kw.items() if k in ('min_area', 'max_lesions')}
    same_all(got, MO.matched(prob, y, continues, *s, **okw))
    lp = linked_call(dm, prob, continues, *s, **kw)
    same(got[:3], lp[:3])
    same_links(got[3], lp[3])
    ly = linked_call(dm, y, continues, float(MO.TRUE_THRESHOLD), spec['rf'], 1, min_area=0, max_lesions=kw.get('max_lesions', 256),
                     mask=False)
    same((got[4], got[5], None), ly[:3])
    same_links(got[6], ly[3])
    return got


def test_pair_table_and_list_at_their_bound(dm):
    """32 x 32: 512 = (hw + 1) / 2 pairs of one pixel per slice: the table of hw + 1 slots and the list are at capacity"""
    got = check_case(dm, 'checker_on_ones', max_lesions=512)
    p = got[7][got[7]['slice'] == 0]
    assert len(p) == 512 and set(p['row_true'].tolist()) == {0} and p['row'].tolist() == list(range(512))
    assert got[7]['overlap'].tolist() == [1] * 1024 and got[5].tolist() == [1, 1]
    got = check_case(dm, 'checker_on_checker', max_lesions=512)
    p = got[7][got[7]['slice'] == 1]
    assert got[5].tolist() == [512, 512] and p['row_true'].tolist() == p['row'].tolist() == list(range(512))
    assert len(got[3]) == len(got[6]) == 512                                  # the two link tables at their bound beside it


def test_no_pairs_at_all(dm):
    got = check_case(dm, 'complementary_checkers', max_lesions=512)
    assert len(got[7]) == 0 and got[1].tolist() == got[5].tolist() == [512, 512]


def test_pairs_across_tiles_and_blocks(dm):
    assert check_case(dm, 'full_planes_shifted')[7].tolist() == [(0, 0, 0, 5760), (1, 0, 0, 5760), (2, 0, 0, 1)]
    assert check_case(dm, 'snake_shifted')[7].tolist() == [(0, 1, 1, 128), (0, 2, 2, 63), (1, 1, 1, 128), (1, 2, 2, 63)]


def test_resized_opened_filtered(dm):
    got = check_case(dm, 'resized_opened')
    assert got[7].tolist() == [(0, 0, 0, 16), (0, 1, 1, 56), (0, 2, 1, 6), (1, 0, 0, 16), (1, 1, 1, 56), (1, 2, 1, 6)]
    assert got[4]['area'].tolist() == [25, 56, 6] * 2                          # 0.75 and nextafter(0.5, 1) are in, 0.5 and 0.25 are out
    assert got[4]['max_prob'].tolist()[2] == float(MC.ABOVE_HALF)             # the statistics are the resized label's
    got = check_case(dm, 'resized_opened', min_area=40)                        # the rows after the filter are the ones in the pairs
    assert got[7].tolist() == [(0, 1, 0, 56), (0, 2, 0, 6), (1, 1, 0, 56), (1, 2, 0, 6)]
    assert got[5].tolist() == [3, 3]                                           # min_area is the prediction's alone
    check_case(dm, 'resized_opened', mask=False)


def test_max_lesions_truncates_both_sides(dm):
    got = check_case(dm, 'checker_on_checker', max_lesions=16)
    assert got[1].tolist() == got[5].tolist() == [512, 512]
    assert [p[1:] for p in got[7].tolist()] == [(r, r, 1) for r in range(16)] * 2
    got = check_case(dm, 'checker_on_ones', max_lesions=16)
    assert [p[1:] for p in got[7].tolist()] == [(0, r, 1) for r in range(16)] * 2


def test_flags(dm):
    got = check_case(dm, 'three_blocks', continues=[0, 1, 0])
    assert set(got[3]['slice'].tolist()) == set(got[6]['slice'].tolist()) == {1}
    whole = check_case(dm, 'three_blocks', continues=[0, 0, 0])
    assert len(whole[3]) == len(whole[6]) == 0
    assert whole[7].tolist() == got[7].tolist() and len(whole[7]) == 11        # the pairs do not look at the flags
    got = check_case(dm, 'three_blocks', continues=[0, 7, 255])                # any non-zero byte is a set flag
    assert len(got[3]) == 5 and len(got[6]) == 5


def _abc(dm, between=None, **kw):
    """A B in one call, C alone with continues[0] = 1 -> (links, true links, pairs) re-indexed to A B C"""
    prob, y, spec = MC.three_blocks()
    s = (spec['threshold'], spec['rf'], spec['k'])
    head = call(dm, prob[:2], y[:2], [0, 1], *s, **kw)
    if between:
        between()
    tail = call(dm, prob[2:], y[2:], [1], *s, **kw)
    out = []
    for i in (3, 6, 7):
        t = tail[i].copy()
        t['slice'] += 2
        out.append(np.concatenate([head[i], t]))
    return out


def test_carries_across_calls(dm):
    prob, y, spec = MC.three_blocks()
    s = (spec['threshold'], spec['rf'], spec['k'])
    whole = call(dm, prob, y, [0, 1, 1], *s)
    want = [whole[3], whole[6], whole[7]]
    assert [len(w) for w in want] == [5, 5, 11]
    for g, w in zip(_abc(dm), want):
        assert g.tolist() == w.tolist()
    other, os_ = MC.KC.graded_half()

    def linked_elsewhere():
        linked_call(dm, other, [0, 1], os_['threshold'], os_['rf'], os_['k'])
        linked_call(dm, prob[:1], [0], *s)                                     # the same plane size: another chain's slice
    for g, w in zip(_abc(dm, between=linked_elsewhere), want):
        assert g.tolist() == w.tolist()
    m3 = MO.matched(prob, y, [0, 1, 1], *s, max_lesions=3)
    for g, w in zip(_abc(dm, max_lesions=3), (m3[3], m3[6], m3[7])):
        assert g.tolist() == w.tolist()
    # a matched call (on other labels and another slice) between two linked calls leaves the linked chain what KO.links says
    linked_call(dm, prob[:2], [0, 1], *s)
    call(dm, prob[2:], y[2:], [0], *s)
    same_links(linked_call(dm, prob[2:], [1], *s)[3], KO.links(prob[2:], [1], *s, carry=KO.row_maps(prob[:2], *s)[-1]))
    # continues[0] = 0 ignores valid carries
    got = call(dm, prob[2:], y[2:], [0], *s)
    assert len(got[3]) == 0 and len(got[6]) == 0


def test_errors_launch_nothing_and_keep_the_carries(gpu):
    from dnncancerannotator_amd._lib import DnncaError
    prob, y, spec = MC.three_blocks()
    s = (spec['threshold'], spec['rf'], spec['k'])
    other, oy, os_ = MC.resized_opened()
    want = MO.matched(prob[2:], y[2:], [1], *s, carry=MO.pred_maps(prob[:2], *s)[-1], true_carry=MO.true_maps(y[:2])[-1])
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    try:
        m.sync()
        m.profile_reset()
        m.profile_enable(1)

        def refused(word, *a, **kw):
            with pytest.raises(DnncaError) as e:
                call(m, *a, **kw)
            assert e.value.code == -1 and word in str(e.value), str(e.value)
            assert m.profile() == []
        refused('continues[0]', prob[2:], y[2:], [1], *s)                            # a fresh model has no matched carry
        m.profile_enable(0)
        linked_call(m, prob[:2], [0, 1], *s)                                         # a linked predecessor is none
        m.profile_reset()
        m.profile_enable(1)
        refused('continues[0]', prob[2:], y[2:], [1], *s)
        m.profile_enable(0)
        call(m, prob[:2], y[:2], [0, 1], *s)
        m.profile_reset()
        m.profile_enable(1)
        tail = (prob[2:], y[2:], [1]) + s
        for word, a, kw in [('continues[0]', (other[:1], oy[:1], [1], os_['threshold'], os_['rf'], os_['k']), {}),   # another plane size
                            ('y_hw', tail, dict(null='y')),
                            ('continues', tail, dict(null='continues')),
                            ('rows', tail, dict(short='rows')),
                            ('links', tail, dict(short='links')),
                            ('mask', tail, dict(short='mask')),
                            ('true_rows', tail, dict(short='true_rows')),
                            ('true_links', tail, dict(short='true_links')),
                            ('pairs', tail, dict(short='pairs')),
                            ('filter_size', (prob[2:], y[2:], [1], 0.5, 1.0, 16), {}),
                            ('threshold', (prob[2:], y[2:], [1], -0.5, 1.0, 1), {}),
                            ('batch', tail, dict(batch=0))]:
            refused(word, *a, **kw)
            m.profile_enable(0)
            same_all(call(m, *tail), want)                                           # still the carries of B
            call(m, prob[:2], y[:2], [0, 1], *s)
            m.profile_reset()
            m.profile_enable(1)
        m.profile_enable(0)
        call(m, other[:1], oy[:1], [0], os_['threshold'], os_['rf'], os_['k'])        # moves the carries to another plane size
        m.profile_enable(1)
        refused('continues[0]', *tail)
    finally:
        m.profile_enable(0)
        m.profile_reset()
        m.close()


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_last_forward_plan_and_nothing_else_changes(gpu, dtype):
    """lesion_table_matched on the last forward's probabilities (DeviceModel): the dry plan is the live profile and holds the pair
    kernel once per chunk and no lesion_link; parameters, state, optimizer slots and last_prob are untouched; two runs agree"""
    m, x = _model(gpu, dtype)
    try:
        prob = m.forward(x, training=False)[..., 0]
        thr = float(np.median(prob))
        y = np.roll(prob >= np.float32(np.quantile(prob, 0.4)), 2, axis=2).astype(np.float32)
        p0, s0, o0 = m.get_params(), m.get_state(), m.get_opt_state()
        kw = dict(threshold=thr, resize_factor=0.5, filter_size=3, min_area=2, max_lesions=64)
        linked = m.lesion_table_linked(batch=3, continues=[False, True, True], mask=True, **kw)
        m.profile_reset()
        m.profile_enable(1)
        dev = m.lesion_table_matched(y, batch=3, continues=[False, True, True], mask=True, **kw)
        live = {name: n for name, n, _, _, _ in m.profile()}
        m.profile_enable(0)
        m.profile_reset()
        plan = [r[0] for r in m.plan(mode='lesion_matched', batch=3)]
        assert plan == LESION_PLAN + ['region_prep'] + TABLE_PLAN + MATCH_PLAN and {k: plan.count(k) for k in plan} == live
        assert plan.count('lesion_match') == 1 and 'lesion_link' not in plan and 'lesion_carry' not in plan
        assert [r[0] for r in m.plan(mode='lesion_linked', batch=3)] == LESION_PLAN + LINK_PLAN
        same(dev[:3], linked[:3])
        same_links(dev[3], linked[3])
        same_all(dev, MO.matched(prob, y, [0, 1, 1], thr, 0.5, 3, 2, 64))
        assert len(dev[7]) > 0 and len(dev[6]) > 0
        again = m.lesion_table_matched(y, batch=3, continues=[False, True, True], mask=True, **kw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(dev, again))
        host = m.lesion_table_matched(y, prob=prob, continues=[True, True, True], **kw)      # slice 0 on slice 2 of the call before
        assert host[2] is None
        same_all(host, MO.matched(prob, y, [1, 1, 1], thr, 0.5, 3, 2, 64, carry=MO.pred_maps(prob, thr, 0.5, 3, 2, 64)[-1],
                                  true_carry=MO.true_maps(y, 0.5, 64)[-1]))
        assert [r[0] for r in m.plan(mode='lesion_matched', batch=3)] == LESION_PLAN[:-1] + ['region_prep'] + TABLE_PLAN + MATCH_PLAN
        assert m.last_prob(3).tobytes() == prob.tobytes()
        assert m.get_params().tobytes() == p0.tobytes() and m.get_state().tobytes() == s0.tobytes()
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(m.get_opt_state(), o0))
        for mode in ('train', 'eval', 'forward', 'lesion', 'lesion_linked'):
            assert not [r[0] for r in m.plan(mode=mode) if r[0] in ('lesion_match', 'lesion_match_carry')]
        with pytest.raises(ValueError):
            m.lesion_table_matched(y, batch=3, continues=[0, 1], **kw)
        with pytest.raises(ValueError):
            m.lesion_table_matched(y[:2], batch=3, continues=[0, 1, 1], **kw)
    finally:
        m.close()


def test_cli_evaluate_exam_lesions_end_to_end(gpu, tmp_path):
    """six slices of one exam from an .npz whose labels hold a blob through slices 0..3 and one in slice 4 alone; train 4 steps,
    then `evaluate --export_csv` with and without --exam_lesions under two tags: the three new files exist only under the first,
    every other file is the same; the new files are DeviceModel.lesion_table_matched + casewise.link_lesions +
    casewise.match_exam_lesions on the checkpoint's probabilities; the labelled tumours do not depend on the threshold"""
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
                               '--save_freq', '4'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    thresholds, texts = [0.3, 0.5], {}
    flags = ['--exam_lesions', '--exam_threshold', '0.3', '0.5', '--exam_filter_size', '3', '--exam_max_lesions', '64']
    for tag, extra in (('exam', flags), ('plain', [])):
        r = subprocess.run(base + ['evaluate', '--save_path', run, '--data_path', npz, '--tag', tag, '--export_csv'] + extra,
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        root, texts[tag] = os.path.join(run, 'tfevents', tag), {}
        for d, _, files in os.walk(root):
            for fn in files:
                with open(os.path.join(d, fn), 'rb') as f:
                    texts[tag][os.path.relpath(os.path.join(d, fn), root)] = f.read()
    new = ['exam_lesion_cases.csv', 'exam_lesion_matches.csv', 'exam_lesion_results.csv']
    assert sorted(set(texts['exam']) - set(texts['plain'])) == new and set(texts['plain']) <= set(texts['exam'])
    assert 'results.csv' in texts['plain'] and 'casewise_results.csv' in texts['plain'] and len(texts['plain']) > 2
    assert all(texts['exam'][k] == texts['plain'][k] for k in texts['plain'])
    # the recomputation: the checkpoints' probabilities batch by batch, then one matched call per threshold over the whole exam
    e = engine.TFKerasModel(cfg)
    ds = make_dataset([npz], cfg['data_options']['eval'], training=False, include_meta=True)
    e._build(ds)
    batches = list(ds)
    assert [list(b[3]) for b in batches] == [[0, 1], [2, 3], [4, 5]] and all(p == npz for b in batches for p in b[2])
    big = gpu.DeviceModel('unet', 1, 16, 16, 6, **UNET)
    results, cases, matches = [], [], []
    try:
        for step, path in e.get_ckpts(os.path.join(run, 'checkpoints')).items():
            e.load(path)
            prob = np.concatenate([e.device_model.forward(b[0], training=False)[..., 0] for b in batches])
            for thr in thresholds:
                o = big.lesion_table_matched(y, prob=prob, continues=[0, 1, 1, 1, 1, 1], threshold=thr, filter_size=3, max_lesions=64)
                sl = lambda rows, tot: [(b, rows[rows['slice'] == b], tot[b]) for b in range(6)]
                of = lambda a: [[tuple(v)[1:] for v in a[a['slice'] == b].tolist()] for b in range(6)]
                ts, ps = sl(o[4], o[5]), sl(o[0], o[1])
                case, lines = CW.match_exam_lesions(npz, ts, ps, CW.link_lesions(npz, ts, of(o[6])), CW.link_lesions(npz, ps, of(o[3])),
                                                    of(o[7]))
                lead = [step, repr(thr)]
                results.append(lead + CW.exam_match_summary([case]))
                cases.append(lead + case)
                matches += [lead + l for l in lines]
    finally:
        big.close()
        e.device_model.close()
    assert results, 'no checkpoint was evaluated'
    lead = ['step', 'threshold']
    assert texts['exam']['exam_lesion_results.csv'].decode() == CW.plain_csv(lead + CW.EXAM_RESULT_COLUMNS, results)
    assert texts['exam']['exam_lesion_cases.csv'].decode() == CW.plain_csv(lead + CW.EXAM_CASE_COLUMNS, cases)
    assert texts['exam']['exam_lesion_matches.csv'].decode() == CW.plain_csv(lead + CW.EXAM_MATCH_COLUMNS, matches)
    got = list(csv.DictReader(texts['exam']['exam_lesion_matches.csv'].decode().splitlines()))
    true = {t: [[g[k] for k in ['step'] + CW.EXAM_MATCH_COLUMNS[:7]] for g in got if g['kind'] == 'true' and g['threshold'] == repr(t)]
            for t in thresholds}
    assert true[0.3] == true[0.5] and len(true[0.3]) >= 2                     # the labelled tumours are the labels' alone
    assert [t[4:7] for t in true[0.3][-2:]] == [['0', '3', '4'], ['4', '4', '1']]
