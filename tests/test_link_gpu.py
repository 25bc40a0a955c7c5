"""-m gpu: the links between neighbouring slices (dnnca_lesion_table_linked: the launches of dnnca_lesion_table, then lesion_link,
lesion_link_emit, lesion_carry per chunk) through the C ABI.  Everything is an integer: links, rows, totals and masks must EQUAL
the numpy oracles (tests/link_oracle.py, tests/lesion_oracle.py) on the drawn cases of tests/link_cases.py.  The host buffers carry
guard regions behind them, pre-filled with a sentinel: nothing may be written past what the call was given.

A chunk boundary (more than 2^24 pixels in one call) is beyond what the numpy oracle can afford; the first slice of every chunk
takes its predecessor from the carry plane, as the first slice of a call does, so the call-boundary tests below cover that path."""

import csv
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lesion_oracle as LO
import link_cases as KC
import link_oracle as KO
from test_lesion_gpu import ROOT, SENTINEL, UNET, call as plain_call, same

pytestmark = pytest.mark.gpu

GUARD_LINKS = 8


@pytest.fixture(scope='module')
def dm(gpu):
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    yield m
    m.close()


def call(dm, prob, continues, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256, mask=True, batch=None, links_short=0,
         null_continues=False):
    """dnnca_lesion_table_linked on host probabilities [B, h, w] with guarded buffers -> (rows, totals, masks, links)"""
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import check, fptr
    prob = np.ascontiguousarray(prob, np.float32)
    B, h, w = prob.shape
    B = B if batch is None else batch
    oh, ow = LO.O.out_size(h, w, rf)
    per = min(max_lesions, (oh * ow + 1) // 2)
    cap = B * per
    rows = np.full(max(cap, 0) + 8, SENTINEL, np.uint8).repeat(LO.ROW_DTYPE.itemsize).view(LO.ROW_DTYPE)
    nmask = B * oh * ow
    masks = np.full(max(nmask, 0) + 64, SENTINEL, np.uint8)
    totals = np.full(B + 4, -7, np.int32)
    lcap = B * min(per * per, (oh * ow + 1) // 2) - links_short
    links = np.full(max(lcap, 0) + GUARD_LINKS, SENTINEL, np.uint8).repeat(KO.LINK_DTYPE.itemsize).view(KO.LINK_DTYPE)
    flags = np.ascontiguousarray(continues, np.uint8)
    n, nl, hw = C.c_int64(-1), C.c_int64(-1), (C.c_int32 * 2)()
    check(dm.lib.dnnca_lesion_table_linked(dm.handle, fptr(prob), B, h, w, threshold, rf, k, min_area, max_lesions,
                                           rows.ctypes.data_as(C.POINTER(_lib.LesionRow)), cap, C.byref(n),
                                           totals.ctypes.data_as(C.POINTER(C.c_int32)), masks.ctypes.data_as(C.c_void_p) if mask else None,
                                           nmask if mask else 0, hw, None if null_continues else flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                           links.ctypes.data_as(C.POINTER(_lib.LesionLink)), lcap, C.byref(nl)))
    assert (hw[0], hw[1]) == (oh, ow)
    assert 0 <= n.value <= cap and 0 <= nl.value <= lcap
    assert (rows[n.value:].view(np.uint8) == SENTINEL).all(), 'rows written past the table'
    assert (links[nl.value:].view(np.uint8) == SENTINEL).all(), 'links written past the list'
    assert (totals[B:] == -7).all() and (masks[nmask:] == SENTINEL).all()
    return rows[:n.value].copy(), totals[:B].copy(), (masks[:nmask].reshape(B, oh, ow).copy() if mask else None), links[:nl.value].copy()


def same_links(got, want):
    assert got.dtype == KO.LINK_DTYPE and got.tolist() == want.tolist()


def check_case(dm, name, continues=None, **kw):
    """the linked call on a drawn case against both oracles, and its table against the plain call's"""
    prob, spec = KC.ALL[name]()
    continues = [b > 0 for b in range(len(prob))] if continues is None else continues
    got = call(dm, prob, continues, spec['threshold'], spec['rf'], spec['k'], **kw)
    okw = {k: v for k, v in kw.items() if k in ('min_area', 'max_lesions')}
    same(got[:3], LO.lesion_table(prob, spec['threshold'], spec['rf'], spec['k'], **okw))
    same(got[:3], plain_call(dm, prob, spec['threshold'], spec['rf'], spec['k'], **kw))
    same_links(got[3], KO.links(prob, continues, spec['threshold'], spec['rf'], spec['k'], **okw))
    return got[3]


def test_pair_table_and_list_at_their_bound(dm):
    """32 x 32: 512 = (hw + 1) / 2 links of one pixel; every wave carries 32 distinct keys, the list is at capacity"""
    links = check_case(dm, 'checker_on_checker', max_lesions=512)
    assert len(links) == 512 and links['row_prev'].tolist() == links['row'].tolist() == list(range(512))
    assert links['overlap'].tolist() == [1] * 512 and links['slice'].tolist() == [1] * 512
    links = check_case(dm, 'checker_on_checker', max_lesions=16)             # only the links among rows below 16
    assert links['row'].tolist() == list(range(16))


def test_crossing_stripes_many_keys_per_lesion(dm):
    links = check_case(dm, 'crossing_stripes')
    assert len(links) == 256 and links['overlap'].tolist() == [1] * 256


def test_wave_grouping_and_counts_over_blocks_and_tiles(dm):
    assert check_case(dm, 'full_planes').tolist() == [(1, 0, 0, 5760), (2, 0, 0, 12)]
    assert check_case(dm, 'shifted_snake').tolist() == [(1, 1, 1, 126), (1, 2, 2, 54)]


def test_resized_opened_filtered(dm):
    links = check_case(dm, 'plateau_half')
    assert [l[:3] for l in links.tolist()] == [(1, 0, 0), (2, 1, 0)]          # frame on frame, block on block, nothing across
    assert [l[:3] for l in check_case(dm, 'graded_half').tolist()] == [(1, 0, 0), (1, 1, 1), (1, 1, 2)]
    assert [l[:3] for l in check_case(dm, 'graded_half', min_area=40).tolist()] == [(1, 0, 1)]      # the rows after the filter
    check_case(dm, 'graded_half', mask=False)


def test_flags(dm):
    links = check_case(dm, 'three_blocks', continues=[0, 1, 0])
    assert links.tolist() == [(1, 0, 0, 3), (1, 2, 2, 80)]                    # nothing into slice 2
    assert len(check_case(dm, 'three_blocks', continues=[0, 0, 0])) == 0
    assert len(check_case(dm, 'three_blocks', continues=[0, 7, 255])) == 5     # any non-zero byte is a set flag


def _abc(dm, between=None, **kw):
    """A B in one call, C alone with continues[0] = 1 -> the links re-indexed to A B C"""
    prob, spec = KC.three_blocks()
    s = (spec['threshold'], spec['rf'], spec['k'])
    head = call(dm, prob[:2], [0, 1], *s, **kw)
    if between:
        between()
    tail = call(dm, prob[2:], [1], *s, **kw)
    same(tail[:3], LO.lesion_table(prob[2:], *s, **kw))
    t = tail[3].copy()
    t['slice'] += 2
    return np.concatenate([head[3], t])


def test_carry_across_calls_is_the_chunk_boundary_path(dm, gpu):
    prob, spec = KC.three_blocks()
    s = (spec['threshold'], spec['rf'], spec['k'])
    whole = call(dm, prob, [0, 1, 1], *s)[3]
    same_links(whole, KO.links(prob, [0, 1, 1], *s))
    assert [l[0] for l in whole.tolist()] == [1, 1, 2, 2, 2]
    same_links(_abc(dm), whole)
    same_links(_abc(dm, max_lesions=3), KO.links(prob, [0, 1, 1], *s, max_lesions=3))

    def other_work():
        """a plain table on another size, a forward and a region_confusion_slices (which regrows and overwrites the workspace)"""
        big, bs = KC.full_planes()
        plain_call(dm, big, bs['threshold'], bs['rf'], bs['k'])
        x = np.random.default_rng(0).random((3, 16, 16, 1)).astype(np.float32)
        dm.forward(x, training=False)
        dm.region_confusion_slices((x[..., 0] > 0.5).astype(np.float32), [([0.3, 0.5, 0.7], 0.3, 1.0, 3)])
    same_links(_abc(dm, between=other_work), whole)
    # continues[0] = 0 ignores a valid carry
    assert len(call(dm, prob[2:], [0], *s)[3]) == 0


def test_errors_launch_nothing_and_keep_the_carry(gpu):
    from dnncancerannotator_amd._lib import DnncaError
    prob, spec = KC.three_blocks()
    s = (spec['threshold'], spec['rf'], spec['k'])
    other, os_ = KC.graded_half()
    want = KO.links(prob[2:], [1], *s, carry=KO.row_maps(prob[:2], *s)[-1])
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
        refused('continues[0]', prob[2:], [1], *s)                                     # a fresh model has no carry
        m.profile_enable(0)
        call(m, prob[:2], [0, 1], *s)
        m.profile_reset()
        m.profile_enable(1)
        for word, a, kw in [('continues[0]', (other[:1], [1], os_['threshold'], os_['rf'], os_['k']), {}),      # another plane size
                            ('links', (prob[2:], [1]) + s, dict(links_short=1)),
                            ('continues', (prob[2:], [1]) + s, dict(null_continues=True)),
                            ('filter_size', (prob[2:], [1], 0.5, 1.0, 16), {}),
                            ('batch', (prob[2:], [1]) + s, dict(batch=0))]:
            refused(word, *a, **kw)
            m.profile_enable(0)
            same_links(call(m, prob[2:], [1], *s)[3], want)                           # still the carry of B
            call(m, prob[:2], [0, 1], *s)
            m.profile_reset()
            m.profile_enable(1)
        # a linked call on another plane size moves the carry there
        m.profile_enable(0)
        call(m, other[:1], [0], os_['threshold'], os_['rf'], os_['k'])
        m.profile_enable(1)
        refused('continues[0]', prob[2:], [1], *s)
    finally:
        m.profile_enable(0)
        m.profile_reset()
        m.close()


def _model(gpu, dtype):
    from oracle import unet_oracle as OU
    opts = dict(UNET, n_filters_first=32) if dtype == 'bf16' else UNET
    m = gpu.DeviceModel('unet', 2, 32, 48, 3, dtype=dtype, **opts)
    spec = OU.ModelSpec('unet', 2, **opts)
    m.set_params(OU.flatten(spec, OU.init_params(spec, seed=5)))
    x, _ = OU.synthetic_batch(3, 32, 48, 2, seed_x=7, seed_y=8)
    return m, x


LESION_PLAN = ['region_prep', 'region_open', 'region_ccl_tile', 'region_ccl_merge', 'region_ccl_compress', 'region_sizes', 'lesion_scan',
               'lesion_stats', 'lesion_mask']
LINK_PLAN = ['lesion_link', 'lesion_link_emit', 'lesion_carry']


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_last_forward_plan_and_nothing_else_changes(gpu, dtype):
    """lesion_table_linked on the last forward's probabilities (DeviceModel): the table of lesion_table, the oracle's links; the dry
    plan is the live profile, the lesion plan plus the three link launches; parameters, state and last_prob are untouched"""
    m, x = _model(gpu, dtype)
    try:
        prob = m.forward(x, training=False)[..., 0]
        thr = float(np.median(prob))
        p0, s0 = m.get_params(), m.get_state()
        kw = dict(threshold=thr, resize_factor=0.5, filter_size=3, min_area=2, max_lesions=64)
        plain = m.lesion_table(batch=3, **kw)
        m.profile_reset()
        m.profile_enable(1)
        dev = m.lesion_table_linked(batch=3, continues=[False, True, True], **kw)
        live = {name: n for name, n, _, _, _ in m.profile()}
        m.profile_enable(0)
        m.profile_reset()
        plan = [r[0] for r in m.plan(mode='lesion_linked', batch=3)]
        assert plan == LESION_PLAN + LINK_PLAN and {k: plan.count(k) for k in plan} == live
        assert [r[0] for r in m.plan(mode='lesion', batch=3)] == LESION_PLAN
        same(dev[:3], plain)
        same(dev[:3], LO.lesion_table(prob, thr, 0.5, 3, 2, 64))
        same_links(dev[3], KO.links(prob, [0, 1, 1], thr, 0.5, 3, 2, 64))
        assert len(dev[3]) > 0
        host = m.lesion_table_linked(prob=prob, continues=[True, True, True], **kw)      # slice 0 on slice 2 of the call before
        same_links(host[3], KO.links(prob, [1, 1, 1], thr, 0.5, 3, 2, 64, carry=KO.row_maps(prob, thr, 0.5, 3, 2, 64)[-1]))
        assert m.lesion_table_linked(batch=3, continues=[0, 0, 0], mask=False, **kw)[2] is None
        assert [r[0] for r in m.plan(mode='lesion_linked', batch=3)] == LESION_PLAN[:-1] + LINK_PLAN
        assert m.last_prob(3).tobytes() == prob.tobytes()
        assert m.get_params().tobytes() == p0.tobytes() and m.get_state().tobytes() == s0.tobytes()
        for mode in ('train', 'eval', 'forward', 'lesion'):
            assert not [r[0] for r in m.plan(mode=mode) if r[0] in LINK_PLAN]
        with pytest.raises(ValueError):
            m.lesion_table_linked(batch=3, continues=[0, 1], **kw)
    finally:
        m.close()


def test_cli_predict_link_slices_end_to_end(gpu, tmp_path):
    """train three steps on synthetic:64x64x2 (four slices of one exam, batches of 2), then `predict` with and without
    --link_slices: the old files are byte-identical, the linked run adds exactly the two exam files, and exam_lesions.csv is
    casewise.link_lesions on the oracle's links of the device's probabilities"""
    import yaml
    from dnncancerannotator_amd import casewise as CW, engine
    from dnncancerannotator_amd.runs.train import make_dataset
    cfg = {'model': 'UNetAnnotator', 'model_options': UNET,
           'deploy_options': {'optimizer': 'adam', 'enable_multigpu': False},
           'data_options': {'train': {'batch_size': 2}, 'eval': {'batch_size': 2}}}
    cfg_path, run = str(tmp_path / 'cfg.yaml'), str(tmp_path / 'run')
    with open(cfg_path, 'w') as f:
        yaml.safe_dump(cfg, f)
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, '-m', 'dnncancerannotator_amd']
    data = 'synthetic:64x64x2'
    r = subprocess.run(base + ['train', '--config', cfg_path, '--save_path', run, '--data_path', data, '--max_steps', '3',
                               '--save_freq', '3'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    e = engine.TFKerasModel(cfg)
    ds = make_dataset([data], cfg['data_options']['eval'], training=False, include_meta=True, labels=False)
    e._build(ds)
    e.load(e.get_ckpts(os.path.join(run, 'checkpoints'))[3])
    batches = list(ds)
    assert [list(b[2]) for b in batches] == [[0, 1], [2, 3]] and all(p == data for b in batches for p in b[1])
    prob = np.concatenate([e.device_model.forward(b[0], training=False)[..., 0] for b in batches])
    e.device_model.close()
    thr = float(np.median(prob[:2]))                                 # as the unlinked CLI test: something to find
    kw = dict(threshold=thr, rf=1.0, k=3, min_area=4, max_lesions=32)
    args = ['--threshold', repr(thr), '--filter_size', '3', '--min_area', '4', '--max_lesions', '32']
    texts = {}
    for name, extra in (('plain', []), ('linked', ['--link_slices'])):
        out = str(tmp_path / name)
        r = subprocess.run(base + ['predict', '--save_path', run, '--data_path', data, '--output', out] + args + extra,
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        texts[name] = {}
        for fn in os.listdir(out):
            with open(os.path.join(out, fn), newline='') as f:
                texts[name][fn] = f.read()
    assert sorted(texts['plain']) == ['lesions.csv', 'slices.csv']
    assert sorted(texts['linked']) == ['exam_lesion_parts.csv', 'exam_lesions.csv', 'lesions.csv', 'slices.csv']
    assert all(texts['linked'][k] == texts['plain'][k] for k in texts['plain'])
    rows, totals, _ = LO.lesion_table(prob, **kw)
    links = KO.links(prob, [0, 1, 1, 1], **kw)
    table, parts = CW.link_lesions(data, [(b, rows[rows['slice'] == b], totals[b]) for b in range(4)],
                                   [[tuple(l)[1:] for l in links[links['slice'] == b].tolist()] for b in range(4)])
    assert texts['linked']['exam_lesions.csv'] == CW.plain_csv(CW.EXAM_LESION_COLUMNS, table)
    assert texts['linked']['exam_lesion_parts.csv'] == CW.plain_csv(CW.EXAM_PART_COLUMNS, parts)
    got = list(csv.DictReader(texts['linked']['exam_lesions.csv'].splitlines()))
    assert any(int(g['n_slices']) >= 2 for g in got), 'no exam lesion spans two slices'
    assert any(int(g['first_slice']) <= 1 and int(g['last_slice']) >= 2 for g in got), 'no exam lesion crosses the batch boundary'
