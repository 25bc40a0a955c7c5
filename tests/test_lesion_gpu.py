"""-m gpu: the lesion table of `annotator predict` (dnnca_lesion_table: region_prep / open / ccl / sizes of the prediction plane,
then lesion_scan, lesion_stats, lesion_mask) through the C ABI.  Every field is an integer sum or an extremum, so rows, totals and
masks must EQUAL the numpy oracle (tests/lesion_oracle.py) bit for bit on the drawn cases of tests/lesion_cases.py.  The host
buffers carry guard regions behind them, pre-filled with a sentinel: nothing may be written past what the call was given."""

import csv
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lesion_cases as LC
import lesion_oracle as LO
from test_casewise_host import decode_png

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNET = dict(n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')
GUARD_ROWS, GUARD_BYTES, SENTINEL = 8, 64, 0xAB


@pytest.fixture(scope='module')
def dm(gpu):
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    yield m
    m.close()


def call(dm, prob, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256, mask=True, batch=None, rows_short=0, mask_short=0):
    """dnnca_lesion_table on host probabilities [B, h, w] with guarded buffers -> (rows, totals, masks)"""
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import check, fptr
    prob = np.ascontiguousarray(prob, np.float32)
    B, h, w = prob.shape
    B = B if batch is None else batch
    oh, ow = LO.O.out_size(h, w, rf)
    cap = B * min(max_lesions, (oh * ow + 1) // 2) - rows_short
    rows = np.full(max(cap, 0) + GUARD_ROWS, SENTINEL, np.uint8).repeat(LO.ROW_DTYPE.itemsize).view(LO.ROW_DTYPE)
    nmask = B * oh * ow - mask_short
    masks = np.full(max(nmask, 0) + GUARD_BYTES, SENTINEL, np.uint8)
    totals = np.full(B + 4, -7, np.int32)
    n, hw = C.c_int64(-1), (C.c_int32 * 2)()
    check(dm.lib.dnnca_lesion_table(dm.handle, fptr(prob), B, h, w, threshold, rf, k, min_area, max_lesions,
                                    rows.ctypes.data_as(C.POINTER(_lib.LesionRow)), cap, C.byref(n),
                                    totals.ctypes.data_as(C.POINTER(C.c_int32)), masks.ctypes.data_as(C.c_void_p) if mask else None,
                                    nmask if mask else 0, hw))
    assert (hw[0], hw[1]) == (oh, ow)
    assert 0 <= n.value <= cap
    assert (rows[n.value:].view(np.uint8) == SENTINEL).all(), 'rows written past the table'
    assert (totals[B:] == -7).all()
    if mask:
        assert (masks[nmask:] == SENTINEL).all(), 'mask written past its end'
    else:
        assert (masks == SENTINEL).all()
    return rows[:n.value].copy(), totals[:B].copy(), (masks[:nmask].reshape(B, oh, ow).copy() if mask else None)


def same(got, want):
    assert got[1].tolist() == want[1].tolist(), (got[1], want[1])
    assert got[0].tolist() == want[0].tolist()
    assert got[0].tobytes() == want[0].tobytes()
    if got[2] is not None:
        assert np.array_equal(got[2], want[2])


def check_case(dm, name, **kw):
    prob, spec = LC.ALL[name]()
    got = call(dm, prob, spec['threshold'], spec['rf'], spec['k'], **kw)
    okw = {k: v for k, v in kw.items() if k in ('min_area', 'max_lesions')}
    want = LO.lesion_table(prob, spec['threshold'], spec['rf'], spec['k'], **okw)
    same(got, want)
    return got


def test_tile_borders_and_the_scan_carry(dm):
    """72 x 80, B = 2 of max_batch 3, k = 1: a component through six tiles, one inside a tile, one pixel at (0, 0).  The scan walks a
    slice in passes of 4096 pixels: the drawing shifted down by 20 rows has its third root at pixel 4516, in the second pass of
    5760 pixels, so its row number needs the carry"""
    rows, totals, masks = check_case(dm, 'tile_borders')
    assert totals.tolist() == [3, 3] and rows['area'].tolist() == [1, 171, 81] * 2
    for f in LO.ROW_DTYPE.names[2:]:
        assert rows[f][:3].tolist() == rows[f][3:].tolist(), f
    # roots in the second pass (pixels >= 4096: rows >= 52 of 80 columns) as well: the same drawing shifted down
    prob, spec = LC.tile_borders()
    low = np.roll(prob, 20, axis=1)
    got = call(dm, low, spec['threshold'], spec['rf'], spec['k'])
    same(got, LO.lesion_table(low, spec['threshold'], spec['rf'], spec['k']))
    assert got[0]['y0'][:3].tolist() == [20, 30, 56] and got[0]['row'][:3].tolist() == [0, 1, 2]


@pytest.mark.parametrize('name', ['odd_plateau', 'odd_graded', 'even_graded_half'])
def test_odd_sizes_and_the_mask_store(dm, name):
    """41 x 53 at 0.5 and at 1.0 with k = 5 (2173 and 520 mask bytes: the last word is partial at 1.0), 40 x 48 graded at 0.5"""
    rows, totals, masks = check_case(dm, name)
    assert totals.tolist() == [2]
    if name.startswith('odd'):
        assert tuple(rows[0][f] for f in ('x0', 'y0', 'x1', 'y1')) == (0, 0, masks.shape[2] - 1, masks.shape[1] - 1)
    # three slices, so that slice borders fall inside mask words (2173 is odd)
    prob, spec = LC.ALL[name]()
    three = np.concatenate([prob, np.zeros_like(prob), prob[:, ::-1].copy()])
    same(call(dm, three, spec['threshold'], spec['rf'], spec['k']), LO.lesion_table(three, spec['threshold'], spec['rf'], spec['k']))
    check_case(dm, name, mask=False)


def test_most_components_and_truncation(dm):
    rows, totals, masks = check_case(dm, 'checkerboard', max_lesions=16)
    assert totals.tolist() == [480] and len(rows) == 16 and rows['x0'].tolist() == list(range(0, 32, 2))
    assert int((masks == 255).sum()) == 480
    rows, totals, _ = check_case(dm, 'checkerboard', max_lesions=512)
    assert len(rows) == 480 and rows['row'].tolist() == list(range(480))
    check_case(dm, 'checkerboard', max_lesions=1)


def test_area_filter(dm):
    rows, totals, masks = check_case(dm, 'areas', min_area=5)
    assert totals.tolist() == [2] and rows['area'].tolist() == [9, 100]
    assert int((masks == 255).sum()) == 109
    assert check_case(dm, 'areas')[0]['area'].tolist() == [9, 1, 100, 4]
    assert check_case(dm, 'areas', min_area=101)[1].tolist() == [0]


def test_empty_and_full(dm):
    rows, totals, masks = check_case(dm, 'empty_and_full')
    assert totals.tolist() == [0, 1] and len(rows) == 1
    assert tuple(rows[0][f] for f in ('slice', 'area', 'x0', 'y0', 'x1', 'y1')) == (1, 40 * 72, 0, 0, 71, 39)
    assert not masks[0].any() and (masks[1] == 255).all()


def test_argument_errors_launch_nothing(dm):
    from dnncancerannotator_amd._lib import DnncaError
    prob, spec = LC.areas()
    dm.sync()
    dm.profile_reset()
    dm.profile_enable(1)
    try:
        three = np.repeat(prob, 4, axis=0)
        for kw, word in [(dict(batch=0), 'batch'), (dict(prob=three), 'batch'), (dict(k=0), 'filter_size'), (dict(k=16), 'filter_size'),
                         (dict(threshold=float('nan')), 'threshold'), (dict(max_lesions=0), 'max_lesions'),
                         (dict(rows_short=1), 'rows'), (dict(mask_short=1), 'mask'), (dict(rf=0.0), 'resize'),
                         (dict(min_area=-1), 'min_area')]:
            kw = dict(dict(prob=prob, threshold=0.5, rf=1.0, k=1), **kw)
            with pytest.raises(DnncaError) as e:
                call(dm, kw.pop('prob'), **kw)
            assert e.value.code == -1 and word in str(e.value), (kw, str(e.value))
        assert dm.profile() == []
    finally:
        dm.profile_enable(0)
        dm.profile_reset()


def _model(gpu, dtype):
    from oracle import unet_oracle as OU
    opts = dict(UNET, n_filters_first=32) if dtype == 'bf16' else UNET
    m = gpu.DeviceModel('unet', 2, 32, 48, 3, dtype=dtype, **opts)
    spec = OU.ModelSpec('unet', 2, **opts)
    m.set_params(OU.flatten(spec, OU.init_params(spec, seed=5)))
    x, _ = OU.synthetic_batch(3, 32, 48, 2, seed_x=7, seed_y=8)
    return m, x


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_last_forward_table_plan_and_nothing_else_changes(gpu, dtype):
    """forward(return_prob=True), then lesion_table() on the device copy and lesion_table(prob=that array): equal tables, equal to
    the oracle on those probabilities; parameters, state and the last forward's probabilities are bit-identical across the calls; a
    region_confusion_slices after them returns what it returned before; the dry plan lists the launches the profile shows"""
    m, x = _model(gpu, dtype)
    try:
        prob = m.forward(x, training=False)[..., 0]
        thr = float(np.median(prob))
        y = (x[..., 0] > 0.5).astype(np.float32)
        spec = ([thr], 0.3, 0.5, 3)
        before = m.region_confusion_slices(y, [spec])
        p0, s0 = m.get_params(), m.get_state()
        kw = dict(threshold=thr, resize_factor=0.5, filter_size=3, min_area=2, max_lesions=64)
        m.profile_reset()
        m.profile_enable(1)
        dev = m.lesion_table(batch=3, **kw)
        live = {name: n for name, n, _, _, _ in m.profile()}
        m.profile_enable(0)
        m.profile_reset()
        plan = [r[0] for r in m.plan(mode='lesion', batch=3)]
        assert {k: plan.count(k) for k in plan} == live
        assert plan == ['region_prep', 'region_open', 'region_ccl_tile', 'region_ccl_merge', 'region_ccl_compress', 'region_sizes',
                        'lesion_scan', 'lesion_stats', 'lesion_mask']
        host = m.lesion_table(prob=prob, **kw)
        same(dev, host)
        same(dev, LO.lesion_table(prob, thr, 0.5, 3, 2, 64))
        assert dev[1].sum() > 0
        assert m.lesion_table(batch=3, mask=False, **kw)[2] is None
        assert 'lesion_mask' not in [r[0] for r in m.plan(mode='lesion', batch=3)]
        assert m.last_prob(3).tobytes() == prob.tobytes()
        assert m.get_params().tobytes() == p0.tobytes() and m.get_state().tobytes() == s0.tobytes()
        assert m.region_confusion_slices(y, [spec]).tolist() == before.tolist()
        # the train / eval / forward plans do not know the new launches
        for mode in ('train', 'eval', 'forward'):
            assert not [r[0] for r in m.plan(mode=mode) if r[0].startswith('lesion')]
    finally:
        m.close()


def test_cli_predict_end_to_end(gpu, tmp_path):
    """train three steps on synthetic:64x64x2, then `predict --export_images`: the file set, CSVs that parse, and every mask.png is
    the mask lesion_table returns for that slice"""
    import yaml
    from dnncancerannotator_amd import engine
    from dnncancerannotator_amd.runs.train import make_dataset
    cfg = {'model': 'UNetAnnotator', 'model_options': UNET,
           'deploy_options': {'optimizer': 'adam', 'enable_multigpu': False},
           'data_options': {'train': {'batch_size': 2}, 'eval': {'batch_size': 2}}}
    cfg_path, run, out = str(tmp_path / 'cfg.yaml'), str(tmp_path / 'run'), str(tmp_path / 'out')
    with open(cfg_path, 'w') as f:
        yaml.safe_dump(cfg, f)
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, '-m', 'dnncancerannotator_amd']
    r = subprocess.run(base + ['train', '--config', cfg_path, '--save_path', run, '--data_path', 'synthetic:64x64x2', '--max_steps', '3',
                               '--save_freq', '3'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    # a threshold that leaves something to find in an almost untrained model: the median probability of the first batch
    e = engine.TFKerasModel(cfg)
    ds = make_dataset(['synthetic:64x64x2'], cfg['data_options']['eval'], training=False, include_meta=True, labels=False)
    e._build(ds)
    e.load(e.get_ckpts(os.path.join(run, 'checkpoints'))[3])
    batches = list(ds)
    thr = float(np.median(e.device_model.forward(batches[0][0], training=False)))
    args = ['--threshold', repr(thr), '--filter_size', '3', '--min_area', '4', '--max_lesions', '32']
    r = subprocess.run(base + ['predict', '--save_path', run, '--data_path', 'synthetic:64x64x2', '--output', out, '--export_images'] + args,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert files == ['lesions.csv', 'slices.csv'] + ['synthetic:64x64x2/%02d/mask.png' % i for i in range(4)]
    with open(os.path.join(out, 'lesions.csv'), newline='') as f:
        lesions = list(csv.DictReader(f))
    with open(os.path.join(out, 'slices.csv'), newline='') as f:
        slices = list(csv.DictReader(f))
    assert [s['slice'] for s in slices] == ['0', '1', '2', '3'] and all(s['exam'] == 'synthetic:64x64x2' for s in slices)
    n_rows = 0
    for bi, (x, paths, ids) in enumerate(batches):
        e.device_model.forward(x, training=False, return_prob=False)
        rows, totals, masks = e.device_model.lesion_table(batch=len(x), threshold=thr, filter_size=3, min_area=4, max_lesions=32)
        for b, k in enumerate(ids):
            with open(os.path.join(out, 'synthetic:64x64x2', '%02d' % k, 'mask.png'), 'rb') as f:
                assert np.array_equal(decode_png(f.read())[..., 0], masks[b])
            assert int(slices[k]['n_lesions']) == totals[b] and int(slices[k]['truncated']) == int(totals[b] > 32)
            mine = rows[rows['slice'] == b]
            got = [l for l in lesions if int(l['slice']) == k]
            assert [int(l['area_px']) for l in got] == mine['area'].tolist()
            assert [float(l['centroid_x']) for l in got] == [int(r['sum_x']) / int(r['area']) for r in mine]
            n_rows += len(mine)
    assert n_rows == len(lesions) and n_rows > 0
    e.device_model.close()
