"""-m gpu: the detection map through the C ABI (kernels_detect.hip: det_init, det_peak, det_seed, det_ccl_tile, det_ccl_merge,
det_area, det_commit; dnnca_detection_map) against tests/detection_oracle.py.

Everything is exact: the map D, the candidate rows and the slice records must EQUAL the oracle's bit for bit, and two runs must be
bit-identical.  Host outputs carry guard regions pre-filled with a sentinel.

Planes: 1 x 1, 32 x 32 (one LDS tile), 33 x 65 (one pixel over), 40 x 24 (ragged edges), 65 x 130 (three tiles across, 8450 pixels:
no multiple of 4, so det_peak and det_init take their scalar arm; 32 x 32 and 40 x 24 take the float4 arm).  Batches of 1 and 2 on a
model of max_batch 3."""

import ctypes as C

import numpy as np
import pytest

import detection_oracle as DO
from test_lesion_gpu import UNET
from test_tta_gpu import SENTINEL, drawn, guarded, random_weights, same, unguard

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (32, 32), (33, 65), (40, 24), (65, 130)]
KERNELS = {'det_init', 'det_peak', 'det_seed', 'det_ccl_tile', 'det_ccl_merge', 'det_area', 'det_commit'}


@pytest.fixture(scope='module')
def dm(gpu):
    m = gpu.DeviceModel('unet', 1, 64, 64, 3, **UNET)
    random_weights(m, 41)
    yield m
    m.close()


def raw(n_items, dtype, extra=4):
    return np.full((n_items + extra) * dtype.itemsize, SENTINEL, np.uint8).view(dtype)


def det_call(dm, prob, **cfg):
    """dnnca_detection_map on host planes with guarded outputs -> (D, rows, slices)"""
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import check, fptr
    prob = np.ascontiguousarray(prob, np.float32)
    B, h, w = prob.shape
    c = dict(min_confidence=0.1, factor=0.4, max_candidates=5, min_area=10, rounds=16)
    c.update(cfg)
    cs = _lib.DetectionCfg(c['min_confidence'], c['factor'], c['max_candidates'], c['min_area'], c['rounds'])
    N = c['max_candidates']
    out, rows, slices, n = guarded(prob.size), raw(B * N, DO.ROW_DTYPE), raw(B, DO.SLICE_DTYPE), C.c_int64(-1)
    check(dm.lib.dnnca_detection_map(dm.handle, fptr(prob), B, h, w, C.byref(cs), fptr(out), rows.ctypes.data_as(C.POINTER(_lib.DetectionRow)),
                                     C.byref(n), slices.ctypes.data_as(C.POINTER(_lib.DetectionSlice))))
    assert 0 <= n.value <= B * N
    assert (rows[n.value:].view(np.uint8) == SENTINEL).all() and (slices[B:].view(np.uint8) == SENTINEL).all(), 'written past an output'
    return unguard(out, prob.size, prob.shape), rows[:n.value].copy(), slices[:B].copy()


def check_case(dm, prob, what, **cfg):
    got = det_call(dm, prob, **cfg)
    want = DO.detection_map(prob, **cfg)
    assert got[2].tolist() == want[2].tolist(), '%s: slice records %s, oracle %s' % (what, got[2].tolist(), want[2].tolist())
    assert got[1].tolist() == want[1].tolist(), '%s: rows' % what
    assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes(), what
    assert got[0].tobytes() == want[0].tobytes(), '%s: %d pixels of the map differ' % (what, int((got[0] != want[0]).sum()))
    again = det_call(dm, prob, **cfg)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), what + ': differs from run to run'
    return got


# ---- the planes ------------------------------------------------------------------------------------------------------------------
def spiral(H, W):
    """a one-pixel-wide rectangular spiral from the corner inwards: rings two pixels apart, each opened below its first corner and
    bridged to the next one"""
    m = np.zeros((H, W), bool)
    for k in range(0, (min(H, W) + 1) // 2, 2):
        m[k, k:W - k] = m[H - 1 - k, k:W - k] = True
        m[k:H - k, k] = m[k:H - k, W - 1 - k] = True
        if H - 2 * k > 3 and W - 2 * k > 3:
            m[k + 1, k] = False
            m[k + 2, k + 1] = True
    return m


def background(shape, seed, top=0.05):
    return (drawn(shape, seed) * top).astype(np.float32)


def bumps(shape, seed, n=6):
    """a smooth plane of n Gaussian bumps of different heights on a low background"""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    p = background(shape, seed + 1)
    for b in range(B):
        for _ in range(n):
            cy, cx, s, a = rng.random() * H, rng.random() * W, 1.5 + 4 * rng.random(), 0.15 + 0.85 * rng.random()
            p[b] = np.maximum(p[b], (a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))).astype(np.float32))
    return p


def case_spiral(H, W):
    p = background((2, H, W), 1)
    p[0][spiral(H, W)] = 0.8
    p[1][spiral(H, W)[::-1, ::-1]] = 0.6          # the same path entered from the far end: its lowest index is not the path's start
    return p, dict(min_area=1)


def case_two_plateaus(H, W):
    p = background((1, H, W), 2)
    p[0, H // 2:H // 2 + 4, W // 2:W // 2 + 5] = 0.7      # the later one in index order
    p[0, 0:3, 0:4] = 0.7
    p[0, H // 4:H // 4 + 1, W - 2:] = 0.5
    return p, dict(min_area=1)


def case_shoulder(H, W):
    p = background((1, H, W), 3)
    p[0, H // 3:H // 3 + 9, W // 3:W // 3 + 36] = 0.3     # crosses a tile border where the plane has one
    p[0, H // 3 + 2:H // 3 + 5, W // 3 + 3:W // 3 + 7] = 0.9
    return p, dict(min_area=1)


def case_factor_one(H, W):
    p = bumps((2, H, W), 4)
    p[0, H // 2:H // 2 + 3, 0:7] = 1.0                     # above every bump
    return p, dict(factor=1.0, min_area=1, rounds=8)


def case_small_region(H, W):
    p = background((1, H, W), 5)
    p[0, 1:2, 1:4] = 0.9                                   # three pixels: dropped, the round is spent
    p[0, H // 2:H // 2 + 6, W // 2:W // 2 + 6] = 0.6
    return p, dict(min_area=10)


def case_max_candidates(H, W):
    return bumps((2, H, W), 6, n=9), dict(max_candidates=2, min_area=1, rounds=4)


def case_rounds_exhausted(H, W):
    p = background((1, H, W), 7)
    p[0, ::3, ::3] = 0.2 + 0.6 * drawn(p[0, ::3, ::3].shape, 8)      # isolated pixels, all below min_area
    return p, dict(max_candidates=2, min_area=5, rounds=3)


def case_rounds_exactly_used(H, W):
    p = np.zeros((1, H, W), np.float32)
    for i, v in enumerate((0.9, 0.5, 0.7)):
        p[0, (5 * i) % H, (7 * i + 2) % W] = v
    n = int((p > 0).sum())                                 # 3 isolated pixels (1 on a 1 x 1 plane): every round spent, nothing left
    return p, dict(max_candidates=n, min_area=5, rounds=n)


def case_all_below(H, W):
    return background((2, H, W), 9, top=0.0999), dict()


def case_odd_values(H, W):
    p = bumps((2, H, W), 10)
    q = p.reshape(2, -1)
    rng = np.random.default_rng(11)
    for v in (np.nan, -0.5, -0.0, 1.5, 7.0, np.inf, -np.inf):
        q[rng.integers(0, 2, 5), rng.integers(0, H * W, 5)] = v
    for i, v in enumerate((1.0, 2.0, 1.5)):               # one plateau at the clamp
        p[1, H // 2:H // 2 + 2, W // 3 + i:W // 3 + i + 1] = v
    return p, dict(min_area=1)


def case_mixed_batch(H, W):
    p = np.zeros((2, H, W), np.float32)
    p[0, H // 2:H // 2 + 4, W // 2:W // 2 + 4] = 0.8      # done after the first round
    p[1] = background((H, W), 12)
    p[1, ::2, ::2] = 0.15 + 0.8 * drawn(p[1, ::2, ::2].shape, 13)   # isolated pixels: every round is needed and spent
    return p, dict(min_area=2, rounds=16)


def case_smooth(H, W):
    return bumps((2, H, W), 14), dict()


CASES = {f.__name__[5:]: f for f in (case_spiral, case_two_plateaus, case_shoulder, case_factor_one, case_small_region,
                                     case_max_candidates, case_rounds_exhausted, case_rounds_exactly_used, case_all_below,
                                     case_odd_values, case_mixed_batch, case_smooth)}


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('name', sorted(CASES))
def test_detection_map_equals_the_oracle(dm, name, shape):
    prob, cfg = CASES[name](*shape)
    D, rows, slices = check_case(dm, prob, '%s %s' % (name, shape), **cfg)
    big = shape[0] >= 32
    if name == 'spiral' and big:
        assert slices['candidates'].tolist() == [1, 1] and rows['area'].tolist() == [int(spiral(*shape).sum())] * 2
        assert rows['seed'][0] == 0 and rows['confidence'].tolist() == [np.float32(0.8), np.float32(0.6)]
    if name == 'two_plateaus' and big:
        assert rows['seed'][:2].tolist() == [0, (shape[0] // 2) * shape[1] + shape[1] // 2] and rows['area'][:2].tolist() == [12, 20]
        assert (rows['confidence'][:2] == np.float32(0.7)).all()
    if name == 'shoulder' and big:
        assert rows['area'][:2].tolist() == [12, int((prob[0] == np.float32(0.3)).sum())]
        assert rows['confidence'][:2].tolist() == [np.float32(0.9), np.float32(0.3)]
    if name == 'factor_one':
        assert all(int((D[r['slice']] == r['confidence']).sum()) >= r['area'] for r in rows)
        if big:
            assert rows['area'][0] == 21
    if name == 'small_region' and big:
        assert slices.tolist() == [(1, 2, 1, 0)] and rows['area'].tolist() == [36] and not D[0, 1, 1:4].any()
    if name == 'max_candidates' and big:
        assert slices['candidates'].tolist() == [2, 2] and not slices['exhausted'].any()
    if name == 'rounds_exhausted' and big:
        assert slices.tolist() == [(0, 3, 3, 1)] and not D.any()
    if name == 'rounds_exactly_used':
        n = int((prob > 0).sum())
        assert slices.tolist() == [(0, n, n, 0)] and not D.any()
    if name == 'all_below':
        assert slices.tolist() == [(0, 0, 0, 0)] * 2 and not D.any() and D.tobytes() == bytes(D.nbytes) and not len(rows)
    if name == 'odd_values':
        assert np.isfinite(D).all() and D.min() >= 0 and D.max() <= 1
        if big:
            assert rows['confidence'][rows['slice'] == 1][0] == np.float32(1)
    if name == 'mixed_batch' and big:
        assert slices[0].tolist() == (1, 1, 0, 0) and slices[1]['rounds'] == 16 and slices[1]['exhausted'] == 1
    for r in rows:                                          # a candidate's pixels carry its confidence, the seed among them
        assert D[r['slice']].reshape(-1)[r['seed']] == r['confidence']


def test_candidates_never_overlap_and_cover_the_map(dm):
    prob = bumps((3, 65, 130), 20, n=12)
    D, rows, slices = check_case(dm, prob, 'batch of max_batch', min_area=3, max_candidates=8, rounds=24)
    assert len(rows) == int(slices['candidates'].sum()) and len(rows) > 6
    assert int((D > 0).sum()) == int(rows['area'].sum())
    for b in range(3):
        conf = rows['confidence'][rows['slice'] == b]
        assert (np.diff(conf) <= 0).all() and rows['number'][rows['slice'] == b].tolist() == list(range(len(conf)))


def test_the_python_methods(dm):
    prob = bumps((2, 33, 65), 21)
    got = dm.detection_map_of(prob, min_area=4, max_candidates=3)
    want = DO.detection_map(prob, min_area=4, max_candidates=3)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and got[1].dtype == DO.ROW_DTYPE and got[2].dtype == DO.SLICE_DTYPE


# ---- 2. in place -----------------------------------------------------------------------------------------------------------------
def test_in_place_on_the_last_forward(dm):
    x = drawn((3, 64, 64, 1), 22)
    y = (drawn((3, 64, 64), 23) < 0.2).astype(np.float32)
    cfg = dict(min_confidence=0.05, factor=0.9, min_area=2, max_candidates=6, rounds=12)
    p0, s0 = dm.get_params(), dm.get_state()
    first = dm.forward(x, training=False)
    # a running lesion_table_linked chain: its carry must survive the detection calls
    dm.forward(x, training=False, return_prob=False)
    before = dm.last_prob(3)
    thr = float(np.median(before))
    chain = dm.lesion_table_linked(prob=before[:2], continues=[0, 1], threshold=thr, filter_size=1)
    host = dm.detection_map_of(before, **cfg)
    same(dm.last_prob(3), before)                                            # the host-plane call left the model's plane alone
    want = DO.detection_map(before, **cfg)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(host, want)) and len(host[1]) > 0
    rows, slices = dm.detection_map(3, **cfg)
    same(dm.last_prob(3), host[0])
    assert rows.tobytes() == host[1].tobytes() and slices.tobytes() == host[2].tobytes()
    # the table call afterwards reads the map: its prediction rows carry the confidences
    table = dict(continues=[0, 0, 0], threshold=cfg['min_confidence'], filter_size=1, resize_factor=1.0, min_area=0)
    pred = dm.lesion_table_matched(y, **table)[0]
    assert pred.tobytes() == dm.lesion_table_matched(y, prob=host[0], **table)[0].tobytes() and len(pred)
    for b in range(3):                   # touching candidates join with the larger confidence; the strongest one is always a row's
        conf, got = rows['confidence'][rows['slice'] == b], pred['max_prob'][pred['slice'] == b]
        assert set(got.tolist()) <= set(conf.tolist()) and (not len(conf) or got.max() == conf.max())
    assert int(pred['area'].sum()) == int(rows['area'].sum())
    # the chain goes on from its own carry as if nothing had happened
    nxt = dm.lesion_table_linked(prob=before[2:], continues=[1], threshold=thr, filter_size=1)
    whole = dm.lesion_table_linked(prob=before, continues=[0, 1, 1], threshold=thr, filter_size=1)
    assert nxt[3]['row_prev'].tolist() == whole[3][whole[3]['slice'] == 2]['row_prev'].tolist() and len(chain[0])
    assert nxt[3]['overlap'].tolist() == whole[3][whole[3]['slice'] == 2]['overlap'].tolist()
    # two slices of three with out_hw: a copy of the map; the third slice stays
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import check, fptr
    dm.forward(x, training=False, return_prob=False)
    cs = _lib.DetectionCfg(cfg['min_confidence'], cfg['factor'], cfg['max_candidates'], cfg['min_area'], cfg['rounds'])
    out, r2, s2, n = guarded(2 * 4096), raw(12, DO.ROW_DTYPE), raw(2, DO.SLICE_DTYPE), C.c_int64(-1)
    check(dm.lib.dnnca_detection_map(dm.handle, None, 2, 64, 64, C.byref(cs), fptr(out), r2.ctypes.data_as(C.POINTER(_lib.DetectionRow)),
                                     C.byref(n), s2.ctypes.data_as(C.POINTER(_lib.DetectionSlice))))
    got = unguard(out, 2 * 4096, (2, 64, 64))
    same(got, host[0][:2])
    same(dm.last_prob(3)[:2], got)
    same(dm.last_prob(3)[2:], before[2:])
    assert dm.get_params().tobytes() == p0.tobytes() and dm.get_state().tobytes() == s0.tobytes()
    same(dm.forward(x, training=False), first)


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_touch_nothing(gpu):
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import fptr
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    try:
        random_weights(m, 24)
        lib = m.lib
        p = drawn((4, 16, 32), 25)
        x = drawn((2, 16, 16, 1), 26)
        bufs = [np.full(1 << 16, SENTINEL, np.uint8) for _ in range(3)]
        out = bufs[0].view(np.float32)
        rows, slices = bufs[1].ctypes.data_as(C.POINTER(_lib.DetectionRow)), bufs[2].ctypes.data_as(C.POINTER(_lib.DetectionSlice))
        n = C.c_int64(-7)
        nan = float('nan')

        def det(prob=fptr(p), batch=2, h=16, w=32, cfg=(0.1, 0.4, 5, 10, 16), out=fptr(out), rows=rows, n_rows=C.byref(n), slices=slices):
            cs = None if cfg is None else C.byref(_lib.DetectionCfg(*cfg))
            return lib.dnnca_detection_map(m.handle, prob, batch, h, w, cs, out, rows, n_rows, slices)
        einval = [('batch 0', lambda: det(batch=0)), ('batch max_batch + 1', lambda: det(batch=4)),
                  ('min_confidence 0.0009', lambda: det(cfg=(0.0009, 0.4, 5, 10, 16))), ('min_confidence 1.01', lambda: det(cfg=(1.01, 0.4, 5, 10, 16))),
                  ('min_confidence NaN', lambda: det(cfg=(nan, 0.4, 5, 10, 16))), ('factor 0.009', lambda: det(cfg=(0.1, 0.009, 5, 10, 16))),
                  ('factor 1.01', lambda: det(cfg=(0.1, 1.01, 5, 10, 16))), ('factor NaN', lambda: det(cfg=(0.1, nan, 5, 10, 16))),
                  ('factor 0', lambda: det(cfg=(0.1, 0.0, 5, 10, 16))), ('0 candidates', lambda: det(cfg=(0.1, 0.4, 0, 10, 16))),
                  ('65 candidates', lambda: det(cfg=(0.1, 0.4, 65, 10, 80))), ('min_area 0', lambda: det(cfg=(0.1, 0.4, 5, 0, 16))),
                  ('min_area 2^30 + 1', lambda: det(cfg=(0.1, 0.4, 5, (1 << 30) + 1, 16))),
                  ('rounds below max_candidates', lambda: det(cfg=(0.1, 0.4, 5, 10, 4))), ('257 rounds', lambda: det(cfg=(0.1, 0.4, 5, 10, 257))),
                  ('null cfg', lambda: det(cfg=None)), ('null rows', lambda: det(rows=None)), ('null slices', lambda: det(slices=None)),
                  ('null n_rows', lambda: det(n_rows=None)), ('host plane without out', lambda: det(out=None)),
                  ('empty plane', lambda: det(h=0)), ('2^31 pixels', lambda: det(h=65536, w=32768)),
                  ('the model\'s plane at another size', lambda: det(prob=None, h=16, w=32))]
        estate = [('in place', lambda b: det(prob=None, batch=b, h=0, w=0)), ('in place, size given', lambda b: det(prob=None, batch=b, h=16, w=16))]

        def refused(cases, code, *a):
            m.sync()
            m.profile_reset()
            m.profile_enable(1)
            try:
                for what, call in cases:
                    assert call(*a) == code, what
                    assert lib.dnnca_last_error()
                    assert all((b == SENTINEL).all() for b in bufs) and n.value == -7, what
                assert m.profile() == []
            finally:
                m.profile_enable(0)
                m.profile_reset()
        refused(einval, -1)                          # DNNCA_EINVAL
        refused(estate, -4, 1)                       # DNNCA_ESTATE: a fresh model has no probabilities
        m.forward(x, training=False, return_prob=False)
        before = m.last_prob(2)
        refused(estate, -4, 3)                       # the last forward had two slices
        refused(einval, -1)
        same(m.last_prob(2), before)
    finally:
        m.close()


# ---- 4. launches -----------------------------------------------------------------------------------------------------------------
def test_launches_and_untouched_plans(dm):
    before = {mode: dm.plan(variants=True, mode=mode) for mode in ('train', 'eval', 'forward', 'lesion', 'lesion_matched')}
    x = drawn((3, 64, 64, 1), 27)
    dm.forward(x, training=False, return_prob=False)
    prob = dm.last_prob(3)

    def profiled(call):
        dm.sync()
        dm.profile_reset()
        dm.profile_enable(1)
        try:
            call()
            return {name: n for name, n, _, _, _ in dm.profile()}
        finally:
            dm.profile_enable(0)
            dm.profile_reset()
    R = 7
    want = {'det_init': 1, 'det_peak': R + 1, 'det_seed': R + 1, 'det_ccl_tile': R, 'det_ccl_merge': R, 'det_area': R, 'det_commit': R}
    assert profiled(lambda: dm.detection_map_of(prob, rounds=R)) == want
    assert profiled(lambda: dm.detection_map(3, rounds=R)) == want
    plan = dm.plan(mode='detection', batch=2)
    assert {k: sum(1 for r in plan if r[0] == k) for k in KERNELS} == want          # the parameters of the last call
    for mode, rec in before.items():
        assert dm.plan(variants=True, mode=mode) == rec
        assert not [r[0] for r in rec if r[0] in KERNELS]


# ---- 5. the command line ---------------------------------------------------------------------------------------------------------
def _run_at_64(tmp_path, labels):
    """a run directory with one checkpoint of a small U-Net on the synthetic source at 64 x 64 (4 slices in batches of 2)"""
    import os
    import yaml
    from dnncancerannotator_amd import engine
    from dnncancerannotator_amd.runs.train import make_dataset
    cfg = {'model': 'UNetAnnotator', 'model_options': UNET, 'deploy_options': {'optimizer': 'adam', 'enable_multigpu': False},
           'data_options': {'eval': {'batch_size': 2}}}
    run, data = str(tmp_path / 'run'), 'synthetic:64x64x2'
    e = engine.TFKerasModel(cfg)
    ds = make_dataset([data], cfg['data_options']['eval'], training=False, include_meta=True, labels=labels)
    e._build(ds)
    random_weights(e.device_model, 16)
    e.current_step = 1
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    with open(os.path.join(run, 'options.yaml'), 'w') as f:
        yaml.safe_dump({'config': cfg}, f)
    return e.device_model, list(ds), run, data


DET_FLAGS = ['--detection_factor', '0.95', '--detection_min_confidence', '0.2', '--detection_min_area', '2',
             '--detection_max_candidates', '6', '--detection_rounds', '12']
DET_CFG = dict(min_confidence=0.2, factor=0.95, max_candidates=6, min_area=2, rounds=12)


def test_cli_evaluate_detection_equals_casewise_on_the_oracles_map(gpu, tmp_path):
    from dnncancerannotator_amd import __main__ as cli, casewise as CW
    from test_spread_gpu import _files
    m, batches, run, data = _run_at_64(tmp_path, labels=True)
    base = ['evaluate', '--save_path', run, '--data_path', data, '--export_csv', '--skip_visualization', '--tag', 't']
    runs = {'plain': [], 'det': ['--detection'] + DET_FLAGS,
            'views': ['--detection', '--tta', 'flips', '--temperature', '1.7', '--detection_iou', '0.05'] + DET_FLAGS}
    files = {}
    for name, flags in runs.items():
        assert cli.main(base + ['--export_path', str(tmp_path / name)] + flags) == 0
        files[name] = _files(str(tmp_path / name))
    new = ['t/detection_candidates.csv', 't/detection_cases.csv', 't/detection_froc.csv', 't/detection_results.csv']
    assert sorted(set(files['det']) - set(files['plain'])) == new and files['plain']
    assert all(files['det'][k] == v for k, v in files['plain'].items())
    kw = CW.detection_table_args(DET_CFG)
    for name, forward, T, iou in (('det', lambda x: m.forward(x, training=False), None, 0.10), ('views', lambda x: m.forward_tta(x, 0x0F), 1.7, 0.05)):
        recs, exhausted, last = [], 0, None
        for x, y, paths, ids in batches:
            prob = forward(x)[..., 0]
            prob = prob if T is None else m.scale_temperature(T, len(x), prob=prob)
            D, _, srecs = DO.detection_map(prob, **DET_CFG)
            exhausted += int(srecs['exhausted'].sum())
            cont = []
            for p, k in zip(paths, ids):
                cont.append(last is not None and p == last[0] and int(k) == last[1] + 1)
                last = (p, int(k))
            out = m.lesion_table_matched(y, prob=D, continues=cont, **kw)
            of = lambda a, b, f: [tuple(int(v[g]) for g in f) for v in a[a['slice'] == b]]
            for b in range(len(x)):
                recs.append((paths[b], int(ids[b]), out[0][out[0]['slice'] == b], out[1][b], of(out[3], b, ('row_prev', 'row', 'overlap')),
                             out[4][out[4]['slice'] == b], out[5][b], of(out[6], b, ('row_prev', 'row', 'overlap')),
                             of(out[7], b, ('row_true', 'row', 'overlap'))))
        exam = recs[0][0]
        assert all(r[0] == exam for r in recs)                              # the synthetic source is one exam
        ps, ts = [r[1:4] for r in recs], [(r[1], r[5], r[6]) for r in recs]
        case, lines = CW.detection_match(exam, ts, ps, CW.link_lesions(exam, ts, [r[7] for r in recs]),
                                         CW.link_lesions(exam, ps, [r[4] for r in recs]), [r[8] for r in recs], iou=iou)
        result, froc = CW.detection_summary([case], exhausted)
        got = files[name]
        assert got['t/detection_results.csv'].decode() == CW.plain_csv(['step'] + CW.DETECTION_RESULT_COLUMNS, [[1] + result]), name
        assert got['t/detection_froc.csv'].decode() == CW.plain_csv(['step'] + CW.DETECTION_FROC_COLUMNS, [[1] + l for l in froc]), name
        assert got['t/detection_cases.csv'].decode() == CW.plain_csv(['step'] + CW.DETECTION_CASE_COLUMNS, [[1] + CW.detection_case_values(case)]), name
        assert got['t/detection_candidates.csv'].decode() == CW.plain_csv(['step'] + CW.DETECTION_CANDIDATE_COLUMNS, [[1] + l for l in lines]), name
        assert len(lines) > 0, 'the drawn model gives no candidate: the case checks nothing'
    assert files['views']['t/detection_candidates.csv'] != files['det']['t/detection_candidates.csv']
    m.close()


def test_cli_predict_detection_map(gpu, tmp_path):
    from dnncancerannotator_amd import __main__ as cli, casewise as CW
    from test_spread_gpu import _files
    m, batches, run, data = _run_at_64(tmp_path, labels=False)
    thr = float(np.median(m.forward(batches[0][0], training=False)))
    base = ['predict', '--save_path', run, '--data_path', data, '--threshold', repr(thr), '--filter_size', '1', '--link_slices',
            '--export_images']
    texts = {}
    for name, flags in (('bare', []), ('det', ['--detection_map'] + DET_FLAGS)):
        assert cli.main(base + ['--output', str(tmp_path / name)] + flags) == 0
        texts[name] = _files(str(tmp_path / name))
    new = sorted(set(texts['det']) - set(texts['bare']))
    assert [f for f in new if f.endswith('.csv')] == ['candidates.csv', 'exam_candidates.csv', 'slice_candidates.csv'] and len(new) == 3 + 4
    assert all(texts['det'][k] == v for k, v in texts['bare'].items())       # lesions.csv, the exam tables and the masks: byte for byte
    lines, slices, pngs = [], [], {}
    for x, paths, ids in batches:
        D, _, srecs = DO.detection_map(m.forward(x, training=False)[..., 0], **DET_CFG)
        rows, _, _ = m.lesion_table(prob=D, mask=False, **CW.detection_table_args(DET_CFG))
        for b in range(len(x)):
            lines += [CW.candidate_values(paths[b], ids[b], r) for r in rows[rows['slice'] == b]]
            slices.append([paths[b], int(ids[b])] + list(srecs[b].tolist()))
            pngs[CW.detection_path('', CW.tag_of(paths[b], ids[b])).lstrip('/')] = CW.encode_png(CW.detection_image(D[b]))
    assert texts['det']['candidates.csv'].decode() == CW.plain_csv(CW.CANDIDATE_COLUMNS, lines) and lines
    assert texts['det']['slice_candidates.csv'].decode() == CW.plain_csv(CW.SLICE_CANDIDATE_COLUMNS, slices)
    assert {k: v for k, v in texts['det'].items() if k.endswith('detection.png')} == pngs
    assert len(texts['det']['exam_candidates.csv'].decode().splitlines()) > 1
    m.close()
