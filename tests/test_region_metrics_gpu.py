"""-m gpu: region-based metrics on the device (kernels_region.hip; dnnca_region_confusion_of / dnnca_region_confusion /
dnnca_eval_region_*).  Integer counts, so the device must EQUAL the numpy oracle (tests/region_oracle.py) and, on the reference's
scenarios, the answers known by construction; adversarial shapes stress the union-find labelling (long chains, diagonal contacts,
borders, every tile size) and the opening; the engine's evaluation gives identical rows on the staged and the per-batch path."""

import csv
import os

import numpy as np
import pytest

import region_cases as RC
import region_oracle as O

pytestmark = pytest.mark.gpu

UNET = dict(n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')


@pytest.fixture(scope='module')
def dm(gpu):
    m = gpu.DeviceModel('unet', 1, 16, 16, 1, **UNET)
    yield m
    m.close()


def check(dm, prob, y, thr, iou=0.3, rf=1.0, k=5, expected=None):
    got = dm.region_confusion_of(prob, y, (thr, iou, rf, k))
    want = O.region_counts(prob, y, thr, iou, rf, k)
    assert got.tolist() == want.tolist(), (rf, k, got.tolist(), want.tolist())
    if expected is not None:
        assert [tuple(r) for r in got] == [expected] * len(np.atleast_1d(thr))
    return got


@pytest.mark.parametrize('rf', [1.0, 0.5])
@pytest.mark.parametrize('thr', [RC.THRESHOLDS_1, RC.THRESHOLDS_10], ids=['T1', 'T10'])
def test_reference_scenarios_known_counts(dm, rf, thr):
    for name, y, p, expected in RC.scenarios(seed=11):
        check(dm, p, y, thr, 0.3, rf, 5, expected)


@pytest.mark.parametrize('rf', [1.0, 0.5])
def test_random_graded_circles(dm, rf):
    for seed in (1, 2):
        y, p = RC.random_slices(seed, n=20)
        c = check(dm, p, y, RC.THRESHOLDS_10, 0.3, rf, 5)
        assert c[:, 0].sum() > 0 and c[:, 1].sum() > 0 and c[:, 3].sum() > 0
    # one spec with T thresholds = T specs of one threshold each (test_consistency_multithresholds)
    one = np.concatenate([dm.region_confusion_of(p, y, ([t], 0.3, rf, 5)) for t in RC.THRESHOLDS_10])
    assert one.tolist() == dm.region_confusion_of(p, y, (RC.THRESHOLDS_10, 0.3, rf, 5)).tolist()


def spiral(n):
    m = np.zeros((n, n), bool)
    y0, x0, y1, x1 = 0, 0, n - 1, n - 1
    while y0 <= y1 and x0 <= x1:
        m[y0, x0:x1 + 1] = m[y0:y1 + 1, x1] = m[y1, x0:x1 + 1] = True
        m[y0 + 2:y1 + 1, x0] = True
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
        if y0 <= y1:
            m[y0, x0 - 1] = False
    return m


def comb(h, w, tooth=1, gap=1):
    m = np.zeros((h, w), bool)
    m[h - 1, :] = True
    for x in range(0, w, tooth + gap):
        m[:, x:x + tooth] = True
    return m


def graded(rng, mask):
    return np.where(mask, rng.uniform(0.05, 1.0, mask.shape), rng.uniform(0.0, 0.3, mask.shape)).astype(np.float32)


def test_all_positive_512(dm):
    y = np.ones((1, 512, 512), np.float32)
    for k in (1, 5):
        check(dm, y, y, [0.5], 0.3, 1.0, k, (1, 0, 1, 0))
    check(dm, y, y, RC.THRESHOLDS_10, 0.3, 0.5, 5, (1, 0, 1, 0))


@pytest.mark.parametrize('k', [1, 3, 5])
def test_adversarial_shapes(dm, k):
    rng = np.random.default_rng(k)
    cases = []
    s = spiral(127)
    cases.append((s[None], s[None]))                                           # one long chain through many tiles
    cases.append((spiral(255)[None], np.roll(spiral(255), 1, axis=1)[None]))
    c = comb(100, 130, 1, 1)
    cases.append((c[None], comb(100, 130, 3, 2)[None]))                        # teeth joined only at the bottom row
    d = np.zeros((64, 64), bool)
    d[::2, ::2] = True
    d[1::2, 1::2] = True                                                       # a checkerboard: every pixel its own component
    cases.append((d[None], np.roll(d, 1, axis=0)[None]))
    lines = np.zeros((80, 80), bool)
    lines[10, :] = lines[:, 40] = lines[60:63, :] = True                       # lines thinner than k vanish in the opening
    cases.append((lines[None], lines[None]))
    b = np.zeros((3, 70, 70), bool)
    b[0, :12, :12] = b[0, -9:, -20:] = b[1, :, :5] = b[2, 30:40, -3:] = True  # regions touching the border
    cases.append((b, np.roll(b, 2, axis=2)))
    ns = rng.random((2, 96, 160)) < 0.55                                       # non-square, random texture
    cases.append((ns, rng.random((2, 96, 160)) < 0.6))
    for y, p in cases:
        prob = graded(rng, p)
        for rf in (1.0, 0.5):
            check(dm, prob, y.astype(np.float32), RC.THRESHOLDS_10, 0.3, rf, k)
        check(dm, p.astype(np.float32), y.astype(np.float32), [0.5], 0.0, 1.0, k)


def test_batch_64_and_nonsquare(dm):
    rng = np.random.default_rng(9)
    y, p = RC.random_slices(3, n=64, size=96)
    check(dm, p, y, RC.THRESHOLDS_10, 0.3, 1.0, 5)
    check(dm, p, y, RC.THRESHOLDS_10, 0.3, 0.5, 5)
    y2 = (rng.random((5, 96, 160)) < 0.3).astype(np.float32)
    p2 = rng.random((5, 96, 160)).astype(np.float32)
    check(dm, p2, y2, np.linspace(0, 1, 64).astype(np.float32), 0.1, 0.75, 3)        # 64 thresholds: both mask words
    check(dm, p2, y2, [0.5], 0.5, 0.3, 5)


def test_bad_specs_are_rejected(dm):
    y = np.zeros((1, 16, 16), np.float32)
    for spec in [(np.linspace(0, 1, 65), 0.3, 1.0, 5), ([0.5], 1.0, 1.0, 5), ([0.5], -0.1, 1.0, 5), ([-0.5], 0.3, 1.0, 5),
                 ([np.nan], 0.3, 1.0, 5), ([0.5], 0.3, 0.0, 5), ([0.5], 0.3, 1.0, 0), ([0.5], 0.3, 1.0, 16), ([0.5], 0.3, 0.01, 5)]:
        with pytest.raises(Exception):
            dm.region_confusion_of(y, y, spec)


def test_region_confusion_of_the_last_eval_step(gpu):
    from oracle import unet_oracle as OU
    m = gpu.DeviceModel('unet', 1, 64, 64, 4, **UNET)
    try:
        spec = OU.ModelSpec('unet', 1, **UNET)
        m.set_params(OU.flatten(spec, OU.init_params(spec, seed=3)))
        x, y = OU.synthetic_batch(4, 64, 64, 1, seed_x=1, seed_y=2)
        out, prob = m.eval_step(x, y, m.loss_cfg(), return_prob=True)
        thr = np.quantile(prob, [0.3, 0.5, 0.7, 0.9]).astype(np.float32)
        got = m.region_confusion(y, (thr, 0.2, 1.0, 3))
        assert got.tolist() == O.region_counts(prob, y, thr, 0.2, 1.0, 3).tolist()
    finally:
        m.close()


def test_staged_eval_several_specs_share_the_label_plane(gpu):
    """dnnca_eval_region_begin .. _end over staged batches with three specs: two of one resized size (the label plane is labelled
    once for both, whatever their T) and one of another; every spec's counts equal the oracle on the eval probabilities"""
    from oracle import unet_oracle as OU
    m = gpu.DeviceModel('unet', 1, 64, 64, 4, **UNET)
    try:
        spec = OU.ModelSpec('unet', 1, **UNET)
        m.set_params(OU.flatten(spec, OU.init_params(spec, seed=3)))
        xs, ys = OU.synthetic_batch(12, 64, 64, 1, seed_x=5, seed_y=6)
        cfg = m.loss_cfg()
        probs = np.concatenate([m.eval_step(xs[i:i + 4], ys[i:i + 4], cfg, return_prob=True)[1] for i in range(0, 12, 4)])[..., 0]
        thr = np.quantile(probs, np.linspace(0.05, 0.95, 10)).astype(np.float32)
        specs = [((float(thr[5]),), 0.3, 0.5, 5), (tuple(float(t) for t in thr), 0.3, 0.5, 5), (tuple(float(t) for t in thr), 0.2, 1.0, 3)]
        ring = m.staging()
        ring.eval_begin(np.array([0.8], np.float32))
        ring.eval_region_begin(specs)
        for i in range(3):
            px, py = ring.upload(4 + i, xs[4 * i:4 * i + 4], ys[4 * i:4 * i + 4])
            ring.eval_step(4 + i, px, py, 4, cfg)
        got = ring.eval_region_end()
        ring.eval_end()
        for s, g in zip(specs, got):
            assert g.tolist() == O.region_counts(probs, ys, list(s[0]), s[1], s[2], s[3]).tolist(), s[1:]
    finally:
        m.close()


def _yaml_region_metrics():
    from test_region_metrics_host import METRICS_YAML_REGION
    extra = [{'RegionBasedTruePositives': dict(thresholds=RC.THRESHOLDS_10.tolist(), resize_factor=0.5, name='region/TP10')},
             {'RegionBasedFalsePositives': dict(thresholds=RC.THRESHOLDS_10.tolist(), resize_factor=0.5, name='region/FP10')},
             {'RegionBasedFalseNegatives': dict(thresholds=RC.THRESHOLDS_10.tolist(), resize_factor=1.0, morph_filter_size=3,
                                                name='region/FN10')}]
    return METRICS_YAML_REGION + extra


def test_engine_eval_staged_equals_per_batch_and_oracle(gpu, tmp_path, monkeypatch):
    from dnncancerannotator_amd import data, engine, region_metrics as R
    from oracle import unet_oracle as OU
    from test_region_metrics_host import METRICS_YAML_REGION
    pixel = [{'Precision': dict(thresholds=0.8, name='pixel/precision')}]

    def config(metrics):
        return {'model': 'UNetAnnotator', 'model_options': UNET,
                'deploy_options': {'optimizer': 'adam', 'enable_multigpu': False, 'metrics': metrics, 'region_metrics': 'device'}}
    cfg = config(pixel + _yaml_region_metrics())
    H = W = 64
    train = data.SyntheticDataset(4, H, W, 1, n_batches=2, seed=3)
    xv, yv = OU.synthetic_batch(12, H, W, 1, seed_x=5, seed_y=6)
    val = data.ArrayDataset(xv, yv, 4)
    # validation inside train (the training log takes scalar metrics: metrics.yaml's entries)
    res = engine.TFKerasModel(config(pixel + METRICS_YAML_REGION)).train(train, val_data=val, save_path=str(tmp_path / 'run'),
                                                                        max_steps=2, save_freq=2)
    assert 'val_region/recall' in res.history and 'val_region/F2-score' in res.history
    e = engine.TFKerasModel(cfg)
    rows_staged = e.eval(val, str(tmp_path / 'run'), tag='staged', export_csv=True)
    monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
    e2 = engine.TFKerasModel(cfg)
    rows_plain = e2.eval(val, str(tmp_path / 'run'), tag='plain', export_csv=True)
    monkeypatch.delenv('DNNCA_NO_FEEDER')
    (step, a), = rows_staged.items()
    b = rows_plain[step]
    names = [m.name for m in e.region_metrics]
    assert len(names) == 10 and all(n in a for n in names)
    for n in names:
        assert a[n] == b[n], n
    # the oracle on the probabilities of dnnca_forward, through the metric classes
    probs = np.concatenate([e2.device_model.forward(xv[i:i + 4]) for i in range(0, 12, 4)])[..., 0]
    for spec, ms in R.group_by_spec(e.region_metrics):
        c = O.region_counts(probs, yv, list(spec[0]), spec[1], spec[2], spec[3])
        for m in ms:
            ref = type(m)(**({'beta': m.beta} if hasattr(m, 'beta') else {}), thresholds=spec[0], IoU_threshold=m.IoU_threshold,
                          resize_factor=m.resize_factor, name=m.name)
            ref.morph_filter_size = m.morph_filter_size
            ref.add_counts(c)
            assert a[m.name] == ref.result(), m.name
    with open(os.path.join(str(tmp_path / 'run'), 'tfevents', 'staged', 'results.csv')) as f:
        header = next(csv.reader(f))
    assert [h for h in header if h.startswith('region/')] == [n for n in names]
