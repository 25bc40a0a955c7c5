"""-m gpu: per-step training metrics (deploy_options.train_metrics: device).  Every fused head kernel has a PROB variant that
stores the step's own sigmoid; one histogram launch counts it against the step's raw labels.  For each head path: exact counts
against numpy, probabilities against forward(training=True) and the float64 oracle, and a step whose loss is bit-identical with the
option off (the rest within the run-to-run noise of the float atomics that the step has with the option off too).  Then the
engine: feeder / no feeder / validation in between give the same per-step entries."""

import os

import numpy as np
import pytest

from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

UNET = dict(n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')
# the pixel metrics of configs/additionals/metrics.yaml:2-23 (302 thresholds)
PIXEL_METRICS = [{'Precision': {'thresholds': 0.80, 'name': 'pixel/precision'}},
                 {'Recall': {'thresholds': 0.80, 'name': 'pixel/recall'}},
                 {'AUC': {'curve': 'PR', 'name': 'pixel/AUPRC', 'num_thresholds': 150}},
                 {'AUC': {'curve': 'ROC', 'name': 'pixel/AUROC', 'num_thresholds': 150}},
                 {'FBetaScore': {'thresholds': 0.80, 'beta': 1.0, 'name': 'pixel/F1-score'}},
                 {'FBetaScore': {'thresholds': 0.80, 'beta': 2.0, 'name': 'pixel/F2-score'}}]
# |train-step probability - forward(training=True)|: the same network through other kernels (fused head: hardware exp2 / rcp)
PROB_TOL = {'f32': 1e-4, 'bf16': 2e-2}


def _thresholds():
    from dnncancerannotator_amd import metrics
    return np.concatenate([metrics.solve_metric(s).thresholds for s in PIXEL_METRICS]).astype(np.float32)


def np_counts(prob, y, thr):
    """(tp, fp, fn, tn) per threshold, prob > thr in float32, labels > 0.5 (k_conf_hist's rule)"""
    p, pos = np.asarray(prob, np.float32).ravel(), np.asarray(y, np.float32).ravel() > 0.5
    pp, pn = np.sort(p[pos]), np.sort(p[~pos])
    thr = np.asarray(thr, np.float32)
    tp = pp.size - np.searchsorted(pp, thr, side='right')
    fp = pn.size - np.searchsorted(pn, thr, side='right')
    return np.stack([tp, fp, pp.size - tp, pn.size - fp], 1).astype(np.float64)


def _snapshot(m):
    return m.get_params(), m.get_state(), m.get_opt_state()


def _restore(m, snap):
    p, s, (mm, vv, it) = snap
    m.set_params(p)
    if m.n_state:
        m.set_state(s)
    m.set_opt_state(mm, vv, it)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# (arch, C, options, dtype, B, size, force_generic, env, the launch that must carry the head)
PATHS = {
    'tail3': ('unet', 1, UNET, 'f32', 8, 512, False, {}, 'tail3_3x1_3'),                              # configs/unet.yaml
    'conv_epilogue': ('unet', 1, UNET, 'f32', 8, 512, False, {'DNNCA_NO_TAIL3': '1'}, 'pgfwd_head_3x1_3'),
    'head_train_3': ('unet', 1, UNET, 'f32', 8, 512, False, {'DNNCA_NO_HEAD_IN_CONV': '1'}, 'head_train_3'),
    'mulmo_c16': ('mulmo', 3, dict(UNET, n_filters_first=16, n_downsample=4, bn=True), 'f32', 2, 64, False, {}, 'head_train_16'),
    'unet_big_c64_bf16': ('unet', 1, dict(UNET, n_filters_first=64, n_downsample=4, bn=True), 'bf16', 2, 64, False, {}, 'head_train_64'),
    'generic': ('unet', 1, UNET, 'f32', 2, 64, True, {}, 'g_loss'),
}


@pytest.mark.parametrize('path', list(PATHS))
def test_train_step_counts_every_head_path(gpu, monkeypatch, path):
    arch, C, opts, dtype, B, S, generic, env, head = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    x, y = O.synthetic_batch(B, S, S, C, seed_x=3)
    m = gpu.DeviceModel(arch, C, S, S, B, dtype=dtype, force_generic=generic, **opts)
    m.init_glorot(seed=5)
    thr = _thresholds()
    assert head in [r[0] for r in m.plan()]
    cfg = m.loss_cfg(weight_mul=3.0)
    m.train_step(x, y, 0.0, cfg)                 # one step first: Adam slots and BN statistics that are not the initial ones
    before = _snapshot(m)

    def step(on):
        _restore(m, before)
        m.train_metrics(thr if on else None)
        out = m.train_step(x, y, 1e-3, cfg)
        return out, m.get_grads(), m.get_params(), m.get_state(), m.get_opt_state()

    off = step(False)
    off2 = step(False)
    on = step(True)
    counts = np.asarray(m.last_step_confusion(), np.float64)
    prob = m.last_prob(B)
    m.train_metrics(None)
    # the option changes no arithmetic: the loss (a fixed-order reduction) is bit-identical.  Gradients, updated weights, BN
    # statistics and Adam slots go through float atomics whose order varies from run to run with the option off as well
    # (two off steps differ in their last bits): the on step must stay within that noise
    assert _bits(on[0].loss).tolist() == _bits(off[0].loss).tolist() == _bits(off2[0].loss).tolist()
    for a, b, c in zip(on[1:4] + on[4][:2], off[1:4] + off[4][:2], off2[1:4] + off2[4][:2]):
        a, b, c = (np.asarray(t, np.float64) for t in (a, b, c))
        if b.size:
            assert np.abs(a - b).max() <= 4 * np.abs(b - c).max() + 1e-6 * np.abs(b).max()
    assert on[4][2] == off[4][2]
    # counts: exactly numpy's on the probabilities the step left in the buffer; every pixel counted once
    assert np.array_equal(counts, np_counts(prob, y, thr))
    npos = float((y > 0.5).sum())
    assert np.all(counts[:, 0] + counts[:, 2] == npos) and np.all(counts.sum(1) == B * S * S)
    assert 0 < npos < B * S * S and 0 < counts[:, 0].max()
    # the probabilities are those of the step's own forward pass: forward(training=True) from the same pre-step variables
    _restore(m, before)
    ref = m.forward(x, training=True)[..., 0]
    assert np.all(np.isfinite(prob)) and np.abs(prob - ref).max() <= PROB_TOL[dtype], np.abs(prob - ref).max()
    m.close()


def test_train_step_probabilities_match_the_float64_oracle(gpu):
    """small unet.yaml shape: the step's probabilities against sigmoid(logits) of the float64 oracle's training=True forward"""
    B, S = 2, 64
    spec = O.ModelSpec('unet', 1, **UNET)
    params = O.init_params(spec, seed=2)
    x, y = O.synthetic_batch(B, S, S, 1, seed_x=4)
    m = gpu.DeviceModel('unet', 1, S, S, B, **UNET)
    m.set_params(O.flatten(spec, params))
    thr = _thresholds()
    m.train_metrics(thr)
    m.train_step(x, y, 1e-3, m.loss_cfg(weight_mul=3.0))
    prob = m.last_prob(B)
    counts = np.asarray(m.last_step_confusion(), np.float64)
    p64 = {n: v.astype(np.float64) for n, v in params.items()}
    _, _, logits, _ = O.loss_and_grads(spec, p64, x.astype(np.float64), y, dict(weight_mul=3.0), training=True)
    ref = 1.0 / (1.0 + np.exp(-np.asarray(logits, np.float64).reshape(prob.shape)))
    assert np.abs(prob - ref).max() <= 1e-4, np.abs(prob - ref).max()
    assert np.array_equal(counts, np_counts(prob, y, thr))
    m.close()


def test_label_smoothing_counts_use_the_raw_labels(gpu):
    """utils/losses.py:62-67 blurs the labels inside the loss only: the counts see the labels as given"""
    B, S = 2, 128
    x, y = O.synthetic_batch(B, S, S, 1, seed_x=6)
    m = gpu.DeviceModel('unet', 1, S, S, B, **UNET)
    m.init_glorot(seed=1)
    thr = _thresholds()
    m.train_metrics(thr)
    m.train_step(x, y, 1e-3, m.loss_cfg(weight_mul=3.0, label_smoothing=True))
    counts = np.asarray(m.last_step_confusion(), np.float64)
    assert np.array_equal(counts, np_counts(m.last_prob(B), y, thr))
    assert np.all(counts[:, 0] + counts[:, 2] == float((y > 0.5).sum()))
    m.close()


def test_plan_unchanged_without_the_option(gpu):
    """the launch plan of a model whose option was never on, switched on (one histogram launch more), and switched off again"""
    B, S = 8, 512
    m = gpu.DeviceModel('unet', 1, S, S, B, **UNET)
    base = m.plan(variants=True)
    m.train_metrics(_thresholds())
    on = m.plan(variants=True)
    m.train_metrics(None)
    assert m.plan(variants=True) == base
    names_on, names_base = [r[0] for r in on], [r[0] for r in base]
    assert names_on == names_base + ['train_conf_hist']
    m.close()


def _config(**deploy):
    d = {'optimizer': 'adam', 'LearningRateScheduler': 'lambda epoch, current_lr: 0.0',      # fixed weights: exact comparisons
         'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}}, 'enable_multigpu': False,
         'metrics': PIXEL_METRICS + [{'RegionBasedPrecision': {'thresholds': 0.8, 'IoU_threshold': 0.3, 'resize_factor': 0.5,
                                                                'name': 'region/precision'}}]}
    d.update(deploy)
    return {'model': 'UNetAnnotator', 'model_options': UNET, 'deploy_options': d}


METRIC_NAMES = [list(s.values())[0]['name'] for s in PIXEL_METRICS]


def test_engine_train_metrics_feeder_no_feeder_and_validation(gpu, tmp_path, monkeypatch):
    from dnncancerannotator_amd import data, engine
    ds = lambda: data.SyntheticDataset(4, 64, 64, 1, n_batches=5, seed=3)       # noqa: E731
    val = data.SyntheticDataset(4, 64, 64, 1, n_batches=2, seed=9, repeat=False)
    cfg = _config(train_metrics='device', region_metrics='device')
    runs = {}
    m = engine.TFKerasModel(cfg)
    runs['feeder'] = m.train(ds(), max_steps=20, save_freq=100)
    assert getattr(m.device_model, '_ring', None) is not None
    runs['validation'] = engine.TFKerasModel(cfg).train(ds(), val_data=val, save_path=str(tmp_path / 'v'), max_steps=20, save_freq=7)
    monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
    m = engine.TFKerasModel(cfg)
    runs['no_feeder'] = m.train(ds(), max_steps=20, save_freq=100)
    assert getattr(m.device_model, '_ring', None) is None
    a = runs['feeder'].history
    assert list(a)[:len(METRIC_NAMES) + 2] == ['loss'] + METRIC_NAMES + ['lr'] and len(a['pixel/AUROC']) == 20
    assert len(set(a['pixel/AUROC'])) > 1 and all(0.0 <= v <= 1.0 for v in a['pixel/AUROC'])
    assert 'region/precision' not in a and 'val_region/precision' in runs['validation'].history
    for k in ('validation', 'no_feeder'):
        for name in METRIC_NAMES:
            assert runs[k].history[name] == a[name], (k, name)
    # the entries are the metrics of each step's own batch: numpy on forward probabilities of the (fixed) weights
    from dnncancerannotator_amd import metrics
    dm = m.device_model
    thr = _thresholds()
    for i, (x, y) in zip(range(5), ds()):
        prob = dm.forward(np.asarray(x), training=True)
        counts = np_counts(prob, y, thr)
        lo = 0
        for spec, name in zip(PIXEL_METRICS, METRIC_NAMES):
            mt = metrics.solve_metric(spec)
            mt.counts += counts[lo:lo + len(mt.thresholds)]
            lo += len(mt.thresholds)
            assert abs(mt.result() - a[name][i]) <= 1e-3, (i, name)
    lines = open(tmp_path / 'v' / 'tfevents' / 'train_log.csv').read().splitlines()
    assert [kv.split('=')[0] for kv in lines[6].split(',')[1:]] == ['loss'] + METRIC_NAMES + ['lr'] + \
        ['val_loss'] + ['val_' + n for n in METRIC_NAMES] + ['val_region/precision']


def test_engine_label_smoothing_counts_raw_labels(gpu):
    from dnncancerannotator_amd import data, engine, metrics
    cfg = _config(train_metrics='device')
    cfg['deploy_options']['loss'] = {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0, 'label_smoothing': True}}
    ds = lambda: data.SyntheticDataset(4, 64, 64, 1, n_batches=3, seed=5)        # noqa: E731
    m = engine.TFKerasModel(cfg)
    h = m.train(ds(), max_steps=3).history
    thr = _thresholds()
    for i, (x, y) in zip(range(3), ds()):
        prob = m.device_model.forward(np.asarray(x), training=True)
        counts = np_counts(prob, y, thr)
        rec = metrics.solve_metric(PIXEL_METRICS[1])
        rec.counts += counts[:1]
        assert abs(rec.result() - h['pixel/recall'][i]) <= 1e-3


def test_engine_without_the_key_is_unchanged(gpu, tmp_path):
    from dnncancerannotator_amd import data, engine
    cfg = _config()
    m = engine.TFKerasModel(cfg)
    res = m.train(data.SyntheticDataset(4, 64, 64, 1, n_batches=3, seed=3), save_path=str(tmp_path / 'r'), max_steps=6,
                  save_freq=100)
    assert list(res.history) == ['loss', 'lr']
    text = open(tmp_path / 'r' / 'tfevents' / 'train_log.csv').read()
    assert text == ''.join('%d,loss=%.8g,lr=%.8g\n' % (i + 1, l, r) for i, (l, r) in enumerate(zip(res.history['loss'],
                                                                                                    res.history['lr'])))
    fresh = gpu.DeviceModel('unet', 1, 64, 64, 4, **UNET)
    assert m.device_model.plan(variants=True) == fresh.plan(variants=True)
    fresh.close()
