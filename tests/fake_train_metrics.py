"""Test double for the per-step training metrics (deploy_options.train_metrics: device): tests/fake_device.FakeDeviceModel plus
the DeviceModel methods the engine calls when the option is on.  A train step keeps the sigmoid of its own training=True forward
pass (the oracle's logits before the update) and counts it against the raw labels, prob > threshold, labels > 0.5, like
k_conf_hist<true>.  Test infrastructure only."""

import numpy as np

from fake_device import FakeDeviceModel
from oracle import unet_oracle as O


class FakeTrainMetricsDevice(FakeDeviceModel):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.tm_thr = None
        self.tm_counts = None
        self.pre_step_params = []        # the trainable variables in front of every train step (the tests' single-process replay)

    def train_metrics(self, thresholds):
        t = np.asarray(() if thresholds is None else thresholds, np.float32).ravel()
        self.tm_thr = t if t.size else None

    def train_step(self, x, y, lr, cfg):
        self.pre_step_params.append(self.get_params().tolist())
        if self.tm_thr is not None:
            _, _, logits, _ = O.loss_and_grads(self.spec, self.params, np.asarray(x, np.float64), y, cfg, training=True)
            prob = (1.0 / (1.0 + np.exp(-np.asarray(logits, np.float64)))).astype(np.float32)
            self.tm_counts = counts(prob, y, self.tm_thr)
        return super().train_step(x, y, lr, cfg)

    def last_step_confusion(self):
        return [tuple(r) for r in self.tm_counts.tolist()]


def counts(prob, y, thr):
    """[(tp, fp, fn, tn)] per threshold as float64 rows"""
    p, pos = np.asarray(prob, np.float32).ravel(), np.asarray(y, np.float32).ravel() > 0.5
    out = []
    for t in np.asarray(thr, np.float32).ravel():
        pp = p > t
        out.append((float((pp & pos).sum()), float((pp & ~pos).sum()), float((~pp & pos).sum()), float((~pp & ~pos).sum())))
    return np.asarray(out, np.float64)


def install(patch=setattr, seed_offset=0):
    """the engine's device layer -> FakeTrainMetricsDevice (as tests/dp_engine_worker.py does with FakeDeviceModel).  patch: setattr,
    or pytest's monkeypatch.setattr (undone after the test).  Returns the list of models built."""
    from dnncancerannotator_amd import device, models
    patch(device, 'init_device', lambda ordinal=0: None)
    patch(device, 'device_count', lambda: 1)
    patch(device, 'DeviceModel', FakeTrainMetricsDevice)
    built = []

    def build(self, input_shape, max_batch=None, seed=None, force_generic=False):
        b, h, w, c = input_shape
        opts = {k: v for k, v in self.configs.items() if k in ('n_filters_first', 'n_downsample', 'rate', 'kernel_size', 'conv_stride',
                                                               'bn', 'padding')}
        self.device_model = FakeTrainMetricsDevice(self.arch, c, h, w, max_batch or b, **opts)
        self.device_model.init_glorot(seed=(seed or 0) + seed_offset)
        built.append(self.device_model)
        return self.device_model
    patch(models.UNetAnnotator, 'build', build)
    return built
