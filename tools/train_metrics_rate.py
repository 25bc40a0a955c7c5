#!/usr/bin/env python3
"""train_metrics_rate.py -- cost of the per-step training metrics (deploy_options.train_metrics: device): the engine.train rate in
slices/s with the option off and on (the pixel metrics of configs/additionals/metrics.yaml, 302 thresholds) for configs/unet.yaml,
mulmo_unet and unet_big, and the per-kernel device time of the launches that differ (dnnca_profile_*: the histogram launch and
the head kernels' PROB variants).

    python tools/train_metrics_rate.py [--steps 300] [--only unet]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dnncancerannotator_amd import device as dev                # noqa: E402
from dnncancerannotator_amd.engine import TFKerasModel          # noqa: E402
from dnncancerannotator_amd.synthetic import synthetic_batch    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=300)
ap.add_argument('--only', default=None)
a = ap.parse_args()
dev.init_device(0)

PIXEL = [{'Precision': {'thresholds': 0.8, 'name': 'pixel/precision'}},
         {'Recall': {'thresholds': 0.8, 'name': 'pixel/recall'}},
         {'AUC': {'curve': 'PR', 'name': 'pixel/AUPRC', 'num_thresholds': 150}},
         {'AUC': {'curve': 'ROC', 'name': 'pixel/AUROC', 'num_thresholds': 150}},
         {'FBetaScore': {'thresholds': 0.8, 'beta': 1.0, 'name': 'pixel/F1-score'}},
         {'FBetaScore': {'thresholds': 0.8, 'beta': 2.0, 'name': 'pixel/F2-score'}}]
BASE = dict(rate=2, kernel_size=3, conv_stride=1, padding='same')
# name -> (model, model_options, channels, batch, size): the shipped configs (configs/*.yaml) at their train batch
CONFIGS = {
    'unet': ('UNetAnnotator', dict(BASE, n_filters_first=3, n_downsample=3, bn=False), 1, 8, 512),
    'mulmo_unet': ('MulmoUNetAnnotator', dict(BASE, n_filters_first=16, n_downsample=4, bn=True), 3, 8, 512),
    'unet_big': ('UNetAnnotator', dict(BASE, n_filters_first=64, n_downsample=4, bn=True), 1, 8, 512),
}


class Gen:
    def __init__(self, batches, n):
        self.batches, self.n = batches, n

    def __iter__(self):
        for i in range(self.n):
            yield self.batches[i % len(self.batches)]


def engine(model, opts, on):
    deploy = dict(optimizer='adam', loss=dict(class_name='WeightedCrossentropy', config=dict(weight_mul=3.0)), enable_multigpu=False,
                  metrics=PIXEL)
    if on:
        deploy['train_metrics'] = 'device'
    return TFKerasModel(dict(model=model, model_options=opts, deploy_options=deploy))


for name, (model, opts, C, B, S) in CONFIGS.items():
    if a.only and name != a.only:
        continue
    batches = [synthetic_batch(B, S, S, C, seed_x=10 + i, seed_y=20 + i) for i in range(4)]
    rates, engines = {}, {}
    for on in (False, True, False, True):          # interleaved: drift shows up as a difference between the two runs of an arm
        e = engine(model, opts, on)
        e.train(Gen(batches, 20), max_steps=20, save_freq=10 ** 9)              # warm-up (build, first launches)
        t0 = time.perf_counter()
        e.train(Gen(batches, a.steps), max_steps=20 + a.steps, save_freq=10 ** 9, auto_resume=False)
        dt = time.perf_counter() - t0
        rates.setdefault(on, []).append(B * a.steps / dt)
        if on in engines:
            engines[on].device_model.close()
        engines[on] = e
    off, on = max(rates[False]), max(rates[True])
    print('%-11s off %8.1f slices/s (%s)  on %8.1f slices/s (%s)  ratio %.3f' % (
        name, off, ' '.join('%.1f' % r for r in rates[False]), on, ' '.join('%.1f' % r for r in rates[True]), on / off), flush=True)
    # per-kernel device time of the launches that change (HIP events around every launch: the rates above are the honest numbers)
    for arm in (False, True):
        dm = engines[arm].device_model
        dm.profile_reset()
        dm.profile_enable(1)
        engines[arm].train(Gen(batches, 40), max_steps=engines[arm].current_step + 40, save_freq=10 ** 9, auto_resume=False)
        dm.sync()
        for k, n, ms, by, fl in sorted(dm.profile(), key=lambda r: -r[2]):
            if k.startswith(('train_conf_hist', 'tail3', 'pgfwd_head', 'head_train', 'g_loss')):
                print('  %-4s %-20s launches %4d  %8.2f us per launch  %7.1f GB/s algorithmic' % (
                    'on' if arm else 'off', k, n, ms / n * 1e3, by / (ms / n * 1e-3) / 1e9 if ms else 0.0), flush=True)
        dm.profile_enable(0)
    for e in engines.values():
        e.device_model.close()
