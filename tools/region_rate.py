#!/usr/bin/env python3
"""region_rate.py -- cost of the region-based metrics in `annotator evaluate`: the staged engine.eval rate (configs/unet.yaml,
512 x 512 slices) with the pixel metrics of configs/additionals/metrics.yaml alone and with its seven region metrics added
(deploy_options.region_metrics: device), the per-kernel device time of the region launches (dnnca_profile_*), and the rate of the
numpy oracle (tests/region_oracle.py, one CPU thread) on the same probabilities for comparison.

    python tools/region_rate.py [--batch 8] [--batches 64]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from dnncancerannotator_amd import device as dev                # noqa: E402
from dnncancerannotator_amd.engine import TFKerasModel          # noqa: E402
from dnncancerannotator_amd.synthetic import synthetic_batch    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--batches', type=int, default=64)
ap.add_argument('--size', type=int, default=512)
a = ap.parse_args()
B, S, NE = a.batch, a.size, a.batches
dev.init_device(0)
batches = [synthetic_batch(B, S, S, 1, seed_x=10 + i, seed_y=20 + i) for i in range(4)]

PIXEL = [{'Precision': {'thresholds': 0.8, 'name': 'pixel/precision'}},
         {'Recall': {'thresholds': 0.8, 'name': 'pixel/recall'}},
         {'AUC': {'curve': 'PR', 'name': 'pixel/AUPRC', 'num_thresholds': 150}},
         {'AUC': {'curve': 'ROC', 'name': 'pixel/AUROC', 'num_thresholds': 150}},
         {'FBetaScore': {'thresholds': 0.8, 'beta': 1.0, 'name': 'pixel/F1-score'}},
         {'FBetaScore': {'thresholds': 0.8, 'beta': 2.0, 'name': 'pixel/F2-score'}}]
REGION = [{cls: dict(thresholds=0.8, IoU_threshold=0.3, resize_factor=0.5, name=name, **extra)}
          for cls, name, extra in [('RegionBasedPrecision', 'region/precision', {}), ('RegionBasedRecall', 'region/recall', {}),
                                   ('RegionBasedTruePositives', 'region/TP', {}), ('RegionBasedFalsePositives', 'region/FP', {}),
                                   ('RegionBasedFalseNegatives', 'region/FN', {}),
                                   ('RegionBasedFBetaScore', 'region/F1-score', {'beta': 1.0}),
                                   ('RegionBasedFBetaScore', 'region/F2-score', {'beta': 2.0})]]


class Gen:
    def __init__(self, n):
        self.n = n

    def __iter__(self):
        for i in range(self.n):
            yield batches[i % 4]


def engine(region):
    deploy = dict(optimizer='adam', loss=dict(class_name='WeightedCrossentropy', config=dict(weight_mul=3.0)), enable_multigpu=False,
                  metrics=PIXEL + (REGION if region else []))
    if region:
        deploy['region_metrics'] = 'device'
    e = TFKerasModel(dict(model='UNetAnnotator', deploy_options=deploy,
                          model_options=dict(n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False,
                                             padding='same')))
    e._build(Gen(1))
    return e


rates = {}
for region in (False, True):
    e = engine(region)
    e._evaluate(Gen(4), staged=True)
    t0 = time.perf_counter()
    r = e._evaluate(Gen(NE), staged=True)
    dt = time.perf_counter() - t0
    rates[region] = B * NE / dt
    extra = '  region/TP %s FP %s FN %s' % (r['region/TP'], r['region/FP'], r['region/FN']) if region else ''
    print('%-22s %8.3f ms/batch %9.1f slices/s (loss %.6f)%s' % ('eval-ring ' + ('+ region' if region else 'pixel only'), dt / NE * 1e3,
                                                               rates[region], r['loss'], extra), flush=True)
print('ratio (with / without region metrics): %.3f' % (rates[True] / rates[False]), flush=True)

# per-kernel device time of the region launches (HIP events around every launch: the rates above are the honest numbers)
dm = e.device_model
dm.profile_reset()
dm.profile_enable(1)
e._evaluate(Gen(16), staged=True)
dm.sync()
rows = [r for r in dm.profile() if r[0].startswith('region_')]
dm.profile_enable(0)
print('region kernels over 16 batches of %d: %.3f ms per batch (event-bracketed)' % (B, sum(r[2] for r in rows) / 16), flush=True)
for name, n, ms, by, fl in sorted(rows, key=lambda r: -r[2]):
    us = ms / n * 1e3
    print('  %-22s launches %5d  %8.2f us per launch  %7.1f GB/s algorithmic' % (name, n, us, by / (us * 1e-6) / 1e9 if us else 0.0))

# the numpy oracle on the same probabilities (one CPU thread)
import region_oracle as O                                       # noqa: E402
x, y = batches[0]
prob = dm.forward(x)[..., 0]
t0 = time.perf_counter()
c = O.region_counts(prob, y, [0.8], 0.3, 0.5, 5)
dt = time.perf_counter() - t0
print('numpy oracle (CPU)     %8.3f ms/batch %9.1f slices/s  counts %s' % (dt * 1e3, B / dt, c.tolist()), flush=True)
