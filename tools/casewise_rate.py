#!/usr/bin/env python3
"""casewise_rate.py -- cost of the Visualizer pass of `annotator evaluate --export_csv [--export_images]` (engine._visualize): slices/s
over batches of 8 x 512 x 512 for configs/unet.yaml (C = 1) and configs/mulmo_unet.yaml (C = 5), casewise counts alone and with the
PNG images, files written to a temporary directory; then the device time per launch of the pass's kernels (dnnca_profile_*), the
host PNG encoding rate, and the forward alone for scale.

    python tools/casewise_rate.py [--batch 8] [--batches 16]"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dnncancerannotator_amd import casewise as CW                 # noqa: E402
from dnncancerannotator_amd import device as dev                  # noqa: E402
from dnncancerannotator_amd.data import ArrayDataset              # noqa: E402
from dnncancerannotator_amd.engine import TFKerasModel            # noqa: E402
from dnncancerannotator_amd.synthetic import synthetic_batch      # noqa: E402
import numpy as np                                                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--batches', type=int, default=16)
ap.add_argument('--size', type=int, default=512)
a = ap.parse_args()
B, S, NB = a.batch, a.size, a.batches
dev.init_device(0)

CONFIGS = [('configs/unet.yaml', 'UNetAnnotator', 1, dict(n_filters_first=3, n_downsample=3, bn=False)),
           ('configs/mulmo_unet.yaml', 'MulmoUNetAnnotator', 5, dict(n_filters_first=16, n_downsample=4, bn=True))]
DEPLOY = dict(optimizer='adam', loss=dict(class_name='WeightedCrossentropy', config=dict(weight_mul=3.0)), enable_multigpu=False)

for cfg, model, C, opts in CONFIGS:
    x, y = synthetic_batch(B * 4, S, S, C, seed_x=3, seed_y=4)
    ds = ArrayDataset(np.concatenate([x] * (NB // 4)), np.concatenate([y] * (NB // 4)), B, meta_path='/synthetic/p0/e0/mri')
    e = TFKerasModel(dict(model=model, deploy_options=DEPLOY,
                          model_options=dict(rate=2, kernel_size=3, conv_stride=1, padding='same', **opts)))
    e._build(ds)
    dm = e.device_model
    print('%s (C = %d): %d batches of %d x %d x %d' % (cfg, C, NB, B, S, S), flush=True)
    for xb, _ in ArrayDataset(x, y, B):                       # warm-up, and the forward alone for scale
        dm.forward(xb, return_prob=False)
    t0 = time.perf_counter()
    for xb, _, _, _ in ds:
        dm.forward(xb, return_prob=False)
    dm.sync()
    print('  %-28s %9.1f slices/s' % ('forward only', B * NB / (time.perf_counter() - t0)), flush=True)
    for images in (False, True):
        with tempfile.TemporaryDirectory() as tmp:
            w = CW.Writer()
            e._visualize(ds, 0, tmp, True, images, False, [], w)    # warm-up (directories, pool)
            w.close()
            rows, w = [], CW.Writer()
            t0 = time.perf_counter()
            e._visualize(ds, 1, tmp, True, images, False, rows, w)
            w.close()
            dt = time.perf_counter() - t0
            n = sum(len(fs) for _, _, fs in os.walk(tmp))
        print('  %-28s %9.1f slices/s  (%.2f ms per batch; %d files)' % ('counts + CSV' + (' + PNG' if images else ''),
                                                                         B * NB / dt, dt / NB * 1e3, n), flush=True)
    # device time per launch of the pass's kernels (HIP events around every launch)
    dm.profile_reset()
    dm.profile_enable(1)
    for xb, yb, _, _ in ds:
        dm.forward(xb, return_prob=False)
        dm.region_confusion_slices(yb, [CW.device_spec()])
        dm.render_composite(None, len(xb), CW.RATIO, False)
    dm.sync()
    rows = [r for r in dm.profile() if r[0].startswith('region_')]
    dm.profile_enable(0)
    print('  region / render kernels: %.3f ms per batch (event-bracketed)' % (sum(r[2] for r in rows) / NB), flush=True)
    for name, n, ms, by, fl in sorted(rows, key=lambda r: -r[2]):
        us = ms / n * 1e3
        print('    %-22s launches %5d  %9.2f us per launch' % (name, n, us), flush=True)
    img = dm.render_composite(None, B, CW.RATIO, False)
    t0 = time.perf_counter()
    for im in img:
        CW.encode_png(im)
    dt = time.perf_counter() - t0
    print('  PNG encode (one thread)   %9.1f images/s (%d x %d grey)' % (B / dt, img.shape[1], img.shape[2]), flush=True)
    dm.close()
