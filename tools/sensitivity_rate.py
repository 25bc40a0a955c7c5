#!/usr/bin/env python3
"""sensitivity_rate.py -- cost of `annotator evaluate --visualize_sensitivity`: slices/s of the evaluate visualisation pass
(engine._visualize with --export_csv --export_images, files written to a temporary directory) without and with the flag, over
batches of 8 x 512 x 512 for configs/unet.yaml's network with 3 input channels and for configs/mulmo_unet.yaml's with 3; then the
device time per launch of the input-sensitivity pass (dnnca_profile_*).  Writes profiles/sensitivity_rate.txt.

    python tools/sensitivity_rate.py [--batch 8] [--batches 8] [--out profiles/sensitivity_rate.txt]"""
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
ap.add_argument('--batches', type=int, default=8)
ap.add_argument('--size', type=int, default=512)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sensitivity_rate.txt'))
a = ap.parse_args()
B, S, NB = a.batch, a.size, a.batches
dev.init_device(0)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


CONFIGS = [('configs/unet.yaml', 'UNetAnnotator', 3, dict(n_filters_first=3, n_downsample=3, bn=False)),
           ('configs/mulmo_unet.yaml', 'MulmoUNetAnnotator', 3, dict(n_filters_first=16, n_downsample=4, bn=True))]
DEPLOY = dict(optimizer='adam', loss=dict(class_name='WeightedCrossentropy', config=dict(weight_mul=3.0)), enable_multigpu=False)

say('# tools/sensitivity_rate.py: evaluate visualisation pass (--export_csv --export_images), %d batches of %d x %d x %d' % (NB, B, S, S))
for cfg, model, C, opts in CONFIGS:
    x, y = synthetic_batch(B * 2, S, S, C, seed_x=3, seed_y=4)
    ds = ArrayDataset(np.concatenate([x] * (NB // 2)), np.concatenate([y] * (NB // 2)), B, meta_path='/synthetic/p0/e0/mri')
    e = TFKerasModel(dict(model=model, deploy_options=DEPLOY,
                          model_options=dict(rate=2, kernel_size=3, conv_stride=1, padding='same', **opts)))
    e._build(ds)
    dm = e.device_model
    say('%s (C = %d)' % (cfg, C))
    for flag in (False, True):
        with tempfile.TemporaryDirectory() as tmp:
            w = CW.Writer()
            e._visualize(ds, 0, tmp, True, True, False, [], w, sensitivity=flag)    # warm-up (directories, pool, one-time tables)
            w.close()
            w = CW.Writer()
            t0 = time.perf_counter()
            e._visualize(ds, 1, tmp, True, True, False, [], w, sensitivity=flag)
            w.close()
            dt = time.perf_counter() - t0
        say('  %-34s %9.1f slices/s  (%.2f ms per batch)' % ('with --visualize_sensitivity' if flag else 'without the flag', B * NB / dt, dt / NB * 1e3))
    xb = x[:B]
    dm.forward(xb, return_prob=False)
    dm.input_sensitivity(batch=B)
    t0 = time.perf_counter()
    for _ in range(4):
        dm.input_sensitivity(batch=B)
    say('  input_sensitivity alone            %9.2f ms per batch of %d' % ((time.perf_counter() - t0) / 4 * 1e3, B))
    dm.profile_reset()
    dm.profile_enable(1)
    for _ in range(2):
        dm.input_sensitivity(batch=B)
    dm.sync()
    rows = dm.profile()
    dm.profile_enable(0)
    say('  launches of the pass: %.3f ms per batch (event-bracketed)' % (sum(r[2] for r in rows) / 2))
    for name, n, ms, by, fl in sorted(rows, key=lambda r: -r[2]):
        say('    %-22s launches %4d  %10.2f us per launch' % (name, n // 2, ms / n * 1e3))
    dm.close()
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
