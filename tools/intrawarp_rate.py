#!/usr/bin/env python3
"""intrawarp_rate.py -- cost of random_intrachannelwarp (configs/additionals/intra_channelwarp_std*.yaml) at the shipped shape:
8 x 256 x 256, five feature channels + label, five groups [[0, label], [1], [2], [3], [4]], stddev 10 / max_diff 100.

  (a) the one `aug_warp_groups` launch of dnnca_warp_groups_f32, in both layouts (one group per block: the shipped one; one pixel
      per thread looping over the groups: DNNCA_WARP_GROUPS_PIXEL=1);
  (b) the only route to the same result without it: five `aug_warp` launches (dnnca_warp_f32) on single-group tensors -- kernel
      time only, the gathers, the scatter and the five uploads are left out in the baseline's favour;
  (c) the staged engine.train rate on a synthetic .tfrecords exam with data_options.yaml's augmentations (configs/unet.yaml model),
      with and without the option.

(a) and (b): HIP events around every launch (dnnca_profile_*), `--repeats` repeats of `--launches` launches each, alternating;
medians and the spread (min .. max) are printed, and (a) <= (b) is required unless (a) lies inside (b)'s own spread.

    python tools/intrawarp_rate.py [--repeats 5] [--launches 20] [--steps 200] [--out profiles/intrawarp_rate.txt]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dnncancerannotator_amd import augment, tfrecord            # noqa: E402
from dnncancerannotator_amd import device as dev                # noqa: E402
from dnncancerannotator_amd.engine import TFKerasModel          # noqa: E402
from dnncancerannotator_amd.runs.train import make_dataset      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--launches', type=int, default=20)
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'intrawarp_rate.txt'))
a = ap.parse_args()
B, S, C, G = 8, a.size, 5, 5
SLICE_TYPES = ['TRA', 'ADC', 'DWI', 'DCEE', 'DCEL', 'label']
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


dev.init_device(0)
rng = np.random.default_rng(0)
dm = dev.DeviceModel('unet', C, S, S, B, n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, padding='same')
x = dev.DeviceBuffer(rng.random((B, S, S, C), np.float32))
y = dev.DeviceBuffer(rng.random((B, S, S), np.float32))
x1 = dev.DeviceBuffer(rng.random((B, S, S, 1), np.float32))
groups = augment.channel_groups(C + 1)
group_of = augment.group_table(groups, C + 1)               # the label is the last raw channel: already features, then label
ctrl, wv = augment.solve_intrawarp(*augment.draw_intrawarp(rng, B, S, G, 100, 10.0))


def kernel_ms(name, run):
    """device time of the launches called `name` that one call of `run` makes (mean over --launches calls)"""
    dm.profile_reset()
    dm.profile_enable(1)
    for _ in range(a.launches):
        run()
    dm.sync()
    rows = [r for r in dm.profile() if r[0] == name]
    dm.profile_enable(0)
    return sum(r[2] for r in rows) / a.launches


def grouped():
    dm.warp_groups(x, y, group_of, ctrl, wv)


def grouped_pixel():
    os.environ['DNNCA_WARP_GROUPS_PIXEL'] = '1'
    try:
        dm.warp_groups(x, y, group_of, ctrl, wv)
    finally:
        del os.environ['DNNCA_WARP_GROUPS_PIXEL']


def five_single():
    for g in range(G):
        dm.warp(x1, y, ctrl[:, g], wv[:, g])


ARMS = [('(a) aug_warp_groups, one group per block', 'aug_warp_groups', grouped),
        ('(a\') aug_warp_groups, one pixel per thread', 'aug_warp_groups', grouped_pixel),
        ('(b) 5 x aug_warp on single-group tensors', 'aug_warp', five_single)]
for _, _, run in ARMS:          # warm up: code objects, scratch, pinned rows
    run()
dm.sync()
times = {label: [] for label, _, _ in ARMS}
for _ in range(a.repeats):
    for label, name, run in ARMS:
        times[label].append(kernel_ms(name, run))
say('%d x %d x %d x %d features + label, %d groups, 100 control points, stddev 10 / max_diff 100; %d repeats of %d calls, ms per call'
    % (B, S, S, C, G, a.repeats, a.launches))
med = {}
for label, _, _ in ARMS:
    t = times[label]
    med[label] = statistics.median(t)
    say('  %-46s median %.4f  min %.4f  max %.4f' % (label, med[label], min(t), max(t)))
ta, tb = med[ARMS[0][0]], med[ARMS[2][0]]
inside = min(times[ARMS[2][0]]) <= ta <= max(times[ARMS[2][0]])
flops = B * S * S * G * 100
say('  (a) / (b) = %.3f%s; (a) evaluates %.1f G r*log(r) terms per second in double' % (ta / tb, ' (inside (b)\'s spread)' if inside else '', flops / (ta * 1e-3) / 1e9))
dm.close()

# (c) the staged train loop on exam files
tmp = tempfile.mkdtemp(prefix='intrawarp_rate_')
rec = os.path.join(tmp, 'exam.tfrecords')
slices = rng.integers(0, 256, (64, S + 16, S + 16, len(SLICE_TYPES))).astype(np.uint8)
slices[..., -1] = (slices[..., -1] > 250) * 255
tfrecord.write_records(rec, [tfrecord.make_example(slices, 1, 1, 'p', 'cancer', SLICE_TYPES)])
BASE_AUG = {'random_crop': None, 'random_flip': None, 'random_contrast': None, 'random_warp': None}
rates = {}
for on in (False, True):
    aug = dict(BASE_AUG, random_intrachannelwarp=dict(n_points=50, max_diff=100, stddev=10.0)) if on else dict(BASE_AUG)
    opts = dict(batch_size=B, buffer_size=64, output_size=[S, S], slice_types=SLICE_TYPES, augment_options=aug)
    e = TFKerasModel(dict(model='UNetAnnotator', deploy_options=dict(optimizer='adam', enable_multigpu=False, loss=dict(
        class_name='WeightedCrossentropy', config=dict(weight_mul=3.0))), model_options=dict(
            n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')))
    ds = make_dataset([rec], opts, training=True)
    e.train(ds, max_steps=20, save_freq=10 ** 9)
    t0 = time.perf_counter()
    e.train(ds, max_steps=20 + a.steps, save_freq=10 ** 9)
    dt = time.perf_counter() - t0
    rates[on] = B * a.steps / dt
    say('(c) engine.train, staged, %d steps %-32s %8.3f ms/step %9.1f slices/s'
        % (a.steps, 'with random_intrachannelwarp' if on else 'data_options.yaml augmentations', dt / a.steps * 1e3, rates[on]))
say('    ratio (with / without): %.3f  (the host solves %d spline systems per batch for it, %d without)' % (rates[True] / rates[False], B * G + B, B))
os.remove(rec)
os.rmdir(tmp)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
if ta > tb and not inside:
    sys.exit('aug_warp_groups (%.4f ms) is slower than five aug_warp launches (%.4f ms)' % (ta, tb))
