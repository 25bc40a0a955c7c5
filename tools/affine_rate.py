#!/usr/bin/env python3
"""affine_rate.py -- cost of random_affine (configs/additionals/affine_augment.yaml, d4_augment.yaml) at 8 x 512 x 512 x 3 + label.

  (a) the one `aug_affine` launch of dnnca_affine_f32 for identity matrices, for `symmetry: d4` draws and for affine_augment.yaml's
      draws, with every tile of output pixels the kernel can be built for (DNNCA_AFFINE_TILE); beside it, in the same process,
      `aug_apply` (dnnca_augment_u8), `aug_warp` (dnnca_warp_f32, 100 points) and `tta_view_in` (the eight views of forward_tta).
      HIP events around every launch (dnnca_profile_*), `--repeats` repeats of `--launches` launches, alternating; medians and
      the spread (min .. max).  aug_affine is a single pass over batch * h * w * (c + 1) * 8 bytes: its rate is printed in GB/s
      and as a share of the rate at which tta_view_in, the project's plain copy kernel, moves its 8 bytes per float.
  (b) the staged engine.train rate on synthetic exam files (the train leg of tools/tfrecord_rate.py: 256 x 256 crops of 512 x 512
      slices, shuffle buffer, data_options.yaml's crop / flip / contrast / warp chain) without an overlay, with affine_augment.yaml
      and with d4_augment.yaml -- one fresh process per measurement, the arms alternating, `--repeats` times.
  (c) with --parent-root DIR (a built checkout of the commit before random_affine): leg (b) without overlay from that tree,
      alternating with this one, to show the existing chain costs what it did.

    python tools/affine_rate.py [--repeats 3] [--launches 20] [--steps 100] [--parent-root DIR] [--out profiles/affine_rate.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=3)
ap.add_argument('--launches', type=int, default=20)
ap.add_argument('--steps', type=int, default=100)
ap.add_argument('--parent-root', default=None)
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'affine_rate.txt'))
ap.add_argument('--root', default=HERE, help=argparse.SUPPRESS)              # the tree a child process imports the package from
ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)               # child: kernels | train
ap.add_argument('--overlay', default='none', help=argparse.SUPPRESS)         # child, leg train: none | affine | d4
ap.add_argument('--dir', default=None, help=argparse.SUPPRESS)               # child, leg train: where the exam files are
a = ap.parse_args()
sys.path.insert(0, a.root)
B, S, C = 8, 512, 3
TILES = ('16x16', '32x8', '8x32', '64x4', '8x8', '256x1')
AFFINE = dict(rotate_deg=15, scale=[0.9, 1.1], shift=8)
TYPES = ['TRA', 'ADC', 'DWI', 'label']
BASE_AUG = {'random_crop': None, 'random_flip': None, 'random_contrast': None, 'random_warp': None}


def leg_kernels():
    from dnncancerannotator_amd import augment
    from dnncancerannotator_amd import device as dev
    dev.init_device(0)
    rng = np.random.default_rng(0)
    dm = dev.DeviceModel('unet', C, S, S, B, n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, padding='same')
    dm.init_glorot(0)
    xh = rng.random((B, S, S, C), np.float32)
    x, y = dev.DeviceBuffer(xh), dev.DeviceBuffer(rng.random((B, S, S), np.float32))
    raw = rng.integers(0, 256, (B, S + 12, S + 12, C + 1)).astype(np.uint8)
    params = augment.draw_params(rng, B, augment.parse_augment_options(BASE_AUG, (S, S)))
    ctrl, wv = augment.solve_warp(*augment.draw_warp(rng, B, S))
    parse = lambda conf: augment.parse_augment_options({'random_affine': conf}, (S, S)).affine        # noqa: E731
    mats = {'identity': augment.draw_affine(rng, B, parse({}), (S, S)),
            'd4 draws': augment.draw_affine(rng, B, parse({'symmetry': 'd4'}), (S, S)),
            'affine_augment.yaml draws': augment.draw_affine(rng, B, parse(AFFINE), (S, S))}

    def affine(tile, m):
        def run():
            os.environ['DNNCA_AFFINE_TILE'] = tile
            try:
                dm.affine(x, y, m)
            finally:
                del os.environ['DNNCA_AFFINE_TILE']
        return run

    arms = [('aug_affine %-5s %s' % (tile, name), 'aug_affine', affine(tile, m), 1) for name, m in mats.items() for tile in TILES]
    arms += [('aug_apply (crop, flip, contrast, / 255, split)', 'aug_apply', lambda: dm.augment_u8(raw, params, (S, S), C), 1),
             ('aug_warp, 100 control points', 'aug_warp', lambda: dm.warp(x, y, ctrl, wv), 1),
             ('tta_view_in, mean of the 8 views', 'tta_view_in', lambda: dm.forward_tta(xh, 0xFF, return_prob=False), 8)]

    def kernel_ms(name, run, per_call):
        dm.profile_reset()
        dm.profile_enable(1)
        for _ in range(a.launches):
            run()
        dm.sync()
        rows = [r for r in dm.profile() if r[0] == name]
        dm.profile_enable(0)
        return sum(r[2] for r in rows) / sum(r[1] for r in rows), sum(r[1] for r in rows) / a.launches / per_call

    for _, _, run, _ in arms:
        run()
    dm.sync()
    times = {label: [] for label, _, _, _ in arms}
    for _ in range(a.repeats):
        for label, name, run, per_call in arms:
            ms, ratio = kernel_ms(name, run, per_call)
            assert 0.8 <= ratio <= 1.0, (label, ratio)           # forward_tta launches tta_view_in for seven of its eight views
            times[label].append(ms)
    for label, _, _, _ in arms:
        t = times[label]
        print('KERNEL\t%s\t%.5f\t%.5f\t%.5f' % (label, statistics.median(t), min(t), max(t)), flush=True)
    dm.close()


def leg_train():
    from dnncancerannotator_amd import tfrecord
    from dnncancerannotator_amd.engine import TFKerasModel
    aug = dict(BASE_AUG)
    if a.overlay == 'affine':
        aug['random_affine'] = dict(AFFINE)
    elif a.overlay == 'd4':
        aug['random_affine'] = {'symmetry': 'd4'}
    paths = sorted(os.path.join(a.dir, f) for f in os.listdir(a.dir) if f.endswith('.tfrecords'))
    e = TFKerasModel(dict(model='UNetAnnotator', deploy_options=dict(optimizer='adam', enable_multigpu=False, loss=dict(
        class_name='WeightedCrossentropy', config=dict(weight_mul=3.0))), model_options=dict(
            n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')))
    ds = tfrecord.TFRecordDataset(paths, TYPES, B, output_size=(256, 256), augment_options=aug, buffer_size=64, repeat=True,
                                  drop_remainder=True, normalize_exams=True)
    e.train(ds, max_steps=30, save_freq=10 ** 9, auto_resume=False)
    t0 = time.perf_counter()
    e.train(ds, max_steps=30 + a.steps, save_freq=10 ** 9, auto_resume=False)
    print('RATE\t%.3f' % (B * a.steps / (time.perf_counter() - t0)), flush=True)


def child(root, leg, **kw):
    cmd = [sys.executable, os.path.abspath(__file__), '--root', root, '--leg', leg, '--repeats', str(a.repeats), '--launches', str(a.launches),
           '--steps', str(a.steps)]
    for k, v in kw.items():
        cmd += ['--' + k, v]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        sys.exit('%s failed (%d):\n%s' % (' '.join(cmd), out.returncode, out.stderr[-3000:]))
    return [l.split('\t') for l in out.stdout.splitlines() if l.startswith(('KERNEL\t', 'RATE\t'))]


def main():
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say('%d x %d x %d x %d features + label; %d repeats of %d launches, ms per launch: median (min .. max)' % (B, S, S, C, a.repeats, a.launches))
    rows = child(HERE, 'kernels')
    med = {r[1]: float(r[2]) for r in rows}
    nbytes = B * S * S * (C + 1) * 8
    copy_rate = B * S * S * C * 8 / (med['tta_view_in, mean of the 8 views'] * 1e-3) / 1e9
    for _, label, m, lo, hi in rows:
        extra = ''
        if label.startswith('aug_affine'):
            rate = nbytes / (float(m) * 1e-3) / 1e9
            extra = '  %7.1f GB/s, %.2f of tta_view_in\'s rate' % (rate, rate / copy_rate)
        elif label.startswith('tta_view_in'):
            extra = '  %7.1f GB/s' % copy_rate
        say('  %-48s %.4f (%.4f .. %.4f)%s' % (label, float(m), float(lo), float(hi), extra))
    tmp = tempfile.mkdtemp(prefix='affine_rate_')
    from dnncancerannotator_amd import tfrecord
    rng = np.random.default_rng(0)
    for e in range(4):
        sl = rng.integers(0, 256, size=(24, S, S, len(TYPES)), dtype=np.uint8)
        sl[..., -1] = (sl[..., -1] > 250) * 255
        tfrecord.write_records(os.path.join(tmp, 'exam%d.tfrecords' % e), [tfrecord.make_example(sl, 1, e, 'p', 'c', TYPES)])
    arms = [('data_options.yaml chain (crop, flip, contrast, warp)', HERE, 'none'), ('+ affine_augment.yaml', HERE, 'affine'),
            ('+ d4_augment.yaml', HERE, 'd4')]
    if a.parent_root:
        arms.append(('data_options.yaml chain, parent commit\'s tree', a.parent_root, 'none'))
    rates = {label: [] for label, _, _ in arms}
    for _ in range(a.repeats):
        for label, root, overlay in arms:
            rates[label].append(float(child(root, 'train', overlay=overlay, dir=tmp)[0][1]))
    say('engine.train, staged, exam files (4 x 24 slices of %d x %d x %d, 256 x 256 crops, batch %d), %d steps, slices/s: median (min .. max)'
        % (S, S, len(TYPES), B, a.steps))
    base = statistics.median(rates[arms[0][0]])
    for label, _, _ in arms:
        r = rates[label]
        say('  %-52s %8.1f (%8.1f .. %8.1f)  %.3f of the first row' % (label, statistics.median(r), min(r), max(r), statistics.median(r) / base))
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if a.leg == 'kernels':
    leg_kernels()
elif a.leg == 'train':
    leg_train()
else:
    main()
