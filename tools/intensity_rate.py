#!/usr/bin/env python3
"""intensity_rate.py -- cost of random_intensity (configs/additionals/intensity_augment.yaml) at 8 x 512 x 512 x 3.

  (a) the one `aug_intensity` launch of dnnca_intensity_f32 for five sets of records
          all flags 0            every plane is copied (the halo-less instantiation)
          pointwise              gamma and bias field on every plane
          noise                  Rician noise on every plane
          overlay draws          what intensity_augment.yaml draws for the batch (about a fifth of the planes blur: the halo launch)
          blur R = 8             every plane blurred at sigma 8 / 3
      with every tile of output pixels the kernel can be built for (DNNCA_INTENSITY_TILE); beside them, in the same process,
      `aug_apply` (dnnca_augment_u8) and `aug_affine` (dnnca_affine_f32, identity and d4 draws).  HIP events around every launch
      (dnnca_profile_*), `--repeats` repeats of `--launches` launches, alternating; medians and the spread (min .. max).
      aug_intensity reads and writes batch * h * w * c floats once, 8 bytes per float (a blurred plane reads its halo again from
      the caches: (TX + 2 R) (TY + 2 R) / (TX TY) loads and steps 1 and 2 per pixel); its rate is printed in GB/s and as a share
      of what aug_affine reaches on identity matrices over ITS bytes, batch * h * w * (c + 1) * 8.
  (b) the staged engine.train rate on synthetic exam files (the train leg of tools/affine_rate.py: 256 x 256 crops of 512 x 512
      slices, shuffle buffer, data_options.yaml's crop / flip / contrast / warp chain) without an overlay and with
      intensity_augment.yaml -- one fresh process per measurement, the arms alternating and starting one arm later in every
      repeat, `--repeats` times.
  (c) with --parent-root DIR (a built checkout of the commit before random_intensity): leg (b) without overlay from that tree,
      alternating with this one, to show the existing chain costs what it did.

    python tools/intensity_rate.py [--repeats 3] [--launches 20] [--steps 100] [--parent-root DIR] [--out profiles/intensity_rate.txt]"""
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
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'intensity_rate.txt'))
ap.add_argument('--root', default=HERE, help=argparse.SUPPRESS)              # the tree a child process imports the package from
ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)               # child: kernels | train
ap.add_argument('--overlay', default='none', help=argparse.SUPPRESS)         # child, leg train: none | intensity
ap.add_argument('--dir', default=None, help=argparse.SUPPRESS)               # child, leg train: where the exam files are
a = ap.parse_args()
sys.path.insert(0, a.root)
B, S, C = 8, 512, 3
TILES = ('32x8', '16x16', '64x4', '32x16', '32x32')
TYPES = ['TRA', 'ADC', 'DWI', 'label']
BASE_AUG = {'random_crop': None, 'random_flip': None, 'random_contrast': None, 'random_warp': None}
CASES = ('all flags 0', 'pointwise', 'noise', 'overlay draws', 'blur R = 8')


def overlay_conf():
    from dnncancerannotator_amd import load
    over = load._load_config_single(os.path.join(HERE, 'configs', 'additionals', 'intensity_augment.yaml'))
    return over['data_options.train.augment_options.random_intensity']


def leg_kernels():
    from dnncancerannotator_amd import augment
    from dnncancerannotator_amd import device as dev
    dev.init_device(0)
    rng = np.random.default_rng(0)
    dm = dev.DeviceModel('unet', C, S, S, B, n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, padding='same')
    dm.init_glorot(0)
    x, y = dev.DeviceBuffer(rng.random((B, S, S, C), np.float32)), dev.DeviceBuffer(rng.random((B, S, S), np.float32))
    raw = rng.integers(0, 256, (B, S + 12, S + 12, C + 1)).astype(np.uint8)
    params = augment.draw_params(rng, B, augment.parse_augment_options(BASE_AUG, (S, S)))
    parse = lambda name, conf: getattr(augment.parse_augment_options({name: conf}, (S, S)), name[len('random_'):])        # noqa: E731
    draw = lambda conf: augment.draw_intensity(rng, B, parse('random_intensity', conf), C)                                  # noqa: E731
    recs = {'all flags 0': np.zeros((B, C, augment.INTENSITY_WORDS), np.uint32),
            'pointwise': draw(dict(gamma={'range': [0.7, 1.5]}, bias_field={'strength': 0.3})),
            'noise': draw(dict(noise={'sigma': [0.0, 0.05]})),
            'overlay draws': augment.draw_intensity(np.random.default_rng(8), B, parse('random_intensity', overlay_conf()), C),
            'blur R = 8': draw(dict(blur={'sigma': 8 / 3}))}
    assert (recs['blur R = 8'][..., 11] == 8).all() and (recs['pointwise'][..., 0] == 3).all() and (recs['noise'][..., 0] == 24).all()
    flags = recs['overlay draws'][..., 0]
    print('NOTE\toverlay draws: of %d planes %d gamma, %d bias, %d blur, %d noise, %d untouched'
          % (flags.size, *[int(((flags & bit) != 0).sum()) for bit in (1, 2, 4, 8)], int((flags == 0).sum())), flush=True)
    mats = {'identity': augment.draw_affine(rng, B, parse('random_affine', {}), (S, S)),
            'd4 draws': augment.draw_affine(rng, B, parse('random_affine', {'symmetry': 'd4'}), (S, S))}

    def intensity(tile, r):
        def run():
            os.environ['DNNCA_INTENSITY_TILE'] = tile
            try:
                dm.intensity(x, r)
            finally:
                del os.environ['DNNCA_INTENSITY_TILE']
        return run

    # the halo-less cases run one code path whatever the tile's shape does to coalescing: they are walked too, the table is small
    arms = [('aug_intensity %-5s %s' % (tile, name), 'aug_intensity', intensity(tile, recs[name])) for name in CASES for tile in TILES]
    arms += [('aug_apply (crop, flip, contrast, / 255, split)', 'aug_apply', lambda: dm.augment_u8(raw, params, (S, S), C))]
    arms += [('aug_affine 32x8  %s' % name, 'aug_affine', (lambda m: lambda: dm.affine(x, y, m))(m)) for name, m in mats.items()]

    def kernel_ms(name, run):
        dm.profile_reset()
        dm.profile_enable(1)
        for _ in range(a.launches):
            run()
        dm.sync()
        rows = [r for r in dm.profile() if r[0] == name]
        dm.profile_enable(0)
        assert sum(r[1] for r in rows) == a.launches, (name, rows)
        return sum(r[2] for r in rows) / sum(r[1] for r in rows)

    for _, _, run in arms:
        run()
    dm.sync()
    times = {label: [] for label, _, _ in arms}
    for _ in range(a.repeats):
        for label, name, run in arms:
            times[label].append(kernel_ms(name, run))
    for label, _, _ in arms:
        t = times[label]
        print('KERNEL\t%s\t%.5f\t%.5f\t%.5f' % (label, statistics.median(t), min(t), max(t)), flush=True)
    dm.close()


def leg_train():
    from dnncancerannotator_amd import tfrecord
    from dnncancerannotator_amd.engine import TFKerasModel
    aug = dict(BASE_AUG)
    if a.overlay == 'intensity':
        aug['random_intensity'] = overlay_conf()
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
    return [l.split('\t') for l in out.stdout.splitlines() if l.startswith(('KERNEL\t', 'RATE\t', 'NOTE\t'))]


def main():
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say('%d x %d x %d x %d features; %d repeats of %d launches, ms per launch: median (min .. max)' % (B, S, S, C, a.repeats, a.launches))
    rows = child(HERE, 'kernels')
    for r in rows:
        if r[0] == 'NOTE':
            say('  ' + r[1])
    rows = [r for r in rows if r[0] == 'KERNEL']
    med = {r[1]: float(r[2]) for r in rows}
    nbytes, affine_bytes = B * S * S * C * 8, B * S * S * (C + 1) * 8
    affine_rate = affine_bytes / (med['aug_affine 32x8  identity'] * 1e-3) / 1e9
    say('  aug_intensity moves %.1f MB per launch (read + write of %d floats), aug_affine %.1f MB' % (nbytes / 1e6, B * S * S * C, affine_bytes / 1e6))
    for _, label, m, lo, hi in rows:
        extra = ''
        if label.startswith('aug_intensity'):
            rate = nbytes / (float(m) * 1e-3) / 1e9
            extra = '  %7.1f GB/s, %.2f of aug_affine\'s rate on identity matrices' % (rate, rate / affine_rate)
        elif label.startswith('aug_affine'):
            extra = '  %7.1f GB/s' % (affine_bytes / (float(m) * 1e-3) / 1e9)
        say('  %-48s %.4f (%.4f .. %.4f)%s' % (label, float(m), float(lo), float(hi), extra))
    tmp = tempfile.mkdtemp(prefix='intensity_rate_')
    from dnncancerannotator_amd import tfrecord
    rng = np.random.default_rng(0)
    for e in range(4):
        sl = rng.integers(0, 256, size=(24, S, S, len(TYPES)), dtype=np.uint8)
        sl[..., -1] = (sl[..., -1] > 250) * 255
        tfrecord.write_records(os.path.join(tmp, 'exam%d.tfrecords' % e), [tfrecord.make_example(sl, 1, e, 'p', 'c', TYPES)])
    arms = [('data_options.yaml chain (crop, flip, contrast, warp)', HERE, 'none'), ('+ intensity_augment.yaml', HERE, 'intensity')]
    if a.parent_root:
        arms.append(('data_options.yaml chain, parent commit\'s tree', a.parent_root, 'none'))
    rates = {label: [] for label, _, _ in arms}
    for i in range(a.repeats):
        for label, root, overlay in arms[i % len(arms):] + arms[:i % len(arms)]:      # every arm takes every place in the cycle
            rates[label].append(float(child(root, 'train', overlay=overlay, dir=tmp)[0][1]))
    say('engine.train, staged, exam files (4 x 24 slices of %d x %d x %d, 256 x 256 crops, batch %d), %d steps, slices/s: median (min .. max)'
        % (S, S, len(TYPES), B, a.steps))
    base = statistics.median(rates[arms[0][0]])
    for label, _, _ in arms:
        r = rates[label]
        say('  %-52s %8.1f (%8.1f .. %8.1f)  %.3f of the first row' % (label, statistics.median(r), min(r), max(r), statistics.median(r) / base))
        say('      in the order run: ' + ' '.join('%.0f' % v for v in r))
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
