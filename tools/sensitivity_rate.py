#!/usr/bin/env python3
"""sensitivity_rate.py -- cost of `annotator evaluate --visualize_sensitivity`: slices/s of the evaluate visualisation pass
(engine._visualize with --export_csv --export_images, files written to a temporary directory) without and with the flag, over
batches of 8 x 512 x 512 for configs/unet.yaml's network with 3 input channels and for configs/mulmo_unet.yaml's with 3; then the
device time per launch of the input-sensitivity pass (dnnca_profile_*).  Then the cost of `--visualize_attribution`
(DeviceModel.integrated_gradients) on the same two networks: one call at steps = 8 and 32 beside steps x one input_sensitivity call
of the same build, and attr_first beside sens_first per launch with the bytes/s its accumulator traffic reaches.  With
--parent_lib PATH (a libdnnca.so built from the parent commit) input_sensitivity of this build and of that one, alternated in fresh
processes.  Writes profiles/sensitivity_rate.txt.

    python tools/sensitivity_rate.py [--batch 8] [--batches 8] [--parent_lib PATH] [--out profiles/sensitivity_rate.txt]"""
import argparse
import os
import subprocess
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
ap.add_argument('--parent_lib', default=None, help="the parent commit's libdnnca.so: input_sensitivity of both builds, alternated")
ap.add_argument('--ab_rounds', type=int, default=3)
ap.add_argument('--sens_only', action='store_true', help='(the child of --parent_lib) print input_sensitivity ms per config and stop')
a = ap.parse_args()
B, S, NB = a.batch, a.size, a.batches
if a.sens_only:
    # an older build of the library (DNNCA_LIB) lacks the entry points added since: declare only what it has
    import ctypes                                                 # noqa: E402
    from dnncancerannotator_amd import _lib                       # noqa: E402
    probe = ctypes.CDLL(_lib.LIB_PATH)
    for missing in [n for n in _lib.SIGNATURES if not hasattr(probe, n)]:
        del _lib.SIGNATURES[missing]
dev.init_device(0)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


CONFIGS = [('configs/unet.yaml', 'UNetAnnotator', 3, dict(n_filters_first=3, n_downsample=3, bn=False)),
           ('configs/mulmo_unet.yaml', 'MulmoUNetAnnotator', 3, dict(n_filters_first=16, n_downsample=4, bn=True))]
DEPLOY = dict(optimizer='adam', loss=dict(class_name='WeightedCrossentropy', config=dict(weight_mul=3.0)), enable_multigpu=False)



def timed(fn, reps):
    """ms per call: host clock around `reps` calls, each of which ends in a device synchronise"""
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


if a.sens_only:
    for cfg, model, C, opts in CONFIGS:
        dm = dev.DeviceModel('unet' if model == 'UNetAnnotator' else 'mulmo', C, S, S, B, rate=2, kernel_size=3, conv_stride=1,
                             padding='same', **opts)
        dm.forward(synthetic_batch(B, S, S, C, seed_x=3, seed_y=4)[0], return_prob=False)
        print('SENS %s %.4f' % (cfg, timed(lambda: dm.input_sensitivity(batch=B), 20)), flush=True)
        dm.close()
    sys.exit(0)

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
    # ---- integrated gradients on the same model and slices
    sens_ms = timed(lambda: dm.input_sensitivity(batch=B), 8)
    say('  integrated_gradients (black baseline, sums only) beside steps x input_sensitivity (%.2f ms per call, this build)' % sens_ms)
    for steps in (8, 32):
        ms = timed(lambda: dm.integrated_gradients(batch=B, steps=steps), 3)
        say('    steps %2d: %8.2f ms per call = %.2f x (steps x input_sensitivity = %.2f ms); per step %.2f ms' % (
            steps, ms, ms / (steps * sens_ms), steps * sens_ms, ms / steps))
    ms_map = timed(lambda: dm.integrated_gradients(batch=B, steps=8, baseline='mean', return_map=True), 3)
    say('    steps  8, mean baseline, map fetched to the host: %8.2f ms per call' % ms_map)
    dm.profile_reset()
    dm.profile_enable(1)
    for _ in range(2):
        dm.integrated_gradients(batch=B, steps=8, baseline='mean', return_map=True)
        dm.input_sensitivity(batch=B)
    dm.sync()
    rows = {r[0]: r for r in dm.profile()}
    dm.profile_enable(0)
    acc_bytes = 4.0 * B * S * S * C
    for name in ('sens_first', 'attr_first', 'attr_path_in', 'attr_base_in', 'attr_finish', 'attr_baseline_part', 'attr_prob_part',
                 'attr_sums', 'attr_baseline', 'attr_prob_sum'):
        if name in rows:
            _, n, ms, by, fl = rows[name]
            say('    %-22s launches %4d  %10.2f us per launch  (%.1f GB/s of its algorithmic bytes)' % (
                name, n // 2, ms / n * 1e3, by / (ms / n * 1e-3) / 1e9))      # `by`: per launch already
    if 'attr_first' in rows and 'sens_first' in rows:
        af, sf = rows['attr_first'][2] / rows['attr_first'][1] * 1e3, rows['sens_first'][2] / rows['sens_first'][1] * 1e3
        # 7 of the 8 launches read and write the accumulator, the first only writes it
        rmw = acc_bytes * (2 * 7 + 1) / 8
        say('    attr_first - sens_first = %.2f us per launch for %.1f MB of accumulator traffic (mean over the 8 steps): %s' % (
            af - sf, rmw / 1e6, ('%.0f GB/s' % (rmw / ((af - sf) * 1e-6) / 1e9)) if af > sf else 'no extra time measured'))
    dm.close()
if a.parent_lib:
    say('input_sensitivity, ms per batch of %d: this build and the parent commit\'s library, alternated, a fresh process each (20 calls)' % B)
    table = {}
    for r in range(a.ab_rounds):
        for which, lib in (('this', None), ('parent', os.path.abspath(a.parent_lib))):
            env = dict(os.environ)
            env.pop('DNNCA_LIB', None)
            if lib:
                env['DNNCA_LIB'] = lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--sens_only', '--batch', str(B), '--size', str(S)], env=env,
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError('the %s build failed:\n%s' % (which, r.stderr[-2000:]))
            for line in r.stdout.splitlines():
                if line.startswith('SENS '):
                    _, cfg, ms = line.split()
                    table.setdefault(cfg, {}).setdefault(which, []).append(float(ms))
    for cfg, t in table.items():
        say('  %-24s this build %s   parent %s' % (cfg, ' '.join('%.3f' % v for v in t['this']), ' '.join('%.3f' % v for v in t['parent'])))
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
