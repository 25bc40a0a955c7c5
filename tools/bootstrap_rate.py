#!/usr/bin/env python3
"""bootstrap_rate.py -- cost of `evaluate --bootstrap` on one GPU.

  (a) call time: DeviceModel.bootstrap_detection at (E exams, N candidates, R replicates) = (100, 500, 2 000), (1 000, 5 000, 10 000)
      and (16 384, 2^20, 2 000), and DeviceModel.bootstrap_sums at K = 24 columns over the same (E, R): HIP events around every
      launch (dnnca_profile_*) and the wall time of the call (host checks, packing, sorting, copies and the synchronisation
      included), `--reps` calls each, median and spread.  Drawn inputs: a third of the exams positive, hits on half of their
      candidates, levels in runs of 1 .. 3.
  (b) share of a checkpoint: engine._detection_pass over `--exams` synthetic exams of `--slices` slices of `--size`^2 with the
      random network, without and with bootstrap = 2 000 replicates, alternated in one process, `--reps` times.
  (c) with --parent-lib PATH (a library built from the parent commit): the `aug_intensity` launch (Rician noise on every plane of
      8 x 512 x 512 x 3: the arm that runs Philox) on that library and on this one, one fresh process per measurement, alternated;
      the run-to-run spread of either arm is the margin.

    python tools/bootstrap_rate.py [--reps 10] [--parent-lib PATH] [--out profiles/bootstrap_rate.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--exams', type=int, default=100)
ap.add_argument('--slices', type=int, default=4)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--parent-lib', default=None)
ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'bootstrap_rate.txt'))
ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)               # child: intensity
a = ap.parse_args()
SHAPES = ((100, 500, 2000), (1000, 5000, 10000), (16384, 1 << 20, 2000))
UNET = dict(n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, padding='same', bn=False)


def spread(ts):
    return statistics.median(ts), min(ts), max(ts)


def leg_intensity():
    """child: the aug_intensity launch with noise on every plane, event-bracketed; the library is DNNCA_LIB's"""
    from dnncancerannotator_amd import _lib
    if os.environ.get('DNNCA_LIB'):
        for name in ('dnnca_bootstrap_sums', 'dnnca_bootstrap_detection'):
            _lib.SIGNATURES.pop(name, None)                                   # a library built from the parent does not export them
    from dnncancerannotator_amd import augment
    from dnncancerannotator_amd import device as dev
    dev.init_device(0)
    B, S, C = 8, 512, 3
    rng = np.random.default_rng(0)
    dm = dev.DeviceModel('unet', C, S, S, B, **UNET)
    dm.init_glorot(0)
    x = dev.DeviceBuffer(rng.random((B, S, S, C), np.float32))
    conf = augment.parse_augment_options({'random_intensity': dict(noise={'sigma': [0.0, 0.05]})}, (S, S)).intensity
    rec = augment.draw_intensity(rng, B, conf, C)
    for _ in range(5):
        dm.intensity(x, rec)
    dm.sync()
    ts = []
    for _ in range(a.reps):
        dm.profile_reset()
        dm.profile_enable(1)
        for _ in range(20):
            dm.intensity(x, rec)
        dm.sync()
        rows = [r for r in dm.profile() if r[0] == 'aug_intensity']
        dm.profile_enable(0)
        ts.append(sum(r[2] for r in rows) / sum(r[1] for r in rows))
    print('INTENSITY\t%.5f\t%.5f\t%.5f' % spread(ts), flush=True)
    dm.close()


def drawn_inputs(E, N, seed):
    from dnncancerannotator_amd import _lib
    rng = np.random.default_rng(seed)
    exams = np.zeros(E, _lib.BOOTSTRAP_EXAM_DTYPE)
    exams['tumours'] = (rng.random(E) < 1 / 3) * rng.integers(1, 3, E)
    exams['score_rank'] = np.unique(rng.integers(0, E, E), return_inverse=True)[1]
    cands = np.zeros(N, _lib.BOOTSTRAP_CANDIDATE_DTYPE)
    cands['exam'] = rng.integers(0, E, N)
    cands['hit'] = (rng.random(N) < 0.5) & (exams['tumours'][cands['exam']] > 0)
    step = (rng.random(N) < 0.5).astype(np.int32)
    step[0] = 0
    cands['level'] = np.cumsum(step)
    return exams, cands


class Exams:
    """`exams` synthetic exams of `slices` slices: batches (x, y, paths, sliceIDs) of 8 slices"""

    def __init__(self, exams, slices, size):
        from dnncancerannotator_amd.data import Spec
        from dnncancerannotator_amd.synthetic import synthetic_batch
        self.x, self.y = synthetic_batch(exams * slices, size, size, 1, seed_x=3, seed_y=4)
        self.y[::3] = 0                                                       # exams without a tumour among them
        self.paths = ['/synthetic/p%d/e0/mri' % (i // slices) for i in range(exams * slices)]
        self.ids = [i % slices for i in range(exams * slices)]
        self.element_spec = (Spec((8,) + self.x.shape[1:], np.float32), Spec((8,) + self.y.shape[1:], np.float32))

    def __iter__(self):
        for i in range(0, len(self.x), 8):
            yield self.x[i:i + 8], self.y[i:i + 8], self.paths[i:i + 8], self.ids[i:i + 8]


def main():
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    from dnncancerannotator_amd import _lib, casewise
    from dnncancerannotator_amd import device as dev
    from dnncancerannotator_amd import engine
    dev.init_device(0)
    dm = dev.DeviceModel('unet', 1, 64, 64, 3, **UNET)
    say('bootstrap over exams, library %s, %d calls per figure (median; min .. max)' % (os.path.basename(_lib.LIB_PATH), a.reps))

    def measure(what, name, fn):
        fn()                                                                  # warm-up: the workspace
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        dm.profile_reset()
        dm.profile_enable(1)
        for _ in range(a.reps):
            fn()
        dm.sync()
        rows = [r for r in dm.profile() if r[0] == name]
        dm.profile_enable(0)
        dm.profile_reset()
        n, ms = sum(r[1] for r in rows), sum(r[2] for r in rows)
        say('  %-58s wall %9.3f ms (%.3f .. %.3f); %s %.1f launches per call, %9.3f ms per launch' % (
            (what,) + spread(ts) + (name, n / a.reps, ms / max(n, 1))))
    for E, N, R in SHAPES:
        exams, cands = drawn_inputs(E, N, E)
        cols = np.random.default_rng(E).integers(0, 9, (E, 24)).astype(np.int32)
        strata = casewise.bootstrap_pool(exams['tumours'] > 0, True)
        measure('bootstrap_detection E %d N %d R %d' % (E, N, R), 'boot_detect', lambda: dm.bootstrap_detection(exams, cands, R, seed=1))
        measure('bootstrap_detection E %d N %d R %d stratified' % (E, N, R), 'boot_detect',
                lambda: dm.bootstrap_detection(exams, cands, R, seed=1, strata=strata))
        measure('bootstrap_sums      E %d K 24 R %d' % (E, R), 'boot_sums', lambda: dm.bootstrap_sums(cols, R, seed=1))
    dm.close()

    # (b) the pass of evaluate --detection without and with the bootstrap
    e = engine.TFKerasModel(dict(model='UNetAnnotator', deploy_options=dict(optimizer='adam', enable_multigpu=False),
                                 model_options=dict(UNET)))
    ds = Exams(a.exams, a.slices, a.size)
    e._build(ds)
    det = engine.check_detection(True, min_area=4)
    boot = engine.check_bootstrap(2000, detection=True)
    found = e._detection_pass(ds, 1, det, bootstrap=boot)                     # warm-up of either arm
    e._detection_pass(ds, 1, det)
    took = {False: [], True: []}
    for i in range(a.reps):
        for arm in ((False, True), (True, False))[i % 2]:
            t0 = time.perf_counter()
            e._detection_pass(ds, 1, det, **(dict(bootstrap=boot) if arm else {}))
            took[arm].append((time.perf_counter() - t0) * 1e3)
    res = found[0][0]
    say('  evaluate --detection pass, %d exams x %d slices of %d^2 (%s candidates, %s tumours):' % (a.exams, a.slices, a.size, res[4], res[3]))
    say('    without --bootstrap       %9.2f ms (%.2f .. %.2f)' % spread(took[False]))
    say('    with    --bootstrap 2000  %9.2f ms (%.2f .. %.2f)' % spread(took[True]))
    say('    the flag adds %.1f %% to the pass (device call, replicate values, intervals and the lines of the two files)' % (
        100.0 * (statistics.median(took[True]) / statistics.median(took[False]) - 1.0)))

    # (c) aug_intensity on the parent's library and on this one
    if a.parent_lib:
        got = {'parent': [], 'this': []}
        for i in range(4):
            for arm in (('parent', 'this'), ('this', 'parent'))[i % 2]:
                env = dict(os.environ)
                env.pop('DNNCA_LIB', None)
                if arm == 'parent':
                    env['DNNCA_LIB'] = os.path.abspath(a.parent_lib)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', 'intensity', '--reps', str(a.reps)], env=env,
                                     capture_output=True, text=True, timeout=300)
                if out.returncode != 0:
                    raise SystemExit('the intensity leg failed (%d):\n%s' % (out.returncode, out.stderr[-2000:]))
                got[arm].append(float([l for l in out.stdout.splitlines() if l.startswith('INTENSITY')][0].split('\t')[1]))
        say('  aug_intensity, Rician noise on every plane of 8 x 512 x 512 x 3, ms per launch (medians of 4 fresh processes, alternated):')
        for arm in ('parent', 'this'):
            say('    %-7s %s  median %.5f, spread %.5f' % (arm, ' '.join('%.5f' % t for t in got[arm]), statistics.median(got[arm]),
                                                           max(got[arm]) - min(got[arm])))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    leg_intensity() if a.leg == 'intensity' else main()
