#!/usr/bin/env python3
"""accumulate_rate.py -- what gradient accumulation (DeviceModel.set_accumulation) costs at 512 x 512 on device-resident batches
(DeviceModel.train_step_dev) for configs/unet.yaml, mulmo_unet.yaml and unet_big.yaml at their own batch and dtype:

  * ms per train step, averaged over whole cycles, at k = 1, 2 and 8, and the micro-step alone (k = 4096: no update falls into the
    run); the update step follows from them, cycle(k) = (k - 1) micro + update;
  * the k = 1 step against a library built from the parent commit
        git worktree add <dir> <parent>;  cd <dir>;  DNNCA_BUILD_TAG=parent python -m dnncancerannotator_amd.build
    (-> dnncancerannotator_amd/libdnnca_parent.so, copied beside this build's), alternated with this build's in one visit, with the
    run-to-run spread of an arm beside it: without the key the step must be the step it was;
  * device time per launch of grad_accumulate when it starts a cycle (a = g, 8 bytes per parameter) and when it adds (a += g, 12),
    with the achieved TB/s, at the three parameter counts; and of pg_fold_acc beside pg_fold on the pixel-group plan;
  * the launches of one unet.yaml step at k = 1 and of one micro-step.

Every arm is a child process of its own (a library is chosen when it is loaded, DNNCA_LIB), one at a time.

    python tools/accumulate_rate.py [--steps 48] [--only unet] [--parent-lib PATH] [--out profiles/accumulate_rate.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE = dict(rate=2, kernel_size=3, conv_stride=1, padding='same')
# name -> (arch, options, channels, batch, size, dtype): the shipped configs as they are benchmarked
CONFIGS = {
    'unet': ('unet', dict(BASE, n_filters_first=3, n_downsample=3, bn=False), 1, 8, 512, 'f32'),
    'mulmo_unet': ('mulmo', dict(BASE, n_filters_first=16, n_downsample=4, bn=True), 3, 8, 512, 'f32'),
    'unet_big': ('unet', dict(BASE, n_filters_first=64, n_downsample=4, bn=True), 1, 4, 512, 'bf16'),
}
MICRO = 4096          # the largest cycle: a run shorter than it holds micro-steps only
LAUNCHES = ('grad_accumulate', 'pg_fold_acc', 'pg_fold', 'pg_fold_adam', 'g_adam')
NEW_SYMBOLS = ('dnnca_model_set_accumulation', 'dnnca_get_accumulation', 'dnnca_grad_accumulate_of', 'dnnca_comm_collective_floats')


def child(name, k, steps, profile):
    """profile: '' (wall time per step), 'add' (every launch of the run adds), 'first' (every launch of the run starts a cycle)"""
    from dnncancerannotator_amd import _lib, device as dev
    from dnncancerannotator_amd.synthetic import synthetic_batch
    if os.environ.get('DNNCA_LIB'):                      # a library built from the parent does not export them
        for sym in NEW_SYMBOLS:
            _lib.SIGNATURES.pop(sym, None)
    arch, opts, C, B, S, dtype = CONFIGS[name]
    dev.init_device(0)
    m = dev.DeviceModel(arch, C, S, S, B, dtype=dtype, **opts)
    m.init_glorot(seed=2)
    if k > 1:
        m.set_accumulation(k)
    x, y = synthetic_batch(B, S, S, C, seed_x=100, seed_y=200)
    xb, yb = dev.DeviceBuffer(x), dev.DeviceBuffer(y)
    cfg = m.loss_cfg(weight_mul=3.0)
    steps = max(k, steps // k * k) if k < MICRO else steps          # whole cycles
    for _ in range(24):                                              # a multiple of every measured k: the run starts on a cycle
        m.train_step_dev(xb, yb, B, 1e-3, cfg)
    m.sync()
    res = dict(name=name, k=k, n=int(m.n_trainable), steps=steps)
    if profile:
        m.profile_reset()
        m.profile_enable(1)
        for _ in range(steps):
            if profile == 'first':
                m.set_accumulation(k)                                # position 0: the next launch starts a cycle
            m.train_step_dev(xb, yb, B, 1e-3, cfg)
        m.sync()
        rows = m.profile()
        res['kernels'] = [(q, n, ms / n * 1e3, by) for q, n, ms, by, fl in rows if n and q in LAUNCHES]
        res['launches_per_step'] = sum(n for _, n, _, _, _ in rows) / steps
    else:
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(steps):
                m.train_step_dev(xb, yb, B, 1e-3, cfg)
            m.sync()
            dt = (time.perf_counter() - t0) / steps * 1e3
            best = dt if best is None else min(best, dt)
        res['ms'] = best
    if k > 1 and not profile:
        res['plan_micro'] = [r[0] for r in m.plan(mode='train')] if k == MICRO else None
    m.close()
    print('RESULT ' + json.dumps(res), flush=True)


def run_child(name, k, steps, profile='', lib=None, env_extra=None):
    env = dict(os.environ)
    if lib:
        env['DNNCA_LIB'] = lib
    env.update(env_extra or {})
    cmd = [sys.executable, os.path.abspath(__file__), '--child', name, '--k', str(k), '--steps', str(steps)] + (['--profile', profile] if profile else [])
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    if out.returncode != 0:
        raise RuntimeError('%s failed (%d): %s' % (' '.join(cmd), out.returncode, out.stderr[-2000:]))
    return json.loads([line for line in out.stdout.splitlines() if line.startswith('RESULT ')][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=48)
    ap.add_argument('--only', default=None)
    ap.add_argument('--parent-lib', default=os.path.join(ROOT, 'dnncancerannotator_amd', 'libdnnca_parent.so'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'accumulate_rate.txt'))
    ap.add_argument('--child', default=None)
    ap.add_argument('--k', type=int, default=1)
    ap.add_argument('--profile', default='')
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.k, a.steps, a.profile)
    parent = a.parent_lib if os.path.exists(a.parent_lib) else None
    lines = ['gradient accumulation: ms per train step at 512 x 512, %d steps x 3 (best), device-resident batches; every arm twice, '
             'alternated' % a.steps]
    if not parent:
        lines.append('parent-commit library %s not found: the k = 1 step on the parent build was not measured' % a.parent_lib)
    fmt = lambda v: '%.4f (%s)' % (min(v), ' '.join('%.4f' % t for t in v))      # noqa: E731
    for name in CONFIGS:
        if a.only and name != a.only:
            continue
        arms = {'k=1': (1, None), 'k=2': (2, None), 'k=8': (8, None), 'micro-step': (MICRO, None)}
        if parent:
            arms['k=1, parent build'] = (1, parent)
        ms, plan = {q: [] for q in arms}, None
        for _ in range(2):                       # alternated: drift shows as a difference between the two runs of an arm
            for q in sorted(arms):
                r = run_child(name, arms[q][0], a.steps, lib=arms[q][1])
                ms[q].append(r['ms'])
                plan = r.get('plan_micro') or plan
        best = {q: min(v) for q, v in ms.items()}
        lines.append('%-11s %s' % (name, '  '.join('%s %s' % (q, fmt(ms[q])) for q in sorted(arms))))
        updates = ['from k=%d %.4f' % (k, k * best['k=%d' % k] - (k - 1) * best['micro-step']) for k in (2, 8)]
        lines.append('%-11s micro-step %.4f ms (%+.1f us against the k = 1 step); update step = k avg(k) - (k - 1) micro: %s ms; spread of an '
                     'arm (largest difference of its two runs) %.1f us%s' % (
                         '', best['micro-step'], (best['micro-step'] - best['k=1']) * 1e3, ', '.join(updates),
                         max(abs(v[0] - v[1]) for v in ms.values()) * 1e3,
                         '; k = 1 %+.1f us against the parent build' % ((best['k=1'] - best['k=1, parent build']) * 1e3) if parent else ''))
        # device time per launch.  The pixel-group plan folds the add into pg_fold_acc: DNNCA_NO_FOLD_ACC shows the launch alone
        alone = {'DNNCA_NO_FOLD_ACC': '1'}
        for label, k, profile, env in (('k=1', 1, 'add', None), ('micro-step', MICRO, 'add', None),
                                       ('add, unfused', MICRO, 'add', alone), ('first, unfused', MICRO, 'first', alone)):
            r = run_child(name, k, 40, profile=profile, env_extra=env)
            if name == 'unet' and label in ('k=1', 'micro-step'):
                lines.append('  %-15s %.1f launches per step%s' % (label, r['launches_per_step'],
                                                                    ': ' + ' '.join(plan) if label == 'micro-step' and plan else ''))
            for q, n, us, by in sorted(r['kernels']):
                rate = ' %5.1f B/parameter  %6.3f TB/s' % (by / r['n'], by / (us * 1e-6) / 1e12) if by else ''
                lines.append('  %-15s %-16s %5d launches  %8.2f us per launch %s (%d parameters)' % (label, q, n, us, rate, r['n']))
        print('\n'.join(lines[-24:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
