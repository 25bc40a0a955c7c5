#!/usr/bin/env python3
"""optimizer_rate.py -- what the configurable optimizers (DeviceModel.set_optimizer) cost: ms per train step at 512 x 512
(device-resident batches, DeviceModel.train_step_dev) for configs/unet.yaml, mulmo_unet.yaml and unet_big.yaml at their own batch and
dtype with `optimizer: adam` and with each overlay of configs/additionals (adamw, clip_global_norm, sgd_nesterov); and the device
time per launch of grad_sqnorm, grad_clip_scale and opt_* beside g_adam / pg_fold_adam / pg_fold from the same visit, with the
achieved TB/s.

The plain step is also measured on a second library, built from the parent commit
    git worktree add <dir> <parent>;  cd <dir>;  DNNCA_BUILD_TAG=parent python -m dnncancerannotator_amd.build
(-> dnncancerannotator_amd/libdnnca_parent.so, copied beside this build's), alternated with this build's in one visit: with
`optimizer: adam` the step must be the step it was, i.e. inside the spread that two runs of one arm show.
Every arm is a child process of its own (a library is chosen when it is loaded, DNNCA_LIB), one at a time.

    python tools/optimizer_rate.py [--steps 100] [--only unet] [--parent-lib PATH] [--out profiles/optimizer_rate.txt]"""
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
# arm -> the keywords of set_optimizer (None: no call, `optimizer: adam`); the overlays' values
ARMS = {
    'adam': None,
    'adamw': dict(kind='adamw', weight_decay=0.004),
    'clip_global_norm': dict(kind='adam', global_clipnorm=1.0),
    'sgd_nesterov': dict(kind='sgd', momentum=0.9, nesterov=True),
    'opt_adam': dict(kind='adam', clipvalue=1e30),          # opt_adam alone, for the comparison with g_adam
}
LAUNCHES = ('pg_fold_adam', 'pg_fold', 'g_adam', 'grad_sqnorm', 'grad_clip_scale', 'opt_adam', 'opt_adamw', 'opt_sgd')
NEW_SYMBOLS = ('dnnca_model_set_optimizer', 'dnnca_last_grad_norm', 'dnnca_apply_gradients')


def child(name, arm, steps, profile):
    from dnncancerannotator_amd import _lib, device as dev
    from dnncancerannotator_amd.synthetic import synthetic_batch
    if os.environ.get('DNNCA_LIB'):                      # a library built from the parent does not export them
        for sym in NEW_SYMBOLS:
            _lib.SIGNATURES.pop(sym, None)
    arch, opts, C, B, S, dtype = CONFIGS[name]
    dev.init_device(0)
    m = dev.DeviceModel(arch, C, S, S, B, dtype=dtype, **opts)
    m.init_glorot(seed=2)
    if ARMS[arm] is not None:
        m.set_optimizer(**ARMS[arm])
    lr = 1e-2 if arm == 'sgd_nesterov' else 1e-3
    x, y = synthetic_batch(B, S, S, C, seed_x=100, seed_y=200)
    xb, yb = dev.DeviceBuffer(x), dev.DeviceBuffer(y)
    cfg = m.loss_cfg(weight_mul=3.0)
    for _ in range(20):
        m.train_step_dev(xb, yb, B, lr, cfg)
    m.sync()
    res = dict(name=name, arm=arm, n=int(m.n_trainable))
    if profile:
        m.profile_reset()
        m.profile_enable(1)
        for _ in range(steps):
            m.train_step_dev(xb, yb, B, lr, cfg)
        m.sync()
        res['kernels'] = [(k, n, ms / n * 1e3, by) for k, n, ms, by, fl in m.profile() if n and k in LAUNCHES]
    else:
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(steps):
                m.train_step_dev(xb, yb, B, lr, cfg)
            m.sync()
            dt = (time.perf_counter() - t0) / steps * 1e3
            best = dt if best is None else min(best, dt)
        res['ms'] = best
    m.close()
    print('RESULT ' + json.dumps(res), flush=True)


def run_child(name, arm, steps, profile=False, lib=None):
    env = dict(os.environ)
    if lib:
        env['DNNCA_LIB'] = lib
    cmd = [sys.executable, os.path.abspath(__file__), '--child', name, '--arm', arm, '--steps', str(steps)] + (['--profile'] if profile else [])
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    if out.returncode != 0:
        raise RuntimeError('%s failed (%d): %s' % (' '.join(cmd), out.returncode, out.stderr[-2000:]))
    return json.loads([l for l in out.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--only', default=None)
    ap.add_argument('--parent-lib', default=os.path.join(ROOT, 'dnncancerannotator_amd', 'libdnnca_parent.so'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optimizer_rate.txt'))
    ap.add_argument('--child', default=None)
    ap.add_argument('--arm', default='adam')
    ap.add_argument('--profile', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.arm, a.steps, a.profile)
    parent = a.parent_lib if os.path.exists(a.parent_lib) else None
    lines = ['configurable optimizers: ms per train step at 512 x 512, %d steps x 3 (best), device-resident batches; every arm twice, '
             'alternated' % a.steps]
    if not parent:
        lines.append('parent-commit library %s not found: the plain step on the parent build was not measured' % a.parent_lib)
    fmt = lambda v: '%.4f (%s)' % (min(v), ' '.join('%.4f' % t for t in v))      # noqa: E731
    for name in CONFIGS:
        if a.only and name != a.only:
            continue
        arms = {k: (k, None) for k in ('adam', 'adamw', 'clip_global_norm', 'sgd_nesterov')}
        if parent:
            arms['adam, parent build'] = ('adam', parent)
        ms = {k: [] for k in arms}
        for _ in range(2):                       # alternated: drift shows as a difference between the two runs of an arm
            for k in sorted(arms):
                ms[k].append(run_child(name, arms[k][0], a.steps, lib=arms[k][1])['ms'])
        lines.append('%-11s %s' % (name, '  '.join('%s %s' % (k, fmt(ms[k])) for k in sorted(arms))))
        lines.append('%-11s over adam: %s%s; spread of an arm (largest difference of its two runs) %.1f us' % (
            '', '  '.join('%s %+.1f us' % (k, (min(ms[k]) - min(ms['adam'])) * 1e3) for k in ('adamw', 'clip_global_norm', 'sgd_nesterov')),
            '; adam %+.1f us against the parent build' % ((min(ms['adam']) - min(ms['adam, parent build'])) * 1e3) if parent else '',
            max(abs(v[0] - v[1]) for v in ms.values()) * 1e3))
        for arm in ('adam', 'opt_adam', 'adamw', 'clip_global_norm', 'sgd_nesterov'):
            r = run_child(name, arm, 40, profile=True)
            for k, n, us, by in sorted(r['kernels']):
                rate = ' %5.1f B/parameter  %6.3f TB/s' % (by / r['n'], by / (us * 1e-6) / 1e12) if by else ''
                lines.append('  %-16s %-16s %5d launches  %8.2f us per launch %s (%d parameters)' % (arm, k, n, us, rate, r['n']))
        print('\n'.join(lines[-24:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
