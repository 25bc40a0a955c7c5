#!/usr/bin/env python3
"""multires_rate.py -- what one MultiResUnet step costs at the reference's widths (n_filters_first 32) on 512 x 512 x 5 slices:
ms per train step and slices/s, the rate of the evaluation step, the per-kernel table of the train step (every launch between
HIP events), and the same train step with DNNCA_NO_JOIN=1 -- the residual joins composed of g_join_fwd / g_join_bwd and the generic
BatchNorm passes instead of the kernels of csrc/kernels_join.hip.  Both arms are models of ONE process on one GPU (the switch is
read when a model is created) and are timed in alternation, A B A B ..., so that clock and box differences fall on both.

    python tools/multires_rate.py [--batch 8] [--size 512] [--steps 5] [--rounds 3] [--budget 240] [--out profiles/multires_rate.txt]

The batch is halved until the allocation succeeds; steps and rounds shrink to keep the timed part within --budget seconds.  Times
are device times (HIP events around `steps` host-fed steps).  The step-level A/B cannot resolve the joins while the generic
convolutions take nearly all of the step, so the report ends with the kernels that differ between the arms, from the profile
tables of alternated steps: join_fwd + join_bwd against g_join_fwd + g_join_bwd + the 19 g_bn_stats_mean passes they bring back."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                # noqa: E402

from dnncancerannotator_amd import _lib                           # noqa: E402
from dnncancerannotator_amd import device as dev                  # noqa: E402
from dnncancerannotator_amd import models                         # noqa: E402
from dnncancerannotator_amd.synthetic import synthetic_batch      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--size', type=int, default=512)
ap.add_argument('--filters', type=int, default=32)
ap.add_argument('--steps', type=int, default=5)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--budget', type=float, default=240.0, help='seconds of timed train steps at most')
ap.add_argument('--out', default=None, help='append the report to this file as well')
a = ap.parse_args()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def build(batch, no_join):
    if no_join:
        os.environ['DNNCA_NO_JOIN'] = '1'
    try:
        return models.MultiResUnet(n_channels=5, n_filters_first=a.filters).build([batch, a.size, a.size, 5], seed=0)
    finally:
        os.environ.pop('DNNCA_NO_JOIN', None)


dev.init_device(0)
B = a.batch
arms = None
while B >= 1:
    built = []
    try:
        for no_join in (False, True):
            built.append(build(B, no_join))
        arms = {'join kernels': built[0], 'DNNCA_NO_JOIN=1': built[1]}
        break
    except _lib.DnncaError as e:
        for m in built:              # the retry must not hold what this attempt allocated
            m.close()
        if 'out of memory' not in str(e).lower():
            raise                    # not an allocation failure: a smaller batch would not help
        say('batch %d: %s' % (B, str(e).splitlines()[0][:120]))
        B //= 2
if arms is None:
    sys.exit('no batch fits')
x, y = synthetic_batch(B, a.size, a.size, 5, seed_x=3, seed_y=4)
say('MultiResUnet n_filters_first %d, %d x %d x %d x 5, f32, %d trainable values' % (a.filters, B, a.size, a.size, arms['join kernels'].n_trainable))


def timed(dm, fn, steps):
    dm.sync()
    dm.timer_start()
    for _ in range(steps):
        fn()
    return dm.timer_stop() / steps


cfg = {k: m.loss_cfg() for k, m in arms.items()}
train = {k: (lambda m=m, c=cfg[k]: m.train_step(x, y, 1e-4, c)) for k, m in arms.items()}
evalf = {k: (lambda m=m, c=cfg[k]: m.eval_step(x, y, c)) for k, m in arms.items()}
for k in arms:                       # warm-up: first launches, one-time tables
    train[k]()
    evalf[k]()
one = timed(arms['join kernels'], train['join kernels'], 1)
say('one train step: %.1f ms' % one)
while a.steps > 1 and one * 1e-3 * a.steps * a.rounds * 2 > a.budget:
    a.steps -= 1
while a.rounds > 2 and one * 1e-3 * a.steps * a.rounds * 2 > a.budget:
    a.rounds -= 1
ms = {k: [] for k in arms}
for r in range(a.rounds):
    for k in arms:                   # alternated: A B A B ...
        ms[k].append(timed(arms[k], train[k], a.steps))
    say('  round %d: ' % r + ', '.join('%s %.2f ms' % (k, ms[k][-1]) for k in arms))
for k in arms:
    med = float(np.median(ms[k]))
    say('train step, %-16s median %.2f ms (min %.2f, max %.2f; host-fed, %d steps x %d rounds) = %.1f slices/s' % (
        k + ':', med, min(ms[k]), max(ms[k]), a.steps, a.rounds, B / med * 1e3))
ja, jb = float(np.median(ms['join kernels'])), float(np.median(ms['DNNCA_NO_JOIN=1']))
say('join kernels against the generic composition: %.3f x the step time (%.2f ms less per step)' % (ja / jb, jb - ja))
ev = {k: timed(arms[k], evalf[k], a.steps) for k in arms}
for k in arms:
    say('eval step,  %-16s %.2f ms = %.1f slices/s' % (k + ':', ev[k], B / ev[k] * 1e3))

# per-kernel tables (every launch between events of its own: the sum exceeds the step), two steps per arm, alternated
for m in arms.values():
    m.profile_reset()
for r in range(2):
    for k, m in arms.items():
        m.profile_enable(1)
        train[k]()
        m.sync()
        m.profile_enable(0)
tables = {}
for k, m in arms.items():
    rows = sorted(m.profile(), key=lambda r: -r[2])
    m.profile_reset()
    tables[k] = {r[0]: r for r in rows}
    total = sum(r[2] for r in rows)
    say('per-kernel table of two train steps, %s (sum %.2f ms, %d launches):' % (k, total, sum(r[1] for r in rows)))
    for name, n, t, by, fl in rows:
        say('    %-18s launches %4d  total %9.3f ms  %5.1f %%  %8.1f us per launch  %7.1f GB/s  %8.1f GFLOP/s' % (
            name, n, t, 100 * t / total, t / n * 1e3, by * n / (t * 1e-3) / 1e9 if t else 0, fl * n / (t * 1e-3) / 1e9 if t else 0))
pick = lambda k, names: sum(tables[k][n][2] for n in names if n in tables[k]) / 2          # noqa: E731
ta = pick('join kernels', ('join_fwd', 'join_bwd', 'g_bn_stats_mean'))
tb = pick('DNNCA_NO_JOIN=1', ('g_join_fwd', 'g_join_bwd', 'g_bn_stats_mean'))
say('the kernels that differ, per train step: join_fwd + join_bwd + g_bn_stats_mean %.3f ms; g_join_fwd + g_join_bwd + g_bn_stats_mean '
    '%.3f ms (the composition) -> %.3f x, %.3f ms less' % (ta, tb, ta / tb if tb else 0, tb - ta))
for m in arms.values():
    m.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')
