#!/usr/bin/env python3
"""lesion_rate.py -- cost of the lesion table of `annotator predict` at 8 x 512 x 512 (configs/unet.yaml): the dnnca_lesion_table
call alone on probabilities resident in the model's buffer (wall time per call and device time per launch, HIP events around
every launch), `annotate` with and without masks, and the forward alone for scale.  The yardstick is
dnnca_region_confusion_slices with one one-threshold spec on the same probabilities: it runs the shared stages twice (label plane
and prediction plane) plus pairs, match and count.

    python tools/lesion_rate.py [--batch 8] [--size 512] [--reps 20] [--out profiles/lesion_rate.txt]
    DNNCA_LIB=<a library built from the parent commit> python tools/lesion_rate.py --yardstick      # the yardstick alone
    python tools/lesion_rate.py --link              # also: lesion_table_linked, annotate(link_slices=True), the pair table's worst case
    DNNCA_LIB=<a library from before the links> python tools/lesion_rate.py                         # the unlinked legs on it
    python tools/lesion_rate.py --link --match      # also: lesion_table_matched against lesion_table_linked
    DNNCA_LIB=<a library built from the parent commit> python tools/lesion_rate.py --link            # the linked legs on it
    python tools/lesion_rate.py --link --match --surface         # also: surface_distances against lesion_table_matched
    DNNCA_LIB=<a library built from the parent commit> python tools/lesion_rate.py --link --match    # the matched legs on it
    python tools/lesion_rate.py --tta flips         # test-time augmentation alone: forward_tta against the plain forward
    python tools/lesion_rate.py --tta flips --uncertainty        # also: the spread of the views against the mean alone
    python tools/lesion_rate.py --calibration       # calibration and temperature scaling alone
    DNNCA_LIB=<a library built from the parent commit> python tools/lesion_rate.py --tta flips      # forward / forward_tta on it
    python tools/lesion_rate.py --features          # per-lesion features alone: the two launches, the call against its siblings
    DNNCA_LIB=<a library built from the parent commit> python tools/lesion_rate.py --table_only     # plain lesion_table on it
    python tools/lesion_rate.py --detection         # the detection map alone: its launches, the call beside lesion_table, the pass
    DNNCA_LIB=<a library built from the parent commit> python tools/lesion_rate.py --matched_only   # plain lesion_table_matched on it
    python tools/lesion_rate.py --ensemble 5 [--tta flips] [--uncertainty]     # forward_ensemble alone, against its parts
    python tools/lesion_rate.py --refine            # mask refinement alone: its launches, the refined call against the plain one

--link adds the cost of linking neighbouring slices: lesion_table_linked against lesion_table (wall time per call, device time of
the three link launches), its worst case for the pair table (a checkerboard on itself: every other pixel a lesion of its own in
both slices, (hw + 1) / 2 keys per slice) and `annotate` with link_slices.

--match adds the cost of `evaluate --exam_lesions`: lesion_table_matched (both planes, three sets of pair tables) against
lesion_table_linked on the same probabilities, and passes over the data set in the manner of `annotate` -- a forward and one call
per batch, the flags from the slice numbers -- with the linked and the matched call alternated in one process.

--surface adds the cost of `evaluate --surface_distances`: surface_distances (the prediction plane's shared stages, the label's
prep, then surface_edges / surface_cols / surface_sample) per call with its launches event-bracketed, and a forward + surface pass
against a forward + matched pass over the same batches, alternated in one process.

--tta MODE (flips, d4) measures DeviceModel.forward_tta against DeviceModel.forward on the same host batch and nothing else: wall time
per call (both upload the batch once), device time per call (every launch event-bracketed) and the share of the two kernels of
kernels_tta.hip (tta_view_in, tta_accumulate) in it.

--tta MODE --uncertainty adds the spread of the views: forward_tta_spread against forward_tta (wall and device time per call, the
two alternated), tta_moments against tta_accumulate per launch, lesion_table_spread against lesion_table on the mean and spread that
forward_tta_spread left on the device, and spread_by_outcome alone (one and three thresholds).

--calibration measures DeviceModel.calibration and DeviceModel.scale_temperature and nothing else: device time per launch of
calib_bins on a uniform random plane and on a real-like one (99 % of the pixels below 0.01 and of class 0: what the grouping of a
wave's lanes by key is for), of calib_nll / calib_nll_sum at the 41 temperatures of casewise.CALIBRATION_GRID and of prob_temperature;
wall time per call; and a forward_tta_spread + calibration pass against a forward_tta_spread + spread_by_outcome pass (the pass of
`evaluate --uncertainty`: the same forward, one table call), alternated in one process.

--features measures DeviceModel.lesion_table_features on a model of 3 input channels and nothing else: lesion_features and
lesion_ring per launch (event-bracketed) and the call's wall time against lesion_table and lesion_table_spread, alternated, on the
mean that forward_tta_spread left on the device at the two thresholds of --uncertainty (next to no lesion; thousands of specks), on
the drawn discs, and on the worst case (every slice one lesion: every pixel adds to one record and to its histogram).
--table_only measures plain lesion_table on the drawn discs and nothing else: run it on this build and on a library built from the
parent commit, in turns.

--detection measures DeviceModel.detection_map (in place, the plane put back before every call) and nothing else, on three planes:
the output of the random network as it is (smooth, pushed up: a candidate grows over much of the plane), the drawn discs, and the
network's output above its 99th percentile on zeros (thousands of specks: every round finds a region below min_area).  Per plane the
det_* launches event-bracketed and the call's wall time beside lesion_table on the same plane; then a forward + detection_map +
lesion_table_matched pass against a forward + lesion_table_matched pass, alternated in one process.
--matched_only measures plain lesion_table_matched on the drawn discs and nothing else: run it on this build and on a library built
from the parent commit, in turns.

--ensemble M measures DeviceModel.forward_ensemble of M members (under --tta MODE when given, with the spread under --uncertainty,
which here needs no --tta) and nothing else: wall time per call against M plain forwards and against M forward_tta_spread calls on
the same host batch, alternated; device time per call and ens_join per launch (event-bracketed); and what one more member costs
beyond its forward -- the device-to-device copy of its weights and BatchNorm state -- for the widths of configs/unet.yaml,
mulmo_unet.yaml and unet_big.yaml on a 1 x 16 x 16 batch, where the forward is small: (ensemble of M - ensemble of 1) / (M - 1)
against the plain forward there.  (forward / forward_tta on this build against a library built from the parent commit: --tta MODE
on either, in turns.)

--refine measures DeviceModel.set_lesion_refine and nothing else, on the three planes of --detection (the random network's output
as it is, the drawn discs, specks): hysteresis, a 5 x 5 closing and hole filling each alone and all three together.  Per plane and
setting the refined lesion_table against the plain one (wall time per call, alternated, and the ratio of the best medians) and the
region_* launches of the refined call event-bracketed: the stage's own six and the region_ccl_* sets it adds.  (Plain lesion_table /
lesion_table_matched on this build against a library built from the parent commit: --table_only / --matched_only on either, in turns.)

The probabilities are drawn: the synthetic labels' discs at 0.55 .. 0.95 on a background of 0 .. 0.45 (a few lesions per slice,
as a trained model gives), put into the model's probability buffer by pixel_confusion_of."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dnncancerannotator_amd import _lib                           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--size', type=int, default=512)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--batches', type=int, default=8)
ap.add_argument('--yardstick', action='store_true', help='region_confusion_slices alone (also on a library without the lesion table)')
ap.add_argument('--link', action='store_true', help='also measure lesion_table_linked and annotate(link_slices=True)')
ap.add_argument('--match', action='store_true', help='also measure lesion_table_matched against lesion_table_linked (needs --link)')
ap.add_argument('--surface', action='store_true', help='also measure surface_distances against lesion_table_matched (needs --match)')
ap.add_argument('--tta', default=None, metavar='MODE', help='measure forward_tta(MODE) against the plain forward, and nothing else')
ap.add_argument('--uncertainty', action='store_true', help='with --tta: also measure forward_tta_spread, lesion_table_spread, spread_by_outcome')
ap.add_argument('--calibration', action='store_true', help='measure calibration and scale_temperature, and nothing else')
ap.add_argument('--features', action='store_true', help='measure lesion_table_features against lesion_table / lesion_table_spread, and nothing else')
ap.add_argument('--table_only', action='store_true', help='measure plain lesion_table, and nothing else (also on a library built from the parent)')
ap.add_argument('--detection', action='store_true', help='measure detection_map beside lesion_table and in an evaluation pass, and nothing else')
ap.add_argument('--matched_only', action='store_true', help='measure plain lesion_table_matched, and nothing else (also on a library built from the parent)')
ap.add_argument('--ensemble', type=int, default=0, metavar='M', help='measure forward_ensemble of M members against its parts, and nothing else')
ap.add_argument('--refine', action='store_true', help='measure the mask refinement against the plain lesion_table, and nothing else')
ap.add_argument('--out', default=None, help='append the report to this file as well')
a = ap.parse_args()
if a.features:                                                   # its siblings are lesion_table and lesion_table_spread
    a.tta, a.uncertainty = a.tta or 'flips', True
else:
    _lib.SIGNATURES.pop('dnnca_lesion_table_features', None)     # a library built from the parent does not export it
if a.calibration:                                                # its yardstick is the pass of --tta flips --uncertainty
    a.tta, a.uncertainty = a.tta or 'flips', True
else:
    for name in ('dnnca_calibration', 'dnnca_prob_temperature'):
        _lib.SIGNATURES.pop(name, None)                          # a library built from the parent does not export them
if a.detection or a.matched_only:                                # their yardstick is lesion_table_matched
    a.link = a.match = True
if not a.detection:
    _lib.SIGNATURES.pop('dnnca_detection_map', None)             # a library built from the parent does not export it
if not a.refine:
    for name in ('dnnca_model_set_lesion_refine', 'dnnca_model_get_lesion_refine'):
        _lib.SIGNATURES.pop(name, None)                          # a library built from the parent does not export them
if a.yardstick:
    _lib.SIGNATURES.pop('dnnca_lesion_table', None)              # a library built from the parent does not export it
if not a.link:
    _lib.SIGNATURES.pop('dnnca_lesion_table_linked', None)       # nor does one from before the links

if a.match and not a.link:
    ap.error('--match needs --link')
if not a.match:
    _lib.SIGNATURES.pop('dnnca_lesion_table_matched', None)      # nor does one from before the matched call

if a.surface and not a.match:
    ap.error('--surface needs --link --match')
if not a.surface:
    _lib.SIGNATURES.pop('dnnca_surface_distances', None)         # nor does one from before the boundary distances

if not a.tta and not a.ensemble:
    for name in ('dnnca_forward_tta', 'dnnca_tta_view_of', 'dnnca_tta_mean_of'):
        _lib.SIGNATURES.pop(name, None)                          # nor does one from before test-time augmentation

if not a.ensemble:
    for name in ('dnnca_model_set_members', 'dnnca_member_store', 'dnnca_member_get', 'dnnca_forward_ensemble', 'dnnca_get_ensemble_spread',
                 'dnnca_ensemble_of'):
        _lib.SIGNATURES.pop(name, None)                          # nor does one from before the ensembles
elif not 1 <= a.ensemble <= 16:
    ap.error('--ensemble M: 1..16')

if a.uncertainty and not a.tta and not a.ensemble:
    ap.error('--uncertainty needs --tta MODE')
if not a.uncertainty and not a.ensemble:
    for name in ('dnnca_forward_tta_spread', 'dnnca_tta_spread_of', 'dnnca_get_tta_spread', 'dnnca_lesion_table_spread',
                 'dnnca_spread_by_outcome'):
        _lib.SIGNATURES.pop(name, None)                          # nor does one from before the spread

from dnncancerannotator_amd import device as dev                  # noqa: E402
from dnncancerannotator_amd.data import ArrayDataset              # noqa: E402
from dnncancerannotator_amd.engine import TFKerasModel            # noqa: E402
from dnncancerannotator_amd.synthetic import synthetic_batch      # noqa: E402
import numpy as np                                                # noqa: E402

B, S, R, NB = a.batch, a.size, a.reps, a.batches
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def wall(fn):
    fn()                                                          # warm-up (workspace, buffers)
    ts = []
    for _ in range(R):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def per_launch(dm, fn, prefixes):
    dm.profile_reset()
    dm.profile_enable(1)
    for _ in range(R):
        fn()
    dm.sync()
    rows = [r for r in dm.profile() if r[0].startswith(prefixes)]
    dm.profile_enable(0)
    dm.profile_reset()
    say('    device time %.3f ms per call (event-bracketed launches)' % (sum(r[2] for r in rows) / R))
    for name, n, ms, by, fl in sorted(rows, key=lambda r: -r[2]):
        say('      %-22s launches/call %4.1f  %9.2f us per launch' % (name, n / R, ms / n * 1e3))


dev.init_device(0)
x, y = synthetic_batch(B, S, S, 3 if a.features else 1, seed_x=3, seed_y=4)
yy, xx = np.mgrid[0:S, 0:S]
prob = np.where(y > 0.5, 0.55 + ((xx * 5 + yy * 3) % 27) / 64.0, ((xx * 7 + yy * 11) % 30) / 64.0).astype(np.float32)
DEPLOY = dict(optimizer='adam', enable_multigpu=False)
e = TFKerasModel(dict(model='UNetAnnotator', deploy_options=DEPLOY,
                      model_options=dict(rate=2, kernel_size=3, conv_stride=1, padding='same', n_filters_first=3, n_downsample=3, bn=False)))
ds = ArrayDataset(np.concatenate([x] * NB), None, B, meta_path='/synthetic/p0/e0/mri', labels=False) if not a.yardstick else \
    ArrayDataset(x, y, B)
e._build(ds)
dm = e.device_model
say('%s: %d x %d x %d, library %s' % ('yardstick' if a.yardstick else 'lesion features' if a.features else 'plain lesion table' if a.table_only else
                                      'mask refinement' if a.refine else 'detection map' if a.detection else 'plain matched table' if a.matched_only else
                                      'ensemble' if a.ensemble else 'calibration' if a.calibration else 'test-time augmentation' if a.tta else 'lesion table', B, S, S, os.path.basename(_lib.LIB_PATH)))
if a.ensemble:
    from dnncancerannotator_amd import tta as tta_modes           # noqa: E402
    M = a.ensemble
    views = tta_modes.mask_of(a.tta, S, S) if a.tta else 1
    n_views = bin(views).count('1')
    spread = bool(a.uncertainty)

    def drawn_members(model, n):
        rng = np.random.default_rng(11)
        out = []
        for _ in range(n):
            model.init_glorot(seed=int(rng.integers(1 << 30)))
            out.append((model.get_params(), model.get_state()))
        return out
    dm.set_members(drawn_members(dm, M))
    say('  %d members, %d view(s) each, spread %s; %d weights + %d state floats per member' % (M, n_views, spread, dm.n_trainable, dm.n_state))

    def ensemble():
        dm.forward_ensemble(x, views, spread=spread, return_prob=False)
        dm.sync()

    def forwards():
        for _ in range(M):
            dm.forward(x, return_prob=False)
        dm.sync()

    def spreads():
        for _ in range(M):
            dm.forward_tta_spread(x, 0x0F, return_prob=False, return_spread=False)
        dm.sync()
    took = {}
    arms = (('forward_ensemble', ensemble), ('%d x forward' % M, forwards), ('%d x forward_tta_spread(flips)' % M, spreads))
    for name, fn in arms * 3:                                     # alternated
        took.setdefault(name, []).append(wall(fn))
    for name, runs in took.items():
        for med, lo, hi in runs:
            say('  %-32s %.3f ms per call, upload(s) included (median of %d; %.3f .. %.3f)' % (name, med, R, lo, hi))
    best = {name: min(r[0] for r in runs) for name, runs in took.items()}
    say('  forward_ensemble / %d x forward, wall (best medians): %.3f;  / %d x forward_tta_spread(flips): %.3f' % (
        M, best[arms[0][0]] / best[arms[1][0]], M, best[arms[0][0]] / best[arms[2][0]]))
    say('  run-to-run, forward_ensemble: medians %s' % ', '.join('%.3f' % r[0] for r in took[arms[0][0]]))
    dm.profile_reset()
    dm.profile_enable(1)
    for _ in range(R):
        ensemble()
    rows = dm.profile()
    dm.profile_enable(0)
    dm.profile_reset()
    total = sum(r[2] for r in rows) / R
    say('  device time per call (event-bracketed launches; the weight copies are not launches): %.3f ms' % total)
    for name, n, ms, by, fl in [r for r in rows if r[0].startswith(('ens_', 'tta_'))]:
        say('    %-22s launches/call %4.1f  %9.2f us per launch  %7.1f GB/s' % (name, n / R, ms / n * 1e3, by / (ms / n * 1e-3) / 1e9))
    dm.close()
    # what one more member costs beyond its forward: the copy of its weights
    BASE = dict(rate=2, kernel_size=3, conv_stride=1, padding='same')
    for name, arch, opts, ch, dtype in (('unet', 'unet', dict(BASE, n_filters_first=3, n_downsample=3, bn=False), 1, 'f32'),
                                        ('mulmo_unet', 'mulmo', dict(BASE, n_filters_first=16, n_downsample=4, bn=True), 3, 'f32'),
                                        ('unet_big', 'unet', dict(BASE, n_filters_first=64, n_downsample=4, bn=True), 1, 'bf16')):
        m = dev.DeviceModel(arch, ch, 16, 16, 1, dtype=dtype, **opts)
        xs = np.random.default_rng(12).random((1, 16, 16, ch)).astype(np.float32)
        members = drawn_members(m, M)
        res = {}
        for rnd in range(2):
            for k in (1, M):
                m.set_members(members[:k])
                res.setdefault(k, []).append(wall(lambda: (m.forward_ensemble(xs, 1, return_prob=False), m.sync()))[0])
            res.setdefault('forward', []).append(wall(lambda: (m.forward(xs, return_prob=False), m.sync()))[0])
        one, many, fwd = min(res[1]), min(res[M]), min(res['forward'])
        step = (many - one) / max(M - 1, 1)
        say('  %-11s %9d floats per member: ensemble of 1 %.3f ms, of %d %.3f ms: %.1f us per further member; forward alone %.3f ms; '
            'further member - forward: %.1f us (%.1f MB copied)' % (name, m.n_trainable + m.n_state, one, M, many, step * 1e3, fwd,
                                                                   (step - fwd) * 1e3, (m.n_trainable + m.n_state) * 4 / 1e6))
        m.close()
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0)
if a.table_only:
    dm.pixel_confusion_of(prob, y, [0.5])
    for mask in (True, False) * 2:
        med, lo, hi = wall(lambda: dm.lesion_table(batch=B, threshold=0.5, filter_size=5, mask=mask))
        say('  lesion_table(mask=%s): %.3f ms per call (median of %d; %.3f .. %.3f)' % (mask, med, R, lo, hi))
    dm.close()
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0)
if a.matched_only:
    dm.pixel_confusion_of(prob, y, [0.5])
    flags = [b > 0 for b in range(B)]
    for _ in range(4):
        med, lo, hi = wall(lambda: dm.lesion_table_matched(y, continues=flags, batch=B, threshold=0.5, filter_size=5))
        say('  lesion_table_matched(mask=False): %.3f ms per call (median of %d; %.3f .. %.3f)' % (med, R, lo, hi))
    dm.close()
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0)
if a.refine:
    dm.forward(x, return_prob=False)
    net = dm.last_prob(B)
    specks = np.where(net >= np.percentile(net, 99.0), net, 0).astype(np.float32)
    planes = (('network output as it is', net, float(np.percentile(net, 60.0)), float(np.percentile(net, 40.0))),
              ('drawn discs', prob, 0.5, 0.3),
              ('network output above its 99th percentile', specks, float(np.percentile(net, 99.5)), float(np.percentile(net, 98.0))))
    settings = (('hysteresis', dict(hysteresis=True)), ('closing 5', dict(closing=5)), ('fill_holes', dict(fill_holes=True)),
                ('all three', dict(hysteresis=True, closing=5, fill_holes=True)))
    for what, plane, thr, low in planes:
        dm.pixel_confusion_of(plane, y, [0.5])                    # the plane into the model's buffer (synchronises)
        kw = dict(batch=B, threshold=thr, filter_size=5, mask=False, max_lesions=4096)
        say('  %s: threshold %.6f, hysteresis %.6f' % (what, thr, low))
        for name, cfg in settings:
            cfg = dict(cfg, hysteresis=low) if cfg.get('hysteresis') else cfg
            took = {False: [], True: []}
            for on in (False, True) * 2:                          # alternated
                dm.set_lesion_refine(**(cfg if on else {}))
                took[on].append(wall(lambda: dm.lesion_table(**kw)))
            for on in (False, True):
                for med, lo, hi in took[on]:
                    say('  %-28s %.3f ms per call (median of %d; %.3f .. %.3f)' % ('lesion_table, ' + (name if on else 'plain'), med, R, lo, hi))
            plain_runs, refined_runs = [r[0] for r in took[False]], [r[0] for r in took[True]]
            areas = []
            for on in (False, True):
                dm.set_lesion_refine(**(cfg if on else {}))
                rows = dm.lesion_table(**kw)[0]
                areas.append((len(rows), int(rows['area'].sum())))
            say('  %s: refined / plain, wall (best medians): %.3f; plain run to run %.3f; %d -> %d lesions, %d -> %d pixels' % (
                name, min(refined_runs) / min(plain_runs), max(plain_runs) / min(plain_runs), areas[0][0], areas[1][0], areas[0][1],
                areas[1][1]))
            dm.set_lesion_refine(**cfg)
            per_launch(dm, lambda: dm.lesion_table(**kw), ('region_',))
        dm.set_lesion_refine()
    dm.close()
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0)
if a.detection:
    dm.forward(x, return_prob=False)
    net = dm.last_prob(B)
    planes = (('network output as it is', net), ('drawn discs', prob),
              ('network output above its 99th percentile', np.where(net >= np.percentile(net, 99.0), net, 0).astype(np.float32)))
    for what, plane in planes:
        def put_back():
            dm.pixel_confusion_of(plane, y, [0.5])                # the plane into the model's buffer (synchronises)

        def timed(fn):
            ts = []
            for _ in range(R + 1):                                # the first one warms up
                put_back()
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts = sorted(ts[1:])
            return ts[len(ts) // 2], ts[0], ts[-1]
        put_back()
        rows, recs = dm.detection_map(B)
        say('  %s: %d candidates, %d rounds, %d dropped, %d slices exhausted, largest %d pixels' % (
            what, len(rows), int(recs['rounds'].sum()), int(recs['dropped'].sum()), int(recs['exhausted'].sum()),
            int(rows['area'].max()) if len(rows) else 0))
        for name, fn in (('detection_map', lambda: dm.detection_map(B)),
                         ('lesion_table', lambda: dm.lesion_table(batch=B, threshold=0.5, filter_size=5, mask=False))) * 2:
            med, lo, hi = timed(fn)
            say('  %-28s %.3f ms per call (median of %d; %.3f .. %.3f)' % (name, med, R, lo, hi))
        per_launch(dm, lambda: (put_back(), dm.detection_map(B)), ('det_',))
    ys = np.concatenate([y] * NB)
    table = dict(threshold=0.1, filter_size=1, resize_factor=1.0, min_area=0)

    def eval_pass(detect):
        """a forward and the calls of engine._detection_pass per batch; without `detect` the matched call alone"""
        t0 = time.perf_counter()
        for i, (xb, _, _) in enumerate(ds):
            dm.forward(xb, return_prob=False)
            if detect:
                dm.detection_map(len(xb))
            dm.lesion_table_matched(ys[i * B:i * B + len(xb)], batch=len(xb), continues=[i > 0 or b > 0 for b in range(len(xb))], **table)
        return time.perf_counter() - t0
    eval_pass(False), eval_pass(True)                             # warm-up: the carries, either workspace
    took = {False: [], True: []}
    for i in range(8):
        took[bool(i % 2)].append(eval_pass(bool(i % 2)))
        say('  %-44s %9.1f slices/s  (%.2f ms per batch)' % ('forward + ' + ('detection_map + ' if i % 2 else '') + 'matched pass',
                                                             B * NB / took[bool(i % 2)][-1], took[bool(i % 2)][-1] / NB * 1e3))
    say('  detection / plain matched pass (medians of 4, alternated): %.3f' % (sorted(took[True])[2] / sorted(took[False])[2]))
    dm.close()
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0)
if a.features:
    from dnncancerannotator_amd import tta as tta_modes
    views = tta_modes.mask_of(a.tta, S, S)

    def legs(what, kw, spread, **fkw):
        """lesion_table, lesion_table_spread (where the spread plane is valid) and lesion_table_features on the same plane, alternated"""
        say('  %s' % what)
        calls = [('lesion_table', lambda: dm.lesion_table(**kw))]
        if spread:
            calls.append(('lesion_table_spread', lambda: dm.lesion_table_spread(**kw)))
        calls.append(('lesion_table_features', lambda: dm.lesion_table_features(**kw, **fkw)))
        took = {}
        for name, fn in calls * 2:
            took.setdefault(name, []).append(wall(fn))
        for name, runs in took.items():
            for med, lo, hi in runs:
                say('  %-28s %.3f ms per call (median of %d; %.3f .. %.3f)' % (name, med, R, lo, hi))
        best = {name: min(r[0] for r in runs) for name, runs in took.items()}
        rows = dm.lesion_table_features(**kw, **fkw)[0]
        say('  lesion_table_features / lesion_table, wall (best medians): %.3f; %d lesions, largest %d pixels' % (
            best['lesion_table_features'] / best['lesion_table'], len(rows), int(rows['area'].max()) if len(rows) else 0))
        per_launch(dm, lambda: dm.lesion_table_features(**kw, **fkw), ('lesion_features', 'lesion_ring', 'lesion_stats', 'lesion_spread'))
    dm.forward_tta_spread(x, views, return_prob=False, return_spread=False)
    last = dm.last_prob(B)
    for thr, k in ((float(np.median(last)), 5), (float(np.percentile(last, 99.0)), 1)):
        kw = dict(batch=B, threshold=thr, filter_size=k, mask=False, max_lesions=4096)
        legs('threshold %.6f, filter_size %d, 32 bins, ring 3' % (thr, k), kw, True)
        legs('the same, ring 8', kw, True, ring=8)
        legs('the same, no histogram, no ring', kw, True, bins=0, ring=0)
    dm.forward(x, return_prob=False)
    dm.pixel_confusion_of(prob, y, [0.5])
    legs('drawn discs, threshold 0.5, filter_size 5, 32 bins, ring 3', dict(batch=B, threshold=0.5, filter_size=5, mask=False), False)
    dm.pixel_confusion_of(np.ones((B, S, S), np.float32), y, [0.5])
    legs('every slice one lesion, 32 bins, ring 3', dict(batch=B, threshold=0.5, filter_size=5, mask=False), False)
    legs('every slice one lesion, no histogram', dict(batch=B, threshold=0.5, filter_size=5, mask=False), False, bins=0)
    dm.close()
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0)
if a.calibration:
    from dnncancerannotator_amd import casewise, tta as tta_modes
    views = tta_modes.mask_of(a.tta, S, S)
    grid = casewise.calibration_grid()
    rng = np.random.default_rng(5)
    uniform = rng.random((B, S, S)).astype(np.float32)
    hot = rng.random((B, S, S)) < 0.01
    real = np.where(hot, rng.random((B, S, S)), 0.01 * rng.random((B, S, S))).astype(np.float32)
    y_real = (hot & (rng.random((B, S, S)) < 0.7)).astype(np.float32)
    for what, p, lab in (('uniform plane, labels 30 % positive', uniform, (rng.random((B, S, S)) < 0.3).astype(np.float32)),
                         ('real-like plane (99 % below 0.01, class 0)', real, y_real)):
        dm.forward(x, return_prob=False)                          # a forward of B slices, then the plane into the model's buffer
        dm.pixel_confusion_of(p, lab, [0.5])
        bins, totals, nll = dm.calibration(lab, 15, grid, batch=B)
        table = casewise.calibration_table(bins)
        say('  %s: %d of %d pixels in bin 0, ECE %.4f, fitted temperature %.3f' % (
            what, table[0][3], B * S * S, casewise.calibration_errors(table)[0], casewise.fit_temperature(grid, nll.sum(axis=0))[0]))
        for name, temps in (('15 bins, no temperatures', ()), ('15 bins, 41 temperatures', grid)):
            med, lo, hi = wall(lambda: dm.calibration(lab, 15, temps, batch=B))
            say('  calibration, %s: %.3f ms per call, labels uploaded (median of %d; %.3f .. %.3f)' % (name, med, R, lo, hi))
            per_launch(dm, lambda: dm.calibration(lab, 15, temps, batch=B), ('calib_',))
        med, lo, hi = wall(lambda: dm.calibration(lab, 256, (), batch=B))
        say('  calibration, 256 bins, no temperatures: %.3f ms per call (median of %d; %.3f .. %.3f)' % (med, R, lo, hi))
        per_launch(dm, lambda: dm.calibration(lab, 256, (), batch=B), ('calib_',))
    med, lo, hi = wall(lambda: dm.scale_temperature(1.0, B))          # T = 1 keeps the plane where it is, rep after rep
    say('  scale_temperature in place: %.3f ms per call (median of %d; %.3f .. %.3f)' % (med, R, lo, hi))
    per_launch(dm, lambda: dm.scale_temperature(1.0, B), ('prob_temperature',))
    ys = np.concatenate([y] * NB)

    def tta_pass(calibrate):
        """the forward of `evaluate --tta flips --uncertainty` and one table call per batch"""
        t0 = time.perf_counter()
        for i, (xb, _, _) in enumerate(ds):
            dm.forward_tta_spread(xb, views, return_prob=False, return_spread=False)
            yb = ys[i * B:i * B + len(xb)]
            if calibrate:
                dm.calibration(yb, 15, grid, batch=len(xb))
            else:
                dm.spread_by_outcome(yb, [0.5], batch=len(xb))
        return time.perf_counter() - t0
    tta_pass(False), tta_pass(True)                               # warm-up: the spread planes, either workspace
    took = {False: [], True: []}
    for i in range(8):
        took[bool(i % 2)].append(tta_pass(bool(i % 2)))
        say('  %-44s %9.1f slices/s  (%.2f ms per batch)' % ('forward_tta_spread + ' + ('calibration' if i % 2 else 'spread_by_outcome') + ' pass',
                                                             B * NB / took[bool(i % 2)][-1], took[bool(i % 2)][-1] / NB * 1e3))
    cal, out = sorted(took[True])[2], sorted(took[False])[2]
    say('  calibration / spread_by_outcome pass (medians of 4, alternated): %.3f' % (cal / out))

    def plain_pass(calibrate, scale):
        t0 = time.perf_counter()
        for i, (xb, _, _) in enumerate(ds):
            dm.forward(xb, return_prob=False)
            if scale:
                dm.scale_temperature(1.7, len(xb))
            if calibrate:
                dm.calibration(ys[i * B:i * B + len(xb)], 15, grid, batch=len(xb))
        dm.sync()
        return time.perf_counter() - t0
    plain_pass(True, True)
    for i in range(2):
        for name, args in (('forward', (False, False)), ('forward + scale_temperature', (False, True)),
                           ('forward + calibration', (True, False)), ('forward + scale_temperature + calibration', (True, True))):
            dt = plain_pass(*args)
            say('  %-44s %9.1f slices/s  (%.2f ms per batch)' % (name + ' pass', B * NB / dt, dt / NB * 1e3))
    dm.close()
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0)
if a.tta:
    from dnncancerannotator_amd import tta as tta_modes
    views = tta_modes.mask_of(a.tta, S, S)
    n_views = bin(views).count('1')

    def plain():
        dm.forward(x, return_prob=False)

    def augmented():
        dm.forward_tta(x, views, return_prob=False)
        dm.sync()

    def device_rows(fn):
        dm.profile_reset()
        dm.profile_enable(1)
        for _ in range(R):
            fn()
        dm.sync()
        rows = dm.profile()
        dm.profile_enable(0)
        dm.profile_reset()
        return rows
    took = {}
    for name, fn in (('forward', plain), ('forward_tta', augmented)) * 2:          # alternated
        took.setdefault(name, []).append(wall(fn))
    for name, runs in took.items():
        for med, lo, hi in runs:
            say('  %-28s %.3f ms per call, upload included (median of %d; %.3f .. %.3f)' % (name, med, R, lo, hi))
    say('  forward_tta(%s, %d views) / forward, wall: %.2f' % (a.tta, n_views, min(r[0] for r in took['forward_tta']) /
                                                                min(r[0] for r in took['forward'])))
    rows_p, rows_t = device_rows(plain), device_rows(augmented)
    dev_p, dev_t = sum(r[2] for r in rows_p) / R, sum(r[2] for r in rows_t) / R
    say('  device time per call (event-bracketed launches): forward %.3f ms, forward_tta %.3f ms: ratio %.2f' % (dev_p, dev_t, dev_t / dev_p))
    mine = [r for r in rows_t if r[0].startswith('tta_')]
    for name, n, ms, by, fl in mine:
        say('    %-22s launches/call %4.1f  %9.2f us per launch  %7.1f GB/s' % (name, n / R, ms / n * 1e3, by / (ms / n * 1e-3) / 1e9))
    say('    share of the two tta kernels in forward_tta: %.2f %%' % (100.0 * sum(r[2] for r in mine) / R / dev_t))
    if a.uncertainty:
        def with_spread():
            dm.forward_tta_spread(x, views, return_prob=False, return_spread=False)
            dm.sync()
        took = {}
        for name, fn in (('forward_tta', augmented), ('forward_tta_spread', with_spread)) * 3:      # alternated
            took.setdefault(name, []).append(wall(fn))
        for name, runs in took.items():
            for med, lo, hi in runs:
                say('  %-28s %.3f ms per call, upload included (median of %d; %.3f .. %.3f)' % (name, med, R, lo, hi))
        say('  forward_tta_spread / forward_tta, wall (best medians): %.3f' % (min(r[0] for r in took['forward_tta_spread']) /
                                                                              min(r[0] for r in took['forward_tta'])))
        rows_s = device_rows(with_spread)
        dev_s = sum(r[2] for r in rows_s) / R
        say('  device time per call: forward_tta %.3f ms, forward_tta_spread %.3f ms: ratio %.3f' % (dev_t, dev_s, dev_s / dev_t))
        per = {}
        for name, n, ms, by, fl in [r for r in rows_s if r[0].startswith('tta_')] + [r for r in mine if r[0] == 'tta_accumulate']:
            per[name] = ms / n * 1e3
            say('    %-22s launches/call %4.1f  %9.2f us per launch  %7.1f GB/s' % (name, n / R, ms / n * 1e3, by / (ms / n * 1e-3) / 1e9))
        say('    tta_moments / tta_accumulate per launch: %.2f' % (per['tta_moments'] / per['tta_accumulate']))
        with_spread()
        last = dm.last_prob(B)
        # a random network draws no tumours: the median under a 5 x 5 opening leaves next to nothing, the 99th percentile without
        # an opening thousands of specks -- the two ends between which a trained model's few lesions per slice lie
        for thr, k in ((float(np.median(last)), 5), (float(np.percentile(last, 99.0)), 1)):
            kw = dict(batch=B, threshold=thr, filter_size=k, mask=False, max_lesions=4096)
            say('  threshold %.6f, filter_size %d' % (thr, k))
            took = {}
            for name, fn in (('lesion_table', lambda: dm.lesion_table(**kw)), ('lesion_table_spread', lambda: dm.lesion_table_spread(**kw))) * 2:
                took.setdefault(name, []).append(wall(fn))
            for name, runs in took.items():
                for med, lo, hi in runs:
                    say('  %-28s %.3f ms per call (median of %d; %.3f .. %.3f)' % (name, med, R, lo, hi))
            say('  lesion_table_spread / lesion_table, wall (best medians): %.3f; %d lesions' % (
                min(r[0] for r in took['lesion_table_spread']) / min(r[0] for r in took['lesion_table']), len(dm.lesion_table_spread(**kw)[0])))
            per_launch(dm, lambda: dm.lesion_table_spread(**kw), ('region_', 'lesion_'))
        for thrs in ([thr], [0.25, thr, 0.75]):
            med, lo, hi = wall(lambda: dm.spread_by_outcome(y, thrs))
            say('  spread_by_outcome, %d threshold(s): %.3f ms per call, labels uploaded (median of %d; %.3f .. %.3f)' % (len(thrs), med, R, lo, hi))
            per_launch(dm, lambda: dm.spread_by_outcome(y, thrs), ('spread_',))
    dm.close()
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
    sys.exit(0)
dm.pixel_confusion_of(prob, y, [0.5])                             # the drawn probabilities into the model's buffer
spec = ([0.5], 0.30, 1.0, 5)
med, lo, hi = wall(lambda: dm.region_confusion_slices(y, [spec]))
say('  region_confusion_slices, 1 spec x 1 threshold: %.3f ms per call (median of %d; %.3f .. %.3f)' % (med, R, lo, hi))
per_launch(dm, lambda: dm.region_confusion_slices(y, [spec]), ('region_',))
if not a.yardstick:
    for mask in (True, False):
        med, lo, hi = wall(lambda: dm.lesion_table(batch=B, threshold=0.5, filter_size=5, mask=mask))
        say('  lesion_table(mask=%s): %.3f ms per call (median of %d; %.3f .. %.3f)' % (mask, med, R, lo, hi))
    rows, totals, _ = dm.lesion_table(batch=B, threshold=0.5, filter_size=5)
    say('    %d lesions in %d slices, largest %d pixels' % (len(rows), B, int(rows['area'].max()) if len(rows) else 0))
    per_launch(dm, lambda: dm.lesion_table(batch=B, threshold=0.5, filter_size=5), ('region_', 'lesion_'))
    one = np.ones((B, S, S), np.float32)                          # the worst case of lesion_stats: one lesion of S x S pixels per slice
    dm.pixel_confusion_of(one, y, [0.5])
    med, lo, hi = wall(lambda: dm.lesion_table(batch=B, threshold=0.5, filter_size=5))
    say('  lesion_table, every pixel one lesion: %.3f ms per call (median; %.3f .. %.3f)' % (med, lo, hi))
    per_launch(dm, lambda: dm.lesion_table(batch=B, threshold=0.5, filter_size=5), ('lesion_',))
    if a.link:
        dm.pixel_confusion_of(prob, y, [0.5])
        flags = [b > 0 for b in range(B)]
        kw = dict(batch=B, threshold=0.5, filter_size=5)
        for mask in (True, False):
            med, lo, hi = wall(lambda: dm.lesion_table_linked(continues=flags, mask=mask, **kw))
            say('  lesion_table_linked(mask=%s): %.3f ms per call (median of %d; %.3f .. %.3f)' % (mask, med, R, lo, hi))
        say('    %d links between %d slices' % (len(dm.lesion_table_linked(continues=flags, **kw)[3]), B))
        per_launch(dm, lambda: dm.lesion_table_linked(continues=flags, **kw), ('lesion_link', 'lesion_carry'))
        # the worst case of the pair table: a checkerboard on itself, k = 1: S S / 2 lesions per slice, as many keys per table
        board = np.broadcast_to(((xx + yy) % 2 == 0).astype(np.float32), (B, S, S)).copy()
        dm.pixel_confusion_of(board, y, [0.5])
        wkw = dict(batch=B, threshold=0.5, filter_size=1, max_lesions=S * S)
        med, lo, hi = wall(lambda: dm.lesion_table(**wkw))
        say('  lesion_table, checkerboard (k = 1, no row limit): %.3f ms per call (median; %.3f .. %.3f)' % (med, lo, hi))
        med, lo, hi = wall(lambda: dm.lesion_table_linked(continues=flags, **wkw))
        say('  lesion_table_linked, checkerboard on itself: %.3f ms per call (median; %.3f .. %.3f)' % (med, lo, hi))
        say('    %d links between %d slices' % (len(dm.lesion_table_linked(continues=flags, **wkw)[3]), B))
        per_launch(dm, lambda: dm.lesion_table_linked(continues=flags, **wkw), ('lesion_link', 'lesion_carry'))
    if a.match:
        dm.pixel_confusion_of(prob, y, [0.5])
        flags = [b > 0 for b in range(B)]
        kw = dict(batch=B, threshold=0.5, filter_size=5)
        med, lo, hi = wall(lambda: dm.lesion_table_matched(y, continues=flags, **kw))
        say('  lesion_table_matched(mask=False): %.3f ms per call (median of %d; %.3f .. %.3f)' % (med, R, lo, hi))
        out = dm.lesion_table_matched(y, continues=flags, **kw)
        say('    %d predicted and %d labelled lesions, %d / %d links, %d pairs in %d slices' % (len(out[0]), len(out[4]), len(out[3]),
                                                                                             len(out[6]), len(out[7]), B))
        per_launch(dm, lambda: dm.lesion_table_matched(y, continues=flags, **kw), ('region_', 'lesion_'))
        ys = np.concatenate([y] * NB)

        def one_pass(matched):
            """a forward and one call per batch; slice b of batch i is slice i * B + b of one exam"""
            t0 = time.perf_counter()
            for i, (xb, _, _) in enumerate(ds):
                dm.forward(xb, return_prob=False)
                cont = [i > 0 or b > 0 for b in range(len(xb))]
                if matched:
                    dm.lesion_table_matched(ys[i * B:i * B + len(xb)], batch=len(xb), continues=cont, threshold=0.5, filter_size=5)
                else:
                    dm.lesion_table_linked(batch=len(xb), continues=cont, threshold=0.5, filter_size=5, mask=False)
            return time.perf_counter() - t0
        one_pass(False), one_pass(True)                           # warm-up: both carries, the larger workspace
        took = {False: [], True: []}
        for i in range(8):
            took[bool(i % 2)].append(one_pass(bool(i % 2)))
            say('  %-34s %9.1f slices/s  (%.2f ms per batch)' % ('forward + ' + ('matched' if i % 2 else 'linked') + ' pass',
                                                                 B * NB / took[bool(i % 2)][-1], took[bool(i % 2)][-1] / NB * 1e3))
        mt, lk = sorted(took[True])[len(took[True]) // 2], sorted(took[False])[len(took[False]) // 2]
        say('  matched / linked pass (medians of 4, alternated): %.3f' % (mt / lk))
    if a.surface:
        dm.pixel_confusion_of(prob, y, [0.5])
        kw = dict(batch=B, threshold=0.5, filter_size=5)
        med, lo, hi = wall(lambda: dm.surface_distances(y, **kw))
        say('  surface_distances(edges=False): %.3f ms per call (median of %d; %.3f .. %.3f)' % (med, R, lo, hi))
        counts, samples, _ = dm.surface_distances(y, **kw)
        say('    %d / %d boundary pixels of %d / %d, %d samples in %d slices, largest distance %.3f' % (
            counts[:, 3].sum(), counts[:, 4].sum(), counts[:, 0].sum(), counts[:, 1].sum(), len(samples), B,
            float(np.sqrt(samples['d2'].max())) if len(samples) else 0.0))
        per_launch(dm, lambda: dm.surface_distances(y, **kw), ('region_', 'surface_'))
        ys = np.concatenate([y] * NB)

        def eval_pass(surface):
            """a forward and one call per batch, as engine._surface_pass / _exam_lesion_pass make them"""
            t0 = time.perf_counter()
            for i, (xb, _, _) in enumerate(ds):
                dm.forward(xb, return_prob=False)
                yb = ys[i * B:i * B + len(xb)]
                if surface:
                    dm.surface_distances(yb, batch=len(xb), threshold=0.5, filter_size=5)
                else:
                    dm.lesion_table_matched(yb, batch=len(xb), continues=[i > 0 or b > 0 for b in range(len(xb))], threshold=0.5,
                                            filter_size=5)
            return time.perf_counter() - t0
        eval_pass(False), eval_pass(True)                         # warm-up: the carries, either workspace
        took = {False: [], True: []}
        for i in range(8):
            took[bool(i % 2)].append(eval_pass(bool(i % 2)))
            say('  %-34s %9.1f slices/s  (%.2f ms per batch)' % ('forward + ' + ('surface' if i % 2 else 'matched') + ' pass',
                                                                 B * NB / took[bool(i % 2)][-1], took[bool(i % 2)][-1] / NB * 1e3))
        sf, mt = sorted(took[True])[len(took[True]) // 2], sorted(took[False])[len(took[False]) // 2]
        say('  surface / matched pass (medians of 4, alternated): %.3f' % (sf / mt))
    for xb, _, _ in ds:
        dm.forward(xb, return_prob=False)
    t0 = time.perf_counter()
    for xb, _, _ in ds:
        dm.forward(xb, return_prob=False)
    dm.sync()
    say('  %-34s %9.1f slices/s' % ('forward only', B * NB / (time.perf_counter() - t0)))
    with tempfile.TemporaryDirectory() as tmp:
        e.current_step = 1
        e.save(os.path.join(tmp, 'run', 'checkpoints', 'ckpt-1'))
        thr = float(np.median(dm.forward(x, training=False)))
        for images in (False, True, False, True):
            t0 = time.perf_counter()
            res = e.annotate(ds, os.path.join(tmp, 'run'), os.path.join(tmp, 'out%d' % images), threshold=thr, export_images=images)
            dt = time.perf_counter() - t0
            say('  %-34s %9.1f slices/s  (%.2f ms per batch; %d lesions)' % ('annotate' + (' + mask.png' if images else ''),
                                                                            B * NB / dt, dt / NB * 1e3, res['lesions']))
        if a.link:
            rate = {}
            for i, linked in enumerate((False, True, False, True)):
                t0 = time.perf_counter()
                res = e.annotate(ds, os.path.join(tmp, 'run'), os.path.join(tmp, 'link%d' % i), threshold=thr, link_slices=linked)
                dt = time.perf_counter() - t0
                rate[linked] = dt
                say('  %-34s %9.1f slices/s  (%.2f ms per batch; %d lesions%s)' % (
                    'annotate' + (' --link_slices' if linked else ''), B * NB / dt, dt / NB * 1e3, res['lesions'],
                    ', %d exam lesions' % res['exam_lesions'] if linked else ''))
            say('  linked / unlinked annotate (the second pass of each): %.3f' % (rate[True] / rate[False]))
dm.close()
if a.out:
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')
