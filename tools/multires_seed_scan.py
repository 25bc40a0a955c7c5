"""Which input seeds of tests/test_multires_gpu.py's train-step cases are free of the flip lottery?  ReLU is
fixed in MultiResUnet, so a pre-activation within float32 rounding of zero, or two max-pool candidates within rounding of each
other, makes a float32 run differentiate a different function than the float64 reference.  CPU only, the reference alone
(tests/multires_ref.py): a seed is clean when the float64 and the float32 run take EVERY ReLU and max-pool decision the same way.
Per seed: clean or not, and the float32 run's loss and worst per-tensor gradient error on the tensor's own scale.
    python tools/multires_seed_scan.py [first_seed] [n_seeds] [4,32]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import multires_ref as R          # noqa: E402

first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
PARAM_SEED, PERTURB = 7, 0.1          # as the test
for nff in ([int(v) for v in sys.argv[3].split(',')] if len(sys.argv) > 3 else (4, 32)):
    p, s = R.init(5, nff, PARAM_SEED, PERTURB)
    clean = []
    for seed in range(first, first + n):
        x = np.random.default_rng(seed).standard_normal((2, 32, 32, 5)).astype(np.float32)
        y = R.discs(2, 32, 32, seed + 1000)
        r64 = R.run(p, s, x, y, nff, training=True)
        r32 = R.run(p, s, x, y, nff, training=True, dtype=torch.float32)
        same = R.same_decisions(r64['decisions'], r32['decisions'])
        # other float32 summation orders of the same code: all threads; the plain (non-oneDNN) convolutions
        others = [R.run(p, s, x, y, nff, training=True, dtype=torch.float32, threads=None)]
        with torch.backends.mkldnn.flags(enabled=False):
            others.append(R.run(p, s, x, y, nff, training=True, dtype=torch.float32))
        across = min([R.decision_safety(r64, r32)[1]] + [R.decision_safety(r64, o)[1] for o in others])
        worst = 0.0
        for name, (o, shape, t) in r64['lay'].items():
            if t:
                sl = slice(o, o + int(np.prod(shape)))
                scale = np.abs(r64['grads'][sl]).max()
                if scale > 1e-6:          # (not the analytically-zero ones)
                    worst = max(worst, np.abs(r32['grads'][sl] - r64['grads'][sl]).max() / scale)
        by_tensor, safety = R.decision_safety(r64, r32)
        print('n_filters_first %2d seed %3d: safety by tensor %5.2f by element %6.2f (three float32 orders: %5.2f) %s  loss %.6f (float32 %+.1e)  worst tensor %.1e' % (
            nff, seed, by_tensor, safety, across, 'clean' if same else 'FLIPS', r64['loss'], r32['loss'] / r64['loss'] - 1, worst), flush=True)
        if same:
            clean.append((across, seed))
    print('   clean seeds by safety over the three orders:', ' '.join('%d (%.1f)' % (s_, m_) for m_, s_ in sorted(clean, reverse=True)[:8]), flush=True)
