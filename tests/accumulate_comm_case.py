"""Child process of tests/test_accumulate_gpu.py: a k = 2 cycle of gradient accumulation behind the data-parallel arm of the optimizer
step on a one-rank communicator, made the way tools/rccl_one_rank.py makes one (DNNCA_FORCE_RCCL=1, set by the parent before this
process starts), and the same cycle on a model without a communicator.  Prints one JSON line: whether the weights and slots after
the cycle are bit-identical, the collectives of each micro-step and the floats they covered, and the launches that ran."""

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from dnncancerannotator_amd import device as dev                      # noqa: E402

K, LR = 2, 1e-2
UNET3 = dict(n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')


def cycle(m, batches, cfg, comm):
    """one cycle of K micro-steps -> per micro-step dict(collectives, floats, position, gradient, loss)"""
    recs = []
    for x, y in batches:
        out = m.train_step(x, y, LR, cfg)
        rec = dict(position=m.get_accumulation()[2], g=m.get_grads(), loss=float(out.loss))
        if comm:
            rec.update(collectives=m.comm_collectives(), floats=m.comm_collective_floats())
        recs.append(rec)
    return recs


def main():
    assert os.environ.get('DNNCA_FORCE_RCCL') == '1'
    dev.init_device(0)
    rng = np.random.default_rng(6)
    batches = [(rng.random((2, 64, 256, 1)).astype(np.float32), (rng.random((2, 64, 256)) < 0.1).astype(np.float32)) for _ in range(K)]
    models = [dev.DeviceModel('unet', 1, 64, 256, 2, **UNET3) for _ in range(2)]
    single, ranked = models
    single.init_glorot(seed=5)
    p0 = (single.get_params() + rng.uniform(-0.05, 0.05, single.n_trainable)).astype(np.float32)
    n = single.n_trainable
    m0 = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    v0 = (rng.random(n) * 1e-6).astype(np.float32)
    cfg = single.loss_cfg(weight_mul=3.0)
    for m in models:
        m.set_params(p0)
        m.set_opt_state(m0, v0, 6)
        m.set_accumulation(K)
    ranked.comm_init(0, 1, dev.DeviceModel.comm_unique_id())
    ranked.comm_broadcast_weights(0)
    assert ranked.get_params().tobytes() == p0.tobytes()
    a = cycle(single, batches, cfg, False)
    ranked.sync()
    ranked.profile_reset()
    ranked.profile_enable(1)
    b = cycle(ranked, batches, cfg, True)
    rows = {name: k for name, k, _, _, _ in ranked.profile()}
    ranked.profile_enable(0)
    ranked.profile_reset()
    same = {}
    for key, get in (('params', lambda m: m.get_params()), ('m', lambda m: m.get_opt_state()[0]), ('v', lambda m: m.get_opt_state()[1]),
                     ('accumulator', lambda m: m.get_accumulation()[0])):
        same[key] = get(single).tobytes() == get(ranked).tobytes()
    out = dict(n=n, same=same, same_grads=[ra['g'].tobytes() == rb['g'].tobytes() for ra, rb in zip(a, b)],
               losses=[[r['loss'] for r in recs] for recs in (a, b)],
               collectives=[r['collectives'] for r in b], floats=[r['floats'] for r in b],
               positions=[[r['position'] for r in recs] for recs in (a, b)],
               iterations=[m.get_opt_state()[2] for m in models], moved=float(np.abs(ranked.get_params() - p0).max()),
               launches={k: rows.get(k, 0) for k in ('grad_accumulate', 'pg_fold', 'pg_fold_acc', 'g_adam', 'g_finalize_scalars')})
    for m in models:
        m.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
