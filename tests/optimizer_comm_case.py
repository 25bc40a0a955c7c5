"""Child process of tests/test_optimizer_gpu.py: AdamW with global_clipnorm behind the data-parallel arm of the optimizer step (no
finalize in the optimizer launch, gscale = 1 / world, after the all-reduce) on a one-rank communicator, made the way
tools/rccl_one_rank.py makes one (DNNCA_FORCE_RCCL=1, set by the parent before this process starts).  Prints one JSON line: the
launches that ran and the worst error / bound against tests/optim_oracle.py."""

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import optim_oracle as OO                                             # noqa: E402
from dnncancerannotator_amd import device as dev                      # noqa: E402

T, LR = 5, 1e-2


def main():
    assert os.environ.get('DNNCA_FORCE_RCCL') == '1'
    dev.init_device(0)
    m = dev.DeviceModel('unet', 1, 64, 256, 2, n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False,
                        padding='same')
    m.init_glorot(seed=5)
    rng = np.random.default_rng(6)
    m.set_params((m.get_params() + rng.uniform(-0.05, 0.05, m.n_trainable)).astype(np.float32))
    x = rng.random((2, 64, 256, 1)).astype(np.float32)
    y = (rng.random((2, 64, 256)) < 0.1).astype(np.float32)
    cfg = m.loss_cfg(weight_mul=3.0)
    m.train_step(x, y, 0.0, cfg)                          # one gradient, to scale the planted slots and to choose the clip
    g0 = m.get_grads()
    scale = np.abs(g0) + 1e-6
    m.set_opt_state((rng.standard_normal(m.n_trainable) * scale).astype(np.float32),
                    (rng.random(m.n_trainable) * scale ** 2).astype(np.float32), 6)
    spec = OO.spec('adamw', weight_decay=0.05, global_clipnorm=0.05 * float(np.linalg.norm(g0.astype(np.float64))))
    decay, slices = m.decay_mask(), OO.variable_slices(m.param_infos())
    m.set_optimizer(decay_mask=decay, **OO.device_kwargs(spec))
    m.comm_init(0, 1, dev.DeviceModel.comm_unique_id())
    m.comm_broadcast_weights(0)
    p_start = m.get_params()
    m.sync()
    m.profile_reset()
    m.profile_enable(1)
    worst, clipped = {}, 0
    for _ in range(T):
        p, (mm, vv, it) = m.get_params(), m.get_opt_state()
        m.train_step(x, y, LR, cfg)
        want = OO.step(spec, slices, decay, p, mm, vv, m.get_grads(), it + 1, LR, gscale=1.0)
        m1, v1, _ = m.get_opt_state()
        w = OO.check(m.get_params(), m1, v1, want)
        total, _ = m.last_grad_norm()
        w['norm'] = float(abs(total - want['norm']) / OO.norm_tol(want['norm'], m.n_trainable))
        clipped += int(np.all(want['scales'] < 1.0))
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
    rows = {name: k for name, k, _, _, _ in m.profile()}
    m.profile_enable(0)
    m.profile_reset()
    names = ('opt_adamw', 'grad_sqnorm', 'grad_clip_scale', 'g_finalize_scalars')
    out = dict(launches={k: rows.get(k, 0) for k in names}, plain=rows.get('g_adam', 0) + rows.get('pg_fold_adam', 0),
               collectives=m.comm_collectives(), iterations=m.get_opt_state()[2], worst=worst, clipped_steps=clipped,
               moved=float(np.abs(m.get_params() - p_start).max()))
    m.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
