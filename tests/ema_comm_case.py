"""Child process of tests/test_ema_gpu.py: the weight average behind the data-parallel Adam launch (g_adam without finalize,
gscale = 1 / world) on a one-rank communicator, made the way tools/rccl_one_rank.py makes one (DNNCA_FORCE_RCCL=1, set by the parent
before this process starts).  Prints one JSON line: per mode the launches that ran and the worst error / bound against the oracle."""

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import ema_oracle as EO                                               # noqa: E402
from dnncancerannotator_amd import device as dev                      # noqa: E402

T, LR = 5, 1e-2
MODES = {'fixed': (0.5, False), 'warmup': (0.999, True)}


def main():
    assert os.environ.get('DNNCA_FORCE_RCCL') == '1'
    dev.init_device(0)
    m = dev.DeviceModel('unet', 1, 64, 256, 2, n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False,
                        padding='same')
    m.init_glorot(seed=5)
    rng = np.random.default_rng(6)
    m.set_params((m.get_params() + rng.uniform(-0.05, 0.05, m.n_trainable)).astype(np.float32))
    m.comm_init(0, 1, dev.DeviceModel.comm_unique_id())
    x = rng.random((2, 64, 256, 1)).astype(np.float32)
    y = (rng.random((2, 64, 256)) < 0.1).astype(np.float32)
    cfg = m.loss_cfg(weight_mul=3.0)
    out = {}
    for mode, (decay, warmup) in MODES.items():
        m.set_ema(decay, warmup)
        m.comm_broadcast_weights(0)                       # the average and its count travel too
        e0, n0 = m.get_ema()
        assert n0 == 0 and np.array_equal(e0, m.get_params())
        m.sync()
        m.profile_reset()
        m.profile_enable(1)
        thetas = []
        for _ in range(T):
            m.train_step(x, y, LR, cfg)
            thetas.append(m.get_params())
        rows = {name: k for name, k, _, _, _ in m.profile()}
        m.profile_enable(0)
        m.profile_reset()
        eT, n = m.get_ema()
        err = np.abs(eT.astype(np.float64) - EO.run(thetas, e0, decay, warmup))
        out[mode] = dict(ran=sorted(k for k in rows if k.endswith('_ema')), launches=rows.get('g_adam_ema', 0),
                         finalize_launches=rows.get('g_finalize_scalars', 0), plain=rows.get('g_adam', 0) + rows.get('pg_fold_adam', 0),
                         collectives=m.comm_collectives(), n=n, worst=float((err / EO.bound(thetas, e0)).max()),
                         moved=float(np.abs(eT - thetas[-1]).max()))
    m.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
