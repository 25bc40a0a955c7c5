"""Worker of tests/test_accumulate_host.py::test_two_ranks_call_the_same_sequence: engine.TFKerasModel.train with
deploy_options.gradient_accumulation_steps: 2 on WORLD_SIZE gloo ranks, tests/fake_accumulate_device.py in place of the HIP device."""

import json
import os
import sys

import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from dnncancerannotator_amd import data, distributed, engine              # noqa: E402
from fake_accumulate_device import install                                 # noqa: E402
from fake_device import FakeDeviceModel                                    # noqa: E402
from oracle import unet_oracle as O                                        # noqa: E402
from test_accumulate_host import config                                    # noqa: E402


def main():
    out_dir = sys.argv[1]
    ctx = distributed.context()
    dist.init_process_group('gloo', rank=ctx.rank, world_size=ctx.world)
    FakeDeviceModel.dist = dist
    install(seed_offset=100 * ctx.rank)       # ranks start DIFFERENT: the broadcast of rank 0's weights must fix it
    x, y = O.synthetic_batch(8, 16, 16, 1, seed_x=3, seed_y=4)
    m = engine.TFKerasModel(config(2, enable_multigpu=True))
    res = m.train(data.ArrayDataset(x, y, 4, repeat=True), max_steps=4, save_freq=2)
    dm = m.device_model
    with open(os.path.join(out_dir, 'rank%d.json' % ctx.rank), 'w') as f:
        json.dump(dict(loss=res.history['loss'], calls=[list(c) for c in dm.calls if c[0] in ('set_accumulation', 'train', 'allreduce')],
                       params=dm.get_params().tolist(), iterations=dm.iterations, n=dm.n_trainable), f)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
