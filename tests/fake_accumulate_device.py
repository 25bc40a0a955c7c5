"""Test double for the CPU tests of deploy_options.gradient_accumulation_steps: tests/fake_device.FakeDeviceModel plus
DeviceModel.set_accumulation / get_accumulation with the library's semantics -- every train step is a micro-step whose float32
gradient is added to the accumulator in micro-step order; micro-steps 1 .. k-1 change nothing else (under data parallel they
all-reduce the loss alone), the k-th all-reduces [accumulator, loss] and applies Adam to the mean, counting one iteration.  Every
set_accumulation call and every collective (with the floats it covered) goes into `calls`.  Test infrastructure only."""

import numpy as np

from fake_device import FakeDeviceModel, StepOut
from oracle import unet_oracle as O


class AccumulateDeviceModel(FakeDeviceModel):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.acc, self.acc_steps, self.acc_pos = None, 1, 0

    def set_accumulation(self, steps):
        if isinstance(steps, bool) or not isinstance(steps, int) or not 1 <= steps <= 4096:
            raise ValueError('dnnca_model_set_accumulation: steps %r outside [1, 4096]' % (steps,))
        self.calls.append(('set_accumulation', steps))
        self.acc = None if steps == 1 else (self.acc if self.acc is not None else np.zeros(self.n_trainable, np.float32))
        self.acc_steps, self.acc_pos = steps, 0

    def get_accumulation(self):
        if self.acc is None:
            raise RuntimeError('dnnca_get_accumulation: gradient accumulation is off')
        return self.acc.copy(), self.acc_steps, self.acc_pos

    def set_params(self, flat):
        super().set_params(flat)
        self.acc_pos = 0

    def set_opt_state(self, m, v, iterations):
        super().set_opt_state(m, v, iterations)
        self.acc_pos = 0

    def _allreduce(self, flat):
        self.calls.append(('allreduce', int(flat.size)))
        if self.world > 1:
            import torch
            t = torch.from_numpy(flat)
            self.dist.all_reduce(t)
            flat = t.numpy()
        return flat

    def train_step(self, x, y, lr, cfg):
        if self.acc is None:
            return super().train_step(x, y, lr, cfg)
        self._check(x)
        self.calls.append(('train', len(x)))
        loss, grads, _, state = O.loss_and_grads(self.spec, self.params, np.asarray(x, np.float64), y, cfg, training=True)
        self.grads = O.flatten(self.spec, grads)
        g = self.grads.astype(np.float32)
        self.acc = g.copy() if self.acc_pos == 0 else self.acc + g
        self.acc_pos += 1
        if self.acc_pos < self.acc_steps:
            loss = float(self._allreduce(np.array([loss], np.float64))[0]) / self.world
        else:
            flat = self._allreduce(np.concatenate([self.acc.astype(np.float64), [loss]]))
            self.acc, loss = flat[:-1].astype(np.float32), float(flat[-1]) / self.world
            self.acc_pos = 0
            self.iterations += 1
            mean = O.unflatten(self.spec, self.acc.astype(np.float64) * float(np.float32(1.0 / (self.acc_steps * self.world))))
            self.params.update(O.adam_step({n: self.params[n] for n in mean}, mean, self.m, self.v, self.iterations, lr))
        self.params.update(state)                              # BatchNorm moving statistics: per micro-batch
        w = O.loss_weight(y, **{k: cfg[k] for k in ('weight', 'weight_add', 'weight_mul') if k in cfg})
        return StepOut(float(loss), float(O.positive_rate(y)), float(w), float(y.min()), float(y.max()))


def install(patch=setattr, seed_offset=0):
    """the engine's device layer -> AccumulateDeviceModel (as tests/fake_optimizer_device.install).  Returns the list of models built."""
    from dnncancerannotator_amd import device, models
    patch(device, 'init_device', lambda ordinal=0: None)
    patch(device, 'device_count', lambda: 1)
    patch(device, 'DeviceModel', AccumulateDeviceModel)
    built = []

    def build(self, input_shape, max_batch=None, seed=None, force_generic=False):
        b, h, w, c = input_shape
        opts = {k: v for k, v in self.configs.items() if k in ('n_filters_first', 'n_downsample', 'rate', 'kernel_size', 'conv_stride',
                                                               'bn', 'padding')}
        self.device_model = AccumulateDeviceModel(self.arch, c, h, w, max_batch or b, **opts)
        self.device_model.init_glorot(seed=(seed or 0) + seed_offset)
        built.append(self.device_model)
        return self.device_model
    patch(models.UNetAnnotator, 'build', build)
    return built
