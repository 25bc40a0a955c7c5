"""Test double for the CPU tests of deploy_options.optimizer: tests/fake_device.FakeDeviceModel plus DeviceModel.set_optimizer /
last_grad_norm / apply_gradients with the library's semantics -- kind 'adam' with nothing else leaves the model as it was, anything
else makes a train step apply tests/optim_oracle.step to the oracle's gradient (SGD's accumulator lives in the m slot, v stays
zeros).  Every set_optimizer call goes into `calls` with its keywords and decay mask.  Test infrastructure only."""

import numpy as np

import optim_oracle as OO
from fake_device import FakeDeviceModel, StepOut
from oracle import unet_oracle as O


class OptimizerDeviceModel(FakeDeviceModel):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.opt, self.decay, self.norms = None, None, None

    def trainable_names(self):
        return [n for n, _, t, _ in self.param_infos() if t]

    def set_optimizer(self, kind='adam', decay_mask=None, **kw):
        mask = None if decay_mask is None else [int(b) for b in decay_mask]
        self.calls.append(('set_optimizer', kind, dict(kw), mask))
        if mask is not None and len(mask) != len(self.trainable_names()):
            raise ValueError('n_variables')
        s = OO.spec(kind, **kw)
        if s.clipnorm and s.global_clipnorm:
            raise ValueError('clipnorm and global_clipnorm exclude each other')
        if kind != 'sgd':
            self.adam = (s.beta1, s.beta2, s.epsilon)
        plain = kind == 'adam' and not (s.clipvalue or s.clipnorm or s.global_clipnorm)
        self.opt, self.decay = (None, None) if plain else (s, mask or [0] * len(self.trainable_names()))

    def last_grad_norm(self):
        if self.opt is None or not (self.opt.clipnorm or self.opt.global_clipnorm):
            raise RuntimeError('no clipping by norm is set')
        return self.norms

    def _apply(self, g, lr):
        self.iterations += 1
        m, v, _ = self.get_opt_state()
        r = OO.step(self.opt, OO.variable_slices(self.param_infos()), self.decay, self.get_params(), m, v, g, self.iterations, lr)
        self.norms = (r['norm'], r['norms'])
        FakeDeviceModel.set_params(self, r['p'])
        self.m = dict(O.unflatten(self.spec, r['m']))
        self.v = dict(O.unflatten(self.spec, r['v']))

    def apply_gradients(self, g, lr):
        assert self.opt is not None, 'the fake applies planted gradients only with an optimizer set'
        self.calls.append(('apply_gradients',))
        self._apply(np.asarray(g, np.float32), lr)

    def train_step(self, x, y, lr, cfg):
        if self.opt is None:
            return super().train_step(x, y, lr, cfg)
        self._check(x)
        self.calls.append(('train', len(x)))
        loss, grads, _, state = O.loss_and_grads(self.spec, self.params, np.asarray(x, np.float64), y, cfg, training=True)
        self.grads = O.flatten(self.spec, grads)
        self._apply(self.grads.astype(np.float32), lr)
        self.params.update(state)
        w = O.loss_weight(y, **{k: cfg[k] for k in ('weight', 'weight_add', 'weight_mul') if k in cfg})
        return StepOut(float(loss), float(O.positive_rate(y)), float(w), float(y.min()), float(y.max()))


def install(patch=setattr):
    """the engine's device layer -> OptimizerDeviceModel (as tests/fake_ema_device.install).  Returns the list of models built."""
    from dnncancerannotator_amd import device, models
    patch(device, 'init_device', lambda ordinal=0: None)
    patch(device, 'device_count', lambda: 1)
    patch(device, 'DeviceModel', OptimizerDeviceModel)
    built = []

    def build(self, input_shape, max_batch=None, seed=None, force_generic=False):
        b, h, w, c = input_shape
        opts = {k: v for k, v in self.configs.items() if k in ('n_filters_first', 'n_downsample', 'rate', 'kernel_size', 'conv_stride',
                                                               'bn', 'padding')}
        self.device_model = OptimizerDeviceModel(self.arch, c, h, w, max_batch or b, **opts)
        self.device_model.init_glorot(seed=seed or 0)
        built.append(self.device_model)
        return self.device_model
    patch(models.UNetAnnotator, 'build', build)
    return built
