"""Test double for the CPU tests of deploy_options.ema: tests/fake_device.FakeDeviceModel plus the DeviceModel methods of the weight
average (set_ema / get_ema / set_ema_state / exchange_ema / averaged_weights), with the library's semantics -- the average starts as
a copy of the weights, a train step moves it with the float-rounded 1 - d_n (tests/ema_oracle.py), the exchange swaps contents and
refuses what the library refuses while the average is in use.  Every call goes into `calls`.  Test infrastructure only."""

import numpy as np

import ema_oracle as EO
from fake_device import FakeDeviceModel
from oracle import unet_oracle as O


class EmaDeviceModel(FakeDeviceModel):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.ema = None                  # float64 vector, or None: off
        self.ema_decay, self.ema_warmup, self.ema_updates, self.in_use = 0.0, True, 0, False

    def _refuse(self, what):
        if self.in_use:
            raise RuntimeError('%s: the averaged weights are in use' % what)

    def set_ema(self, decay, warmup=True):
        self._refuse('set_ema')
        self.calls.append(('set_ema', float(decay), bool(warmup)))
        if decay == 0:
            self.ema = None
            return
        if not 0.0 < decay < 1.0:
            raise ValueError('decay')
        self.ema, self.ema_decay, self.ema_warmup, self.ema_updates = self.get_params().astype(np.float64), float(decay), bool(warmup), 0

    def get_ema(self):
        assert self.ema is not None
        return self.ema.astype(np.float32), self.ema_updates

    def set_ema_state(self, flat, num_updates):
        assert self.ema is not None
        self._refuse('set_ema_state')
        self.calls.append(('set_ema_state', int(num_updates)))
        self.ema, self.ema_updates = np.asarray(flat, np.float64).copy(), int(num_updates)

    def exchange_ema(self):
        assert self.ema is not None
        self.calls.append(('exchange_ema',))
        p = np.asarray(O.flatten(self.spec, self.params), np.float64).copy()          # contents, exactly
        FakeDeviceModel.set_params(self, self.ema)
        self.ema, self.in_use = p, not self.in_use

    def averaged_weights(self):
        dm = self

        class Ctx:
            def __enter__(self):
                dm.exchange_ema()
                return dm

            def __exit__(self, *exc):
                dm.exchange_ema()
                return False
        return Ctx()

    def set_params(self, flat):
        self._refuse('set_params')
        super().set_params(flat)

    def set_opt_state(self, m, v, iterations):
        self._refuse('set_opt_state')
        super().set_opt_state(m, v, iterations)

    def train_step(self, x, y, lr, cfg):
        self._refuse('train_step')
        out = super().train_step(x, y, lr, cfg)
        if self.ema is not None:
            self.ema_updates += 1
            self.ema = EO.run([self.get_params()], self.ema, self.ema_decay, self.ema_warmup, first_update=self.ema_updates)
        return out

    def eval_step(self, x, y, cfg, return_prob=False):
        self.calls.append(('eval_in_use', self.in_use))
        return super().eval_step(x, y, cfg, return_prob)


def install(patch=setattr):
    """the engine's device layer -> EmaDeviceModel (as tests/fake_train_metrics.install).  Returns the list of models built."""
    from dnncancerannotator_amd import device, models
    patch(device, 'init_device', lambda ordinal=0: None)
    patch(device, 'device_count', lambda: 1)
    patch(device, 'DeviceModel', EmaDeviceModel)
    built = []

    def build(self, input_shape, max_batch=None, seed=None, force_generic=False):
        b, h, w, c = input_shape
        opts = {k: v for k, v in self.configs.items() if k in ('n_filters_first', 'n_downsample', 'rate', 'kernel_size', 'conv_stride',
                                                               'bn', 'padding')}
        self.device_model = EmaDeviceModel(self.arch, c, h, w, max_batch or b, **opts)
        self.device_model.init_glorot(seed=seed or 0)
        built.append(self.device_model)
        return self.device_model
    patch(models.UNetAnnotator, 'build', build)
    return built
