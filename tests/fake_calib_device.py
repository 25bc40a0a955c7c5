"""Test double for the CPU tests of `--calibration` and `--temperature`: tests/fake_spread_device.SpreadDeviceModel plus calibration
and scale_temperature, served by tests/calib_oracle.py, and a render_composite that only records its call (the Visualizer's order of
calls).  Like the library scale_temperature scales the probability plane in place -- a second call scales again -- and leaves the
spread plane alone; the host-plane form leaves the model's plane alone.  Test infrastructure only."""

import numpy as np

import calib_oracle as CO
from fake_link_device import fake_engine as _fake_engine
from fake_spread_device import SpreadDeviceModel


class CalibDeviceModel(SpreadDeviceModel):
    def calibration(self, y, n_bins=15, temperatures=(), batch=None, prob=None):
        assert prob is None and batch == len(self.prob) and len(temperatures) <= 64
        self.calls.append(('calibration', batch, int(n_bins), [float(t) for t in temperatures]))
        p = np.asarray(self.prob, np.float32).reshape(batch, -1)
        y = np.asarray(y, np.float32).reshape(batch, -1)
        return CO.tables(p, y, int(n_bins)) + (CO.nll(p, y, temperatures),)

    def scale_temperature(self, temperature, batch, prob=None):
        if not 0.05 <= float(temperature) <= 20.0:
            raise ValueError('temperature %r outside [0.05, 20]' % (temperature,))
        if prob is not None:
            return CO.scale(prob, temperature)
        assert batch == len(self.prob)
        self.calls.append(('scale_temperature', batch, float(temperature)))
        self.prob = CO.scale(self.prob, temperature)

    def render_composite(self, y, batch, ratio=0.5, overlay=False):
        assert batch == len(self.prob)
        self.calls.append(('render_composite', batch))
        return [np.zeros((2, 6, 1), np.uint8)] * batch


def fake_engine(monkeypatch, max_batch=None):
    """fake_link_device.fake_engine whose model builds a CalibDeviceModel"""
    import fake_link_device
    monkeypatch.setattr(fake_link_device, 'LinkDeviceModel', CalibDeviceModel)
    return _fake_engine(monkeypatch, max_batch)
