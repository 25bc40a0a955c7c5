"""Test double for the CPU tests of `evaluate --visualize_attribution`: tests/fake_calib_device.CalibDeviceModel plus an
integrated_gradients that records its call and returns values drawn from the probabilities the last forward left (attribution_of
below: two 'modalities', whatever the input has), an input_sensitivity and a region_confusion_slices that only record theirs.  Test
infrastructure only."""

import numpy as np

from dnncancerannotator_amd.device import Attribution
from fake_calib_device import CalibDeviceModel
from fake_link_device import fake_engine as _fake_engine


def attribution_of(prob, steps, baseline, return_map):
    """prob [B, H, W] -> Attribution: the map is (prob, -prob / 2) scaled by 1 / steps, the sums are its sums, F(x) = sum(prob) and
    F(baseline) = 1 for 'mean', 0 for 'black'"""
    p = np.asarray(prob, np.float64)
    amap = np.stack([p, -0.5 * p], -1) / float(steps)
    ends = np.stack([p.sum((1, 2)), np.full(len(p), 1.0 if baseline == 'mean' else 0.0)], 1)
    return Attribution(amap.sum((1, 2)), np.abs(amap).sum((1, 2)), ends, amap.astype(np.float32) if return_map else None)


class AttrDeviceModel(CalibDeviceModel):
    def integrated_gradients(self, x=None, batch=None, steps=32, baseline='black', return_map=False):
        assert x is None and batch == len(self.prob) and 1 <= steps <= 256 and baseline in ('black', 'mean')
        self.calls.append(('integrated_gradients', batch, int(steps), baseline, bool(return_map)))
        return attribution_of(self.prob, steps, baseline, return_map)

    def input_sensitivity(self, x=None, batch=None):
        assert x is None and batch == len(self.prob)
        self.calls.append(('input_sensitivity', batch))
        return np.ones((batch, 2), np.float64)

    def region_confusion_slices(self, y, specs):
        self.calls.append(('region_confusion_slices', len(y)))
        return np.zeros((len(y), len(specs[0][0]), 4), np.int64)


def fake_engine(monkeypatch, max_batch=None):
    """fake_link_device.fake_engine whose model builds an AttrDeviceModel"""
    import fake_link_device
    monkeypatch.setattr(fake_link_device, 'LinkDeviceModel', AttrDeviceModel)
    return _fake_engine(monkeypatch, max_batch)
