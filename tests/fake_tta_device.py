"""Test double for the CPU tests of `--tta`: tests/fake_surface_device.SurfaceDeviceModel (a tests/fake_device.FakeDeviceModel) plus
forward_tta, served by tests/tta_oracle.py around the same fake network (the drawn probability rides in channel 0 of x).  Every
forward, plain or augmented, goes into `calls`.  Test infrastructure only."""

import numpy as np

import tta_oracle as TO
from fake_link_device import fake_engine as _fake_engine
from fake_surface_device import SurfaceDeviceModel


class TtaDeviceModel(SurfaceDeviceModel):
    def forward_tta(self, x, views, return_prob=True):
        assert not return_prob
        self._check(x)
        self.calls.append(('forward_tta', len(x), int(views)))
        x = np.asarray(x, np.float32)
        planes = [self.probs_of(TO.apply_view(x, k)) for k in TO.views_of(int(views))]
        self.prob = TO.mean_of(planes, int(views))


def fake_engine(monkeypatch, max_batch=None):
    """fake_link_device.fake_engine whose model builds a TtaDeviceModel"""
    import fake_link_device
    monkeypatch.setattr(fake_link_device, 'LinkDeviceModel', TtaDeviceModel)
    return _fake_engine(monkeypatch, max_batch)
