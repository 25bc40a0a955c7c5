"""Test double for the CPU tests of `annotator evaluate --surface_distances`: tests/fake_match_device.MatchDeviceModel plus
surface_distances served by tests/surface_oracle.py.  Like the library the call reads the last forward's probabilities, keeps
nothing between calls and leaves the carries of the linked and of the matched call alone.  Test infrastructure only."""

import numpy as np

import surface_oracle as SO
from fake_link_device import fake_engine as _fake_engine
from fake_match_device import LabelledSlices, MatchDeviceModel          # noqa: F401 (LabelledSlices: for the tests)


class SurfaceDeviceModel(MatchDeviceModel):
    def surface_distances(self, y, batch=None, prob=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0,
                          max_samples=65536, edges=False):
        assert prob is None and not edges and batch == len(self.prob)
        self.calls.append(('surface_distances', batch, float(threshold), int(max_samples)))
        y = np.asarray(y, np.float32).reshape(self.prob.shape)
        counts, samples, _ = SO.surface(self.prob, y, threshold, resize_factor, filter_size, min_area, max_samples)
        return counts, samples, None


def fake_engine(monkeypatch, max_batch=None):
    """fake_link_device.fake_engine whose model builds a SurfaceDeviceModel"""
    import fake_link_device
    monkeypatch.setattr(fake_link_device, 'LinkDeviceModel', SurfaceDeviceModel)
    return _fake_engine(monkeypatch, max_batch)
