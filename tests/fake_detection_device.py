"""Test double for the CPU tests of `annotator evaluate --detection` and `annotator predict --detection_map`:
tests/fake_match_device.MatchDeviceModel plus detection_map served by tests/detection_oracle.py.  Like the library the in-place call
replaces the last forward's probabilities by the map, so every later table call reads the map.  Test infrastructure only."""

import numpy as np

import detection_oracle as DO
from fake_match_device import LabelledSlices, MatchDeviceModel          # noqa: F401 (LabelledSlices: for the tests)
from fake_match_device import fake_engine as _fake_engine


class DetectionDeviceModel(MatchDeviceModel):
    def detection_map(self, batch, **cfg):
        assert batch == len(self.prob)
        self.calls.append(('detection_map', batch, dict(cfg)))
        D, rows, slices = DO.detection_map(self.prob, **cfg)
        self.prob = D
        return rows, slices

    def detection_map_of(self, prob, **cfg):
        self.calls.append(('detection_map_of', len(prob), dict(cfg)))
        return DO.detection_map(prob, **cfg)


def fake_engine(monkeypatch, max_batch=None):
    """fake_link_device.fake_engine whose model builds a DetectionDeviceModel"""
    import fake_match_device
    monkeypatch.setattr(fake_match_device, 'MatchDeviceModel', DetectionDeviceModel)
    return _fake_engine(monkeypatch, max_batch)
