"""Test double for the CPU tests of `predict --lesion_features`: tests/fake_spread_device.SpreadDeviceModel that also keeps the batch
its last forward staged -- the untransformed one, whatever views ran -- plus lesion_table_features, served by
tests/features_oracle.py on that batch.  FeatureSlices is fake_link_device.Slices with more than one channel: the drawn probability
rides in channel 0, the other channels are the caller's.  Test infrastructure only."""

import numpy as np

import features_oracle as FO
from fake_link_device import fake_engine as _fake_engine
from fake_spread_device import SpreadDeviceModel


class FeaturesDeviceModel(SpreadDeviceModel):
    x = None

    def forward(self, x, *a, **kw):
        self.x = np.asarray(x, np.float32).copy()
        return super().forward(x, *a, **kw)

    def forward_tta(self, x, *a, **kw):
        self.x = np.asarray(x, np.float32).copy()
        return super().forward_tta(x, *a, **kw)

    def forward_tta_spread(self, x, *a, **kw):
        self.x = np.asarray(x, np.float32).copy()
        return super().forward_tta_spread(x, *a, **kw)

    def lesion_table_features(self, batch=None, prob=None, x=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0,
                              max_lesions=256, mask=True, bins=32, ring=3):
        assert prob is None and x is None and batch == len(self.prob) == len(self.x)
        self.calls.append(('lesion_table_features', batch, mask, bins, ring))
        s = (threshold, resize_factor, filter_size, min_area, max_lesions)
        rows, totals, masks = FO.LO.lesion_table(self.prob, *s)
        return (rows, totals, masks if mask else None) + FO.lesion_features(self.prob, self.x, *s, bins=bins, ring=ring)


def fake_engine(monkeypatch, max_batch=None):
    """fake_link_device.fake_engine whose model builds a FeaturesDeviceModel"""
    import fake_link_device
    monkeypatch.setattr(fake_link_device, 'LinkDeviceModel', FeaturesDeviceModel)
    return _fake_engine(monkeypatch, max_batch)


class FeatureSlices:
    """a label-free data set with meta: batches (x, paths, sliceIDs) of `batch` slices; x [N, H, W, C] with the probability in
    channel 0"""

    def __init__(self, x, exams, ids, batch, slice_types=None):
        from dnncancerannotator_amd.data import Spec
        self.x, self.exams, self.ids, self.batch = np.asarray(x, np.float32), list(exams), np.asarray(ids), batch
        self.element_spec = (Spec((batch,) + self.x.shape[1:], np.float32),)
        if slice_types:
            self.slice_types = list(slice_types)

    def __iter__(self):
        for i in range(0, len(self.x), self.batch):
            j = i + self.batch
            yield self.x[i:j], self.exams[i:j], self.ids[i:j]
