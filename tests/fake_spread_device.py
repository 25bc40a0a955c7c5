"""Test double for the CPU tests of `--uncertainty`: tests/fake_tta_device.TtaDeviceModel whose views DISAGREE -- view k of the fake
network scales the drawn probability by 1 - k / 32, in forward_tta and in forward_tta_spread alike, so that the spread is not zero
and both calls leave the same mean -- plus forward_tta_spread, last_spread, lesion_table_spread and spread_by_outcome, served by
tests/spread_oracle.py.  Like the library the spread plane is valid only behind forward_tta_spread.  Test infrastructure only."""

import numpy as np

import spread_oracle as SO
import tta_oracle as TO
from fake_link_device import fake_engine as _fake_engine
from fake_tta_device import TtaDeviceModel


class SpreadDeviceModel(TtaDeviceModel):
    spread = None

    def _views(self, x, views):
        x = np.asarray(x, np.float32)
        return np.stack([(self.probs_of(TO.apply_view(x, k)) * np.float32(1 - k / 32)).astype(np.float32) for k in TO.views_of(int(views))])

    def forward(self, *a, **kw):
        self.spread = None
        return super().forward(*a, **kw)

    def eval_step(self, *a, **kw):
        self.spread = None
        return super().eval_step(*a, **kw)

    def forward_tta(self, x, views, return_prob=True):
        assert not return_prob
        self._check(x)
        self.calls.append(('forward_tta', len(x), int(views)))
        self.prob, self.spread = TO.mean_of(self._views(x, views), int(views)), None

    def forward_tta_spread(self, x, views, return_prob=True, return_spread=True):
        assert not return_prob and not return_spread
        self._check(x)
        self.calls.append(('forward_tta_spread', len(x), int(views)))
        planes = self._views(x, views)
        self.prob, self.spread = TO.mean_of(planes, int(views)), SO.spread_of(planes, int(views)).astype(np.float32)
        return None, None

    def _valid(self, batch):
        if self.spread is None or batch != len(self.spread):
            raise ValueError('the spread plane is not valid: forward_tta_spread makes it valid')

    def last_spread(self, batch):
        self._valid(batch)
        self.calls.append(('last_spread', batch))
        return self.spread.copy()

    def lesion_table_spread(self, batch=None, prob=None, spread=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0,
                            max_lesions=256, mask=True):
        assert prob is None and spread is None and batch == len(self.prob)
        self._valid(batch)
        self.calls.append(('lesion_table_spread', batch, mask))
        s = (threshold, resize_factor, filter_size, min_area, max_lesions)
        rows, totals, masks = SO.LO.lesion_table(self.prob, *s)
        return (rows, totals, masks if mask else None) + SO.lesion_spread(self.prob, self.spread, *s)

    def spread_by_outcome(self, y, thresholds=(0.5,), batch=None, prob=None, spread=None):
        assert prob is None and spread is None and batch == len(self.prob) and 1 <= len(thresholds) <= 64
        self._valid(batch)
        self.calls.append(('spread_by_outcome', batch, [float(t) for t in thresholds]))
        return SO.outcome(self.prob, self.spread, np.asarray(y, np.float32).reshape(self.prob.shape), thresholds)


def fake_engine(monkeypatch, max_batch=None):
    """fake_link_device.fake_engine whose model builds a SpreadDeviceModel"""
    import fake_link_device
    monkeypatch.setattr(fake_link_device, 'LinkDeviceModel', SpreadDeviceModel)
    return _fake_engine(monkeypatch, max_batch)
