"""Test double for the CPU tests of `--ensemble`: tests/fake_spread_device.SpreadDeviceModel plus set_members, member,
forward_ensemble and last_ensemble_spread, served by tests/ensemble_oracle.py.  Member m of the fake ensemble scales what the fake
network gives (the drawn probability in channel 0 of x, view k scaled by 1 - k / 32) by 1 - m / 8, so that the members disagree;
spread_by_outcome also takes the host planes the engine hands it for the two components.  Test infrastructure only."""

import numpy as np

import ensemble_oracle as EO
import spread_oracle as SO
import tta_oracle as TO
from fake_link_device import fake_engine as _fake_engine
from fake_spread_device import SpreadDeviceModel


def member_planes(x, views, n):
    """(means [n, B, H, W], withins [n, B, H, W]) of the fake ensemble of n members on the batch x"""
    x = np.asarray(x, np.float32)
    views = int(views)
    back = SO.back(np.stack([(TO.apply_view(x, k)[..., 0] * np.float32(1 - k / 32)).astype(np.float32) for k in TO.views_of(views)]), views)
    means, withins = [], []
    for m in range(n):
        planes = (back * np.float32(1 - m / 8)).astype(np.float32)
        means.append(EO.mean_of(planes))
        withins.append(planes.astype(np.float64).std(axis=0).astype(np.float32))
    return np.stack(means), np.stack(withins)


class EnsembleDeviceModel(SpreadDeviceModel):
    members = ()
    between = within = None

    def set_members(self, members):
        self.calls.append(('set_members', len(members)))
        self.members = [(np.array(p, np.float32), np.array(s, np.float32)) for p, s in members]

    def member(self, m):
        return self.members[m]

    def forward(self, *a, **kw):
        self.between = self.within = None
        return super().forward(*a, **kw)

    def forward_tta(self, *a, **kw):
        self.between = self.within = None
        return super().forward_tta(*a, **kw)

    def forward_tta_spread(self, *a, **kw):
        self.between = self.within = None
        return super().forward_tta_spread(*a, **kw)

    def forward_ensemble(self, x, views=1, spread=False, return_prob=True):
        assert not return_prob and self.members
        self._check(x)
        self.calls.append(('forward_ensemble', len(x), int(views), bool(spread)))
        means, withins = member_planes(x, views, len(self.members))
        self.prob = EO.mean_of(means)
        self.spread = self.between = self.within = None
        if spread:
            self.between = EO.between_of(means).astype(np.float32)
            self.within = EO.within_of(means, withins).astype(np.float32)
            self.spread = EO.total_of(means, withins).astype(np.float32)

    def last_prob(self, batch):
        assert batch == len(self.prob)
        return self.prob.copy()

    def last_ensemble_spread(self, batch):
        self._valid(batch)
        if self.between is None:
            raise ValueError('the spread plane is not an ensemble\'s')
        self.calls.append(('last_ensemble_spread', batch))
        return self.between.copy(), self.within.copy()

    def spread_by_outcome(self, y, thresholds=(0.5,), batch=None, prob=None, spread=None):
        if prob is None:
            return super().spread_by_outcome(y, thresholds, batch=batch)
        assert spread is not None and 1 <= len(thresholds) <= 64
        self.calls.append(('spread_by_outcome_of', len(prob), [float(t) for t in thresholds]))
        return SO.outcome(prob, spread, np.asarray(y, np.float32).reshape(np.shape(prob)), thresholds)


def fake_engine(monkeypatch, max_batch=None):
    """fake_link_device.fake_engine whose model builds an EnsembleDeviceModel"""
    import fake_link_device
    monkeypatch.setattr(fake_link_device, 'LinkDeviceModel', EnsembleDeviceModel)
    return _fake_engine(monkeypatch, max_batch)
