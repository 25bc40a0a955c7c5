"""Test double for the CPU tests of `annotator evaluate --bootstrap`: tests/fake_detection_device.DetectionDeviceModel plus
bootstrap_sums / bootstrap_detection served by tests/bootstrap_oracle.py, with the return types of DeviceModel.  Test infrastructure
only."""

import numpy as np

import bootstrap_oracle as BO
from fake_detection_device import DetectionDeviceModel, LabelledSlices          # noqa: F401 (LabelledSlices: for the tests)
from fake_match_device import fake_engine as _fake_engine


def _resampling(E, strata):
    return BO.plain(E) if strata is None else (np.asarray(strata[0], np.int32), np.asarray(strata[1], np.int32))


class BootstrapDeviceModel(DetectionDeviceModel):
    def bootstrap_sums(self, cols, replicates, seed=0, strata=None, multiplicities=False):
        cols = np.asarray(cols, np.int32)
        E, K = cols.shape
        pool, sizes = _resampling(E, strata)
        self.calls.append(('bootstrap_sums', cols.tolist(), int(replicates), int(seed), sizes.tolist()))
        mult = BO.multiplicities(E, pool, sizes, int(replicates), int(seed))
        out = np.zeros(int(replicates), [('sums', '<i8', (K,))] + ([('multiplicities', '<u2', (E,))] if multiplicities else []))
        out['sums'] = BO.sums(cols, mult)
        if multiplicities:
            out['multiplicities'] = mult
        return out

    def bootstrap_detection(self, exams, candidates, replicates, seed=0, strata=None, multiplicities=False):
        E = len(exams)
        pool, sizes = _resampling(E, strata)
        self.calls.append(('bootstrap_detection', E, len(candidates), int(replicates), int(seed), pool.tolist(), sizes.tolist()))
        mult = BO.multiplicities(E, pool, sizes, int(replicates), int(seed))
        rows, _ = BO.detection(exams, candidates, mult)
        if not multiplicities:
            return rows
        out = np.zeros(len(rows), BO.ROW_DTYPE.descr + [('multiplicities', '<u2', (E,))])
        for name in rows.dtype.names:
            out[name] = rows[name]
        out['multiplicities'] = mult
        return out


def fake_engine(monkeypatch, max_batch=None):
    """fake_link_device.fake_engine whose model builds a BootstrapDeviceModel"""
    import fake_match_device
    monkeypatch.setattr(fake_match_device, 'MatchDeviceModel', BootstrapDeviceModel)
    return _fake_engine(monkeypatch, max_batch)
