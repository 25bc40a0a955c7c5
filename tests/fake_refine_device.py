"""Test double for the CPU tests of the `--refine_*` flags: tests/fake_surface_device.SurfaceDeviceModel and
tests/fake_detection_device.DetectionDeviceModel in one, plus set_lesion_refine / lesion_refine.  Like the library the setting is
model state that every later table call reads: while it is on, lesion_table, lesion_table_linked, the prediction side of
lesion_table_matched and surface_distances are served by tests/refine_oracle.py; while it is off they are the parents' calls, which
never see it.  A kept plane counts only under the configuration that made it.  Test infrastructure only."""

import numpy as np

import link_oracle as KO
import match_oracle as MO
import refine_oracle as RO
from fake_detection_device import DetectionDeviceModel
from fake_link_device import fake_engine as _fake_engine
from fake_match_device import LabelledSlices                              # noqa: F401 (for the tests)
from fake_surface_device import SurfaceDeviceModel


class RefineDeviceModel(SurfaceDeviceModel, DetectionDeviceModel):
    refine = None                        # the oracle's refine spec; None: off
    carry_refine = match_carry_refine = None

    def set_lesion_refine(self, hysteresis=None, closing=0, fill_holes=False):
        self.calls.append(('set_lesion_refine', hysteresis, closing, fill_holes))
        on = hysteresis is not None or closing > 1 or fill_holes
        self.refine = dict(hysteresis=hysteresis, closing=closing, fill_holes=bool(fill_holes)) if on else None

    def lesion_refine(self):
        r = self.refine or RO.OFF
        return r['hysteresis'], r['closing'], r['fill_holes']

    def lesion_table(self, batch=None, prob=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0, max_lesions=256,
                     mask=True):
        if self.refine is None:
            return super().lesion_table(batch, prob, threshold, resize_factor, filter_size, min_area, max_lesions, mask)
        assert prob is None and batch == len(self.prob)
        self.calls.append(('lesion_table', batch, mask))
        rows, totals, masks = RO.lesion_table(self.prob, threshold, resize_factor, filter_size, min_area, max_lesions, refine=self.refine)
        return rows, totals, (masks if mask else None)

    def lesion_table_linked(self, batch=None, prob=None, continues=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0,
                            max_lesions=256, mask=True):
        if continues[0] and self.carry_refine != self.refine:
            raise ValueError('continues[0] is set, but no linked call under this refinement precedes this one')
        if self.refine is None:
            out = super().lesion_table_linked(batch, prob, continues, threshold, resize_factor, filter_size, min_area, max_lesions, mask)
        else:
            assert prob is None and batch == len(self.prob) and len(continues) == batch
            flags = [bool(c) for c in continues]
            self.calls.append(('lesion_table_linked', batch, mask, flags))
            s = (threshold, resize_factor, filter_size, min_area, max_lesions)
            rows, totals, masks = RO.lesion_table(self.prob, *s, refine=self.refine)
            maps = RO.row_maps(self.prob, *s, refine=self.refine)
            links = KO.links_of_maps(maps, flags, self.carry if flags[0] else None)
            self.carry = maps[-1]
            out = rows, totals, (masks if mask else None), links
        self.carry_refine = self.refine
        return out

    def lesion_table_matched(self, y, batch=None, prob=None, continues=None, threshold=0.5, resize_factor=1.0, filter_size=5,
                             min_area=0, max_lesions=256, mask=False):
        if continues[0] and self.match_carry_refine != self.refine:
            raise ValueError('continues[0] is set, but no matched call under this refinement precedes this one')
        if self.refine is None:
            out = super().lesion_table_matched(y, batch, prob, continues, threshold, resize_factor, filter_size, min_area, max_lesions, mask)
        else:
            p = self.prob if prob is None else np.asarray(prob, np.float32)
            y = np.asarray(y, np.float32).reshape(p.shape)
            assert not mask and len(continues) == len(p) and (prob is not None or batch == len(p))
            flags = [bool(c) for c in continues]
            self.calls.append(('lesion_table_matched', len(p), 'host' if prob is not None else 'last', float(threshold), flags))
            carry, true_carry = self.match_carry if flags[0] else (None, None)
            s = (threshold, resize_factor, filter_size, min_area, max_lesions)
            pm, tm = RO.row_maps(p, *s, refine=self.refine), MO.true_maps(y, resize_factor, max_lesions)
            rows, totals, _ = RO.lesion_table(p, *s, refine=self.refine)
            true_rows, true_totals = MO.true_table(y, resize_factor, max_lesions)
            self.match_carry = pm[-1], tm[-1]
            out = (rows, totals, None, KO.links_of_maps(pm, flags, carry), true_rows, true_totals, KO.links_of_maps(tm, flags, true_carry),
                   MO.pairs_of_maps(tm, pm))
        self.match_carry_refine = self.refine
        return out

    def surface_distances(self, y, batch=None, prob=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0,
                          max_samples=65536, edges=False):
        if self.refine is None:
            return super().surface_distances(y, batch, prob, threshold, resize_factor, filter_size, min_area, max_samples, edges)
        assert prob is None and not edges and batch == len(self.prob)
        self.calls.append(('surface_distances', batch, float(threshold), int(max_samples)))
        y = np.asarray(y, np.float32).reshape(self.prob.shape)
        counts, samples, _ = RO.surface(self.prob, y, threshold, resize_factor, filter_size, min_area, max_samples, refine=self.refine)
        return counts, samples, None


def fake_engine(monkeypatch, max_batch=None):
    """fake_link_device.fake_engine whose model builds a RefineDeviceModel"""
    import fake_link_device
    monkeypatch.setattr(fake_link_device, 'LinkDeviceModel', RefineDeviceModel)
    return _fake_engine(monkeypatch, max_batch)
