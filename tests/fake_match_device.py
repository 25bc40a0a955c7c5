"""Test double for the CPU tests of `annotator evaluate --exam_lesions`: tests/fake_link_device.LinkDeviceModel plus
lesion_table_matched served by tests/match_oracle.py.  Like the library it keeps the two row maps of the last slice of the last
matched call -- whatever threshold that call had -- apart from the linked call's, refuses a set continues[0] without them, and
leaves the last forward's probabilities alone when it is given `prob`.  Test infrastructure only."""

import numpy as np

import match_oracle as MO
from fake_link_device import LinkDeviceModel, fake_engine as _fake_engine


class MatchDeviceModel(LinkDeviceModel):
    match_carry = None

    def last_prob(self, batch):
        self.calls.append(('last_prob', batch))
        return np.asarray(self.prob[:batch], np.float32).copy()

    def lesion_table_matched(self, y, batch=None, prob=None, continues=None, threshold=0.5, resize_factor=1.0, filter_size=5,
                             min_area=0, max_lesions=256, mask=False):
        p = self.prob if prob is None else np.asarray(prob, np.float32)
        y = np.asarray(y, np.float32).reshape(p.shape)
        assert not mask and len(continues) == len(p) and (prob is not None or batch == len(p))
        flags = [bool(c) for c in continues]
        self.calls.append(('lesion_table_matched', len(p), 'host' if prob is not None else 'last', float(threshold), flags))
        if flags[0] and self.match_carry is None:
            raise ValueError('continues[0] is set, but no matched call precedes this one')
        carry, true_carry = self.match_carry or (None, None)
        s = (threshold, resize_factor, filter_size, min_area, max_lesions)
        out = MO.matched(p, y, flags, *s, carry=carry, true_carry=true_carry)
        self.match_carry = MO.pred_maps(p, *s)[-1], MO.true_maps(y, resize_factor, max_lesions)[-1]
        return out[:2] + (None,) + out[3:]


def fake_engine(monkeypatch, max_batch=None):
    """fake_link_device.fake_engine whose model builds a MatchDeviceModel"""
    import fake_link_device
    monkeypatch.setattr(fake_link_device, 'LinkDeviceModel', MatchDeviceModel)
    return _fake_engine(monkeypatch, max_batch)


class LabelledSlices:
    """a labelled data set with meta: batches (x, y, paths, sliceIDs) of `batch` slices from prob / y [N, H, W], exams [N], ids [N]"""

    def __init__(self, prob, y, exams, ids, batch):
        from dnncancerannotator_amd.data import Spec
        self.prob, self.y, self.exams, self.ids, self.batch = prob, y, list(exams), np.asarray(ids), batch
        self.element_spec = (Spec((batch,) + prob.shape[1:] + (1,), np.float32), Spec((batch,) + prob.shape[1:], np.float32))

    def __iter__(self):
        for i in range(0, len(self.prob), self.batch):
            j = i + self.batch
            yield self.prob[i:j][..., None], self.y[i:j], self.exams[i:j], self.ids[i:j]
