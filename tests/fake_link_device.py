"""Test double for the CPU tests of `annotator predict --link_slices`: tests/fake_device.FakeDeviceModel whose forward leaves drawn
probabilities 'on the device' and whose lesion_table / lesion_table_linked are served by the numpy oracles (tests/lesion_oracle.py,
tests/link_oracle.py).  Like the library it keeps the row map of the last linked slice, so continues[0] links across calls, and
refuses a set continues[0] without one.  Test infrastructure only."""

import numpy as np

import lesion_oracle as LO
import link_oracle as KO
from fake_device import FakeDeviceModel


class LinkDeviceModel(FakeDeviceModel):
    probs_of = staticmethod(lambda x: x[..., 0])     # the drawn probability rides in channel 0 of x
    carry = None

    def forward(self, x, training=False, return_logits=False, return_prob=True):
        assert not training and not return_prob
        self._check(x)
        self.calls.append(('forward', len(x)))
        self.prob = self.probs_of(np.asarray(x))

    def lesion_table(self, batch=None, prob=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0, max_lesions=256,
                     mask=True):
        assert prob is None and batch == len(self.prob)
        self.calls.append(('lesion_table', batch, mask))
        rows, totals, masks = LO.lesion_table(self.prob, threshold, resize_factor, filter_size, min_area, max_lesions)
        return rows, totals, (masks if mask else None)

    def lesion_table_linked(self, batch=None, prob=None, continues=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0,
                            max_lesions=256, mask=True):
        assert prob is None and batch == len(self.prob) and len(continues) == batch
        flags = [bool(c) for c in continues]
        self.calls.append(('lesion_table_linked', batch, mask, flags))
        if flags[0] and self.carry is None:
            raise ValueError('continues[0] is set, but no linked call precedes this one')
        rows, totals, masks = LO.lesion_table(self.prob, threshold, resize_factor, filter_size, min_area, max_lesions)
        maps = KO.row_maps(self.prob, threshold, resize_factor, filter_size, min_area, max_lesions)
        links = KO.links_of_maps(maps, flags, self.carry)
        self.carry = maps[-1]
        return rows, totals, (masks if mask else None), links


def fake_engine(monkeypatch, max_batch=None):
    """engine.TFKerasModel whose model builds a LinkDeviceModel (of at most max_batch slices per call, when given)"""
    from dnncancerannotator_amd import device, engine, models

    def build(self, input_shape, max_batch_=None, seed=None, force_generic=False):
        b, h, w, c = input_shape
        if max_batch and b > max_batch and getattr(self, 'device_model', None) is not None:
            raise MemoryError('fake device: no room for %d slices per call' % b)      # the engine keeps the model it has and splits
        c_ = self.configs
        self.device_model = LinkDeviceModel(self.arch, c, h, w, min(b, max_batch) if max_batch else (max_batch_ or b or 1),
                                            c_['n_filters_first'], c_['n_downsample'], rate=c_['rate'], kernel_size=c_['kernel_size'],
                                            conv_stride=c_['conv_stride'], bn=c_['bn'], padding=c_['padding'])
        return self.device_model
    monkeypatch.setattr(device, 'init_device', lambda ordinal=0: None)
    monkeypatch.setattr(device, 'device_count', lambda: 1)
    monkeypatch.setattr(models.UNetAnnotator, 'build', build)
    cfg = {'model': 'UNetAnnotator',
           'model_options': dict(n_filters_first=2, n_downsample=1, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same'),
           'deploy_options': {'optimizer': 'adam', 'enable_multigpu': False}}
    return engine.TFKerasModel(cfg)


class Slices:
    """a label-free data set with meta: batches (x, paths, sliceIDs) of `batch` slices from prob [N, H, W], exams [N], ids [N]"""

    def __init__(self, prob, exams, ids, batch):
        from dnncancerannotator_amd.data import Spec
        self.prob, self.exams, self.ids, self.batch = prob, list(exams), np.asarray(ids), batch
        self.element_spec = (Spec((batch,) + prob.shape[1:] + (1,), np.float32),)

    def __iter__(self):
        for i in range(0, len(self.prob), self.batch):
            j = i + self.batch
            yield self.prob[i:j][..., None], self.exams[i:j], self.ids[i:j]
