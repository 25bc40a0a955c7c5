"""-m gpu: what the eight analysis entry points of the C ABI answer for every kind of plane input, as one table.

dnnca_lesion_table, _linked, _spread, _matched, dnnca_surface_distances, dnnca_spread_by_outcome, dnnca_calibration and
dnnca_prob_temperature all take either host planes (prob_hw with h and w) or the model's own (prob_hw NULL; h = w = 0 or the model's
size), and resolve, refuse and stage them alike.  This file pins down where they do NOT answer alike: the return code of every entry
in every state of the model, what a host-plane call leaves of the model's state, and which scratch buffer it stages into (one of the
two forgets the labels kept for dnnca_render_composite).

The expected codes are literals.  They were taken from a run of this file against the library as it stood BEFORE the plane inputs
got one resolver and one stager, and characterise that library: a change of any of them is a change of behaviour, wanted or not.
Every refused call must leave the sentinel-filled output buffers untouched and, under profile_enable(1), record no launch."""

import ctypes as C

import numpy as np
import pytest

from test_lesion_gpu import UNET
from test_tta_gpu import drawn, random_weights

pytestmark = pytest.mark.gpu

OK, EINVAL, ESTATE = 0, -1, -4
SENTINEL = 0xAB
UNTOUCHED = -7
ENTRIES = ('lesion_table', 'lesion_table_linked', 'lesion_table_spread', 'lesion_table_matched', 'surface_distances',
           'spread_by_outcome', 'calibration', 'prob_temperature')
SPREAD = (OK, OK, ESTATE, OK, OK, ESTATE, OK, OK)           # everything runs but the two consumers of the model's spread plane
STALE = (OK, OK, ESTATE, OK, OK, ESTATE, ESTATE, ESTATE)    # more slices than the model holds: only some entries look
# state of the model, planes -> the codes of ENTRIES.  `own`: prob_hw NULL (batch, h, w); `host`: 16 x 32 planes of `batch` slices
EXPECTED = [
    ('fresh', 'own', (1, 0, 0), STALE),
    ('fresh', 'own', (1, 16, 16), STALE),
    ('fresh', 'own', (1, 16, 32), (EINVAL,) * 8),
    ('fresh', 'own', (0, 0, 0), (EINVAL,) * 8),
    ('fresh', 'own', (4, 0, 0), (EINVAL,) * 8),
    ('fresh', 'host', (0, 16, 32), (EINVAL,) * 8),
    ('fresh', 'host', (4, 16, 32), (EINVAL,) * 8),
    ('forward of 2', 'own', (2, 0, 0), SPREAD),
    ('forward of 2', 'own', (3, 0, 0), STALE),
    ('forward_tta_spread of 2', 'own', (2, 0, 0), (OK,) * 8),
    ('forward_tta_spread of 2', 'own', (2, 16, 16), (OK,) * 8),
    ('forward_tta_spread of 2', 'own', (3, 0, 0), STALE),
    ('forward_tta_spread of 2', 'own', (2, 16, 32), (EINVAL,) * 8),
    ('forward_tta_spread of 2', 'host', (2, 16, 32), (OK,) * 8),
    ('pixel_confusion_of', 'own', (2, 0, 0), SPREAD),
    ('pixel_confusion_of', 'host', (2, 16, 32), (OK,) * 8),
]
# dnnca_render_composite with NULL labels after dnnca_region_confusion_slices and then the entry: the entries that stage into the
# region inputs forget the kept labels (the matched and the surface call stage their labels there for the model's planes too)
RENDER = {'host': (ESTATE, ESTATE, ESTATE, ESTATE, ESTATE, OK, OK, OK), 'own': (OK, OK, OK, ESTATE, ESTATE, OK, OK, OK)}


class Harness:
    """one model, the sentinel-filled output buffers, and the eight entries as functions of (prob, batch, h, w)"""

    def __init__(self, gpu, seed):
        from dnncancerannotator_amd import _lib
        self.L = _lib
        self.m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
        random_weights(self.m, seed)
        self.p = drawn((4, 16, 32), seed + 1)                # host probabilities, spread and labels alike
        self.x = drawn((2, 16, 16, 1), seed + 2)
        self.bufs = {k: np.full(1 << 17, SENTINEL, np.uint8) for k in
                     ('rows', 'totals', 'mask', 'links', 'n', 'srows', 'stotals', 'trows', 'ttotals', 'tlinks', 'pairs', 'out', 'aux')}
        self.hw = (C.c_int32 * 2)()                          # written before some refusals: not among the guarded buffers
        self.structs = []

    def ptr(self, name, ctype, offset=0):
        return C.cast(self.bufs[name].ctypes.data + offset, C.POINTER(ctype))

    def cap(self, name, ctype):
        return self.bufs[name].size // C.sizeof(ctype)

    def entry(self, name, prob, batch, h, w):
        L, lib, H, ptr, cap = self.L, self.m.lib, self.m.handle, self.ptr, self.cap
        fp = None if prob is None else L.fptr(prob)
        y = L.fptr(self.p)
        zeros = np.zeros(8, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
        les = (H, fp, batch, h, w, 0.5, 1.0, 5, 0, 256)
        out = (ptr('rows', L.LesionRow), cap('rows', L.LesionRow), ptr('n', C.c_int64), ptr('totals', C.c_int32),
               self.bufs['mask'].ctypes.data_as(C.c_void_p), self.bufs['mask'].size, self.hw)
        if name == 'lesion_table':
            return lib.dnnca_lesion_table(*les, *out)
        if name == 'lesion_table_linked':
            return lib.dnnca_lesion_table_linked(*les, *out, zeros, ptr('links', L.LesionLink), cap('links', L.LesionLink),
                                                 ptr('n', C.c_int64, 8))
        if name == 'lesion_table_spread':
            return lib.dnnca_lesion_table_spread(*les, *out, fp, ptr('srows', L.LesionSpread), ptr('stotals', L.SliceSpread))
        if name == 'lesion_table_matched':
            pred = L.LesionPlaneOut(ptr('rows', L.LesionRow), cap('rows', L.LesionRow), UNTOUCHED, ptr('totals', C.c_int32),
                                    ptr('links', L.LesionLink), cap('links', L.LesionLink), UNTOUCHED)
            truth = L.LesionPlaneOut(ptr('trows', L.LesionRow), cap('trows', L.LesionRow), UNTOUCHED, ptr('ttotals', C.c_int32),
                                     ptr('tlinks', L.LesionLink), cap('tlinks', L.LesionLink), UNTOUCHED)
            pairs = L.LesionPairsOut(ptr('pairs', L.LesionPair), cap('pairs', L.LesionPair), UNTOUCHED)
            self.structs = [pred, truth, pairs]
            return lib.dnnca_lesion_table_matched(H, fp, y, batch, h, w, 0.5, 1.0, 5, 0, 256, zeros, C.byref(pred),
                                                  self.bufs['mask'].ctypes.data_as(C.c_void_p), self.bufs['mask'].size, C.byref(truth),
                                                  C.byref(pairs), self.hw)
        if name == 'surface_distances':
            return lib.dnnca_surface_distances(H, fp, y, batch, h, w, 0.5, 1.0, 5, 0, 65536, ptr('totals', C.c_int32),
                                               ptr('rows', L.SurfaceSample), cap('rows', L.SurfaceSample), ptr('n', C.c_int64),
                                               self.bufs['mask'].ctypes.data_as(C.c_void_p), self.bufs['mask'].size, self.hw)
        if name == 'spread_by_outcome':
            return lib.dnnca_spread_by_outcome(H, fp, fp, y, batch, h, w, L.fptr(np.array([0.5], np.float32)), 1,
                                               ptr('out', L.SpreadOutcome))
        if name == 'calibration':
            return lib.dnnca_calibration(H, fp, y, batch, h, w, 10, L.fptr(np.array([1.0, 2.0], np.float32)), 2, ptr('rows', L.CalibBin),
                                         ptr('totals', L.CalibTotal), ptr('aux', C.c_double))
        assert name == 'prob_temperature'
        return lib.dnnca_prob_temperature(H, fp, batch, h, w, 1.5, None if prob is None else ptr('out', C.c_float))

    def call(self, name, planes, batch, h, w):
        """the code of one call; a refused one must have written nothing and launched nothing"""
        m = self.m
        m.sync()
        m.profile_reset()
        m.profile_enable(1)
        try:
            self.structs = []
            code = self.entry(name, self.p if planes == 'host' else None, batch, h, w)
            if code != OK:
                assert m.lib.dnnca_last_error(), name
                assert all((b == SENTINEL).all() for b in self.bufs.values()), '%s wrote to an output before it refused' % name
                assert all(getattr(s, f) == UNTOUCHED for s in self.structs for f in ('n_rows', 'n_links', 'n_pairs') if hasattr(s, f))
                assert m.profile() == [], '%s launched before it refused' % name
        finally:
            m.profile_enable(0)
            m.profile_reset()
        for b in self.bufs.values():
            b[:] = SENTINEL
        return code

    def spread_valid(self):
        out = np.empty(2 * 256, np.float32)
        return self.m.lib.dnnca_get_tta_spread(self.m.handle, 2, self.L.fptr(out))

    def enter(self, state):
        m = self.m
        if state == 'forward of 2':
            m.forward(self.x, training=False, return_prob=False)
        elif state == 'forward_tta_spread of 2':
            m.forward_tta_spread(self.x, 0x03, return_prob=False, return_spread=False)
        elif state == 'pixel_confusion_of':
            m.pixel_confusion_of(self.p[:2, :, :16], self.p[2:, :, :16], (0.5,))


def test_the_codes_of_every_entry_in_every_state(gpu):
    hs = Harness(gpu, 41)
    try:
        got, state = [], 'fresh'
        for want_state, planes, (batch, h, w), _ in EXPECTED:
            if want_state != state:
                state = want_state
                hs.enter(state)
            if planes == 'host':
                prob, valid = hs.m.last_prob(2), hs.spread_valid()
            codes = tuple(hs.call(name, planes, batch, h, w) for name in ENTRIES)
            if planes == 'host':      # a call on host planes leaves the model's own alone
                assert hs.m.last_prob(2).tobytes() == prob.tobytes(), (state, batch)
                assert hs.spread_valid() == valid == (OK if state == 'forward_tta_spread of 2' else ESTATE), (state, batch)
            print('%-24s %-4s %-12s %s' % (state, planes, (batch, h, w), codes))
            got.append((state, planes, (batch, h, w), codes))
        assert got == EXPECTED
    finally:
        hs.m.close()


@pytest.mark.parametrize('planes', ['host', 'own'])
def test_which_entries_forget_the_labels_kept_for_render_composite(gpu, planes):
    hs = Harness(gpu, 43)
    try:
        m, got = hs.m, []
        y = (hs.p[:2, :, :16] < 0.3).astype(np.float32)
        hwc = (C.c_int32 * 3)()
        out = np.empty(1 << 16, np.uint8)
        for name in ENTRIES:
            hs.enter('forward_tta_spread of 2')
            m.region_confusion_slices(y, [((0.5,), 0.3, 1.0, 5)])
            assert hs.call(name, planes, 2, 16 if planes == 'host' else 0, 32 if planes == 'host' else 0) == OK, name
            got.append(m.lib.dnnca_render_composite(m.handle, None, 2, 0.5, 0, out.ctypes.data_as(C.c_void_p), out.size, hwc))
        print(planes, got)
        assert tuple(got) == RENDER[planes]
    finally:
        hs.m.close()
