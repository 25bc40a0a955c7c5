"""-m gpu: the backward launch of the last decoder block (`pgbwd_tc_3x2_3`: the two-source 3-channel conv with the 6 -> 3 transposed
conv's backward riding along, k_pgbwd VW + TCF in its counted-wait form CW) against the float64 oracle.

The launch writes the skip gradient, the gradient of the transposed conv's input (the 256^2-level tensor at the real size), and
the weight / bias gradients of both layers.  Against the oracle the two data gradients are held through everything computed from
them: the skip gradient feeds the whole first encoder block, the gradient of the transposed conv's input every layer below the
last decoder block.  Every variable of the network is compared on its own scale with the per-tensor bound of the block-backward
tests (test_parity_gpu.GRAD_TOL = 2e-5, on top of 10 x what plain float32 numpy costs on that tensor).  The comparison of the two
forms of the kernel reads the two data-gradient buffers themselves (dnnca_debug_tcf_dgrads, csrc/debug_tools.hip).

Shapes: the kernel's tile is BW<3, 2, 3>::TW = 128 pixels wide and TH = 8 rows tall, and the launch needs whole tiles.
  (1,  8, 128)   one tile: every edge is a halo and the first prefetch past the end fires at once
  (1, 24, 256)   2 x 3 tiles: interior seams, a tile count that is no multiple of 8 (no XCD-aware order)
  (3, 24, 256)   the same in a model built for 4: a batch below max_batch
  (1, 32, 256)   8 tiles: 8 | ntiles, the XCD-aware order runs
The grid of the launch is min(tiles, resident blocks), so at these sizes every block has ONE tile.  The steady state of the tile
loop -- a prefetched tile committed behind the previous tile's stores, the LDS tiles reused, the prefetch past the end -- needs a
grid below the tile count: DNNCA_NBLOCKS (read once per model) fixes the grid of the pixel-group launches.
  (3, 24, 256) on 4 blocks   18 tiles: 5, 5, 4, 4 tiles per block (odd and even counts, a tile count that is no multiple of the grid)
  (2, 32, 256) on 8 blocks   16 tiles, two per block, 8 | ntiles and 8 | grid: the XCD-aware order with a grid below the tile count
"""

import ctypes as C

import numpy as np
import pytest

import helpers as Hp
from oracle import unet_oracle as O
from test_parity_gpu import GRAD_TOL

pytestmark = pytest.mark.gpu

UNET = dict(n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')
KERNEL = 'pgbwd_tc_3x2_3'
ATOMIC_SPREAD = 4e-9        # bench.py: relative difference of the gradients between two runs of one step (float atomics)
CFG = dict(weight_mul=3.0)

_cache = {}


def _case(B, H, W):
    """inputs and the oracle's answer for a shape: computed once, shared, never written to"""
    if (B, H, W) not in _cache:
        spec = O.ModelSpec('unet', 1, **UNET)
        params = Hp.perturbed_params(spec, np.float64)
        rng = np.random.default_rng(17)
        x = rng.random((B, H, W, 1)).astype(np.float32)
        y = (rng.random((B, H, W)) < 0.05).astype(np.float32)
        loss, grads, _, _ = O.loss_and_grads(spec, params, x.astype(np.float64), y, CFG, training=True)
        p32 = {n: v.astype(np.float32) for n, v in params.items()}
        _, g32, _, _ = O.loss_and_grads(spec, p32, x, y, CFG, training=True)
        gref, g32 = O.flatten(spec, grads), O.flatten(spec, g32).astype(np.float64)
        floor = [10 * np.abs(g32[sl] - gref[sl]).max() for _, sl in Hp.tensor_slices(spec)]
        for a in (x, y, gref):
            a.setflags(write=False)
        _cache[(B, H, W)] = (spec, O.flatten(spec, params), x, y, float(loss), gref, floor)
    return _cache[(B, H, W)]


def _dgrads(m, B, H, W):
    """(skip gradient [B, H, W, 3], gradient of the transposed conv's input [B, H/2, W/2, 6]) as the step left them"""
    fn = m.lib.dnnca_debug_tcf_dgrads
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_float), C.c_size_t]
    dskip, dtc = np.empty((B, H, W, 3), np.float32), np.empty((B, H // 2, W // 2, 6), np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert fn(m.handle, B, fp(dskip), dskip.size, fp(dtc), dtc.size) == 0
    return dskip, dtc


def _step(gpu, B, H, W, max_batch, dgrads=False):
    """one train step (lr 0) through the library; returns (loss, gradients[, data gradients]); asserts that KERNEL was what ran"""
    spec, p0, x, y, _, _, _ = _case(B, H, W)
    m = gpu.DeviceModel('unet', 1, H, W, max_batch, **UNET)
    try:
        m.set_params(p0)
        m.profile_enable()
        out = m.train_step(x, y, 0.0, m.loss_cfg(**CFG))
        g = m.get_grads()
        if dgrads:
            g = (g,) + _dgrads(m, B, H, W)
        ran = {r[0]: r[1] for r in m.profile()}
        assert ran.get(KERNEL) == 1, sorted(ran)            # launched once -- not declined to the per-layer path
        assert not any(k.startswith('tconv') and k.endswith('_3') for k in ran), sorted(ran)
        return float(out.loss), g
    finally:
        m.close()


@pytest.mark.parametrize('B, H, W, max_batch, nblocks', [(1, 8, 128, 1, None), (1, 24, 256, 1, None), (3, 24, 256, 4, None),
                                                         (1, 32, 256, 1, None), (3, 24, 256, 4, 4), (2, 32, 256, 2, 8)])
def test_last_decoder_block_backward_against_oracle(gpu, monkeypatch, B, H, W, max_batch, nblocks):
    if nblocks:
        monkeypatch.setenv('DNNCA_NBLOCKS', str(nblocks))
    spec, _, _, _, loss_ref, gref, floor = _case(B, H, W)
    loss, g = _step(gpu, B, H, W, max_batch)
    assert abs(loss - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref))
    errs = Hp.per_tensor_err(spec, g, gref)
    print('per-tensor error', errs)
    Hp.assert_grads_per_tensor(spec, g, gref, GRAD_TOL, floor=floor)


def test_counted_wait_form_equals_the_form_before_it(gpu, monkeypatch):
    """DNNCA_PGBWD_OLD=1 selects the kernel without the counted waits.  The change re-schedules memory operations only: the two
    data gradients of the two forms are the same bits (no atomics in them); the weight gradients may differ by the order of the
    float atomics alone.  On 4 blocks for 18 tiles, so that both forms run their steady state."""
    B, H, W = 3, 24, 256
    spec = _case(B, H, W)[0]
    monkeypatch.setenv('DNNCA_NBLOCKS', '4')
    _, (g_new, dskip_new, dtc_new) = _step(gpu, B, H, W, 4, dgrads=True)
    monkeypatch.setenv('DNNCA_PGBWD_OLD', '1')
    _, (g_old, dskip_old, dtc_old) = _step(gpu, B, H, W, 4, dgrads=True)
    assert np.abs(dskip_old).max() > 0 and np.abs(dtc_old).max() > 0
    assert np.array_equal(dskip_new, dskip_old), 'skip gradient: %d elements differ' % (dskip_new != dskip_old).sum()
    assert np.array_equal(dtc_new, dtc_old), 'gradient of the transposed conv input: %d elements differ' % (dtc_new != dtc_old).sum()
    for n, sl in Hp.tensor_slices(spec):
        d, s = np.abs(g_new[sl].astype(np.float64) - g_old[sl]).max(), np.abs(g_old[sl]).max()
        print(n, 'relative difference %.3e' % (d / max(s, 1e-300)))
        assert d <= ATOMIC_SPREAD * s, (n, d / max(s, 1e-300))
