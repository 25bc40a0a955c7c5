"""The five augmentation entry points of csrc/kernels_aug.hip share one upload mechanism (HostRowRing, csrc/model.h), a ring per
entry point.  tests/test_augment_edges_gpu.py, test_affine_gpu.py and test_intensity_gpu.py put four of the rings under more calls
than they have rows and under a row that outgrows them; here the fifth, dnnca_warp_f32's, which also has to return with its outputs
complete, and the five together on one model in the order of the train loop.

Bounds are those of the files named above and nothing else: crop / flip / contrast E.X_BOUND (label exact), affine affine_oracle.BOUND
times the largest tap, intensity intensity_oracle.BOUND units, warps E.POSITION_BOUND pixels of sampling position and E.SMOOTH_BOUND
on the smooth channel.  In the chain a warp's input is no ramp, so the position bound is applied as what it says about any plane:
the bilinear interpolant moves by at most (largest difference of vertical neighbours) per pixel of row error plus (largest difference
of horizontal neighbours) per pixel of column error, so |device - oracle| <= POSITION_BOUND * (the two differences added) -- on the
row ramp yy / H that is the ramp check itself, err * H <= POSITION_BOUND."""

import ctypes as C

import numpy as np
import pytest

import affine_oracle
import augment_edges as E
import intensity_oracle
from oracle import augment_oracle as A

pytestmark = pytest.mark.gpu
F32 = np.float32
B, H, W, CH = 2, 8, 8, 2
dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731


@pytest.fixture
def model(gpu):
    m = gpu.DeviceModel('unet', CH, H, W, B, n_filters_first=2, n_downsample=1, rate=2, kernel_size=3, conv_stride=1, padding='same')
    yield m
    m.close()


def _spline(rng, shape, n, i):
    """ctrl shape + (n, 2), wv shape + (n + 3, 2): small weights and a shift of a pixel or two that differs from call to call"""
    ctrl = rng.uniform(0, 1, shape + (n, 2)) * [H, W]
    wv = np.zeros(shape + (n + 3, 2))
    wv[..., :n, :] = rng.normal(0.0, 2e-4, shape + (n, 2))
    wv[..., n + 2, :] = rng.choice([-1.0, 1.0], shape + (2,)) * (1.25 + 0.25 * (i % 4))
    return ctrl, wv


def test_warp_returns_complete_through_the_ring_and_a_regrow(gpu, model):
    """dnnca_warp_f32 at 2 x 8 x 8 x 2 with 3 control points: six calls through ONE pair of host arrays, overwritten after every
    call, then one with 9 control points (its row outgrows the ring's); every output is read straight after its call, with no sync"""
    kinds = ('row', 'col', 'smooth')
    x0, y0 = E.ramp_images(B, H, W, kinds)
    full = np.concatenate([x0, y0[..., None]], -1)
    xd, yd = gpu.DeviceBuffer(x0), gpu.DeviceBuffer(y0)
    rng = np.random.default_rng(31)
    hosts = {3: (np.zeros((B, 3, 2)), np.zeros((B, 6, 2))), 9: (np.zeros((B, 9, 2)), np.zeros((B, 12, 2)))}
    worst = 0.0
    for i in range(7):
        n = 3 if i < 6 else 9
        ctrl, wv = _spline(rng, (B,), n, i)
        hc, hw = hosts[n]
        hc[...], hw[...] = ctrl, wv
        xw, yw = model.warp(xd, yd, hc, hw)
        out = np.concatenate([xw.to_host(), yw.to_host()[..., None]], -1)      # no sync: the call returned complete
        hc[...], hw[...] = np.nan, np.nan
        for b in range(B):
            ref = A.warp_image_coeffs(full[b], ctrl[b], wv[b])
            for c, kind in enumerate(kinds):
                err = float(np.abs(out[b, ..., c] - ref[..., c]).max())
                if kind == 'smooth':
                    assert err <= E.SMOOTH_BOUND, 'call %d image %d: smooth error %.3g' % (i, b, err)
                else:
                    err *= H if kind == 'row' else W
                    worst = max(worst, err)
                    assert err <= E.POSITION_BOUND, 'call %d image %d channel %d: position error %.3g px' % (i, b, c, err)
                    assert np.abs(out[b, ..., c] - full[b, ..., c]).max() * (H if kind == 'row' else W) > 1.0, (i, b, c)
    print('warp through its ring: worst position error %.3g px over 7 calls' % worst)


def _warp_bound(plane):
    """POSITION_BOUND on a plane [h, w] that is no ramp (module docstring)"""
    plane = plane.astype(np.float64)
    return E.POSITION_BOUND * (np.abs(np.diff(plane, axis=0)).max() + np.abs(np.diff(plane, axis=1)).max())


def _held_to_warp(got, src, table, ctrl, wv, what):
    """got, src [B, h, w, C + 1] (label last); table: the group of every channel; ctrl, wv [B, G, ...]"""
    worst = 0.0
    for b in range(len(got)):
        for g in range(ctrl.shape[1]):
            chans = [c for c in range(got.shape[-1]) if table[c] == g]
            ref = A.warp_image_coeffs(src[b][..., chans], ctrl[b, g], wv[b, g])
            for k, c in enumerate(chans):
                err, bound = float(np.abs(got[b, ..., c] - ref[..., k]).max()), _warp_bound(src[b, ..., c])
                assert bound > 0 and err <= bound, (what, b, c, err, bound)
                worst = max(worst, err / bound)
    return worst


def test_five_entry_points_in_chain_order_keep_their_own_rows(gpu, model):
    """six rounds of augment_u8 -> affine -> warp -> warp_groups -> intensity on one model, every call with draws, host arrays
    (overwritten on return) and output buffers of its own, one sync at the end; then every stage of every round against its
    oracle on the input the device gave it -- the composition, stage by stage, each at its file's bound"""
    m, lib = model, model.lib
    rng = np.random.default_rng(41)
    hs, ws, cs, label, n = H + 2, W + 2, CH + 1, CH, 3
    table = np.array([0, 1, 0], np.int32)                # channel 0 + label | channel 1
    zeros = lambda *shape: gpu.DeviceBuffer(np.zeros(shape, F32))        # noqa: E731
    rounds = []
    for i in range(6):
        raw = rng.integers(0, 256, (B, hs, ws, cs), dtype=np.uint8)
        params = [(int(rng.integers(-1, 2)), int(rng.integers(-1, 2)), (i + b) % 2, float(F32(0.8 + 0.05 * i + 0.02 * b))) for b in range(B)]
        mats = np.stack([affine_oracle.matrix(H, W, 12.0 * i - 30.0 + 5.0 * b, 0.9 + 0.04 * i, (0.3 * i - 0.7, 0.2 * b)) for b in range(B)])
        rec = intensity_oracle.random_records(rng, B, CH, intensity_oracle.TERMS[i])
        src = gpu.RawDeviceBuffer()
        src.upload(raw)
        rounds.append(dict(raw=raw, params=params, mats=mats, warp=_spline(rng, (B,), n, i), groups=_spline(rng, (B, 2), n, i + 1), rec=rec,
                           src=src, x=[zeros(B, H, W, CH) for _ in range(5)], y=[zeros(B, H, W) for _ in range(4)]))
    m.sync()
    for r in rounds:
        x, y = r['x'], r['y']
        prm = (gpu._lib.AugParam * B)(*[gpu._lib.AugParam(*p) for p in r['params']])
        assert lib.dnnca_augment_u8(m.handle, r['src'].ptr, B, hs, ws, cs, label, 0b011, prm, H, W, x[0].ptr, y[0].ptr) == 0
        C.memset(prm, 0xff, C.sizeof(prm))               # every caller's buffer is free when its call returns
        mats = r['mats'].copy()
        assert lib.dnnca_affine_f32(m.handle, x[0].ptr, y[0].ptr, B, H, W, CH, dptr(mats), x[1].ptr, y[1].ptr) == 0
        mats.fill(np.nan)
        ctrl, wv = (a.copy() for a in r['warp'])
        assert lib.dnnca_warp_f32(m.handle, x[1].ptr, y[1].ptr, B, H, W, CH, n, dptr(ctrl), dptr(wv), x[2].ptr, y[2].ptr) == 0
        ctrl.fill(np.nan), wv.fill(np.nan)
        ctrl, wv, tab = (a.copy() for a in r['groups'] + (table,))
        assert lib.dnnca_warp_groups_f32(m.handle, x[2].ptr, y[2].ptr, B, H, W, CH, 2, tab.ctypes.data_as(C.POINTER(C.c_int)), n,
                                         dptr(ctrl), dptr(wv), x[3].ptr, y[3].ptr) == 0
        ctrl.fill(np.nan), wv.fill(np.nan), tab.fill(7)
        rec = r['rec'].copy()
        assert lib.dnnca_intensity_f32(m.handle, x[3].ptr, B, H, W, CH, rec.ctypes.data_as(C.POINTER(C.c_uint32)), x[4].ptr) == 0
        rec.fill(0)
    m.sync()
    for i, r in enumerate(rounds):
        x, y = [b.to_host() for b in r['x']], [b.to_host() for b in r['y']]
        xr, yr = A.augment_batch(r['raw'], r['params'], (H, W), label)
        assert np.array_equal(y[0], yr) and np.abs(x[0] - xr).max() <= E.X_BOUND, i
        wx, wy = affine_oracle.affine(x[0], y[0], r['mats'])
        for b in range(B):
            for got, want, src in [(x[1][b, ..., c], wx[b, ..., c], x[0][b, ..., c]) for c in range(CH)] + [(y[1][b], wy[b], y[0][b])]:
                assert np.abs(got - want).max() <= affine_oracle.BOUND * np.abs(src).max(), (i, b)
        full = [np.concatenate([xs, ys[..., None]], -1) for xs, ys in zip(x[1:4], y[1:4])]
        ctrl, wv = r['warp']
        worst = _held_to_warp(full[1], full[0], [0] * cs, ctrl[:, None], wv[:, None], 'round %d, warp' % i)
        worst = max(worst, _held_to_warp(full[2], full[1], table, *r['groups'], 'round %d, warp_groups' % i))
        units = intensity_oracle.worst_units(x[4], intensity_oracle.intensity(x[3], r['rec']), x[3], r['rec'])
        assert units <= intensity_oracle.BOUND, (i, units)
        assert all(np.abs(a - b).max() > 1e-3 for a, b in zip(x[:4], x[1:])), 'round %d: a stage left its input as it was' % i
        print('round %d: warps at %.3g of their bound, intensity %.3f units' % (i, worst, units))
