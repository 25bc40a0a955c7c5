"""random_intrachannelwarp on the device (dnnca_warp_groups_f32, launch `aug_warp_groups`) against the oracle's restatement of
tfa.image.sparse_image_warp, called once per channel group on the gathered channels of that group with that group's control
points -- what annotator/data.py:705-708 does.

Sampling positions are observed through ramp channels (a warped row / column ramp IS the position q - flow(q), clamps included):
they must agree with the oracle to 1e-2 pixel, smooth channels to 1e-3 -- the bounds of test_device_warp_matches_oracle.  A
float32 cast of the oracle's own float64 flow is off by at most 4e-6 pixel at these sizes and strengths, so the bounds leave the
reference three orders of room and still catch any wrong term.

Mutation check (scratch, not committed): every block reading group 0's coefficients (`warp_coeffs_to_lds(p, b, 0, sm)`) is meant to
fail test_groups_match_oracle, test_shipped_extreme_matches_oracle and test_independence_and_pairing; so far that has only been
rehearsed on the CPU, with the oracle standing in for the device (all three fail there).  No figures from a GPU run yet."""

import ctypes as C

import numpy as np
import pytest

from oracle import augment_oracle as A

GROUP_OF = [0, 1, 2, 3, 0]          # four feature channels + label: groups [[0, label], [1], [2], [3]]


def _model(gpu, B, S, c=4):
    return gpu.DeviceModel('unet', c, S, S, B, n_filters_first=3, n_downsample=1, rate=2, kernel_size=3, conv_stride=1, padding='same')


def _images(B, S, swap):
    """x [B, S, S, 4], y [B, S, S]: the pair carries the row ramp in channel 0 and the column ramp in the label, singletons 1 and 2
    one ramp each, channel 3 a smooth image; `swap` exchanges rows and columns everywhere."""
    yy, xx = np.mgrid[:S, :S].astype(np.float32)
    rows, cols = (xx / S, yy / S) if swap else (yy / S, xx / S)
    smooth = 0.5 + 0.25 * np.sin(yy / 7.0) * np.cos(xx / 5.0)
    x0 = np.stack([np.stack([rows, rows, cols, smooth], -1)] * B).astype(np.float32)
    y0 = np.stack([cols] * B).astype(np.float32)
    return x0, y0


def _device(gpu, m, x0, y0, group_of, src, dst):
    from dnncancerannotator_amd import augment
    ctrl, wv = augment.solve_intrawarp(src, dst)
    xw, yw = m.warp_groups(gpu.DeviceBuffer(x0), gpu.DeviceBuffer(y0), group_of, ctrl, wv)
    m.sync()
    return xw.to_host(), yw.to_host()


def _against_oracle(gpu, B, S, max_diff, stddev, seed):
    from dnncancerannotator_amd import augment
    rng = np.random.default_rng(seed)
    m = _model(gpu, B, S)
    src, dst = augment.draw_intrawarp(rng, B, S, 4, max_diff, stddev)
    worst = dict(position=0.0, smooth=0.0)
    for swap in (False, True):
        x0, y0 = _images(B, S, swap)
        xw, yw = _device(gpu, m, x0, y0, GROUP_OF, src, dst)
        for b in range(B):
            pair = A.warp_image(np.stack([x0[b][..., 0], y0[b]], -1), src[b, 0], dst[b, 0])        # group 0: channel 0 + label
            singles = [A.warp_image(x0[b][..., c:c + 1], src[b, c], dst[b, c])[..., 0] for c in (1, 2, 3)]
            position = max(np.abs(xw[b][..., 0] - pair[..., 0]).max(), np.abs(yw[b] - pair[..., 1]).max(),
                           np.abs(xw[b][..., 1] - singles[0]).max(), np.abs(xw[b][..., 2] - singles[1]).max()) * S
            smooth = np.abs(xw[b][..., 3] - singles[2]).max()
            moved = [np.abs(xw[b][..., c] - x0[b][..., c]).max() * S for c in (0, 1, 2)] + [np.abs(yw[b] - y0[b]).max() * S]
            print('S %d stddev %g swap %d image %d: position error %.3g px, smooth error %.3g, moved %s px'
                  % (S, stddev, swap, b, position, smooth, ['%.2f' % v for v in moved]))
            worst['position'], worst['smooth'] = max(worst['position'], position), max(worst['smooth'], smooth)
            assert position <= 1e-2                   # sampling positions, in pixels
            assert smooth <= 1e-3
            assert min(moved) > 1.0                   # and every group did move (by pixels)
    m.close()
    return worst


@pytest.mark.gpu
def test_groups_match_oracle(gpu):
    """B = 3, 48 x 48, groups [[0, label], [1], [2], [3]], 100 points, default strength (max_diff 5, stddev 2.0)"""
    _against_oracle(gpu, 3, 48, 5, 2.0, seed=21)


@pytest.mark.gpu
def test_shipped_extreme_matches_oracle(gpu):
    """intra_channelwarp_std20.yaml: stddev 20, max_diff 100 at 64 x 64 -- positions move by tens of pixels, leave the image, and the
    clamps of the bilinear sampling decide what comes out"""
    _against_oracle(gpu, 3, 64, 100, 20.0, seed=22)


@pytest.mark.gpu
def test_independence_and_pairing(gpu):
    from dnncancerannotator_amd import augment
    rng = np.random.default_rng(23)
    B, S = 3, 48
    m = _model(gpu, B, S)
    x0, y0 = _images(B, S, False)
    y0 = x0[..., 0].copy()                                   # the label holds the image of its paired channel 0
    src, dst = augment.draw_intrawarp(rng, B, S, 4, 5, 2.0)
    xw, yw = _device(gpu, m, x0, y0, GROUP_OF, src, dst)
    for b in range(B):
        assert np.array_equal(x0[b][..., 0], x0[b][..., 1])
        assert np.abs(xw[b][..., 0] - xw[b][..., 1]).max() * S > 1.0        # same image, two groups: more than a pixel apart somewhere
        assert np.array_equal(xw[b][..., 0], yw[b])                         # same image, one group: bit-identical
    # one group holding every channel is random_warp: dnnca_warp_f32 on the same control points (summation order may differ)
    x0, y0 = _images(B, S, False)
    one_src, one_dst = src[:, :1], dst[:, :1]
    xg, yg = _device(gpu, m, x0, y0, [0] * 5, one_src, one_dst)
    xr, yr = m.warp(gpu.DeviceBuffer(x0), gpu.DeviceBuffer(y0), *augment.solve_warp(one_src[:, 0], one_dst[:, 0]))
    xr, yr = xr.to_host(), yr.to_host()
    assert np.abs(xg[..., :3] - xr[..., :3]).max() * S <= 1e-2 and np.abs(yg - yr).max() * S <= 1e-2
    assert np.abs(xg[..., 3] - xr[..., 3]).max() <= 1e-3
    assert np.abs(xr[..., 0] - x0[..., 0]).max() * S > 1.0
    m.close()


@pytest.mark.gpu
def test_cabi_rejects_bad_arguments(gpu):
    """n_groups 0 or c + 2, a group_of entry out of range and out == in: DNNCA_EINVAL with a message, nothing is launched"""
    from dnncancerannotator_amd import _lib
    B, S, c, n = 2, 16, 4, 100
    m = _model(gpu, B, S, c)
    x = gpu.DeviceBuffer(np.zeros((B, S, S, c), np.float32))
    y = gpu.DeviceBuffer(np.zeros((B, S, S), np.float32))
    xo = gpu.DeviceBuffer(np.zeros((B, S, S, c), np.float32))
    yo = gpu.DeviceBuffer(np.zeros((B, S, S), np.float32))
    ctrl, wv = np.zeros((B, c + 2, n, 2)), np.zeros((B, c + 2, n + 3, 2))
    dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731

    def call(n_groups, group_of, xo_=xo, yo_=yo):
        g = np.asarray(group_of, np.int32)
        rc = m.lib.dnnca_warp_groups_f32(m.handle, x.ptr, y.ptr, B, S, S, c, n_groups, g.ctypes.data_as(C.POINTER(C.c_int)), n,
                                         dptr(ctrl), dptr(wv), xo_.ptr, yo_.ptr)
        return rc, m.lib.dnnca_last_error().decode()

    for rc, msg in (call(0, [0] * 5), call(c + 2, [0, 1, 2, 3, 4]), call(4, [0, 1, 2, 4, 0]), call(4, [0, -1, 2, 3, 0]),
                    call(4, GROUP_OF, xo_=x), call(4, GROUP_OF, yo_=y)):
        assert rc == -1 and 'dnnca_warp_groups_f32' in msg, (rc, msg)       # DNNCA_EINVAL
    with pytest.raises(ValueError):
        m.warp_groups(x, y, [0, 1, 2, 0], ctrl[:, :3], wv[:, :3])            # a group entry short
    assert call(4, GROUP_OF)[0] == _lib.OK and call(c + 1, [0, 1, 2, 3, 4])[0] == _lib.OK
    m.sync()
    m.close()


@pytest.mark.gpu
def test_engine_trains_with_intrachannelwarp(gpu, tmp_path):
    """`annotator train`'s dataset with data_options.yaml's four augmentations and the overlay's random_intrachannelwarp: 20 steps,
    every loss finite, one aug_warp and one aug_warp_groups launch per step."""
    from dnncancerannotator_amd import engine, tfrecord
    from dnncancerannotator_amd.runs.train import make_dataset
    rng = np.random.default_rng(24)
    n, s = 12, 80
    label = np.zeros((n, s, s), np.uint8)
    yy, xx = np.mgrid[:s, :s]
    for k in range(n):
        cy, cx = rng.integers(24, s - 24, 2)
        label[k][(yy - cy) ** 2 + (xx - cx) ** 2 < 100] = 255
    tra = (label * 0.6 + rng.integers(0, 90, label.shape)).astype(np.uint8)
    slices = np.stack([tra, rng.integers(0, 256, label.shape).astype(np.uint8), rng.integers(0, 256, label.shape).astype(np.uint8), label], -1)
    rec = str(tmp_path / 'exam.tfrecords')
    tfrecord.write_records(rec, [tfrecord.make_example(slices, 1, 1, 'p', 'cancer', ['TRA', 'ADC', 'DWI', 'label'])])
    opts = dict(batch_size=4, buffer_size=8, output_size=[64, 64], slice_types=['TRA', 'ADC', 'DWI', 'label'],
                augment_options={'random_crop': None, 'random_flip': None, 'random_contrast': None, 'random_warp': None,
                                 'random_intrachannelwarp': dict(n_points=50, max_diff=100, stddev=3.0)})
    ds = make_dataset([rec], opts, training=True)
    assert ds.element_spec[0].shape == (4, 64, 64, 3) and ds.plan.intrawarp['stddev'] == 3.0
    cfg = {'model': 'UNetAnnotator',
           'model_options': dict(n_filters_first=3, n_downsample=2, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same'),
           'deploy_options': {'optimizer': 'adam', 'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}},
                              'enable_multigpu': False}}
    m = engine.TFKerasModel(cfg)
    res = m.train(ds, max_steps=20, save_freq=1000, profile=True)
    loss = res.history['loss']
    assert len(loss) == 20 and np.isfinite(loss).all()
    launches = {row[0]: row[1] for row in m.device_model.profile()}
    assert launches.get('aug_warp_groups') == 20 and launches.get('aug_warp') == 20, launches
