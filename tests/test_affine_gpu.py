"""random_affine on the device (dnnca_affine_f32, launch `aug_affine`) against tests/affine_oracle.py, the float64 statement of
the same resampling: exact cases bit for bit (identity, the eight D4 views, integer and half-pixel shifts, everything outside the
image), general rotations and zooms to 8 * 2^-24 * max|tap| (one rounding of each fraction, three per blend, two levels of blends).
Every batch carries a different matrix per image, so that a wrong image index shows."""

import ctypes as C
import os

import numpy as np
import pytest

import affine_oracle as O

IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


@pytest.fixture(scope='module')
def model(gpu):
    m = gpu.DeviceModel('unet', 3, 8, 8, 8, n_filters_first=2, n_downsample=1, rate=2, kernel_size=3, conv_stride=1, padding='same')
    yield m
    m.close()


def _planes(B, h, w, c, seed, grid=None):
    """x [B, h, w, c] in [0, 1), y [B, h, w]; grid: values on multiples of 1 / grid"""
    rng = np.random.default_rng(seed)
    if grid:
        return (rng.integers(0, grid + 1, (B, h, w, c)) / grid).astype(np.float32), (rng.integers(0, grid + 1, (B, h, w)) / grid).astype(np.float32)
    return rng.random((B, h, w, c)).astype(np.float32), rng.random((B, h, w)).astype(np.float32)


def _device(gpu, m, x, y, mats):
    xo, yo = m.affine(gpu.DeviceBuffer(x), gpu.DeviceBuffer(y), mats)
    m.sync()
    return xo.to_host(), yo.to_host()


def _held_to_oracle(x, y, mats, xo, yo, what):
    """per image and channel: |device - oracle| <= 8 * 2^-24 * max|tap|, with the largest tap the plane holds"""
    wx, wy = O.affine(x, y, mats)
    worst = 0.0
    for b in range(x.shape[0]):
        for got, want, src in [(xo[b][..., c], wx[b][..., c], x[b][..., c]) for c in range(x.shape[-1])] + [(yo[b], wy[b], y[b])]:
            err, bound = np.abs(got.astype(np.float64) - want).max(), O.BOUND * np.abs(src).max()
            worst = max(worst, err / bound)
            assert err <= bound, (what, b, err, bound)
    print('%s: worst error %.3f of the bound (%.3f * 2^-24 max|tap|)' % (what, worst, worst * 8))
    return wx, wy


@pytest.mark.gpu
def test_identity_is_bit_equal(gpu, model):
    x, y = _planes(2, 5, 7, 3, seed=1)
    xo, yo = _device(gpu, model, x, y, np.stack([IDENTITY, IDENTITY]))
    assert np.array_equal(xo.view(np.uint32), x.view(np.uint32)) and np.array_equal(yo.view(np.uint32), y.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize('h,w,views', [(6, 6, 8), (5, 5, 8), (5, 7, 4)])
def test_d4_views_equal_numpy(gpu, model, h, w, views):
    from dnncancerannotator_amd import augment
    x, y = _planes(views, h, w, 3, seed=2)
    mats = np.stack([O.matrix(h, w, g=augment.d4_matrix(k)) for k in range(views)])
    xo, yo = _device(gpu, model, x, y, mats)
    for k in range(views):
        assert np.array_equal(xo[k], O.d4_numpy(x[k:k + 1], k)[0]), k
        assert np.array_equal(yo[k], O.d4_numpy(y[k:k + 1], k)[0]), k


@pytest.mark.gpu
def test_integer_shifts_copy_and_zero_outside(gpu, model):
    shifts = [(3, -2), (-1, 4), (0, 0), (-5, 3)]
    h, w = 5, 7
    x, y = _planes(len(shifts), h, w, 3, seed=3)
    mats = np.stack([[[1.0, 0.0, dy], [0.0, 1.0, dx]] for dy, dx in shifts])
    xo, yo = _device(gpu, model, x, y, mats)
    for b, (dy, dx) in enumerate(shifts):
        wx, wy = np.zeros_like(x[b]), np.zeros_like(y[b])
        for i in range(h):
            for j in range(w):
                if 0 <= i + dy < h and 0 <= j + dx < w:
                    wx[i, j], wy[i, j] = x[b, i + dy, j + dx], y[b, i + dy, j + dx]
        assert np.array_equal(xo[b], wx) and np.array_equal(yo[b], wy), (dy, dx)
        assert (wx == 0).any() == ((dy, dx) != (0, 0))                  # exact zeros where the source is outside
    assert not xo[3].any() and not yo[3].any()                          # five rows up on 5 x 7 is outside everywhere


@pytest.mark.gpu
def test_half_pixel_shifts_give_exact_means(gpu, model):
    h, w = 5, 7
    x, y = _planes(3, h, w, 3, seed=4, grid=256)
    mats = np.array([[[1.0, 0.0, 0.5], [0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0], [0.0, 1.0, 0.5]], [[1.0, 0.0, -0.5], [0.0, 1.0, 0.0]]])
    xo, yo = _device(gpu, model, x, y, mats)

    def mean_with_next(a, axis, back):
        pad = [(0, 0)] * a.ndim
        pad[axis] = (1, 0) if back else (0, 1)
        p = np.pad(a.astype(np.float64), pad)                            # zero outside: the border row or column comes out as the half
        n = a.shape[axis]
        return (np.take(p, range(0, n), axis) + np.take(p, range(1, n + 1), axis)) / 2

    for b, (axis, back) in enumerate([(0, False), (1, False), (0, True)]):
        assert np.array_equal(xo[b].astype(np.float64), mean_with_next(x[b], axis, back)), b
        assert np.array_equal(yo[b].astype(np.float64), mean_with_next(y[b], axis, back)), b
    assert np.array_equal(xo[0][-1], x[0][-1] / 2) and np.array_equal(yo[2][0], y[2][0] / 2)


@pytest.mark.gpu
@pytest.mark.parametrize('c', [1, 3, 5])
def test_rotation_and_zoom_are_held_to_the_oracle(gpu, model, c):
    """3 x 33 x 47 (1551 pixels: partial tiles on both edges): 30 degrees at z = 0.8 (the zero border shows), -75 degrees at z = 1.25
    with a shift, 180 degrees; channel 0 in [-0.3, 1.4] as random_contrast can leave it, the label binary"""
    h, w = 33, 47
    x, y = _planes(3, h, w, c, seed=5 + c)
    x[..., 0] = x[..., 0] * 1.7 - 0.3
    y = (y > 0.5).astype(np.float32)
    mats = np.stack([O.matrix(h, w, 30.0, 0.8), O.matrix(h, w, -75.0, 1.25, (2.5, -3.25)), O.matrix(h, w, 180.0)])
    xo, yo = _device(gpu, model, x, y, mats)
    wx, wy = _held_to_oracle(x, y, mats, xo, yo, 'rotations, C = %d' % c)
    assert not xo[0][0, 0].any() and yo[0][0, 0] == 0 and not wx[0][0, 0].any()      # the corner of the zoomed-out image is outside
    assert xo[0][h // 2, w // 2].any() and np.abs(xo - x).max() > 0.1 and len(np.unique(yo)) > 2
    assert np.abs(xo[2] - x[2][::-1, ::-1]).max() <= 1e-5                             # 180 degrees: sin(pi) is 1.2e-16, not 0


@pytest.mark.gpu
def test_degenerate_planes_and_far_positions(gpu, model):
    for h, w in ((1, 1), (1, 9), (9, 1)):
        x, y = _planes(4, h, w, 3, seed=6, grid=256)
        mats = np.stack([IDENTITY, O.matrix(h, w, g=[[-1, 0], [0, -1]]), [[1.0, 0.0, 0.5], [0.0, 1.0, -0.5]], O.matrix(h, w, 40.0, 0.7)])
        xo, yo = _device(gpu, model, x, y, mats)
        _held_to_oracle(x, y, mats, xo, yo, '%d x %d' % (h, w))
        assert np.array_equal(xo[0], x[0]) and np.array_equal(yo[0], y[0])
        assert np.array_equal(xo[1], x[1][::-1, ::-1]) and np.array_equal(yo[1], y[1][::-1, ::-1])
        assert xo[2].any()
    x, y = _planes(5, 5, 7, 3, seed=7)
    x += 1.0
    y += 1.0
    far = np.stack([[[1.0, 0.0, 1000.0], [0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0], [0.0, 1.0, -1000.0]], [[1.0, 0.0, 1e12], [0.0, 1.0, -1e12]],
                    [[1.0, 0.0, -1e12], [0.0, 1.0, 1e12]], [[1e308, 1e308, 1e308], [0.0, 1.0, 0.0]]])     # the last one overflows to inf from row 1 on
    xo, yo = _device(gpu, model, x, y, far)
    assert not xo.any() and not yo.any()
    xo, yo = _device(gpu, model, x, y, np.stack([IDENTITY] * 5))        # and the run goes on clean
    assert np.array_equal(xo, x) and np.array_equal(yo, y)


@pytest.mark.gpu
def test_workload_shape_with_drawn_matrices(gpu, model):
    """8 x 512 x 512 x 3 with affine_augment.yaml's ranges plus d4"""
    from dnncancerannotator_amd import augment
    opt = augment.parse_augment_options({'random_affine': dict(rotate_deg=15, scale=[0.9, 1.1], shift=8, symmetry='d4')}, (512, 512)).affine
    mats = augment.draw_affine(np.random.default_rng(8), 8, opt, (512, 512))
    assert len({m.tobytes() for m in mats}) == 8
    x, y = _planes(8, 512, 512, 3, seed=9)
    y = (y > 0.5).astype(np.float32)
    xo, yo = _device(gpu, model, x, y, mats)
    _held_to_oracle(x, y, mats, xo, yo, '8 x 512 x 512 x 3')
    assert np.abs(xo - x).max() > 0.1


@pytest.mark.gpu
def test_six_calls_in_flight_and_a_batch_that_outgrows_the_ring(gpu):
    """max_batch 2, 8 x 8 x 2: six calls of batch 2 back to back, more than the pinned ring has rows, through ONE host array that is
    overwritten as soon as a call returns, then a seventh of batch 5 (its matrices outgrow the ring's rows), ONE sync, and all seven
    against the oracle of their own matrices"""
    m = gpu.DeviceModel('unet', 2, 8, 8, 2, n_filters_first=2, n_downsample=1, rate=2, kernel_size=3, conv_stride=1, padding='same')
    try:
        h, w, c = 8, 8, 2
        mats = [np.stack([O.matrix(h, w, 20.0 * i - 50.0 + 7.0 * b, 0.8 + 0.07 * i, (0.5 * i - 1.0, 0.25 * b - 0.5 * i))
                          for b in range(2 if i < 6 else 5)]) for i in range(7)]
        small, big = _planes(2, h, w, c, seed=20), _planes(5, h, w, c, seed=21)
        planes = [small] * 6 + [big]
        dev = {2: tuple(map(gpu.DeviceBuffer, small)), 5: tuple(map(gpu.DeviceBuffer, big))}
        outs = [(gpu.DeviceBuffer(np.zeros_like(x)), gpu.DeviceBuffer(np.zeros_like(y))) for x, y in planes]
        hosts = {2: np.zeros((2, 2, 3)), 5: np.zeros((5, 2, 3))}
        dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731
        m.sync()
        for mt, (xo, yo) in zip(mats, outs):
            (xd, yd), host = dev[len(mt)], hosts[len(mt)]
            host[...] = mt
            assert m.lib.dnnca_affine_f32(m.handle, xd.ptr, yd.ptr, len(mt), h, w, c, dptr(host), xo.ptr, yo.ptr) == 0
            host[...] = np.nan                                          # the caller's array is free when the call returns
        m.sync()
        for i, (mt, (x, y), (xo, yo)) in enumerate(zip(mats, planes, outs)):
            got = xo.to_host()
            _held_to_oracle(x, y, mt, got, yo.to_host(), 'call %d of seven' % i)
            assert np.abs(got - x).max() > 0.05
    finally:
        m.close()


@pytest.mark.gpu
def test_refusals_leave_the_outputs_and_the_profile_alone(gpu, model):
    B, h, w, c = 3, 5, 7, 3
    x, y = _planes(B, h, w, c, seed=10)
    xd, yd = gpu.DeviceBuffer(x), gpu.DeviceBuffer(y)
    guard_x, guard_y = np.full((B, h, w, c), 7.25, np.float32), np.full((B, h, w), -3.5, np.float32)
    xo, yo = gpu.DeviceBuffer(guard_x), gpu.DeviceBuffer(guard_y)
    good = np.stack([IDENTITY] * B)
    dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731

    def call(mats=good, batch=B, x_=xd, y_=yd, xo_=xo, yo_=yo, hh=h, ww=w, cc=c):
        mats = np.ascontiguousarray(mats, np.float64)
        rc = model.lib.dnnca_affine_f32(model.handle, x_.ptr if x_ else None, y_.ptr if y_ else None, batch, hh, ww, cc,
                                        dptr(mats) if mats.size else None, xo_.ptr if xo_ else None, yo_.ptr if yo_ else None)
        return rc, model.lib.dnnca_last_error().decode()

    def poisoned(value, b, r, k):
        m = good.copy()
        m[b, r, k] = value
        return m

    model.sync()
    model.profile_reset()
    model.profile_enable(1)
    try:
        refused = [call(mats=poisoned(np.nan, 2, 1, 2)), call(mats=poisoned(np.inf, 0, 0, 0)), call(mats=poisoned(-np.inf, 1, 1, 1)),
                   call(xo_=xd), call(yo_=yd), call(xo_=yd), call(batch=0), call(batch=-1), call(hh=0), call(ww=0), call(cc=0),
                   call(x_=None), call(y_=None), call(xo_=None), call(yo_=None), call(mats=np.zeros((0, 2, 3)))]
        for rc, msg in refused:
            assert rc == -1 and 'dnnca_affine_f32' in msg, (rc, msg)       # DNNCA_EINVAL
        model.sync()
        assert 'aug_affine' not in [row[0] for row in model.profile()]
        assert np.array_equal(xo.to_host(), guard_x) and np.array_equal(yo.to_host(), guard_y)
        assert np.array_equal(xd.to_host(), x) and np.array_equal(yd.to_host(), y)
        with pytest.raises(ValueError):
            model.affine(xd, yd, good[:2])                                  # a matrix short
        assert call()[0] == 0                                               # and the good call goes through
        model.sync()
        assert {row[0]: row[1] for row in model.profile()}.get('aug_affine') == 1
        assert np.array_equal(xo.to_host(), x) and np.array_equal(yo.to_host(), y)
    finally:
        model.profile_enable(0)
        model.profile_reset()


@pytest.mark.gpu
def test_engine_trains_with_the_d4_overlay(gpu, tmp_path, monkeypatch):
    """configs/additionals/d4_augment.yaml laid over the test's config: three train steps on a tiny exam file through the feeder and
    with DNNCA_NO_FEEDER=1 -- finite losses, bit-equal between the two, one aug_affine launch per step"""
    from dnncancerannotator_amd import engine, load, tfrecord
    from dnncancerannotator_amd.runs.train import make_dataset
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(11)
    n, s = 12, 48                              # 32 x 32 crops with up to 6 pixels of jitter on either side
    types = ['TRA', 'ADC', 'DWI', 'label']
    label = np.zeros((n, s, s), np.uint8)
    yy, xx = np.mgrid[:s, :s]
    for k in range(n):
        cy, cx = rng.integers(12, s - 12, 2)
        label[k][(yy - cy) ** 2 + (xx - cx) ** 2 < 36] = 255
    tra = (label * 0.6 + rng.integers(0, 90, label.shape)).astype(np.uint8)
    slices = np.stack([tra, rng.integers(0, 256, label.shape).astype(np.uint8), rng.integers(0, 256, label.shape).astype(np.uint8), label], -1)
    rec = str(tmp_path / 'exam.tfrecords')
    tfrecord.write_records(rec, [tfrecord.make_example(slices, 1, 1, 'p', 'cancer', types)])
    config = {'model': 'UNetAnnotator',
              'model_options': dict(n_filters_first=3, n_downsample=2, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same'),
              'deploy_options': {'optimizer': 'adam', 'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}},
                                 'enable_multigpu': False},
              'data_options': {'train': dict(batch_size=4, buffer_size=8, output_size=[32, 32], slice_types=types,
                                             augment_options={'random_crop': None, 'random_flip': None, 'random_contrast': None})}}
    config = load._apply_config(config, load._load_config_single(os.path.join(root, 'configs', 'additionals', 'd4_augment.yaml')))
    assert config['data_options']['train']['augment_options']['random_affine'] == {'symmetry': 'd4'}
    losses = []
    for feeder in (True, False):
        if feeder:
            monkeypatch.delenv('DNNCA_NO_FEEDER', raising=False)
        else:
            monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
        ds = make_dataset([rec], config['data_options']['train'], training=True)
        assert ds.plan.affine['symmetry'] == 'd4'
        m = engine.TFKerasModel(config)
        res = m.train(ds, max_steps=3, save_freq=1000, profile=True)
        loss = np.asarray(res.history['loss'], np.float32)
        assert len(loss) == 3 and np.isfinite(loss).all()
        launches = {row[0]: row[1] for row in m.device_model.profile()}
        assert launches.get('aug_affine') == 3 and launches.get('aug_apply') == 3, launches
        losses.append(loss)
    print('d4 overlay, feeder %s, no feeder %s' % (losses[0], losses[1]))
    assert np.array_equal(losses[0].view(np.uint32), losses[1].view(np.uint32))
