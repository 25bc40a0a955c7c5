"""random_intensity on the device (dnnca_intensity_f32, launch `aug_intensity`) against tests/intensity_oracle.py, the float64
statement of the same five steps: planes with flags 0 bit for bit, every term alone and all together to O.BOUND units of
2^-24 (max(1, max|x|) + 6 sigma) -- four times what the float32 numpy restatement of the steps is away from the float64 statement on
the same cases (test_intensity_host.test_restatement_sets_the_device_bound), rounded up to a power of two.  Every batch carries a
different record per image and channel, so that a wrong index shows; a wrong Philox word, key, counter or tap is an error of the
order of sigma, thousands of units."""

import ctypes as C
import os

import numpy as np
import pytest

import intensity_oracle as O


@pytest.fixture(scope='module')
def model(gpu):
    m = gpu.DeviceModel('unet', 3, 8, 8, 8, n_filters_first=2, n_downsample=1, rate=2, kernel_size=3, conv_stride=1, padding='same')
    yield m
    m.close()


def _device(gpu, m, x, rec):
    xo = m.intensity(gpu.DeviceBuffer(x), rec)
    m.sync()
    return xo.to_host()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _held_to_oracle(x, rec, got, what):
    want = O.intensity(x, rec)
    worst = O.worst_units(got, want, x, rec)
    print('%s: worst error %.3f units (bound %g)' % (what, worst, O.BOUND))
    assert worst <= O.BOUND, (what, worst)
    return want, worst


def _odd_values(shape, seed):
    """values as no plane should hold them, to see that a copy is a copy: outside [0, 1], a NaN, an infinity, a negative zero"""
    x = (np.random.default_rng(seed).random(shape) * 3 - 1).astype(np.float32)
    flat = x.reshape(-1)
    flat[0] = np.nan
    if flat.size > 3:
        flat[1], flat[2], flat[3] = np.inf, -0.0, 7.5
    return x


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(2, 5, 7, 3), (1, 1, 1, 1)])
def test_all_zero_records_copy_bit_for_bit(gpu, model, shape):
    x = _odd_values(shape, seed=1)
    got = _device(gpu, model, x, np.zeros(shape[:1] + shape[3:] + (32,), np.uint32))
    assert np.array_equal(_bits(got), _bits(x)) and np.isnan(got.reshape(-1)[0])


@pytest.mark.gpu
def test_mixed_batch_leaves_passive_planes_alone(gpu, model):
    """image 0: channels 0 and 2 active (2 with a blur: the halo launch), channel 1 no target; image 1: nothing drawn"""
    shape = (2, 33, 47, 3)
    x = _odd_values(shape, seed=2)
    x[0, :, :, 0::2] = np.random.default_rng(3).random((33, 47, 2)).astype(np.float32)
    x[1, 2, 3] = [np.nan, -2.5, np.inf]
    rec = np.zeros((2, 3, 32), np.uint32)
    rec[0, 0] = O.record(gamma=0.8, noise=0.03, key=(5, 6))
    rec[0, 2] = O.record(bias=np.linspace(-0.03, 0.03, 9), blur=1.2, noise=0.02, rician=True, key=(7, 8))
    got = _device(gpu, model, x, rec)
    assert np.array_equal(_bits(got[1]), _bits(x[1])) and np.array_equal(_bits(got[0, :, :, 1]), _bits(x[0, :, :, 1]))
    _held_to_oracle(x[:1, :, :, 0::2], rec[:1, 0::2], got[:1, :, :, 0::2], 'active planes of the mixed batch')
    assert np.abs(got[0, :, :, 0::2] - x[0, :, :, 0::2]).max() > 0.05


@pytest.mark.gpu
@pytest.mark.parametrize('shape', O.SHAPES, ids=['x'.join(map(str, s)) for s in O.SHAPES])
def test_each_term_and_all_together_are_held_to_the_oracle(gpu, model, shape):
    worst = {}
    for which in O.TERMS:
        x, rec = O.case(shape, which)
        got = _device(gpu, model, x, rec)
        want, worst['+'.join(which)] = _held_to_oracle(x, rec, got, '%s %s' % (shape, '+'.join(which)))
        assert np.abs(got - x).max() > 1e-3 and got.min() >= 0.0 and got.max() <= 1.0
    print('%s: worst %.3f units' % (shape, max(worst.values())))


@pytest.mark.gpu
def test_workload_shape_with_records_drawn_from_the_overlay(gpu, model):
    x, rec = O.overlay_case()
    assert all(((rec[..., 0] & bit) != 0).sum() >= 3 for bit in (1, 2, 4, 8)) and (rec[..., 0] == 0).sum() >= 3
    got = _device(gpu, model, x, rec)
    _held_to_oracle(x, rec, got, '8 x 512 x 512 x 3, overlay draws')
    passive = rec[..., 0] == 0
    for b, c in zip(*np.nonzero(passive)):
        assert np.array_equal(_bits(got[b, :, :, c]), _bits(x[b, :, :, c])), (b, c)


@pytest.mark.gpu
def test_bias_field_stays_inside_its_strength(gpu, model):
    from dnncancerannotator_amd import augment
    s, v = 0.3, np.float32(0.5)
    opt = augment.parse_augment_options({'random_intensity': {'bias_field': {'strength': s}}}, (33, 47)).intensity
    rec = augment.draw_intensity(np.random.default_rng(4), 4, opt, 3)
    assert (rec[..., 0] == 2).all()
    x = np.full((4, 33, 47, 3), v, np.float32)
    got = _device(gpu, model, x, rec).astype(np.float64)
    slack = O.BOUND * 2.0 ** -24
    assert got.min() >= v * np.exp(-s) - slack and got.max() <= v * np.exp(s) + slack
    assert got.max() - got.min() > 0.05                                       # and the field is there
    _held_to_oracle(x, rec, got, 'drawn bias fields on a constant plane')


@pytest.mark.gpu
def test_noise_statistics(gpu, model):
    x, rec = O.noise_case()
    got = _device(gpu, model, x, rec)
    O.check_noise_statistics(x, got)
    _held_to_oracle(x, rec, got, 'gaussian noise on 256 x 256 x 2')
    x, rec = O.rician_case()
    got = _device(gpu, model, x, rec)
    O.check_rician_mean(got)
    _held_to_oracle(x, rec, got, 'rician noise on a zero plane')


@pytest.mark.gpu
def test_planes_without_blur_are_the_same_bits_in_both_launches(gpu, model):
    """the halo-less instantiation runs when no record of the batch blurs, the halo one as soon as one does"""
    h, w = 33, 47
    x, rec = O.case((3, h, w, 3), ('gamma', 'bias', 'rician'), seed=5)
    alone = _device(gpu, model, x[:2], rec[:2])
    beside = rec.copy()
    beside[2, 0] = O.record(gamma=1.3, blur=2.0, noise=0.02, key=(1, 2))      # image 2: channel 0 blurs, channels 1 and 2 do not
    together = _device(gpu, model, x, beside)
    assert np.array_equal(_bits(together[:2]), _bits(alone))
    pointwise = beside[2:].copy()
    pointwise[0, 0] = 0
    last = _device(gpu, model, x[2:], pointwise)
    assert np.array_equal(_bits(together[2, :, :, 1:]), _bits(last[0, :, :, 1:]))
    _held_to_oracle(x, beside, together, 'batch with one blurred plane')
    assert np.abs(together[2, :, :, 0] - last[0, :, :, 0]).max() > 0.05


@pytest.mark.gpu
def test_calls_repeat_and_six_in_flight_keep_their_own_records(gpu, model):
    """the same call twice gives the same bits; six calls back to back, more than the pinned ring has rows, through ONE host array
    that is overwritten as soon as a call returns, each match the oracle of their own records"""
    shape = (2, 33, 47, 3)
    x, rec = O.case(shape, ('gamma', 'bias', 'blur', 'noise'), seed=6)
    first = _device(gpu, model, x, rec)
    assert np.array_equal(_bits(_device(gpu, model, x, rec)), _bits(first))
    recs = [O.case(shape, which, seed=7 + i)[1] for i, which in enumerate(O.TERMS[:6])]
    xd = gpu.DeviceBuffer(x)
    outs = [gpu.DeviceBuffer(np.zeros(shape, np.float32)) for _ in recs]
    host = np.zeros_like(recs[0])
    model.sync()
    for r, out in zip(recs, outs):
        host[...] = r
        assert model.lib.dnnca_intensity_f32(model.handle, xd.ptr, *shape, host.ctypes.data_as(C.POINTER(C.c_uint32)), out.ptr) == 0
    host[...] = 0
    model.sync()
    for i, (r, out) in enumerate(zip(recs, outs)):
        _held_to_oracle(x, r, out.to_host(), 'call %d of six' % i)


@pytest.mark.gpu
def test_six_calls_in_flight_and_a_batch_that_outgrows_the_ring(gpu):
    """max_batch 2, 8 x 8 x 2: six calls of batch 2 back to back through ONE host array that is overwritten as soon as a call
    returns, then a seventh of batch 5 (its records outgrow the ring's rows), ONE sync, and all seven against the oracle of their
    own records"""
    m = gpu.DeviceModel('unet', 2, 8, 8, 2, n_filters_first=2, n_downsample=1, rate=2, kernel_size=3, conv_stride=1, padding='same')
    try:
        cases = [O.case((2 if i < 6 else 5, 8, 8, 2), which, seed=20 + i) for i, which in enumerate(O.TERMS)]
        assert len(cases) == 7
        ins = [gpu.DeviceBuffer(x) for x, _ in cases]
        outs = [gpu.DeviceBuffer(np.zeros_like(x)) for x, _ in cases]
        hosts = {2: np.zeros((2, 2, 32), np.uint32), 5: np.zeros((5, 2, 32), np.uint32)}
        m.sync()
        for (x, rec), xd, out in zip(cases, ins, outs):
            host = hosts[len(rec)]
            host[...] = rec
            assert m.lib.dnnca_intensity_f32(m.handle, xd.ptr, *x.shape, host.ctypes.data_as(C.POINTER(C.c_uint32)), out.ptr) == 0
            host[...] = 0                                               # the caller's array is free when the call returns
        m.sync()
        for i, ((x, rec), out) in enumerate(zip(cases, outs)):
            got = out.to_host()
            _held_to_oracle(x, rec, got, 'call %d of seven' % i)
            assert np.abs(got - x).max() > 1e-3
    finally:
        m.close()


@pytest.mark.gpu
def test_refusals_leave_the_output_and_the_profile_alone(gpu, model):
    B, h, w, c = 2, 5, 7, 3
    x = np.random.default_rng(10).random((B, h, w, c)).astype(np.float32)
    xd = gpu.DeviceBuffer(x)
    guard = np.full((B, h, w, c), 7.25, np.float32)
    xo = gpu.DeviceBuffer(guard)
    good = np.stack([np.stack([O.record(gamma=1.2, bias=np.full(9, 0.01), blur=1.0, noise=0.02, rician=True, key=(3, 4))] * c)] * B)

    def call(rec=good, batch=B, x_=xd, xo_=xo, hh=h, ww=w, cc=c):
        rec = None if rec is None else np.ascontiguousarray(rec, np.uint32)
        rc = model.lib.dnnca_intensity_f32(model.handle, x_.ptr if x_ else None, batch, hh, ww, cc,
                                           rec.ctypes.data_as(C.POINTER(C.c_uint32)) if rec is not None else None, xo_.ptr if xo_ else None)
        return rc, model.lib.dnnca_last_error().decode()

    def word(k, value, b=1, ch=2, dtype=np.uint32):
        r = good.copy()
        r[b, ch, k] = np.array([value], dtype).view(np.uint32)[0]
        return r

    f32 = np.float32
    taps_off = good.copy()
    taps_off[0, 1, 12] = np.array([good[0, 1, 12:13].view(np.float32)[0] + 1e-4], np.float32).view(np.uint32)[0]
    model.sync()
    model.profile_reset()
    model.profile_enable(1)
    try:
        refused = {
            'null x': call(x_=None), 'null records': call(rec=None), 'null output': call(xo_=None),
            'batch 0': call(batch=0), 'batch -1': call(batch=-1), 'batch 65536': call(batch=65536),
            'h 0': call(hh=0), 'w 0': call(ww=0), 'c 0': call(cc=0), 'h -3': call(hh=-3),
            'output is the input': call(xo_=xd),
            'flag bit 5': word(0, 32 | 1), 'flag bit 31': word(0, 1 << 31),
            'gamma nan': word(1, np.nan, dtype=f32), 'bias inf': word(5, np.inf, dtype=f32), 'tap nan': word(14, np.nan, dtype=f32),
            'sigma -inf': word(21, -np.inf, dtype=f32), 'tap beyond R inf': word(20, np.inf, dtype=f32),
            'gamma 0': word(1, 0.0, dtype=f32), 'gamma -1.2': word(1, -1.2, dtype=f32),
            'R 9': word(11, 9), 'R 2^31': word(11, 1 << 31),
            'tap -0.01': word(13, -0.01, dtype=f32), 'tap beyond R -1': word(20, -1.0, dtype=f32),
            'taps sum to 1.0001': taps_off,
            'sigma -0.02': word(21, -0.02, dtype=f32),
            'reserved word 24': word(24, 1), 'reserved word 31': word(31, 0x3F800000), 'first record': word(27, 5, b=0, ch=0),
        }
        for name, r in refused.items():
            rc, msg = r if isinstance(r, tuple) else call(rec=r)
            assert rc == -1 and 'dnnca_intensity_f32' in msg, (name, rc, msg)       # DNNCA_EINVAL
        model.sync()
        assert 'aug_intensity' not in [row[0] for row in model.profile()]
        assert np.array_equal(xo.to_host(), guard) and np.array_equal(xd.to_host(), x)
        with pytest.raises(ValueError):
            model.intensity(xd, good[:1])                                   # an image short
        with pytest.raises(ValueError):
            model.intensity(xd, good[:, :2])                                # a channel short
        assert call()[0] == 0                                               # and the good call goes through
        model.sync()
        assert {row[0]: row[1] for row in model.profile()}.get('aug_intensity') == 1
        _held_to_oracle(x, good, xo.to_host(), 'the call after the refusals')
    finally:
        model.profile_enable(0)
        model.profile_reset()


@pytest.mark.gpu
def test_engine_trains_with_the_intensity_overlay(gpu, tmp_path, monkeypatch):
    """configs/additionals/intensity_augment.yaml laid over the test's config: three train steps on a tiny exam file through the
    feeder and with DNNCA_NO_FEEDER=1 -- finite losses, bit-equal between the two, one aug_intensity launch per step; without the key
    and with `random_intensity: null` no such launch and one and the same losses"""
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

    def config(**extra):
        return {'model': 'UNetAnnotator',
                'model_options': dict(n_filters_first=3, n_downsample=2, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same'),
                'deploy_options': {'optimizer': 'adam', 'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}},
                                   'enable_multigpu': False},
                'data_options': {'train': dict(batch_size=4, buffer_size=8, output_size=[32, 32], slice_types=types,
                                               augment_options=dict({'random_crop': None, 'random_flip': None, 'random_contrast': None}, **extra))}}

    def run(cfg, feeder):
        if feeder:
            monkeypatch.delenv('DNNCA_NO_FEEDER', raising=False)
        else:
            monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
        ds = make_dataset([rec], cfg['data_options']['train'], training=True)
        m = engine.TFKerasModel(cfg)
        res = m.train(ds, max_steps=3, save_freq=1000, profile=True)
        loss = np.asarray(res.history['loss'], np.float32)
        assert len(loss) == 3 and np.isfinite(loss).all()
        return loss, {row[0]: row[1] for row in m.device_model.profile()}, ds

    overlay = load._apply_config(config(), load._load_config_single(os.path.join(root, 'configs', 'additionals', 'intensity_augment.yaml')))
    assert overlay['data_options']['train']['augment_options']['random_intensity']['bias_field'] == {'strength': 0.3, 'prob': 0.3}
    losses = []
    for feeder in (True, False):
        loss, launches, ds = run(overlay, feeder)
        assert ds.plan.intensity['noise']['distribution'] == 'rician'
        assert launches.get('aug_intensity') == 3 and launches.get('aug_apply') == 3, launches
        losses.append(loss)
    print('intensity overlay, feeder %s, no feeder %s' % (losses[0], losses[1]))
    assert np.array_equal(_bits(losses[0]), _bits(losses[1]))
    plain = []
    for cfg in (config(), config(random_intensity=None)):
        loss, launches, ds = run(cfg, True)
        assert 'aug_intensity' not in launches and launches.get('aug_apply') == 3, launches
        plain.append(loss)
    print('without the key %s, with null %s' % (plain[0], plain[1]))
    assert np.array_equal(_bits(plain[0]), _bits(plain[1])) and not np.array_equal(_bits(plain[0]), _bits(losses[0]))
