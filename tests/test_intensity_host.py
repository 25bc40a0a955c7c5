"""random_intensity, host side (no GPU): option parsing, the records of augment.draw_intensity and the order of their draws, their
place beside every other draw of the dataset (a stream of their own), the split over ranks, the tuples that carry them, the
engine's call of DeviceModel.intensity last in the chain in both of its RawBatch branches -- and the oracle itself: its Philox
against the published known answers, its noise against the statistics the device is held to, and the distance of its float32
restatement from the float64 statement, which sets the device's tolerance.  The device is held to it in test_intensity_gpu.py."""

import os

import numpy as np
import pytest

import affine_oracle
import intensity_oracle as O
from oracle import augment_oracle as A

BASE = {'random_crop': None, 'random_flip': None, 'random_contrast': None, 'random_warp': None}
TYPES = ['TRA', 'ADC', 'DWI', 'label']
OFF = dict(gamma=None, bias_field=None, blur=None, noise=None, target_channels=None)
OVERLAY = dict(gamma=dict(range=(0.7, 1.5), prob=0.3), bias_field=dict(strength=0.3, prob=0.3), blur=dict(sigma=(0.5, 1.5), prob=0.2),
               noise=dict(sigma=(0.0, 0.05), prob=0.15, distribution='rician'), target_channels=None)


def _parse(conf):
    from dnncancerannotator_amd import augment
    return augment.parse_augment_options({'random_intensity': conf}, (8, 8)).intensity


# ------------------------------------------------------------------------------------------------------------------ options
def test_parse_defaults_and_absence():
    from dnncancerannotator_amd import augment
    assert 'random_intensity' in augment._KNOWN
    plan = augment.parse_augment_options({'random_intensity': None}, (64, 64))
    assert plan.intensity == OFF and not augment.intensity_is_on(plan)
    assert augment.parse_augment_options(BASE, (64, 64)).intensity is None
    assert not augment.intensity_is_on(augment.parse_augment_options(BASE, (64, 64))) and not augment.intensity_is_on(None)
    # a term that is there with its defaults, with prob 0 or with the identity as its only value is off
    for conf in (dict(gamma={}), dict(gamma=None), dict(bias_field={}), dict(blur={}), dict(blur={'prob': 0.5}), dict(noise={}),
                 dict(gamma={'range': [0.7, 1.5], 'prob': 0}), dict(bias_field={'strength': 0.3, 'prob': 0.0}),
                 dict(blur={'sigma': 1.0, 'prob': 0}), dict(noise={'sigma': [0, 0.05], 'prob': 0}),
                 dict(gamma={'range': [1, 1]}), dict(bias_field={'strength': 0}), dict(noise={'sigma': [0, 0]}), dict(noise={'sigma': 0})):
        assert _parse(conf) == OFF, conf
    # prob defaults to 1, a range may be one number, the distribution defaults to rician
    assert _parse(dict(gamma={'range': [0.7, 1.5]}))['gamma'] == dict(range=(0.7, 1.5), prob=1.0)
    assert _parse(dict(gamma={'range': 1.2, 'prob': 0.5}))['gamma'] == dict(range=(1.2, 1.2), prob=0.5)
    assert _parse(dict(blur={'sigma': 1}))['blur'] == dict(sigma=(1.0, 1.0), prob=1.0)
    assert _parse(dict(noise={'sigma': 0.02}))['noise'] == dict(sigma=(0.02, 0.02), prob=1.0, distribution='rician')
    assert _parse(dict(noise={'sigma': [0, 0.1], 'distribution': 'gaussian'}))['noise']['distribution'] == 'gaussian'
    plan = augment.parse_augment_options({'random_intensity': dict(bias_field={'strength': 0.3})}, (64, 64))
    assert augment.intensity_is_on(plan) and plan.intensity['gamma'] is None


def test_limits_of_the_ranges_are_accepted():
    got = _parse(dict(gamma={'range': [1e-3, 1e-3], 'prob': 1}, bias_field={'strength': 5, 'prob': 1.0},
                      blur={'sigma': [1e-3, 8 / 3], 'prob': 1}, noise={'sigma': [0, 1], 'prob': 1e-9}, target_channels=[0]))
    assert got == dict(gamma=dict(range=(1e-3, 1e-3), prob=1.0), bias_field=dict(strength=5.0, prob=1.0), blur=dict(sigma=(1e-3, 8 / 3), prob=1.0),
                       noise=dict(sigma=(0.0, 1.0), prob=1e-9, distribution='rician'), target_channels=(0,))


NAN, INF = float('nan'), float('inf')


@pytest.mark.parametrize('conf', [
    dict(gamma={'range': [0, 1]}), dict(gamma={'range': [-1, 1]}), dict(gamma={'range': [1.5, 0.7]}), dict(gamma={'range': [0.7, INF]}),
    dict(gamma={'range': [NAN, 1]}), dict(gamma={'range': '1'}), dict(gamma={'range': [1, 1, 1]}), dict(gamma={'range': True}),
    dict(gamma={'range': None}), dict(gamma={'range': [0.7, 1.5], 'prob': 1.5}), dict(gamma={'range': [0.7, 1.5], 'prob': -0.1}),
    dict(gamma={'range': [0.7, 1.5], 'prob': NAN}), dict(gamma={'prob': True}), dict(gamma={'prob': '0.3'}), dict(gamma=0.7),
    dict(bias_field={'strength': -0.1}), dict(bias_field={'strength': NAN}), dict(bias_field={'strength': INF}),
    dict(bias_field={'strength': None}), dict(bias_field={'strength': [0.1, 0.3]}), dict(bias_field={'strength': 0.3, 'prob': 2}),
    dict(blur={'sigma': 0}), dict(blur={'sigma': [0, 1]}), dict(blur={'sigma': [-1, 1]}), dict(blur={'sigma': 2.7}),
    dict(blur={'sigma': [0.5, 2.6667]}), dict(blur={'sigma': [1.5, 0.5]}), dict(blur={'sigma': NAN}), dict(blur={'sigma': [0.5, INF]}),
    dict(blur={'sigma': 'a'}), dict(blur={'sigma': False}), dict(blur={'sigma': 1.0, 'prob': -1}),
    dict(noise={'sigma': -0.01}), dict(noise={'sigma': [-0.01, 0.05]}), dict(noise={'sigma': [0.05, 0.01]}), dict(noise={'sigma': NAN}),
    dict(noise={'sigma': [0, INF]}), dict(noise={'sigma': 0.05, 'prob': 1.01}), dict(noise={'sigma': 0.05, 'distribution': 'poisson'}),
    dict(noise={'sigma': 0.05, 'distribution': None}), dict(noise={'sigma': 0.05, 'distribution': 'Rician'}), dict(noise=[0, 0.05])])
def test_bad_values_are_value_errors_at_parse_time(conf):
    with pytest.raises(ValueError, match='random_intensity'):
        _parse(conf)


@pytest.mark.parametrize('conf', [dict(brightness={}), dict(gamma={'range': [0.7, 1.5], 'probability': 0.3}), dict(bias_field={'order': 3}),
                                  dict(blur={'sigma': 1, 'radius': 3}), dict(noise={'sigma': 0.05, 'kind': 'rician'}), dict(gamma={'sigma': 1})])
def test_unknown_keys_are_type_errors(conf):
    with pytest.raises(TypeError, match='random_intensity'):
        _parse(conf)


def _exam(tmp_path, n=8, s=24, seed=5, types=TYPES):
    from dnncancerannotator_amd import tfrecord
    rng = np.random.default_rng(seed)
    slices = rng.integers(0, 256, (n, s, s, len(types))).astype(np.uint8)
    rec = str(tmp_path / 'exam.tfrecords')
    tfrecord.write_records(rec, [tfrecord.make_example(slices, 1, 1, 'p', 'cancer', types)])
    return rec


def _dataset(rec, options, output_size=(16, 16), shard=None, batch=4, types=TYPES):
    from dnncancerannotator_amd import tfrecord
    return tfrecord.TFRecordDataset([rec], types, batch, output_size=output_size, augment_options=options, buffer_size=4, seed=9,
                                    shard=shard, workers=1, repeat=True)


def test_target_channels_are_checked_like_random_contrasts(tmp_path):
    from dnncancerannotator_amd import augment
    plan = lambda t: augment.parse_augment_options({'random_intensity': dict(gamma={'range': [0.7, 1.5]}, target_channels=t)}, (8, 8))      # noqa: E731
    assert augment.intensity_channels(plan(None), 4, 3) is None and augment.intensity_channels(None, 4, 3) is None
    assert augment.intensity_channels(augment.parse_augment_options(BASE, (8, 8)), 4, 3) is None
    assert augment.intensity_channels(plan([0, 2]), 4, 3) == (0, 2)
    assert augment.intensity_channels(plan([0, 2, 3]), 4, 1) == (0, 1, 2)            # raw-slice channels -> feature channels round the label
    for bad in ([4], [-1], [3], [0, 7]):
        with pytest.raises(ValueError, match='random_intensity'):
            augment.intensity_channels(plan(bad), 4, 3)
        with pytest.raises(ValueError, match='random_contrast'):                       # the check it mirrors
            augment.contrast_channels(augment.parse_augment_options({'random_contrast': {'target_channels': bad}}, (8, 8)), 4, 3)
    with pytest.raises(ValueError, match='random_intensity'):
        augment.intensity_channels(plan([1.5]), 4, 3)
    # a bad index fails when the dataset is built; a good one reaches the records: only the named channels are drawn for
    rec = _exam(tmp_path)
    conf = dict(gamma={'range': [0.7, 1.5]}, noise={'sigma': 0.05})
    with pytest.raises(ValueError, match='random_intensity.*label'):
        _dataset(rec, dict(BASE, random_intensity=dict(conf, target_channels=[3])))
    types = ['TRA', 'label', 'ADC', 'DWI']                                              # the label in the middle
    rec2 = _exam(tmp_path, types=types)
    got = next(iter(_dataset(rec2, dict(BASE, random_intensity=dict(conf, target_channels=[0, 3])), types=types))).intensity
    assert got.shape == (4, 3, 32) and (got[:, 0, 0] == 9 + 16).all() and (got[:, 2, 0] == 9 + 16).all() and not got[:, 1].any()


def test_shipped_overlay():
    from dnncancerannotator_amd import augment, load
    assert O.overlay_options() == OVERLAY
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    config = {'data_options': {'train': {'augment_options': dict(BASE)}}}
    over = load._apply_config(config, load._load_config_single(os.path.join(root, 'configs', 'additionals', 'intensity_augment.yaml')))
    plan = augment.parse_augment_options(over['data_options']['train']['augment_options'], (256, 256))
    assert plan.intensity == OVERLAY and plan.warp is not None and plan.affine is None and augment.intensity_is_on(plan)


# -------------------------------------------------------------------------------------------------------------------- draws
def test_an_option_that_is_off_draws_nothing_from_the_generator():
    from dnncancerannotator_amd import augment
    rng = np.random.default_rng(1)
    for conf in (None, dict(gamma={'range': [0.7, 1.5], 'prob': 0}), dict(noise={'sigma': 0})):
        rec = augment.draw_intensity(rng, 3, _parse(conf), 5)
        assert rec.shape == (3, 5, 32) and rec.dtype == np.uint32 and not rec.any()
    # point ranges at prob 1 are active and take no draw either; the key of the noise is the one thing that must be drawn
    rec = augment.draw_intensity(rng, 2, _parse(dict(gamma={'range': 1.25}, blur={'sigma': 1.0})), 3)
    assert (rec[..., 0] == 1 + 4).all() and (rec[..., 1].view(np.float32) == 1.25).all() and (rec[..., 11] == 3).all()
    # a non-target channel takes no draw
    rec = augment.draw_intensity(rng, 2, _parse(dict(noise={'sigma': [0, 0.05], 'prob': 0.5})), 3, targets=())
    assert not rec.any()
    assert rng.random() == np.random.default_rng(1).random()


def test_draws_come_in_the_stated_order_and_fill_the_stated_words():
    """images, then channels; gamma, bias, blur, noise; the activity uniform, then the values; non-target channels are skipped"""
    from dnncancerannotator_amd import augment
    opt = dict(OVERLAY, gamma=dict(range=(0.7, 1.5), prob=0.6), bias_field=dict(strength=0.3, prob=0.6), blur=dict(sigma=(0.5, 1.5), prob=0.6),
               noise=dict(sigma=(0.0, 0.05), prob=0.6, distribution='rician'))
    n, C, targets = 12, 3, (2, 0)
    rec = augment.draw_intensity(np.random.default_rng(4), n, opt, C, targets)
    rng = np.random.default_rng(4)                                         # the same stream, drawn here in the stated order
    want = np.zeros((n, C, 32), np.uint32)
    f = want.view(np.float32)
    sigmas = {}
    for b in range(n):
        for c in (0, 2):
            flags = 0
            if rng.random() < 0.6:
                flags |= 1
                f[b, c, 1] = np.exp(rng.uniform(np.log(0.7), np.log(1.5)))
            if rng.random() < 0.6:
                flags |= 2
                a = rng.uniform(-1.0, 1.0, 9)
                t = rng.uniform(0.0, 0.3)
                f[b, c, 2:11] = a * (t / np.abs(a).sum())
            if rng.random() < 0.6:
                flags |= 4
                sigmas[b, c] = rng.uniform(0.5, 1.5)
                want[b, c, 11], f[b, c, 12:21] = O.taps(sigmas[b, c])
            if rng.random() < 0.6:
                flags |= 8 | 16
                f[b, c, 21] = rng.uniform(0.0, 0.05)
                want[b, c, 22:24] = rng.integers(0, 1 << 32, 2, dtype=np.uint64)
            want[b, c, 0] = flags
    bias_words = np.zeros(32, bool)
    bias_words[2:11] = True
    assert np.array_equal(rec[..., ~bias_words], want[..., ~bias_words])
    # (the bias coefficients may have been moved towards 0 by an ulp to keep sum|a| <= strength in float32)
    assert np.abs(rec[..., 2:11].view(np.float32) - f[..., 2:11]).max() <= 2.0 ** -24
    assert not rec[:, 1].any() and not rec[..., 24:].any()
    assert len(set(rec[..., 0].ravel().tolist())) > 8                       # the terms come and go independently
    assert len(sigmas) > 4 and all(rec[b, c, 11] == int(np.ceil(3 * s)) for (b, c), s in sigmas.items())
    # a Gaussian option sets bit 3 alone; an option without a term never draws for it
    g = augment.draw_intensity(np.random.default_rng(4), 4, _parse(dict(noise={'sigma': [0, 0.05], 'distribution': 'gaussian'})), 2)
    assert (g[..., 0] == 8).all() and not g[..., 1:21].any()


def test_records_keep_their_bounds():
    from dnncancerannotator_amd import augment
    opt = _parse(dict(gamma={'range': [0.7, 1.5]}, bias_field={'strength': 0.3}, blur={'sigma': [0.34, 8 / 3]}, noise={'sigma': [0, 0.05]}))
    rec = augment.draw_intensity(np.random.default_rng(6), 64, opt, 3)
    f = np.zeros(rec.shape)
    f[..., 1:22] = rec[..., 1:22].view(np.float32)                         # (words 0, 11, 22 and 23 are integers)
    assert (rec[..., 0] == 31).all()
    assert 0.7 <= f[..., 1].min() < 0.75 and 1.4 < f[..., 1].max() <= 1.5
    assert (np.abs(f[..., 2:11]).sum(-1) <= 0.3).all() and np.abs(f[..., 2:11]).sum(-1).max() > 0.29
    assert (f[..., 21] >= 0).all() and f[..., 21].max() <= np.float32(0.05)
    radii = rec[..., 11].astype(int)
    assert radii.min() == 2 and radii.max() == 8
    for r, w in zip(radii.ravel(), f[..., 12:21].reshape(-1, 9)):
        assert abs(w[0] + 2 * w[1:].sum() - 1) <= 17 * 2.0 ** -23
        assert (np.diff(w[:r + 1]) < 0).all() and (w[:r + 1] > 0).all() and not w[r + 1:].any()
    keys = {(int(a), int(b)) for a, b in rec[..., 22:24].reshape(-1, 2)}
    assert len(keys) == 64 * 3                                              # every record has a noise stream of its own
    for sigma in (0.34, 0.5, 1.0, 1.5, 2.0, 7.9 / 3, 8 / 3):
        r, w = augment.blur_taps(sigma)
        ro, wo = O.taps(sigma)
        assert r == ro == int(np.ceil(3 * sigma)) <= 8 and np.array_equal(w, wo) and w.dtype == np.float32


# ---------------------------------------------------------------------------------------------------- the dataset's batches
CONF = dict(gamma={'range': [0.7, 1.5], 'prob': 0.5}, bias_field={'strength': 0.3, 'prob': 0.5}, blur={'sigma': [0.5, 1.5], 'prob': 0.5},
            noise={'sigma': [0.0, 0.05], 'prob': 0.5})


def test_other_draws_do_not_move_and_ranks_get_their_halves(tmp_path):
    from dnncancerannotator_amd import augment
    rec = _exam(tmp_path)
    base = dict(BASE, random_crop={'stddev': 1, 'max_': 2, 'min_': -2}, random_affine=dict(rotate_deg=15, scale=[0.9, 1.1], shift=2, symmetry='d4'))
    plain = iter(_dataset(rec, base))
    both = iter(_dataset(rec, dict(base, random_intensity=CONF)))
    lead = iter(_dataset(rec, dict({'random_intensity': CONF}, **base)))     # the key's place among the options changes nothing
    null = iter(_dataset(rec, dict(base, random_intensity=None)))
    seen = []
    for _ in range(3):
        p, q, l, z = next(plain), next(both), next(lead), next(null)
        assert p.intensity is None and z.intensity is None
        assert q.intensity.shape == (4, 3, 32) and q.intensity.dtype == np.uint32
        for other in (q, z):
            assert p.params == other.params and np.array_equal(p.raw, other.raw) and np.array_equal(p.affine, other.affine)
            assert np.array_equal(p.warp[0], other.warp[0]) and np.array_equal(p.warp[1], other.warp[1])
        assert np.array_equal(q.intensity, l.intensity) and q.params == l.params
        seen.append(q.intensity)
    assert len({s.tobytes() for s in seen}) == 3 and len(set(np.concatenate(seen)[..., 0].ravel().tolist())) > 4
    # the stream is the seed's third spawn
    want = augment.draw_intensity(np.random.default_rng(np.random.SeedSequence(9, spawn_key=(2,))), 4, _parse(CONF), 3)
    assert np.array_equal(seen[0], want)
    whole = iter(_dataset(rec, dict(base, random_intensity=CONF)))
    parts = [iter(_dataset(rec, dict(base, random_intensity=CONF), shard=(r, 2))) for r in range(2)]
    for _ in range(2):
        w = next(whole)
        for r in range(2):
            part = next(parts[r])
            assert part.raw.shape[0] == 2 and part.intensity.shape == (2, 3, 32)
            assert np.array_equal(part.intensity, w.intensity[2 * r:2 * r + 2])
            assert np.array_equal(part.raw, w.raw[2 * r:2 * r + 2]) and np.array_equal(part.affine, w.affine[2 * r:2 * r + 2])


def test_tuples_keep_their_old_forms():
    from dnncancerannotator_amd import augment
    assert augment.AugmentPlan._fields[-2:] == ('intensity', 'affine') and augment.RawBatch._fields[-2:] == ('intensity', 'affine')
    assert augment.AugmentPlan._fields[-1] == 'affine' and augment.RawBatch._fields[-1] == 'affine'
    p = augment.AugmentPlan(None, False, None, None, (8, 8))
    assert p.intrawarp is None and p.intensity is None and p.affine is None
    p = augment.AugmentPlan(None, False, None, None, (8, 8), 'iw')
    assert p.intrawarp == 'iw' and p.intensity is None and p.affine is None
    b = augment.RawBatch(None, None, (8, 8), 0, None)
    assert b.intrawarp is None and b.contrast_channels is None and b.intensity is None and b.affine is None
    b = augment.RawBatch(None, None, (8, 8), 0, None, None, (1,))
    assert b.contrast_channels == (1,) and b.intensity is None and b.affine is None
    b = augment.RawBatch(None, None, (8, 8), 0, None, intensity='i', affine='a')
    assert (b.intensity, b.affine) == ('i', 'a') and b[-1] == 'a'
    plan = augment.parse_augment_options(dict(BASE, random_affine={'symmetry': 'flips'}, random_intensity=CONF), (8, 8))
    assert plan.affine['symmetry'] == 'flips' and plan.intensity['gamma'] == dict(range=(0.7, 1.5), prob=0.5) and plan[-1] is plan.affine


# ------------------------------------------------------------------------------------------ the engine's call of intensity
class _View:
    def __init__(self, a):
        self.ptr, self.shape = a, a.shape


def _fake_engine(monkeypatch, staged):
    """the engine on tests/fake_device.FakeDeviceModel with the augmentation entry points added (the construction of
    tests/test_affine_host.py): every entry point logs its name; augment_u8, affine and intensity answer with their oracles"""
    from dnncancerannotator_amd import device, models
    from fake_device import FakeDeviceModel

    class Ring:
        slots = 8

        def __init__(self, dm):
            self.dm, self.outs = dm, {}

        def fits(self, a, b=None):
            return True

        def upload(self, slot, a, b=None, wait=True):
            return ('slot', slot), None

        def wait(self, slot):
            pass

        def train_step(self, slot, x, y, n, lr, cfg):
            self.dm.log.append(('step', True))
            self.outs[slot] = self.dm.train_step(x[:n], y[:n], lr, cfg)

        def out(self, slot):
            return self.outs[slot]

    class Dev(FakeDeviceModel):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.log = []

        def augment_u8(self, raw, params, out_size, label_index, contrast_channels=None, src_ptr=None):
            self.log.append(('augment_u8', src_ptr is not None))
            x, y = A.augment_batch(np.asarray(raw), params, tuple(out_size), label_index, contrast_channels)
            return _View(x), _View(y)

        def affine(self, xv, yv, mats):
            self.log.append(('affine', None))
            x, y = affine_oracle.affine(xv.ptr, yv.ptr, mats)
            return _View(x.astype(np.float32)), _View(y.astype(np.float32))

        def warp(self, xv, yv, ctrl, wv):
            self.log.append(('warp', None))
            return xv, yv

        def warp_groups(self, xv, yv, group_of, ctrl, wv, label_index=None):
            self.log.append(('warp_groups', None))
            return xv, yv

        def intensity(self, xv, records):
            self.log.append(('intensity', np.array(records)))
            assert np.shape(records) == (xv.shape[0], xv.shape[3], 32)
            return _View(O.intensity(np.asarray(xv.ptr, np.float32), records, np.float32))

        def check_dev(self, xb, yb, n):
            assert xb.shape[0] >= n

        def train_step_dev(self, xb, yb, n, lr, cfg, want_out=False):
            self.log.append(('step', False))
            return self.train_step(xb.ptr[:n], yb.ptr[:n], lr, cfg)

        if staged:
            def staging(self, slots=8, slot_bytes=0):
                if getattr(self, '_ring', None) is None:
                    self._ring = Ring(self)
                return self._ring

    monkeypatch.setattr(device, 'init_device', lambda ordinal=0: None)
    monkeypatch.setattr(device, 'device_count', lambda: 1)
    built = []

    def build(self, input_shape, max_batch=None, seed=None, force_generic=False):
        b, h, w, c = input_shape
        opts = {k: v for k, v in self.configs.items() if k in ('n_filters_first', 'n_downsample', 'rate', 'kernel_size', 'conv_stride', 'bn', 'padding')}
        self.device_model = Dev(self.arch, c, h, w, max_batch or b, **opts)
        built.append(self.device_model)
        return self.device_model
    monkeypatch.setattr(models.UNetAnnotator, 'build', build)
    return built


@pytest.mark.parametrize('staged', [False, True], ids=['host_path', 'staged_path'])
def test_engine_calls_intensity_last_and_only_with_records(tmp_path, monkeypatch, staged):
    from dnncancerannotator_amd import engine
    rec = _exam(tmp_path)
    cfg = {'model': 'UNetAnnotator',
           'model_options': dict(n_filters_first=2, n_downsample=1, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same'),
           'deploy_options': {'optimizer': 'adam', 'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}},
                              'enable_multigpu': False}}
    if not staged:
        monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
    else:
        monkeypatch.delenv('DNNCA_NO_FEEDER', raising=False)
    base = dict(BASE, random_crop={'stddev': 1, 'max_': 2, 'min_': -2}, random_affine={'symmetry': 'd4'},
                random_intrachannelwarp={'max_diff': 2, 'stddev': 1.0})
    chain = ['augment_u8', 'affine', 'warp', 'warp_groups']
    losses = {}
    for name, options in (('on', dict({'random_intensity': CONF}, **base)), ('null', dict(base, random_intensity=None)), ('absent', base)):
        built = _fake_engine(monkeypatch, staged)
        res = engine.TFKerasModel(cfg).train(_dataset(rec, options, batch=2), max_steps=3, save_freq=1000)
        losses[name] = np.asarray(res.history['loss'])
        assert len(losses[name]) == 3 and np.isfinite(losses[name]).all()
        log = built[0].log
        names = [n for n, _ in log]
        assert names == (chain + (['intensity'] if name == 'on' else []) + ['step']) * 3, names
        assert all(v == staged for n, v in log if n in ('augment_u8', 'step'))
        if name == 'on':
            want = iter(_dataset(rec, options, batch=2))
            for got in (v for n, v in log if n == 'intensity'):
                assert np.array_equal(got, next(want).intensity)
    assert np.array_equal(losses['null'], losses['absent']) and not np.array_equal(losses['on'], losses['absent'])


def test_feeder_hands_the_records_through(monkeypatch):
    """BatchFeeder stages the raw slices of a RawBatch and hands the batch object itself on: the records arrive as they were drawn"""
    from dnncancerannotator_amd import augment, feeder

    class Ring:
        slots = 8

        def fits(self, a, b=None):
            return True

        def upload(self, slot, a, b=None, wait=True):
            return ('slot', slot), None

    class Dev:
        max_batch, in_shape = 4, (8, 8, 1)

        def staging(self, slot_bytes=0):
            return Ring()

    records = np.arange(2 * 1 * 32, dtype=np.uint32).reshape(2, 1, 32)
    batch = augment.RawBatch(np.zeros((2, 12, 12, 2), np.uint8), [(0, 0, 0, 1.0)] * 2, (8, 8), 1, None, intensity=records)
    f = feeder.BatchFeeder(Dev(), iter([batch]), lambda x, y=None: (x, y))
    try:
        item = next(f)
        assert item[0] == 'raw' and item[3] is batch and item[3].intensity is records
    finally:
        f.close()


# --------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize('counter,key,out', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))])
def test_philox_known_answers(counter, key, out):
    got = O.philox4x32_10(np.array([counter, counter], np.uint32), key)
    assert got.dtype == np.uint32 and got.shape == (2, 4)
    assert [int(v) for v in got[0]] == list(out) and np.array_equal(got[0], got[1])


def test_the_oracles_own_noise_passes_the_statistics():
    x, rec = O.noise_case()
    for T in (np.float64, np.float32):
        O.check_noise_statistics(x, O.intensity(x, rec, T))
    x, rec = O.rician_case()
    for T in (np.float64, np.float32):
        O.check_rician_mean(O.intensity(x, rec, T))
    z0, z1 = O.normals(256, 256, O.NOISE_KEYS[0])
    assert abs(np.corrcoef(z0.ravel(), z1.ravel())[0, 1]) < 5 / 256 and abs(z1.mean()) < 5 / 256


def test_restatement_sets_the_device_bound():
    """the float32 restatement against the float64 statement on every case the device runs: its worst is CPU_WORST, and the device
    gets 4 x that, rounded up to a power of two"""
    worst = {}
    for shape, which in O.cases():
        x, rec = O.case(shape, which)
        want, got = O.intensity(x, rec), O.intensity(x, rec, np.float32)
        assert got.dtype == np.float32 and want.dtype == np.float64
        worst[shape, which] = O.worst_units(got, want, x, rec)
        assert np.abs(want - x).max() > 1e-3                               # every case changes its planes
    x, rec = O.overlay_case()
    assert all(((rec[..., 0] & bit) != 0).sum() >= 3 for bit in (1, 2, 4, 8))        # every term is drawn in that batch
    worst['overlay'] = O.worst_units(O.intensity(x, rec, np.float32), O.intensity(x, rec), x, rec)
    top = max(worst, key=worst.get)
    print('float32 restatement: worst %.3f units at %s; overlay case %.3f' % (worst[top], top, worst['overlay']))
    assert 0.5 * O.CPU_WORST < worst[top] <= O.CPU_WORST
    assert O.BOUND == 2.0 ** np.ceil(np.log2(4 * O.CPU_WORST))
    # a wrong key, counter or tap is an error of the order of sigma: thousands of units
    x, rec = O.case((2, 9, 33, 3), ('noise',))
    bad = rec.copy()
    bad[0, 0, 22] ^= 1
    assert O.worst_units(O.intensity(x, bad), O.intensity(x, rec), x, rec) > 1000 * O.BOUND
