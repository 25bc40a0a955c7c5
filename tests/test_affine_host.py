"""random_affine, host side (no GPU): option parsing, the draws of augment.draw_affine, their place behind every other draw of
the dataset, the split over ranks, and the engine's call of DeviceModel.affine between augment_u8 and warp in both of its
RawBatch branches.  The resampling itself is stated in tests/affine_oracle.py; the device is held to it in test_affine_gpu.py."""

import numpy as np
import pytest

import affine_oracle as O
from oracle import augment_oracle as A

BASE = {'random_crop': None, 'random_flip': None, 'random_contrast': None, 'random_warp': None}
TYPES = ['TRA', 'ADC', 'DWI', 'label']


# ------------------------------------------------------------------------------------------------------------------ options
def test_parse_defaults_and_absence():
    from dnncancerannotator_amd import augment, tta
    plan = augment.parse_augment_options({'random_affine': None}, (64, 64))
    assert plan.affine == dict(rotate_deg=0.0, scale=(1.0, 1.0), shift=0.0, symmetry='none')
    plan = augment.parse_augment_options({'random_affine': dict(rotate_deg=15, scale=[0.9, 1.1], shift=8, symmetry='d4')}, (64, 64))
    assert plan.affine == dict(rotate_deg=15.0, scale=(0.9, 1.1), shift=8.0, symmetry='d4')
    assert augment.AFFINE_SYMMETRIES == tta.MODES                                  # the names the TTA modes use
    # without the key the plan is what it was, and the old positional forms still work
    before = augment.parse_augment_options(BASE, (256, 256))
    assert before.affine is None and before.intrawarp is None
    assert before[:5] == (dict(stddev=4, max_=6, min_=-6), True, dict(lower=0.8, upper=1.2, target_channels=None),
                          dict(n_points=100, max_diff=5, stddev=2.0), (256, 256))
    assert augment.AugmentPlan(None, False, None, None, (8, 8)).affine is None
    assert augment.AugmentPlan(None, False, None, None, (8, 8), None).affine is None
    assert augment.RawBatch(None, None, (8, 8), 0, None).affine is None
    assert augment.RawBatch(None, None, (8, 8), 0, None, None, (1,)).affine is None
    assert augment.AugmentPlan._fields[-1] == 'affine' and augment.RawBatch._fields[-1] == 'affine'


@pytest.mark.parametrize('conf', [
    dict(rotate_deg=-1), dict(rotate_deg=180.5), dict(rotate_deg=float('nan')), dict(rotate_deg=float('inf')), dict(rotate_deg='15'),
    dict(scale=[0, 1]), dict(scale=[-1, 1]), dict(scale=[1.2, 0.8]), dict(scale=[1, float('inf')]), dict(scale=[float('nan'), 1]),
    dict(scale=1.0), dict(scale=[1, 1, 1]), dict(scale='ab'),
    dict(shift=-0.5), dict(shift=float('nan')), dict(shift=float('inf')), dict(shift=None),
    dict(symmetry='rot90'), dict(symmetry=None), dict(symmetry='D4')])
def test_bad_values_are_value_errors_at_parse_time(conf):
    from dnncancerannotator_amd import augment
    with pytest.raises(ValueError, match='random_affine'):
        augment.parse_augment_options({'random_affine': conf}, (8, 8))


def test_limits_of_the_ranges_are_accepted_and_unknown_keys_are_type_errors():
    from dnncancerannotator_amd import augment
    plan = augment.parse_augment_options({'random_affine': dict(rotate_deg=180, scale=[0.5, 0.5], shift=0, symmetry='flips')}, (8, 12))
    assert plan.affine == dict(rotate_deg=180.0, scale=(0.5, 0.5), shift=0.0, symmetry='flips')
    with pytest.raises(TypeError, match='random_affine'):
        augment.parse_augment_options({'random_affine': {'rotate': 3}}, (8, 8))
    with pytest.raises(TypeError):
        augment.parse_augment_options({'random_affine': {'rotate_deg': 3, 'shear': 0.1}}, (8, 8))


def _exam(tmp_path, n=8, s=24, seed=5):
    from dnncancerannotator_amd import tfrecord
    rng = np.random.default_rng(seed)
    slices = rng.integers(0, 256, (n, s, s, len(TYPES))).astype(np.uint8)
    rec = str(tmp_path / 'exam.tfrecords')
    tfrecord.write_records(rec, [tfrecord.make_example(slices, 1, 1, 'p', 'cancer', TYPES)])
    return rec


def _dataset(rec, options, output_size=(16, 16), shard=None, batch=4):
    from dnncancerannotator_amd import tfrecord
    return tfrecord.TFRecordDataset([rec], TYPES, batch, output_size=output_size, augment_options=options, buffer_size=4, seed=9,
                                    shard=shard, workers=1, repeat=True)


def test_d4_on_a_non_square_size_fails_when_the_dataset_is_built(tmp_path):
    rec = _exam(tmp_path)
    crop = {'random_crop': {'stddev': 1, 'max_': 2, 'min_': -2}}
    with pytest.raises(ValueError, match='random_affine.*square'):
        _dataset(rec, dict(crop, random_affine={'symmetry': 'd4'}), output_size=(16, 12))
    assert _dataset(rec, dict(crop, random_affine={'symmetry': 'flips'}), output_size=(16, 12)).plan.affine['symmetry'] == 'flips'
    assert _dataset(rec, dict(crop, random_affine={'symmetry': 'd4'}), output_size=(16, 16)).plan.affine['symmetry'] == 'd4'


def test_shipped_overlays():
    import os
    from dnncancerannotator_amd import augment, load
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    config = {'data_options': {'train': {'augment_options': dict(BASE)}}}
    over = load._apply_config(config, load._load_config_single(os.path.join(root, 'configs', 'additionals', 'affine_augment.yaml')))
    plan = augment.parse_augment_options(over['data_options']['train']['augment_options'], (256, 256))
    assert plan.affine == dict(rotate_deg=15.0, scale=(0.9, 1.1), shift=8.0, symmetry='none') and plan.warp is not None
    config = {'data_options': {'train': {'augment_options': dict(BASE)}}}
    over = load._apply_config(config, load._load_config_single(os.path.join(root, 'configs', 'additionals', 'd4_augment.yaml')))
    plan = augment.parse_augment_options(over['data_options']['train']['augment_options'], (256, 256))
    assert plan.affine == dict(rotate_deg=0.0, scale=(1.0, 1.0), shift=0.0, symmetry='d4')


# -------------------------------------------------------------------------------------------------------------------- draws
def _options(**conf):
    from dnncancerannotator_amd import augment
    return augment.parse_augment_options({'random_affine': conf}, (8, 8)).affine


def test_default_options_draw_the_identity_and_nothing_from_the_generator():
    from dnncancerannotator_amd import augment
    rng = np.random.default_rng(1)
    for size in ((5, 7), (6, 6), (1, 1), (512, 512)):
        m = augment.draw_affine(rng, 3, _options(), size)
        assert m.shape == (3, 2, 3) and m.dtype == np.float64
        assert np.array_equal(m, np.broadcast_to(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (3, 2, 3)))
    assert rng.random() == np.random.default_rng(1).random()              # a point range takes no draw


def _planes(B, h, w, C, seed):
    rng = np.random.default_rng(seed)
    return rng.random((B, h, w, C)).astype(np.float32), rng.random((B, h, w)).astype(np.float32)


@pytest.mark.parametrize('size,symmetry,n_views', [((5, 5), 'd4', 8), ((6, 6), 'd4', 8), ((5, 7), 'flips', 4), ((6, 4), 'flips', 4)])
def test_symmetry_draws_are_exact_and_equal_numpy_views(size, symmetry, n_views):
    """every element comes up, every entry is an exact integer or half-integer, and through the oracle the matrix gives numpy's
    flip / transpose of the planes bit for bit"""
    from dnncancerannotator_amd import augment
    n = 96
    mats = augment.draw_affine(np.random.default_rng(2), n, _options(symmetry=symmetry), size)
    assert np.array_equal(mats * 2, np.round(mats * 2))
    assert set(np.unique(mats[:, :, :2])) <= {-1.0, 0.0, 1.0}
    x, y = _planes(1, size[0], size[1], 3, seed=3)
    views = [(O.d4_numpy(x, k), O.d4_numpy(y, k)) for k in range(n_views)]
    seen = {}
    for b in range(n):
        xo, yo = O.affine(x, y, mats[b:b + 1])
        hits = [k for k, (vx, vy) in enumerate(views) if vx.shape == xo.shape and np.array_equal(xo, vx) and np.array_equal(yo, vy)]
        assert len(hits) == 1, (b, mats[b], hits)
        assert np.array_equal(mats[b, :, :2], augment.d4_matrix(hits[0]))
        seen[hits[0]] = seen.get(hits[0], 0) + 1
    assert sorted(seen) == list(range(n_views)), seen


def test_general_draws_are_in_range_in_order_and_composed_as_stated():
    from dnncancerannotator_amd import augment
    opt = _options(rotate_deg=15, scale=[0.9, 1.1], shift=8, symmetry='d4')
    h = w = 32
    n = 200
    mats = augment.draw_affine(np.random.default_rng(4), n, opt, (h, w))
    rng = np.random.default_rng(4)                                         # the same stream, drawn here in the stated order
    c = np.array([(h - 1) / 2.0, (w - 1) / 2.0])
    thetas, zooms = [], []
    for b in range(n):
        theta = rng.uniform(-15.0, 15.0)
        z = np.exp(rng.uniform(np.log(0.9), np.log(1.1)))
        t = rng.uniform(-8.0, 8.0, 2)
        g = augment.d4_matrix(int(rng.integers(8)))
        want = O.matrix(h, w, theta, z, t, g)
        assert np.abs(mats[b] - want).max() <= 1e-12 * 64, (b, mats[b], want)
        lin = mats[b, :, :2]
        assert abs(abs(np.linalg.det(lin)) - 1 / z ** 2) <= 1e-12                  # rotation (or reflection) over z
        assert np.abs(lin @ (c + t) + mats[b, :, 2] - c).max() <= 1e-9            # the shifted centre maps to the centre
        thetas.append(theta)
        zooms.append(z)
    assert -15 <= min(thetas) < -10 and 10 < max(thetas) <= 15 and 0.9 <= min(zooms) < 0.93 and 1.07 < max(zooms) <= 1.1
    # z > 1 enlarges the content: the source footprint of the plane shrinks
    big = augment.draw_affine(np.random.default_rng(0), 1, _options(scale=[2, 2]), (9, 9))[0]
    assert np.array_equal(big, [[0.5, 0.0, 2.0], [0.0, 0.5, 2.0]])
    # one key alone takes only its own draws
    only_shift = augment.draw_affine(np.random.default_rng(6), 2, _options(shift=3), (9, 9))
    r6 = np.random.default_rng(6)
    for b in range(2):
        t = r6.uniform(-3.0, 3.0, 2)
        assert np.array_equal(only_shift[b, :, :2], np.eye(2)) and np.abs(only_shift[b, :, 2] + t).max() <= 4 * np.spacing(8.0)


# ---------------------------------------------------------------------------------------------------- the dataset's batches
def test_other_draws_do_not_move_and_ranks_get_their_halves(tmp_path):
    rec = _exam(tmp_path)
    crop = {'random_crop': {'stddev': 1, 'max_': 2, 'min_': -2}}
    base = dict(BASE, **crop)
    conf = dict(rotate_deg=15, scale=[0.9, 1.1], shift=2, symmetry='d4')
    plain = iter(_dataset(rec, base))
    both = iter(_dataset(rec, dict(base, random_affine=conf)))
    first = dict(base)
    first = dict({'random_affine': conf}, **first)                       # the key's place among the options changes nothing
    lead = iter(_dataset(rec, first))
    for _ in range(3):
        p, q, l = next(plain), next(both), next(lead)
        assert p.affine is None and q.affine.shape == (4, 2, 3) and q.affine.dtype == np.float64
        assert p.params == q.params and np.array_equal(p.raw, q.raw)
        assert np.array_equal(p.warp[0], q.warp[0]) and np.array_equal(p.warp[1], q.warp[1])
        assert np.array_equal(q.affine, l.affine) and q.params == l.params
        assert len({q.affine[b].tobytes() for b in range(4)}) == 4
    whole = next(iter(_dataset(rec, dict(base, random_affine=conf))))
    for r in range(2):
        part = next(iter(_dataset(rec, dict(base, random_affine=conf), shard=(r, 2))))
        assert part.raw.shape[0] == 2 and part.affine.shape == (2, 2, 3)
        assert np.array_equal(part.affine, whole.affine[2 * r:2 * r + 2])
        assert np.array_equal(part.raw, whole.raw[2 * r:2 * r + 2]) and np.array_equal(part.warp[1], whole.warp[1][2 * r:2 * r + 2])


# --------------------------------------------------------------------------------------------- the engine's call of affine
class _View:
    def __init__(self, a):
        self.ptr, self.shape = a, a.shape


def _fake_engine(monkeypatch, staged):
    """the engine on tests/fake_device.FakeDeviceModel with the augmentation entry points added (the construction of
    tests/test_augment_edges.py): every entry point logs its name; augment_u8 and affine answer with their oracles"""
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
            self.log.append(('affine', np.array(mats)))
            x, y = O.affine(xv.ptr, yv.ptr, mats)
            return _View(x.astype(np.float32)), _View(y.astype(np.float32))

        def warp(self, xv, yv, ctrl, wv):
            self.log.append(('warp', None))
            return xv, yv

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
def test_engine_calls_affine_between_augment_u8_and_warp(tmp_path, monkeypatch, staged):
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
    base = dict(BASE, random_crop={'stddev': 1, 'max_': 2, 'min_': -2})
    for conf in (dict(rotate_deg=20, symmetry='d4'), None):
        options = dict(base, random_affine=conf) if conf is not None else base
        built = _fake_engine(monkeypatch, staged)
        res = engine.TFKerasModel(cfg).train(_dataset(rec, options, batch=2), max_steps=3, save_freq=1000)
        assert len(res.history['loss']) == 3 and np.isfinite(res.history['loss']).all()
        log = built[0].log
        names = [name for name, _ in log]
        per_step = ['augment_u8', 'affine', 'warp', 'step'] if conf is not None else ['augment_u8', 'warp', 'step']
        assert names == per_step * 3, names
        assert all(v == staged for name, v in log if name in ('augment_u8', 'step'))
        if conf is not None:
            want = iter(_dataset(rec, options, batch=2))
            for got in (v for name, v in log if name == 'affine'):
                assert np.array_equal(got, next(want).affine)
