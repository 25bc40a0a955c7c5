"""CPU rehearsal of tests/test_augment_edges_gpu.py, and the host-side fixes that came with it.

The checks of tests/augment_edges.py run here on NumpyDevice, a float32 restatement of csrc/kernels_aug.hip.  That proves two
things without a GPU: the oracle and the chosen inputs alone stay inside every bound (with the room stated below), and every
check fails when the restatement carries the defect it is there for (test_mutation_fails_its_named_checks).

Room of the float32 arithmetic, measured here against the float64 oracle (the device tests assert 1e-2 px / 1e-3 / 2e-6):
    warp, worst over all cases of WARP_CASES   position 5.98e-06 px (groups_40x72), smooth 2.19e-07 (warp_40x72)
    warp_clamps_64x48 (flows up to 55 px)      position 4.06e-06 px
    warp_groups burst                          position 1.64e-06 px
    augment, worst |dx| of an adjusted channel 1.19e-07, burst 1.19e-07
test_float32_room asserts the hundredfold room (<= 1e-4 px) for every warp case."""

import numpy as np
import pytest

import augment_edges as E
from oracle import augment_oracle as A


# ------------------------------------------------------------------------------------------------------------------- the oracle
def _warp_image_before_the_split(img, source, dest):
    """oracle.augment_oracle.warp_image as it was before warp_image_coeffs was split out of it (kept here to pin the bits)"""
    img = np.asarray(img, np.float64)
    h, w, _ = img.shape
    c = np.asarray(dest, np.float64)
    f = c - np.asarray(source, np.float64)
    k = len(c)
    phi = lambda r: 0.5 * r * np.log(np.maximum(r, 1e-10))                      # noqa: E731
    lhs = np.zeros((k + 3, k + 3))
    lhs[:k, :k] = phi(((c[:, None] - c[None]) ** 2).sum(-1))
    lhs[:k, k:k + 2] = c
    lhs[:k, k + 2] = 1.0
    lhs[k:, :k] = lhs[:k, k:].T
    rhs = np.zeros((k + 3, 2))
    rhs[:k] = f
    wv = np.linalg.solve(lhs, rhs)
    qy, qx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    q = np.stack([qy, qx], -1).reshape(-1, 2)
    flow = phi(((q[:, None] - c[None]) ** 2).sum(-1)) @ wv[:k] + np.concatenate([q, np.ones((len(q), 1))], 1) @ wv[k:]
    s = q - flow
    fy = np.clip(np.floor(s[:, 0]), 0, h - 2)
    fx = np.clip(np.floor(s[:, 1]), 0, w - 2)
    ay = np.clip(s[:, 0] - fy, 0, 1)[:, None]
    ax = np.clip(s[:, 1] - fx, 0, 1)[:, None]
    iy, ix = fy.astype(int), fx.astype(int)
    tl, tr, bl, br = img[iy, ix], img[iy, ix + 1], img[iy + 1, ix], img[iy + 1, ix + 1]
    top, bot = ax * (tr - tl) + tl, ax * (br - bl) + bl
    return (ay * (bot - top) + top).reshape(h, w, -1)


def test_oracle_warp_split_keeps_the_bits():
    rng = np.random.default_rng(31)
    img = rng.random((20, 28, 3))
    src = rng.uniform(0, 1, (30, 2)) * [20, 28]
    dst = src + np.clip(rng.normal(0, 6.0, (30, 2)), -15, 15)           # strong enough to leave the image at the borders
    old = _warp_image_before_the_split(img, src, dst)
    assert np.array_equal(A.warp_image(img, src, dst), old)
    ctrl, wv = A.solve_warp_coeffs(src, dst)
    assert np.array_equal(A.warp_image_coeffs(img, ctrl, wv), old)
    assert np.abs(old - img).max() > 0.1
    # chosen coefficients: zero is the identity, a constant integer flow is a clipped shift
    ident = A.warp_image_coeffs(img, ctrl, np.zeros_like(wv))
    assert np.array_equal(ident, img)
    shift = np.zeros_like(wv)
    shift[-1] = (3, -5)
    assert np.array_equal(A.warp_image_coeffs(img, ctrl, shift), E.shifted(img, 3, -5))


# -------------------------------------------------------------------------------------------- the checks on the float32 restatement
@pytest.mark.parametrize('variant', E.AUG_VARIANTS)
@pytest.mark.parametrize('name', sorted(E.AUG_SHAPES))
def test_augment_edges(name, variant):
    E.check_augment(E.NumpyDevice(), name, variant)


def test_augment_ring():
    E.check_augment_burst(E.NumpyDevice())


def test_warp_groups_ring():
    E.check_warp_groups_burst(E.NumpyDevice())


@pytest.mark.parametrize('entry', ['warp', 'groups'])
def test_warp_identity(entry):
    E.check_warp_identity(E.NumpyDevice(), entry)


@pytest.mark.parametrize('entry', ['warp', 'groups'])
def test_warp_shift(entry):
    E.check_warp_shift(E.NumpyDevice(), entry)


@pytest.mark.parametrize('name', sorted(E.WARP_CASES))
def test_float32_room(name):
    """a float32 cast of the oracle's own float64 flow, sampled in float32, stays a hundred times inside the 1e-2 px bound (and
    the smooth channels a hundred times inside theirs) on every input the device test uses; the flows of the chosen-coefficient
    cases stay within a few pixels"""
    E.check_warp_case(E.NumpyDevice(), name, position_bound=E.FLOAT32_ROOM, smooth_bound=E.SMOOTH_BOUND / 100)
    if E.WARP_CASES[name][-1][0] != 'solve':
        assert E.warp_case(name)['flow_max'] < 8.0


def test_cases_reach_the_arms_they_are_for():
    """the shapes do what the table in NOTES.md says of them (the launch rules are those of dnnca_augment_u8)"""
    blocks = {}
    for name, (B, hs, ws, cs, label, ho, wo) in E.AUG_SHAPES.items():
        n = ho * wo
        blocks[name] = (n + 4095) // 4096
        p = E.aug_case(name)['params']
        assert (hs - ho) // 2 + p[0][0] == 0 and (ws - wo) // 2 + p[0][1] + wo == ws and p[0][2] == 1 and np.float32(p[0][3]) == np.float32(1.2)
        assert p[1][3] == 1.0
    assert blocks == {'two_blocks_label_first': 2, 'odd_eight_channels': 1, 'no_margin': 1, 'block_cap': 65}
    assert E.AUG_SHAPES['odd_eight_channels'][3] == 8 and (41 - 30) % 2 == 1 and 47 % 2 == 1
    assert E.aug_case('no_margin')['params'][2][:2] == (0, 0)
    assert E.aug_case('no_margin')['label'] in E.aug_case('no_margin')['channels']['subset']
    for name, (entry, B, H, W, kinds, table, n, how) in E.WARP_CASES.items():
        assert (n * 4 + 6) * 8 <= 64 << 10
    assert (E.EXACT['H'] * E.EXACT['W']) % 256 == 64 and (2046 * 4 + 6) * 8 == 65520 and (2047 * 4 + 6) * 8 > 64 << 10
    assert max(s[0] for s in E.EXACT_SHIFTS) > E.EXACT['H']


# --------------------------------------------------------------------------------------------------------------------- mutations
# mutation of the restatement -> the checks (named as the tests of both files name them) that must fail under it
BROKEN_BY = {
    'swap_hw': [('check_warp_shift', 'warp'), ('check_warp_shift', 'groups'), ('check_warp_identity', 'warp'),
                ('check_warp_identity', 'groups'), ('check_warp_case', 'warp_72x40_c8'), ('check_warp_case', 'groups_40x72')],
    'tail_unwritten': [('check_warp_identity', 'warp'), ('check_warp_identity', 'groups'), ('check_warp_shift', 'warp'),
                       ('check_warp_case', 'warp_40x72'), ('check_warp_case', 'groups_72x40_c8')],
    'coeffs_256': [('check_warp_case', 'warp_n150'), ('check_warp_case', 'groups_n150'), ('check_warp_case', 'warp_n2046_c1'),
                   ('check_warp_case', 'groups_n2046_c1')],
    'sums_4096': [('check_augment', 'two_blocks_label_first', 'default'), ('check_augment', 'two_blocks_label_first', 'subset'),
                  ('check_augment', 'block_cap', 'default')],
    'label_bit': [('check_augment', 'no_margin', 'subset'), ('check_augment', 'block_cap', 'subset')],
    'ring_row_0': [('check_augment_burst',), ('check_warp_groups_burst',)],
}


@pytest.mark.parametrize('mutation', E.MUTATIONS)
def test_mutation_fails_its_named_checks(mutation):
    for check, *args in BROKEN_BY[mutation]:
        with pytest.raises(AssertionError):
            getattr(E, check)(E.NumpyDevice(mutation), *args)


def test_single_call_mutations_leave_other_checks_alone():
    """the mutations are narrow: what does not touch their arm still passes (so a failure above is the arm's, not noise)"""
    E.check_augment(E.NumpyDevice('sums_4096'), 'odd_eight_channels', 'default')          # 1410 pixels: one trip
    E.check_warp_case(E.NumpyDevice('coeffs_256'), 'warp_40x72')                            # 200 coefficients: one pass
    E.check_augment(E.NumpyDevice('label_bit'), 'two_blocks_label_first', 'default')
    E.check_augment(E.NumpyDevice('ring_row_0'), 'no_margin', 'default')                   # one call: row 0 is its row


# ------------------------------------------------------------------------------------- random_contrast.target_channels reaches the device
class _View:
    def __init__(self, a):
        self.ptr, self.shape = a, a.shape


def _fake_engine(monkeypatch, staged):
    """the engine on tests/fake_device.FakeDeviceModel with the augmentation entry points added: augment_u8 records what it was
    given and answers with the oracle; `staged` adds a staging ring, so that the feeder hands the loop ('raw', slot, ...) items"""
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
            self.outs[slot] = self.dm.train_step(x[:n], y[:n], lr, cfg)

        def out(self, slot):
            return self.outs[slot]

    class Dev(FakeDeviceModel):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.augment_calls = []

        def augment_u8(self, raw, params, out_size, label_index, contrast_channels=None, src_ptr=None):
            self.augment_calls.append(dict(contrast_channels=contrast_channels, staged=src_ptr is not None))
            x, y = A.augment_batch(np.asarray(raw), params, tuple(out_size), label_index, contrast_channels)
            return _View(x), _View(y)

        def check_dev(self, xb, yb, n):
            assert xb.shape[0] >= n

        def train_step_dev(self, xb, yb, n, lr, cfg, want_out=False):
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


def _exam(tmp_path, types):
    from dnncancerannotator_amd import tfrecord
    rng = np.random.default_rng(41)
    slices = rng.integers(0, 256, (6, 24, 24, len(types))).astype(np.uint8)
    rec = str(tmp_path / 'exam.tfrecords')
    tfrecord.write_records(rec, [tfrecord.make_example(slices, 1, 1, 'p', 'cancer', types)])
    return rec


def _dataset(rec, types, contrast):
    from dnncancerannotator_amd import tfrecord
    return tfrecord.TFRecordDataset([rec], types, 2, output_size=(16, 16), repeat=True, workers=1, seed=3,
                                    augment_options={'random_crop': {'stddev': 1, 'max_': 2, 'min_': -2}, 'random_contrast': contrast})


@pytest.mark.parametrize('staged', [False, True], ids=['host_path', 'staged_path'])
def test_target_channels_reach_augment_u8(tmp_path, monkeypatch, staged):
    """random_contrast.target_channels: the channels named in the options are the ones DeviceModel.augment_u8 is given, on the
    loop's own upload path and on the feeder's staged path; without the option it is given None (every feature channel)"""
    from dnncancerannotator_amd import engine
    types = ['TRA', 'ADC', 'DWI', 'label']
    rec = _exam(tmp_path, types)
    cfg = {'model': 'UNetAnnotator',
           'model_options': dict(n_filters_first=2, n_downsample=1, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same'),
           'deploy_options': {'optimizer': 'adam', 'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}},
                              'enable_multigpu': False}}
    if not staged:
        monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
    else:
        monkeypatch.delenv('DNNCA_NO_FEEDER', raising=False)
    for contrast, want in (({'target_channels': [0]}, (0,)), ({'target_channels': [2, 1]}, (2, 1)), (None, None)):
        built = _fake_engine(monkeypatch, staged)
        ds = _dataset(rec, types, contrast)
        assert next(iter(ds)).contrast_channels == want
        res = engine.TFKerasModel(cfg).train(ds, max_steps=3, save_freq=1000)
        assert len(res.history['loss']) == 3 and np.isfinite(res.history['loss']).all()
        calls = built[0].augment_calls
        assert len(calls) == 3 and all(c['contrast_channels'] == want and c['staged'] == staged for c in calls), calls


def test_target_channels_are_checked_when_the_dataset_is_built(tmp_path):
    """an index outside the raw slice, or the label's, is a ValueError from the dataset's constructor; None keeps every feature
    channel (the project's default wherever the label stands -- augment.contrast_channels says how the reference's differs)"""
    from dnncancerannotator_amd import augment
    types = ['TRA', 'label', 'ADC']
    rec = _exam(tmp_path, types)
    for bad in ([3], [-1], [0, 1], [1]):
        with pytest.raises(ValueError, match='random_contrast'):
            _dataset(rec, types, {'target_channels': bad})
    assert _dataset(rec, types, {'target_channels': [2, 0]}).contrast_channels == (2, 0)
    assert _dataset(rec, types, {}).contrast_channels is None and _dataset(rec, types, None).contrast_channels is None
    assert augment.contrast_channels(None, 3, 1) is None
    assert augment.RawBatch(None, None, (8, 8), 0, None).contrast_channels is None              # the old positional form still works
    assert augment.RawBatch(None, None, (8, 8), 0, None, None, (1,)).contrast_channels == (1,)
