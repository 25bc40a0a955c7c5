"""-m gpu: the boundary (signed-distance) term of the loss (DeviceModel.set_boundary_loss) in the step, against the float64
reference of tests/boundary_oracle.py.  It mirrors tests/test_region_loss_gpu.py: the same three shapes (heads of 3, 16 and 64
channels), B = 3 images on a model of max_batch = 4, image 0 without positives (phi = 0: the term vanishes), image 2 with a lesion on
two borders, weights from helpers.perturbed_params; the tuned plan (fused head kernels) and force_generic (from the logits).

Bounds, the project's own as in that file: loss 1e-4 max(1, |loss|); gradients 2e-5 per tensor (assert_grads_per_tensor_nofixture, as
there); boundary_loss_sums() 1e-6 relative; boundary_distance() bit-equal to the oracle's map.

Measured on an MI355X, one train step at boundary_weight 0.01 and 1.0: loss error 1.3e-8 .. 3.3e-7 relative; boundary_loss_sums()
1.5e-9 .. 2.6e-9 (c3, c64) and 6.8e-8 (c16, BatchNorm) relative -- as for region_loss_sums() the float32 network's logits decide
it, so the bound stays 1e-6; worst gradient tensor 4.1e-7 .. 1.0e-6 of its scale on the unet shapes (mulmo: 2e-5 holds for every
tensor but the analytically zero ones, which assert_grads_per_tensor_nofixture holds to a healthy sibling's scale); the map
bit-equal in every case.  Every bound holds."""

import os

import numpy as np
import pytest

import boundary_oracle as BO
import helpers as Hp
import region_loss_ref as R
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

COMMON = dict(rate=2, kernel_size=3, conv_stride=1, padding='same')
# name -> (arch, in_channels, options, H, W, the launches of the tuned plan that carry the head): tests/test_region_loss_gpu.py's
SHAPES = {
    'c3': ('unet', 1, dict(n_filters_first=3, n_downsample=3, bn=False, **COMMON), 40, 24, ('head_region_fwd_3', 'head_region_train_3')),
    'c16': ('mulmo', 3, dict(n_filters_first=16, n_downsample=2, bn=True, **COMMON), 12, 20, ('head_region_fwd_16', 'head_region_train_16')),
    'c64': ('unet', 1, dict(n_filters_first=64, n_downsample=1, bn=False, **COMMON), 10, 14, ('head_region_fwd_64', 'head_region_train_64')),
}
B, MAXB = 3, 4
TRANSFORM = ('boundary_cols', 'boundary_rows')
LOGITS_ARM = ('region_sums', 'region_loss_finish', 'region_loss_grad')
REGION = dict(weight_mul=3.0)
SMOOTHED = dict(weight_mul=3.0, alpha=0.3, beta=0.7, smooth=0.1, label_smoothing=True, label_smoothing_filter_size=6, label_smoothing_sigma=3)

_cache = {}


def _batch(shape, seed=8, full=False):
    arch, C, opts, H, W, _ = SHAPES[shape]
    key = ('batch', shape, seed, full)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        x = rng.random((B, H, W, C)).astype(np.float32)
        y = np.zeros((B, H, W), np.float32)
        y[1, H // 4:H // 2, W // 4:W // 2 + 2] = 1.0
        y[2, H - H // 4:H, 0:W // 4] = 1.0                    # touches two borders
        if full:
            y[0] = 1.0                                        # all foreground: phi = 0 there too
        x.setflags(write=False)
        y.setflags(write=False)
        _cache[key] = (x, y)
    return _cache[key]


def _spec(shape):
    arch, C, opts, H, W, _ = SHAPES[shape]
    return O.ModelSpec(arch, C, **opts)


def _params(shape):
    key = ('params', shape)
    if key not in _cache:
        _cache[key] = Hp.perturbed_params(_spec(shape), np.float64)
    return _cache[key]


def _reference(shape, cfg, training=True, full=False):
    """(loss, flat gradients, S_b, I/P/Y sums, phi) of the float64 reference, computed once per case"""
    key = ('ref', shape, tuple(sorted(cfg.items())), training, full)
    if key not in _cache:
        x, y = _batch(shape, full=full)
        spec = _spec(shape)
        loss, grads, logits, _ = BO.loss_and_grads(spec, _params(shape), x.astype(np.float64), y, cfg, training=training)
        sums = R.region_sums(R.loss_labels(y, BO.split_cfg(cfg)[0]), logits)
        _cache[key] = (loss, O.flatten(spec, grads), BO.boundary_sums(y, logits), sums, BO.signed_distance(y)[0])
    return _cache[key]


def _model(gpu, shape, force_generic=False, cfg=None, boundary=None):
    """cfg: the region loss is set from its keys; boundary: and the boundary term at this weight"""
    arch, C, opts, H, W, _ = SHAPES[shape]
    spec = _spec(shape)
    m = gpu.DeviceModel(arch, C, H, W, MAXB, force_generic=force_generic, **opts)
    m.set_params(O.flatten(spec, _params(shape)))
    if m.n_state:
        m.set_state(O.flatten(spec, _params(shape), trainable=False))
    if cfg is not None:
        m.set_region_loss({k: v for k, v in cfg.items() if k in R.REGION_KEYS})
    if boundary is not None:
        m.set_boundary_loss(boundary)
    return m


def _names(m, mode='train'):
    return [r[0] for r in m.plan(mode=mode, batch=B)]


def _loss_names(names):
    return [n for n in names if 'region' in n or 'boundary' in n or n == 'g_loss']


def _check_step(gpu, shape, cfg, force_generic, full=False):
    x, y = _batch(shape, full=full)
    spec = _spec(shape)
    region_cfg, bw = BO.split_cfg(cfg)
    loss, gref, S, sums, phi = _reference(shape, cfg, full=full)
    m = _model(gpu, shape, force_generic, cfg=region_cfg, boundary=bw)
    try:
        names = _names(m)
        want = LOGITS_ARM if force_generic else SHAPES[shape][5][:1] + ('region_loss_finish',) + SHAPES[shape][5][1:]
        assert _loss_names(names) == list(TRANSFORM + want), names
        assert not any(n.startswith(('tail3', 'pgfwd_head', 'head_train')) for n in names), names
        out = m.train_step(x, y, 0.0, m.loss_cfg(**R.split_cfg(region_cfg)[0]))
        got_S, got = m.boundary_loss_sums(B), m.region_loss_sums(B)
        err_S = float(np.abs(got_S - S).max() / np.abs(S).max())
        err_loss = abs(out.loss - loss) / max(1.0, abs(loss))
        errs = Hp.per_tensor_err(spec, m.get_grads(), gref)
        print('boundary loss %s generic=%d bw=%g full=%d: loss %.9g ref %.9g (err %.2e) S %s err %.2e grads worst %.2e' % (
            shape, force_generic, bw, full, out.loss, loss, err_loss, S, err_S, max(errs.values())))
        got_phi = m.boundary_distance(B)
        assert np.array_equal(got_phi.view(np.uint32), phi.view(np.uint32))
        assert not got_phi[0].any() and got_S[0] == 0.0          # no lesion (or nothing else): the term vanishes
        assert np.abs(got_S - S).max() <= 1e-6 * np.abs(S).max() and np.all(np.abs(got_S - S) <= 1e-6 * np.maximum(np.abs(S), 1.0))
        assert np.all(np.abs(got - sums) <= 1e-6 * np.maximum(np.abs(sums), 1.0))
        assert err_loss <= 1e-4
        Hp.assert_grads_per_tensor_nofixture(spec, m.get_grads(), gref, 2e-5)
    finally:
        m.close()


@pytest.mark.parametrize('bw', [0.01, 1.0])
@pytest.mark.parametrize('force_generic', [False, True])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_train_step_matches_the_reference(gpu, shape, force_generic, bw):
    """launch names, loss, every gradient tensor, S_b and the map of one train step; fused head kernels and from-logits arm"""
    _check_step(gpu, shape, dict(REGION, boundary_weight=bw), force_generic)


@pytest.mark.parametrize('force_generic', [False, True])
def test_an_all_foreground_image(gpu, force_generic):
    """image 0 all foreground: no background pixel in the plane, phi = 0 on it"""
    _check_step(gpu, 'c64', dict(REGION, boundary_weight=1.0), force_generic, full=True)


@pytest.mark.parametrize('force_generic', [False, True])
def test_under_label_smoothing_the_map_comes_from_the_raw_label(gpu, force_generic):
    """the blurred label feeds the cross-entropy and Tversky terms, the raw one the map (the reference does the same)"""
    _check_step(gpu, 'c3', dict(SMOOTHED, boundary_weight=1.0), force_generic)
    blurred = R.loss_labels(_batch('c3')[1], SMOOTHED).astype(np.float32)
    assert not np.array_equal(BO.signed_distance(blurred)[0], _reference('c3', dict(SMOOTHED, boundary_weight=1.0))[4])


@pytest.mark.parametrize('force_generic', [False, True])
def test_eval_step_carries_the_term(gpu, force_generic):
    x, y = _batch('c3')
    cfg = dict(REGION, boundary_weight=1.0)
    loss, _, S, _, phi = _reference('c3', cfg, training=False)
    m = _model(gpu, 'c3', force_generic, cfg=REGION)
    try:
        lc = m.loss_cfg(**REGION)
        dice, prob_dice = m.eval_step(x, y, lc, return_prob=True)
        m.set_boundary_loss(1.0)
        assert _loss_names(_names(m, 'eval')) == list(TRANSFORM + LOGITS_ARM)
        out, prob = m.eval_step(x, y, lc, return_prob=True)
        got_S = m.boundary_loss_sums(B)
        print('boundary loss eval generic=%d: loss %.9g ref %.9g dice-only %.9g S err %.2e' % (
            force_generic, out.loss, loss, dice.loss, float(np.abs(got_S - S).max() / np.abs(S).max())))
        assert abs(out.loss - loss) <= 1e-4 * max(1.0, abs(loss))
        assert abs(out.loss - dice.loss) > 1e-3
        assert np.array_equal(prob.view(np.uint32), prob_dice.view(np.uint32))
        assert np.abs(got_S - S).max() <= 1e-6 * np.abs(S).max()
        assert np.array_equal(m.boundary_distance(B).view(np.uint32), phi.view(np.uint32))
    finally:
        m.close()


def test_three_adam_steps(gpu):
    """three train steps at lr = 1e-3 on three batches of the dense 16-channel shape, step by step as
    tests/test_region_loss_gpu.py::test_three_adam_steps: before each step the reference takes the device's weights and BatchNorm
    state, and the step's loss and every gradient tensor are held to the one-step bounds"""
    shape, lr = 'c16', 1e-3
    spec = _spec(shape)
    cfg = dict(REGION, boundary_weight=1.0)
    m = _model(gpu, shape, cfg=REGION, boundary=1.0)
    try:
        lc = m.loss_cfg(**REGION)
        start = m.get_params().copy()
        for k in range(1, 4):
            x, y = _batch(shape, seed=7 + k)
            at = dict(_params(shape))
            O.unflatten(spec, m.get_params().astype(np.float64), into=at)
            O.unflatten(spec, m.get_state().astype(np.float64), trainable=False, into=at)
            loss_k, g_k, logits, _ = BO.loss_and_grads(spec, at, x.astype(np.float64), y, cfg, training=True)
            out = m.train_step(x, y, lr, lc)
            S = BO.boundary_sums(y, logits)
            print('boundary loss %s step %d: loss %.9g ref at the device weights %.9g' % (shape, k, out.loss, loss_k))
            assert abs(out.loss - loss_k) <= 1e-4 * max(1.0, abs(loss_k))
            Hp.assert_grads_per_tensor_nofixture(spec, m.get_grads(), O.flatten(spec, g_k), 2e-5, what='step %d gradient' % k)
            assert np.abs(m.boundary_loss_sums(B) - S).max() <= 1e-6 * np.abs(S).max()
            assert m.get_opt_state()[2] == k
        assert np.abs(m.get_params() - start).max() > 0.5 * lr
    finally:
        m.close()


@pytest.mark.parametrize('shape', ['c16', 'c64'])
def test_switching_off_restores_the_dice_only_step(gpu, shape):
    """dense plans (no float atomics): with the term off again, plan, loss and gradients are those of a model that only ever had the
    region loss, bit for bit; set_region_loss(None) clears the term with it; setting a region loss again keeps it"""
    x, y = _batch(shape)
    dice = _model(gpu, shape, cfg=REGION)
    never = _model(gpu, shape)
    m = _model(gpu, shape, cfg=REGION, boundary=1.0)
    try:
        lc = m.loss_cfg(**REGION)
        dice_plan = dice.plan(variants=True, batch=B)
        assert not any('boundary' in r[0] or r[0].endswith('#bd') for r in dice_plan)
        with_plan = m.plan(variants=True, batch=B)
        assert [r[0] for r in with_plan if 'region' in r[0]] == [r[0] + '#bd' for r in dice_plan if 'region' in r[0]]
        want = dice.train_step(x, y, 0.0, lc)
        g_want = dice.get_grads().copy()
        on = m.train_step(x, y, 0.0, lc)
        S = m.boundary_loss_sums(B)
        assert abs((on.loss - want.loss) - float(S.sum()) / (B * y.shape[1] * y.shape[2])) <= 1e-5 * max(1.0, abs(on.loss))
        assert abs(on.loss - want.loss) > 1e-3
        # setting a region loss again keeps the term
        m.set_region_loss({k: v for k, v in REGION.items() if k in R.REGION_KEYS})
        assert m.plan(variants=True, batch=B) == with_plan
        with pytest.raises(Exception):
            m.boundary_loss_sums(B)                              # ... but a new step has to run first
        # off: the Dice-only step
        m.set_boundary_loss(0.0)
        assert m.plan(variants=True, batch=B) == dice_plan
        for mode in ('eval', 'forward'):
            assert m.plan(variants=True, mode=mode, batch=B) == dice.plan(variants=True, mode=mode, batch=B)
        off = m.train_step(x, y, 0.0, lc)
        assert np.float32(off.loss).view(np.uint32) == np.float32(want.loss).view(np.uint32)
        assert np.array_equal(m.get_grads().view(np.uint32), g_want.view(np.uint32))
        with pytest.raises(Exception):
            m.boundary_loss_sums(B)
        # set_region_loss(None) clears it: the plain plan, and a region loss set later comes without the term
        m.set_boundary_loss(1.0)
        m.set_region_loss(None)
        assert m.plan(variants=True, batch=B) == never.plan(variants=True, batch=B)
        m.set_region_loss({})
        assert m.plan(variants=True, batch=B) == dice_plan
    finally:
        m.close()
        dice.close()
        never.close()


def test_the_library_checks_the_value(gpu):
    """DNNCA_EINVAL with nothing changed: without a region loss, and for a negative or non-finite weight"""
    x, y = _batch('c64')
    m = _model(gpu, 'c64')
    try:
        lc = m.loss_cfg(**REGION)
        plain_plan = m.plan(variants=True, batch=B)
        for w in (0.5, 0.0):
            with pytest.raises(gpu._lib.DnncaError) as e:
                m.set_boundary_loss(w)
            assert e.value.code == -1          # DNNCA_EINVAL
        assert m.plan(variants=True, batch=B) == plain_plan
        with pytest.raises(gpu._lib.DnncaError):
            m.boundary_distance(B)
        m.set_region_loss({})
        m.set_boundary_loss(0.5)
        plan = m.plan(variants=True, batch=B)
        before = m.train_step(x, y, 0.0, lc)
        for bad in (-0.5, float('nan'), float('inf'), float('-inf')):
            with pytest.raises(gpu._lib.DnncaError) as e:
                m.set_boundary_loss(bad)
            assert e.value.code == -1          # DNNCA_EINVAL
        assert m.plan(variants=True, batch=B) == plan
        m.boundary_loss_sums(B)                                   # a refused call leaves the last step's results readable
        after = m.train_step(x, y, 0.0, lc)
        assert np.float32(after.loss).view(np.uint32) == np.float32(before.loss).view(np.uint32)
        with pytest.raises(gpu._lib.DnncaError):
            m.boundary_loss_sums(MAXB)                            # the step ran on B images
    finally:
        m.close()


def test_determinism_and_the_map_of_a_step_is_its_own(gpu):
    """the same step twice on a dense plan: loss, gradients, S_b and the map bit-identical; signed_distance_of in between leaves the
    step's map alone"""
    x, y = _batch('c16')
    m = _model(gpu, 'c16', cfg=REGION, boundary=1.0)
    try:
        lc = m.loss_cfg(**REGION)
        runs = []
        for _ in range(2):
            out = m.train_step(x, y, 0.0, lc)
            runs.append((np.float32(out.loss).view(np.uint32), m.get_grads().copy(), m.boundary_loss_sums(B).view(np.uint64),
                         m.boundary_distance(B).view(np.uint32)))
            other = m.signed_distance_of(np.ones((2, 9, 31), np.float32) * (np.arange(31) % 5 == 0))
            assert other.shape == (2, 9, 31) and other.any()
            assert np.array_equal(m.boundary_distance(B).view(np.uint32), runs[-1][3])
        assert runs[0][0] == runs[1][0]
        for a, b in zip(runs[0][1:], runs[1][1:]):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    finally:
        m.close()


def test_engine_trains_with_the_boundary_config_on_a_dense_plan(gpu, monkeypatch):
    """configs/additionals/boundary_loss.yaml through engine.train on the 64-filter plan at the engine's learning rate (1e-3): three
    steps through the feeder and the staged steps log bit for bit the losses of the same batches stepped directly on a DeviceModel
    and leave its weights bit for bit; engine._evaluate reports the direct eval_steps"""
    from dnncancerannotator_amd import data, engine, load
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    unet = dict(SHAPES['c64'][2])
    config = {'model': 'UNetAnnotator', 'model_options': unet,
              'deploy_options': {'optimizer': 'adam', 'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}},
                                 'enable_multigpu': False, 'metrics': []}}
    config = load._apply_config(config, load._load_config_single(os.path.join(root, 'configs', 'additionals', 'boundary_loss.yaml')))
    assert config['deploy_options']['loss']['class_name'] == 'BoundaryCrossentropy'
    monkeypatch.delenv('DNNCA_NO_FEEDER', raising=False)
    H, W = SHAPES['c64'][3:5]
    xs = np.concatenate([_batch('c64', seed=8 + k)[0] for k in range(3)])
    ys = np.concatenate([_batch('c64', seed=8 + k)[1] for k in range(3)])
    ds = lambda: data.ArrayDataset(xs, ys, B, repeat=True)        # noqa: E731
    m = engine.TFKerasModel(config)
    hist = m.train(ds(), max_steps=3).history['loss']
    assert _loss_names([r[0] for r in m.device_model.plan()]) == list(TRANSFORM) + ['head_region_fwd_64', 'region_loss_finish', 'head_region_train_64']
    direct = gpu.DeviceModel('unet', 1, H, W, B, **unet)
    dice = gpu.DeviceModel('unet', 1, H, W, B, **unet)
    try:
        for d in (direct, dice):
            d.init_glorot(0)
            d.set_adam(**m.adam)
            d.set_region_loss({})
        direct.set_boundary_loss(0.01)
        cfg = direct.loss_cfg(weight_mul=3.0)
        first = next(iter(ds()))
        assert abs(dice.train_step(np.asarray(first[0]), np.asarray(first[1]), 0.001, cfg).loss - hist[0]) > 1e-4
        want = [direct.train_step(np.asarray(x), np.asarray(y), 0.001, cfg).loss for _, (x, y) in zip(range(3), ds())]
        print('boundary loss engine dense: %s direct %s' % (hist, want))
        assert np.array_equal(np.asarray(hist, np.float32).view(np.uint32), np.asarray(want, np.float32).view(np.uint32))
        assert np.array_equal(direct.get_params().view(np.uint32), m.device_model.get_params().view(np.uint32))
        ev = lambda: data.ArrayDataset(xs[:2 * B], ys[:2 * B], B)     # noqa: E731
        each = [direct.eval_step(np.asarray(x), np.asarray(y), cfg).loss for x, y in ev()]
        for staged in (False, True):
            res = m._evaluate(ev(), staged=staged)
            assert abs(res['loss'] - float(np.mean(each))) <= 1e-6 * max(1.0, abs(float(np.mean(each)))), (staged, res['loss'], each)
    finally:
        direct.close()
        dice.close()
