"""-m gpu: the region (Tversky / Dice) term of the loss (DeviceModel.set_region_loss) against the float64 reference of
tests/region_loss_ref.py: the fused head kernels of 3, 16 and 64 channels, the from-logits arm (force_generic, eval_step, a head
of 8 channels at an odd pixel count), the parameter sweep, three Adam steps, determinism, switching off, the per-step metrics,
many blocks per image, and the engine on the 3-channel plan (lr 0) and on a dense one (lr 1e-3, bit for bit).

Shared setup: B = 3 images on a model of max_batch = 4 (a ragged batch), image 0 without positives, image 2 with a lesion that
touches two borders, weights from helpers.perturbed_params.  Bounds: loss 1e-4 max(1, |loss|) and gradients 2e-5 per tensor, those
of test_label_smoothing_loss_matches_oracle; region_loss_sums() to 1e-6 relative (double sums of float32 sigmoids).

Measured on an MI355X, one train step: loss error 4e-10 .. 3.7e-7 relative; region_loss_sums() 2.2e-9 (c3), 4.5e-9 (c64), 6.2e-8
(c16) relative -- the float32 network's logits, not the double sums, decide it, so the bound stays 1e-6; worst gradient tensor
4e-7 .. 1.4e-6 of its scale on unet (mulmo: 2e-5 holds for every tensor but the analytically zero ones, see _check_step)."""

import numpy as np
import pytest

import helpers as Hp
import region_loss_ref as R
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

COMMON = dict(rate=2, kernel_size=3, conv_stride=1, padding='same')
# name -> (arch, in_channels, options, H, W, the launches of the tuned plan that carry the head)
SHAPES = {
    # 960 pixels per image: not a multiple of the 1024 a block of the 3-channel kernels takes per trip
    'c3': ('unet', 1, dict(n_filters_first=3, n_downsample=3, bn=False, **COMMON), 40, 24, ('head_region_fwd_3', 'head_region_train_3')),
    # 240 pixels: not a multiple of the 64 a wave of the 16-channel kernels takes per trip
    'c16': ('mulmo', 3, dict(n_filters_first=16, n_downsample=2, bn=True, **COMMON), 12, 20, ('head_region_fwd_16', 'head_region_train_16')),
    # 140 pixels: not a multiple of the 16 of the 64-channel kernels
    'c64': ('unet', 1, dict(n_filters_first=64, n_downsample=1, bn=False, **COMMON), 10, 14, ('head_region_fwd_64', 'head_region_train_64')),
}
B, MAXB = 3, 4
LOGITS_ARM = ('region_sums', 'region_loss_finish', 'region_loss_grad')
DEFAULT = dict(weight_mul=3.0)
SWEEP = {
    'tversky_smoothed': dict(weight_mul=3.0, alpha=0.3, beta=0.7, smooth=0.1, label_smoothing=True, label_smoothing_filter_size=6,
                             label_smoothing_sigma=3),
    'pure_tversky': dict(weight_mul=3.0, alpha=0.3, beta=0.7, smooth=0.1, crossentropy_weight=0.0),
    'explicit_weight': dict(weight=5.0, region_weight=2.0, crossentropy_weight=0.5),
}

_cache = {}


def _batch(shape, seed=8):
    arch, C, opts, H, W, _ = SHAPES[shape]
    key = ('batch', shape, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        x = rng.random((B, H, W, C)).astype(np.float32)
        y = np.zeros((B, H, W), np.float32)
        y[1, H // 4:H // 2, W // 4:W // 2 + 2] = 1.0
        y[2, H - H // 4:H, 0:W // 4] = 1.0                    # touches two borders
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


def _reference(shape, cfg, training=True):
    """(loss, flat gradients, logits, I/P/Y sums) of the float64 reference, computed once per (shape, cfg)"""
    key = ('ref', shape, tuple(sorted(cfg.items())), training)
    if key not in _cache:
        x, y = _batch(shape)
        spec = _spec(shape)
        loss, grads, logits, _ = R.loss_and_grads(spec, _params(shape), x.astype(np.float64), y, cfg, training=training)
        sums = R.region_sums(R.loss_labels(y, cfg), logits)
        _cache[key] = (loss, O.flatten(spec, grads), np.asarray(logits, np.float64), sums)
    return _cache[key]


def _model(gpu, shape, force_generic=False, region=None):
    arch, C, opts, H, W, _ = SHAPES[shape]
    spec = _spec(shape)
    m = gpu.DeviceModel(arch, C, H, W, MAXB, force_generic=force_generic, **opts)
    m.set_params(O.flatten(spec, _params(shape)))
    if m.n_state:
        m.set_state(O.flatten(spec, _params(shape), trainable=False))
    if region is not None:
        m.set_region_loss({k: v for k, v in region.items() if k in R.REGION_KEYS})
    return m


def _names(m, mode='train'):
    return [r[0] for r in m.plan(mode=mode, batch=B)]


def _check_step(gpu, shape, cfg, force_generic):
    x, y = _batch(shape)
    spec = _spec(shape)
    loss, gref, _, sums = _reference(shape, cfg)
    m = _model(gpu, shape, force_generic, region=cfg)
    try:
        names = _names(m)
        want = LOGITS_ARM if force_generic else SHAPES[shape][5][:1] + ('region_loss_finish',) + SHAPES[shape][5][1:]
        assert [n for n in names if 'region' in n] == list(want), names
        assert not any(n.startswith(('tail3', 'pgfwd_head', 'head_train', 'g_loss')) for n in names), names
        out = m.train_step(x, y, 0.0, m.loss_cfg(**R.split_cfg(cfg)[0]))
        got = m.region_loss_sums(B)
        err_sums = float(np.abs(got - sums).max() / np.abs(sums).max())
        err_loss = abs(out.loss - loss) / max(1.0, abs(loss))
        errs = Hp.per_tensor_err(spec, m.get_grads(), gref)
        print('region loss %s generic=%d: loss %.9g ref %.9g (err %.2e) sums err %.2e grads worst %.2e' % (
            shape, force_generic, out.loss, loss, err_loss, err_sums, max(errs.values())))
        assert np.abs(got - sums).max() <= 1e-6 * np.abs(sums).max() and np.all(np.abs(got - sums) <= 1e-6 * np.maximum(np.abs(sums), 1.0))
        assert err_loss <= 1e-4
        # (the nofixture form: the variables whose gradient is analytically zero -- the last BatchNorm of the mulmo encoders whose
        # skips are unused, a transposed-conv bias in front of a BatchNorm -- are float32 noise in any implementation and are held
        # to the same 2e-5 of a healthy sibling's scale; every other tensor exactly as assert_grads_per_tensor(..., 2e-5))
        Hp.assert_grads_per_tensor_nofixture(spec, m.get_grads(), gref, 2e-5)
    finally:
        m.close()


@pytest.mark.parametrize('force_generic', [False, True])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_train_step_matches_the_reference(gpu, shape, force_generic):
    """loss, every gradient tensor and the per-image sums I, P, Y of one train step, fused head kernels and from-logits arm"""
    _check_step(gpu, shape, dict(DEFAULT), force_generic)


@pytest.mark.parametrize('force_generic', [False, True])
@pytest.mark.parametrize('name', list(SWEEP))
def test_parameter_sweep(gpu, name, force_generic):
    """alpha = 0.3, beta = 0.7, smooth = 0.1 under label smoothing; crossentropy_weight = 0 (pure Tversky); an explicit weight"""
    _check_step(gpu, 'c3', SWEEP[name], force_generic)


@pytest.mark.parametrize('shape', list(SHAPES))
def test_it_is_not_a_no_op_and_switching_off_restores_the_plain_step(gpu, shape):
    """with the region term the loss differs from the plain loss by more than 1e-3; after set_region_loss(None) plan, loss and
    gradients are those of a model that never had it: bit for bit on the dense plans (c16, c64), whose backward pass has no float
    atomics; on the 3-channel plan the head's tensors bit for bit and the rest within its own run-to-run noise (test_determinism)"""
    x, y = _batch(shape)
    never = _model(gpu, shape)
    m = _model(gpu, shape, region=DEFAULT)
    try:
        cfg = m.loss_cfg(**DEFAULT)
        plain_plan = never.plan(variants=True, batch=B)
        assert m.plan(variants=True, batch=B) != plain_plan
        plain = never.train_step(x, y, 0.0, cfg)
        g_plain = never.get_grads().copy()
        with_region = m.train_step(x, y, 0.0, cfg)
        assert abs(with_region.loss - plain.loss) > 1e-3
        t = R.tversky_index(m.region_loss_sums(B), 0.5, 0.5, 1.0)
        assert abs((with_region.loss - plain.loss) - float(np.mean(1.0 - t))) <= 1e-5
        m.set_region_loss(None)
        assert m.plan(variants=True, batch=B) == plain_plan
        for mode in ('eval', 'forward'):
            assert m.plan(variants=True, mode=mode, batch=B) == never.plan(variants=True, mode=mode, batch=B)
        off = m.train_step(x, y, 0.0, cfg)
        g_off = m.get_grads().copy()
        assert np.float32(off.loss).view(np.uint32) == np.float32(plain.loss).view(np.uint32)
        # the launches are the plain step's again (the plans above), and so are the head's tensors, bit for bit; the conv weight
        # gradients of this plan go through float atomics (test_determinism): they are held to four times what two steps of the
        # never-set model differ by
        never.train_step(x, y, 0.0, cfg)
        g_again = never.get_grads()
        ndiff = int((g_off.view(np.uint32) != g_plain.view(np.uint32)).sum())
        print('region loss %s switched off: %d of %d gradient words differ from the never-set model' % (shape, ndiff, g_off.size))
        if shape != 'c3':
            assert ndiff == 0
        for n, sl in Hp.tensor_slices(_spec(shape)):
            if n.startswith('head.'):
                assert np.array_equal(g_off[sl].view(np.uint32), g_plain[sl].view(np.uint32)), n
            noise = np.abs(g_again[sl].astype(np.float64) - g_plain[sl]).max()
            assert np.abs(g_off[sl].astype(np.float64) - g_plain[sl]).max() <= 4 * noise + 1e-6 * np.abs(g_plain[sl]).max(), n
        with pytest.raises(Exception):
            m.region_loss_sums(B)
    finally:
        m.close()
        never.close()


def test_the_library_checks_the_values(gpu):
    m = _model(gpu, 'c3')
    try:
        for bad in (dict(region_weight=0.0), dict(crossentropy_weight=-1.0), dict(alpha=-0.1), dict(alpha=0.0, beta=0.0), dict(smooth=0.0),
                    dict(smooth=float('nan'))):
            with pytest.raises(gpu._lib.DnncaError):
                m.set_region_loss(bad)
        with pytest.raises(ValueError):
            m.set_region_loss(gamma=1.0)
        assert 'g_loss' not in _names(m) and not any('region' in n for n in _names(m))       # a refused call leaves it off
    finally:
        m.close()
    arch, C, opts, H, W, _ = SHAPES['c64']
    bf = gpu.DeviceModel(arch, C, H, W, MAXB, dtype='bf16', **opts)
    try:
        with pytest.raises(gpu._lib.DnncaError, match='f32'):
            bf.set_region_loss({})
        bf.set_region_loss(None)                 # switching off is always allowed
    finally:
        bf.close()


@pytest.mark.parametrize('force_generic', [False, True])
def test_eval_step(gpu, force_generic):
    """eval_step with the region loss: the loss against the reference (inference forward), the probabilities bit-equal to those of
    eval_step without it"""
    x, y = _batch('c3')
    loss, _, logits, sums = _reference('c3', DEFAULT, training=False)
    m = _model(gpu, 'c3', force_generic)
    try:
        cfg = m.loss_cfg(**DEFAULT)
        plain, prob_plain = m.eval_step(x, y, cfg, return_prob=True)
        m.set_region_loss({})                    # the defaults: 1, 1, 0.5, 0.5, 1
        assert [n for n in _names(m, 'eval') if 'region' in n or n == 'g_loss'] == list(LOGITS_ARM)
        out, prob = m.eval_step(x, y, cfg, return_prob=True)
        print('region loss eval generic=%d: loss %.9g ref %.9g plain %.9g' % (force_generic, out.loss, loss, plain.loss))
        assert abs(out.loss - loss) <= 1e-4 * max(1.0, abs(loss))
        assert np.array_equal(prob.view(np.uint32), prob_plain.view(np.uint32))
        assert np.abs(prob[..., 0] - 1.0 / (1.0 + np.exp(-logits[..., 0]))).max() <= 1e-4
        got = m.region_loss_sums(B)
        assert np.abs(got - sums).max() <= 1e-6 * np.abs(sums).max()
    finally:
        m.close()


@pytest.mark.parametrize('shape', ['c3', 'c16'])
def test_three_adam_steps(gpu, shape):
    """three train steps at lr = 1e-3 on three batches against the reference's Adam recurrence, in two parts.

    Free running: the three losses against R.train_steps from the same start, each within the one-step bound.

    Step by step, so that a weight whose near-zero gradient takes the other sign (a full step of 2 lr apart, in any float32
    implementation) cannot blur the later steps: before each step the reference takes the device's weights and BatchNorm state,
    and the step's loss and every gradient tensor are held to the one-step bounds (1e-4, 2e-5) -- the head's gradient under the
    new loss at steps 2 and 3 included.  The optimizer is then held to the bounds of
    tests/test_parity_gpu.py::test_adam_kernel_with_history: O.adam_step on the device's own gradients, carried over the three
    steps in float64, gives the weight update to 1e-5 lr + 1.5e-7 and the slots m, v to 1e-6 of their largest entry."""
    spec = _spec(shape)
    lr = 1e-3
    batches = [_batch(shape, seed=8 + k) for k in range(3)]
    key = ('adam', shape)
    if key not in _cache:
        _cache[key] = R.train_steps(spec, dict(_params(shape)), [(x.astype(np.float64), y) for x, y in batches], lr, DEFAULT)
    losses, _, _ = _cache[key]
    m = _model(gpu, shape, region=DEFAULT)
    try:
        cfg = m.loss_cfg(**DEFAULT)
        got, mm, vv = [], {}, {}
        for k, (x, y) in enumerate(batches, 1):
            p_before = m.get_params().astype(np.float64)
            at = dict(_params(shape))
            O.unflatten(spec, p_before, into=at)
            if m.n_state:
                O.unflatten(spec, m.get_state().astype(np.float64), trainable=False, into=at)
            loss_k, g_k, _, _ = R.loss_and_grads(spec, at, x.astype(np.float64), y, DEFAULT, training=True)
            out = m.train_step(x, y, lr, cfg)
            got.append(out.loss)
            g_dev = m.get_grads().astype(np.float64)
            errs = Hp.per_tensor_err(spec, g_dev, O.flatten(spec, g_k))
            print('region loss %s step %d: loss %.9g ref at the device weights %.9g free-running ref %.9g, head grads %.2e %.2e' % (
                shape, k, out.loss, loss_k, losses[k - 1], errs['head.kernel'], errs['head.bias']))
            assert abs(out.loss - loss_k) <= 1e-4 * max(1.0, abs(loss_k))
            Hp.assert_grads_per_tensor_nofixture(spec, g_dev, O.flatten(spec, g_k), 2e-5, what='step %d gradient' % k)
            # (the betas the device holds are float32: 1 - float32(0.999) is 1.3e-5 off 1e-3, which a v that starts at zero
            # shows in full -- test_adam_kernel_with_history starts from slots that hide it)
            new = O.adam_step(O.unflatten(spec, p_before), O.unflatten(spec, g_dev), mm, vv, k, lr,
                              beta1=float(np.float32(0.9)), beta2=float(np.float32(0.999)))
            want = O.flatten(spec, new)
            m1, v1, it = m.get_opt_state()
            assert it == k
            assert np.abs((m.get_params() - p_before) - (want - p_before)).max() <= 1e-5 * lr + 1.5e-7
            assert np.abs(m1 - O.flatten(spec, mm)).max() <= 1e-6 * np.abs(O.flatten(spec, mm)).max()
            assert np.abs(v1 - O.flatten(spec, vv)).max() <= 1e-6 * np.abs(O.flatten(spec, vv)).max()
        for a, b in zip(got, losses):
            assert abs(a - b) <= 1e-4 * max(1.0, abs(b))
        moved = np.abs(m.get_params() - O.flatten(spec, _params(shape)))
        assert moved.max() > 0.5 * lr
    finally:
        m.close()


@pytest.mark.parametrize('shape', list(SHAPES))
def test_determinism(gpu, shape):
    """the same step twice from the same state: loss, region_loss_sums() and everything the new kernels produce -- the head's
    gradient tensors, and through dfeat every other one -- bit-identical.

    The dense plans (c16, c64) have no float atomics behind the head: the whole gradient vector is bit-identical.  The 3-channel
    plan sums its conv weight gradients with float atomics (tests/test_train_metrics_gpu.py: "two off steps differ in their last
    bits"), with the plain loss as well: measured here on an MI355X, 1520 of 8686 gradient words differ between two region-loss
    steps and 1551 between two plain steps of the same model (0 and 0 of 99313 / 164801 on c16 / c64).  There the head's own
    tensors are bit-identical and the rest is held to that file's rule, four times the run-to-run difference of two plain steps."""
    x, y = _batch(shape)
    spec = _spec(shape)
    m = _model(gpu, shape, region=DEFAULT)
    try:
        cfg = m.loss_cfg(**DEFAULT)

        def twice():
            runs = []
            for _ in range(2):
                out = m.train_step(x, y, 0.0, cfg)
                runs.append((np.float32(out.loss).view(np.uint32), m.get_grads().copy()))
            return runs
        runs = twice()
        sums = [m.region_loss_sums(B).view(np.uint64)]
        m.train_step(x, y, 0.0, cfg)
        sums.append(m.region_loss_sums(B).view(np.uint64))
        m.set_region_loss(None)
        plain = twice()
        ndiff = int((runs[0][1].view(np.uint32) != runs[1][1].view(np.uint32)).sum())
        ndiff_plain = int((plain[0][1].view(np.uint32) != plain[1][1].view(np.uint32)).sum())
        print('region loss %s determinism: %d of %d gradient words differ (plain loss: %d)' % (shape, ndiff, runs[0][1].size, ndiff_plain))
        assert runs[0][0] == runs[1][0]
        assert np.array_equal(sums[0], sums[1])
        head = [sl for n, sl in Hp.tensor_slices(spec) if n.startswith('head.')]
        assert len(head) == 2
        for sl in head:
            assert np.array_equal(runs[0][1][sl].view(np.uint32), runs[1][1][sl].view(np.uint32))
        if shape != 'c3':
            assert ndiff == 0
        else:
            d, dp = np.abs(runs[0][1] - runs[1][1]).astype(np.float64), np.abs(plain[0][1] - plain[1][1]).astype(np.float64)
            for n, sl in Hp.tensor_slices(spec):
                assert d[sl].max() <= 4 * dp[sl].max() + 1e-6 * np.abs(runs[0][1][sl]).max(), n
    finally:
        m.close()


def test_multiresunet_goes_through_the_logits_arm(gpu):
    """MultiResUnet's head gradient enters the backward pass through the f32 dlogits buffer (its head BatchNorm's output
    gradient), so the from-logits arm serves it: the launches, the loss against the plain loss plus mean (1 - T) of the step's own
    sums, the sums against the step's own probabilities, and a gradient that the region term really changes"""
    Bm, H, W = 2, 32, 32
    m = gpu.DeviceModel('multires', 5, H, W, Bm, 4, 4, bn=True, padding='same')
    try:
        m.init_glorot(seed=3)
        rng = np.random.default_rng(4)
        x = rng.standard_normal((Bm, H, W, 5)).astype(np.float32)
        y = np.zeros((Bm, H, W), np.float32)
        y[1, 20:32, 0:9] = 1.0
        cfg = m.loss_cfg(weight_mul=3.0)
        plain = m.train_step(x, y, 0.0, cfg)          # lr 0: the training-mode forward of the next step is the same
        g_plain = m.get_grads().astype(np.float64)
        m.set_region_loss(alpha=0.3, beta=0.7)
        assert [n for n in [r[0] for r in m.plan()] if 'region' in n or n == 'g_loss'] == list(LOGITS_ARM)
        out = m.train_step(x, y, 0.0, cfg)
        sums = m.region_loss_sums(Bm)
        prob = m.last_prob(Bm).astype(np.float64)
        want = np.stack([(prob * y).sum((1, 2)), prob.sum((1, 2)), y.astype(np.float64).sum((1, 2))], 1)
        assert np.all(np.abs(sums - want) <= 1e-6 * np.maximum(np.abs(want), 1.0))
        t = R.tversky_index(sums, 0.3, 0.7, 1.0)
        assert abs((out.loss - plain.loss) - float(np.mean(1.0 - t))) <= 1e-5 * max(1.0, abs(out.loss))
        g = m.get_grads().astype(np.float64)
        assert np.isfinite(g).all() and np.abs(g - g_plain).max() > 1e-3 * np.abs(g_plain).max()
    finally:
        m.close()


def test_train_metrics_counts(gpu):
    """train_metrics on: the step's pixel counts equal those computed from the reference probabilities"""
    x, y = _batch('c3')
    _, _, logits, _ = _reference('c3', DEFAULT)
    ref = 1.0 / (1.0 + np.exp(-logits[..., 0]))
    thr = np.array([0.3, 0.5, 0.7], np.float32)
    assert np.abs(ref[..., None] - thr).min() > 1e-4            # no pixel so near a threshold that float32 may decide otherwise
    for force_generic in (False, True):
        m = _model(gpu, 'c3', force_generic, region=DEFAULT)
        try:
            m.train_metrics(thr)
            m.train_step(x, y, 0.0, m.loss_cfg(**DEFAULT))
            counts = np.asarray(m.last_step_confusion(), np.float64)
            prob = m.last_prob(B)
            assert np.abs(prob - ref).max() <= 1e-4
            pos = y > 0.5
            want = [[(ref[pos] > t).sum(), (ref[~pos] > t).sum(), (ref[pos] <= t).sum(), (ref[~pos] <= t).sum()] for t in thr]
            assert np.array_equal(counts, np.asarray(want, np.float64))
            assert counts[0, 0] + counts[0, 2] == pos.sum() and counts[1].sum() == B * y.shape[1] * y.shape[2]
        finally:
            m.close()


def test_engine_trains_and_evaluates_with_dice(gpu, monkeypatch):
    """three steps of engine.train with DiceCrossentropy through the feeder and the staged steps log bit for bit the losses of the
    same batches stepped directly on a DeviceModel; engine._evaluate reports the loss of the direct eval_steps.  Learning rate 0, as in
    tests/test_train_metrics_gpu.py (fixed weights: exact comparisons -- the weight gradients of this plan carry float-atomics noise
    from run to run, which a later step's loss would inherit)"""
    from dnncancerannotator_amd import data, engine
    unet = dict(SHAPES['c3'][2])
    loss_cfg = {'weight_mul': 3.0, 'smooth': 0.5}
    config = {'model': 'UNetAnnotator', 'model_options': unet,
              'deploy_options': {'optimizer': 'adam', 'LearningRateScheduler': 'lambda epoch, current_lr: 0.0',
                                 'loss': {'class_name': 'DiceCrossentropy', 'config': loss_cfg},
                                 'enable_multigpu': False, 'metrics': []}}
    monkeypatch.delenv('DNNCA_NO_FEEDER', raising=False)
    ds = lambda: data.SyntheticDataset(4, 64, 64, 1, n_batches=3, seed=5)        # noqa: E731
    m = engine.TFKerasModel(config)
    hist = m.train(ds(), max_steps=3).history['loss']
    assert getattr(m.device_model, '_ring', None) is not None
    assert any('head_region_train_3' == r[0] for r in m.device_model.plan())
    direct = gpu.DeviceModel('unet', 1, 64, 64, 4, **unet)
    try:
        direct.init_glorot(0)
        direct.set_adam(**m.adam)
        direct.set_region_loss(smooth=0.5)
        cfg = direct.loss_cfg(weight_mul=3.0)
        want = [direct.train_step(np.asarray(x), np.asarray(y), 0.0, cfg).loss for _, (x, y) in zip(range(3), ds())]
        print('region loss engine: %s direct %s' % (hist, want))
        assert np.array_equal(np.asarray(hist, np.float32).view(np.uint32), np.asarray(want, np.float32).view(np.uint32))
        ev = lambda: data.SyntheticDataset(4, 64, 64, 1, n_batches=2, seed=11, repeat=False)     # noqa: E731
        each = [direct.eval_step(np.asarray(x), np.asarray(y), cfg).loss for x, y in ev()]
        plain = gpu.DeviceModel('unet', 1, 64, 64, 4, **unet)
        plain.set_params(direct.get_params())
        assert abs(plain.eval_step(*[np.asarray(a) for a in next(iter(ev()))], cfg).loss - each[0]) > 1e-3
        plain.close()
        for staged in (False, True):
            res = m._evaluate(ev(), staged=staged)
            assert abs(res['loss'] - float(np.mean(each))) <= 1e-6 * max(1.0, abs(float(np.mean(each)))), (staged, res['loss'], each)
    finally:
        direct.close()


def test_engine_trains_with_dice_on_a_dense_plan(gpu, monkeypatch):
    """the same through a dense plan (unet, 64 filters), whose backward pass has no float atomics: three real training steps of
    engine.train at the engine's learning rate (1e-3), feeder and staged steps, log bit for bit the losses of the same batches
    stepped directly on a DeviceModel, and leave bit for bit its weights and Adam slots -- the weight update and the head's
    deferred reduction through the staged path included; engine._evaluate on the trained weights reports the direct eval_steps"""
    from dnncancerannotator_amd import data, engine
    unet = dict(SHAPES['c64'][2])
    config = {'model': 'UNetAnnotator', 'model_options': unet,
              'deploy_options': {'optimizer': 'adam', 'loss': {'class_name': 'TverskyCrossentropy',
                                                                'config': {'weight_mul': 3.0, 'alpha': 0.3, 'beta': 0.7}},
                                 'enable_multigpu': False, 'metrics': []}}
    monkeypatch.delenv('DNNCA_NO_FEEDER', raising=False)
    H, W = SHAPES['c64'][3:5]                    # the shape and batch test_determinism holds bit-identical, three inputs
    xs = np.concatenate([_batch('c64', seed=8 + k)[0] for k in range(3)])
    ys = np.concatenate([_batch('c64', seed=8 + k)[1] for k in range(3)])
    ds = lambda: data.ArrayDataset(xs, ys, B, repeat=True)        # noqa: E731
    m = engine.TFKerasModel(config)
    hist = m.train(ds(), max_steps=3).history['loss']
    assert getattr(m.device_model, '_ring', None) is not None
    assert any('head_region_train_64' == r[0] for r in m.device_model.plan())
    direct = gpu.DeviceModel('unet', 1, H, W, B, **unet)
    try:
        direct.init_glorot(0)
        direct.set_adam(**m.adam)
        direct.set_region_loss(alpha=0.3, beta=0.7)
        cfg = direct.loss_cfg(weight_mul=3.0)
        want = [direct.train_step(np.asarray(x), np.asarray(y), 0.001, cfg).loss for _, (x, y) in zip(range(3), ds())]
        print('region loss engine dense: %s direct %s' % (hist, want))
        assert np.array_equal(np.asarray(hist, np.float32).view(np.uint32), np.asarray(want, np.float32).view(np.uint32))
        assert len(set(want)) == 3 and want[2] != want[0]
        assert np.array_equal(direct.get_params().view(np.uint32), m.device_model.get_params().view(np.uint32))
        for a, b in zip(direct.get_opt_state()[:2], m.device_model.get_opt_state()[:2]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert direct.get_opt_state()[2] == m.device_model.get_opt_state()[2] == 3
        ev = lambda: data.ArrayDataset(xs[:2 * B], ys[:2 * B], B)     # noqa: E731
        each = [direct.eval_step(np.asarray(x), np.asarray(y), cfg).loss for x, y in ev()]
        assert len(each) == 2
        for staged in (False, True):
            res = m._evaluate(ev(), staged=staged)
            assert abs(res['loss'] - float(np.mean(each))) <= 1e-6 * max(1.0, abs(float(np.mean(each)))), (staged, res['loss'], each)
    finally:
        direct.close()


@pytest.mark.parametrize('force_generic', [False, True])
def test_head_without_a_fused_kernel_and_odd_pixel_count(gpu, force_generic):
    """8 filters (no fused head kernel: the tuned plan takes the from-logits arm too) at 9 x 15 with rate 3: 135 pixels per image,
    no multiple of 4, so region_sums / region_loss_grad run their one-pixel-per-thread form.  Bounds of the one-step cases"""
    opts = dict(n_filters_first=8, n_downsample=1, bn=False, kernel_size=3, conv_stride=1, padding='same', rate=3)
    H, W = 9, 15
    spec = O.ModelSpec('unet', 1, **opts)
    params = Hp.perturbed_params(spec, np.float64)
    rng = np.random.default_rng(12)
    x = rng.random((B, H, W, 1)).astype(np.float32)
    y = np.zeros((B, H, W), np.float32)
    y[1, 2:5, 3:9] = 1.0
    y[2, 6:9, 0:4] = 1.0
    cfg = dict(weight_mul=3.0, alpha=0.3, beta=0.7)
    loss, grads, logits, _ = R.loss_and_grads(spec, params, x.astype(np.float64), y, cfg, training=True)
    sums = R.region_sums(y, logits)
    m = gpu.DeviceModel('unet', 1, H, W, MAXB, force_generic=force_generic, **opts)
    try:
        m.set_params(O.flatten(spec, params))
        m.set_region_loss(alpha=0.3, beta=0.7)
        assert [n for n in _names(m) if 'region' in n or n == 'g_loss'] == list(LOGITS_ARM), _names(m)
        out = m.train_step(x, y, 0.0, m.loss_cfg(weight_mul=3.0))
        got = m.region_loss_sums(B)
        errs = Hp.per_tensor_err(spec, m.get_grads(), O.flatten(spec, grads))
        print('region loss c8 generic=%d: loss %.9g ref %.9g sums err %.2e grads worst %.2e' % (
            force_generic, out.loss, loss, float(np.abs(got - sums).max() / np.abs(sums).max()), max(errs.values())))
        assert np.all(np.abs(got - sums) <= 1e-6 * np.maximum(np.abs(sums), 1.0))
        assert abs(out.loss - loss) <= 1e-4 * max(1.0, abs(loss))
        Hp.assert_grads_per_tensor(spec, m.get_grads(), O.flatten(spec, grads), 2e-5)
        ev, prob = m.eval_step(x, y, m.loss_cfg(weight_mul=3.0), return_prob=True)
        assert np.abs(prob[..., 0] - 1.0 / (1.0 + np.exp(-np.asarray(logits, np.float64)[..., 0]))).max() <= 1e-4
        assert abs(ev.loss - loss) <= 1e-4 * max(1.0, abs(loss))          # no BatchNorm: the inference forward is the same
    finally:
        m.close()


def test_many_blocks_per_image(gpu):
    """4 x 1024 x 1024 on the 3-channel plan: an image wants 1024 blocks of the sums and head launches and gets 512 (the rows of
    all images share 2048), so every block makes two trips and region_loss_finish adds 512 rows per column, 8 per lane.  No
    oracle at this size: the sums against numpy on the step's own probabilities (double sums of the same float32 values: 1e-12),
    the loss against the plain loss of the same weights plus mean (1 - T) of those sums; train step (fused head kernels) and
    eval step (from the logits)"""
    arch, C, opts, _, _, launches = SHAPES['c3']
    S, Bm = 1024, 4
    from dnncancerannotator_amd.synthetic import synthetic_batch
    x, y = synthetic_batch(Bm, S, S, 1, seed_x=31, seed_y=32)
    m = gpu.DeviceModel(arch, C, S, S, Bm, **opts)
    try:
        m.init_glorot(seed=2)
        cfg = m.loss_cfg(weight_mul=3.0)
        plain_train = m.train_step(x, y, 0.0, cfg).loss
        plain_eval = m.eval_step(x, y, cfg).loss
        m.set_region_loss({})
        m.train_metrics([0.5])                   # the train step then leaves its probabilities where last_prob reads them
        assert set(launches) <= set(r[0] for r in m.plan())
        y64 = y.astype(np.float64)
        for what, plain, step in (('train', plain_train, lambda: m.train_step(x, y, 0.0, cfg)), ('eval', plain_eval, lambda: m.eval_step(x, y, cfg))):
            out = step()
            sums = m.region_loss_sums(Bm)
            prob = m.last_prob(Bm).astype(np.float64)
            want = np.stack([(prob * y64).sum((1, 2)), prob.sum((1, 2)), y64.sum((1, 2))], 1)
            print('region loss 1024^2 %s: sums err %.2e loss %.9g plain %.9g' % (
                what, float((np.abs(sums - want) / np.maximum(np.abs(want), 1.0)).max()), out.loss, plain))
            assert np.all(np.abs(sums - want) <= 1e-12 * np.maximum(np.abs(want), 1.0))
            t = R.tversky_index(sums, 0.5, 0.5, 1.0)
            assert abs((out.loss - plain) - float(np.mean(1.0 - t))) <= 1e-5 * max(1.0, abs(out.loss))
        m.train_metrics(None)
    finally:
        m.close()
