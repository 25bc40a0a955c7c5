"""-m gpu: the INFERENCE passes (forward(training=False), eval_step, the staged evaluation step) against the float64 oracle.

Inference has no batch statistics, so the oracle runs image by image and the three BASELINE configurations can be compared with
it directly at 8 x 512 x 512 / 4 x 512 x 512 (the train step never could: its float64 backward pass does not fit).  Inference does
not launch the forward half of the train plan: the conv that feeds the head has no head epilogue (g_head_fwd + g_loss / g_sigmoid
follow), the fused first block runs without the label ride-along, the convs in front of a BatchNorm run without their statistics
epilogues, and the BatchNorms hand the MOVING-statistics coefficients to their apply pass or to the convs that normalise on load.
Every test here registers the inference plan it ran (helpers.record_oracle_plan(mode='eval')); tests/test_zz_kernel_coverage.py
closes the loop for the BASELINE plans.

Bounds
  full size (test_baseline_inference_at_full_size_against_oracle): logits within
        min(10 x the error of the SAME oracle in plain float32 numpy on the same inputs, 2e-4 * max(1, max|logit_ref|))
    -- the float32 cost is measured by the test itself at run time (it is the reference's own error, not the device's), 10 x is
    the project's margin for a different float32 summation order, 2e-4 * max(1, .) the bound of tests/test_parity_gpu.py, which
    the new one never exceeds.  Probabilities: the same bound (the sigmoid is 1/4-Lipschitz) + 2^-22 for the float32 rounding of a
    stored probability and of the device's exp.  Loss: 1e-4 relative (test_parity_gpu.py).  Masks at 0.5 / 0.8: bit-exact on every
    pixel whose reference logit is farther from the threshold's logit than the logit bound.
  everything else: the tolerances of tests/test_parity_gpu.py (LOGIT_TOL, loss 1e-4, masks as above)."""

import time

import numpy as np
import pytest

import helpers as Hp
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

LOGIT_TOL = 2e-4         # tests/test_parity_gpu.py: |d| <= LOGIT_TOL * max(1, |logits|max)
UNET = dict(n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')
PROB_ROUNDING = 2.0 ** -22
CFG = dict(weight_mul=3.0)


def _spec(arch, C, opts, alpha=0.0):
    full = dict(rate=2, kernel_size=3, conv_stride=1, padding='same')
    full.update(opts)
    if alpha:
        full['activation'] = {'class_name': 'LeakyReLU', 'config': {'alpha': alpha}}
    return O.ModelSpec(arch, C, **full), {k: v for k, v in full.items() if k != 'activation'}


def _oracle_logits(spec, params, x, dtype=np.float64):
    """O.predict one image at a time (memory: unet_big takes 4.4 GB per 512 x 512 image in float64)"""
    p = {n: v.astype(dtype) for n, v in params.items()}
    return np.concatenate([O.predict(spec, p, x[i:i + 1].astype(dtype))[1] for i in range(x.shape[0])])


def _oracle_loss(spec, params, y, logits, cfg):
    per, _ = O.weighted_crossentropy(y, np.asarray(logits, np.float64), **cfg)
    return float(per.mean(dtype=np.float64)) + O.l2_penalty(spec, params)


def _sigmoid(l):
    return 1.0 / (1.0 + np.exp(-l))


def _assert_inference(what, logits, prob, loss, logit_ref, loss_ref, tol):
    """the checks of one inference pass; returns the device's logit error"""
    prob_ref = _sigmoid(logit_ref)
    err = float(np.abs(logits - logit_ref).max())
    perr = float(np.abs(prob - prob_ref).max())
    print('%s: logit err %.3e (bound %.3e, max|logit| %.3f), prob err %.3e, loss %.8f vs %.8f' % (
        what, err, tol, float(np.abs(logit_ref).max()), perr, float('nan') if loss is None else loss, loss_ref))
    assert np.isfinite(logits).all() and np.isfinite(prob).all(), what
    assert err <= tol, (what, err, tol)
    assert perr <= tol + PROB_ROUNDING, (what, perr, tol)
    if loss is not None:
        assert abs(loss - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref)), (what, loss, loss_ref)
    for thr in (0.5, 0.8):
        decided = np.abs(logit_ref - np.log(thr / (1 - thr))) > tol
        assert np.array_equal((prob > thr)[decided], (prob_ref > thr)[decided]), '%s: mask flip away from the threshold %.1f' % (what, thr)
    return err


def _inference_against_oracle(m, spec, params, x, y, what, tol=None, logit_ref=None):
    """forward(training=False) and eval_step on x[:B] against O.predict; tol None: LOGIT_TOL * max(1, max|logit_ref|)"""
    if logit_ref is None:
        logit_ref = _oracle_logits(spec, params, x)
    if tol is None:
        tol = LOGIT_TOL * max(1.0, float(np.abs(logit_ref).max()))
    loss_ref = _oracle_loss(spec, params, y, logit_ref, CFG)
    prob, logits = m.forward(x, training=False, return_logits=True)
    out, prob_e = m.eval_step(x, y, m.loss_cfg(**CFG), return_prob=True)
    err = _assert_inference(what + ' forward', logits, prob, None, logit_ref, loss_ref, tol)
    _assert_inference(what + ' eval_step', logits, prob_e, out.loss, logit_ref, loss_ref, tol)
    return err, logit_ref


# ---------------------------------------------------------------------------------------------- the dry plans tell the truth
def _live_counts(m, run):
    m.profile_reset()
    m.profile_enable(1)
    run()
    m.sync()
    counts = {r[0]: r[1] for r in m.profile()}
    m.profile_enable(0)
    m.profile_reset()
    return counts


def _plan_counts(m, mode, batch):
    counts = {}
    for k, _, _ in m.plan(mode=mode, batch=batch):
        counts[k] = counts.get(k, 0) + 1
    return counts


def _plan_truth_models(gpu):
    """(name, model factory, x, y): two golden small cases (one with BatchNorm), a dense fp32 BatchNorm model at real widths, a
    bf16 model, a configs/unet.yaml shape made of whole tiles"""
    out = []
    for name in ('unet_yaml_2x32', 'unet_bn_leaky_l2_2x16'):
        z, spec, _ = Hp.load_case(name)
        x, y = z['x'], z['y']
        B, H, W, _ = x.shape
        out.append((name, dict(Hp.device_kwargs(spec, H, W, B)), x, y))
    rng = np.random.default_rng(5)
    dense = dict(arch='mulmo', in_channels=3, height=64, width=64, max_batch=2, n_filters_first=16, n_downsample=4, bn=True, padding='same')
    out.append(('mulmo_f16_2x64', dense, rng.random((2, 64, 64, 3)).astype(np.float32), (rng.random((2, 64, 64)) < 0.05).astype(np.float32)))
    bf16 = dict(arch='unet', in_channels=1, height=64, width=64, max_batch=2, n_filters_first=64, n_downsample=2, bn=True, padding='same',
                dtype='bf16')
    out.append(('unet_f64_bf16_2x64', bf16, rng.random((2, 64, 64, 1)).astype(np.float32), (rng.random((2, 64, 64)) < 0.05).astype(np.float32)))
    tiles = dict(arch='unet', in_channels=1, height=64, width=256, max_batch=2, **UNET)
    out.append(('unet_yaml_2x64x256', tiles, rng.random((2, 64, 256, 1)).astype(np.float32), (rng.random((2, 64, 256)) < 0.05).astype(np.float32)))
    return out


def test_dry_inference_plans_list_the_launches_of_the_live_passes(gpu):
    """DeviceModel.plan(mode='eval' | 'forward', batch=B): the multiset of launch names (variant suffix stripped) equals the
    HIP-event profile of one live eval_step / forward(training=False) at that B, at B = max_batch and at B = 1; a dump of every
    pass changes nothing -- parameters, BatchNorm state and the logits of a following live forward are bit-identical with and
    without it -- and plan() with its defaults is still the text of dnnca_plan_dump."""
    import ctypes as C
    for name, kw, x, y in _plan_truth_models(gpu):
        m = gpu.DeviceModel(**kw)
        try:
            m.init_glorot(seed=4)
            if m.n_state:
                rng = np.random.default_rng(9)
                m.set_state((m.get_state() + rng.uniform(0.05, 0.2, m.n_state)).astype(np.float32))
            cfg = m.loss_cfg(**CFG)
            p0, s0 = m.get_params(), m.get_state()
            _, l0 = m.forward(x, training=False, return_logits=True)          # before any dump
            loss0 = m.eval_step(x, y, cfg).loss
            buf = C.create_string_buffer(1 << 20)
            assert m.lib.dnnca_plan_dump(m.handle, buf, len(buf)) == 0
            train_text = buf.value.decode()
            for B in (m.max_batch, 1):
                live_e = _live_counts(m, lambda: m.eval_step(x[:B], y[:B], cfg))
                live_f = _live_counts(m, lambda: m.forward(x[:B], training=False))
                dry_e, dry_f = _plan_counts(m, 'eval', B), _plan_counts(m, 'forward', B)
                print(name, 'B', B, 'eval', sorted(dry_e.items()), 'forward', sorted(dry_f.items()))
                assert dry_e == live_e, (name, B, dry_e, live_e)
                assert dry_f == live_f, (name, B, dry_f, live_f)
                assert 'g_sigmoid' in dry_f and 'g_loss' in dry_e and 'g_head_fwd' in dry_e, (dry_e, dry_f)
            # every pass dumped, in an order that interleaves them; then the live passes again
            for mode, B in (('forward', 1), ('train', None), ('eval', m.max_batch), ('train', 1), ('forward', m.max_batch), ('eval', 1)):
                assert m.plan(variants=True, mode=mode, batch=B)
            assert np.array_equal(m.get_params(), p0) and np.array_equal(m.get_state(), s0), name
            _, l1 = m.forward(x, training=False, return_logits=True)
            assert np.array_equal(l1, l0), name
            assert m.eval_step(x, y, cfg).loss == loss0, name
            # the train pass is what dnnca_plan_dump has always returned, and plan()'s defaults still go through it
            assert m.lib.dnnca_plan_dump(m.handle, buf, len(buf)) == 0 and buf.value.decode() == train_text
            assert m.lib.dnnca_plan_dump_pass(m.handle, 0, m.max_batch, buf, len(buf)) == 0 and buf.value.decode() == train_text
            lines = [l.split('\t') for l in train_text.splitlines()]
            assert m.plan(variants=True) == [(k, float(b), float(f)) for k, b, f in lines]
            assert m.plan() == [(k.split('#')[0], float(b), float(f)) for k, b, f in lines]
            with pytest.raises(Exception):
                m.plan(mode='eval', batch=m.max_batch + 1)
            with pytest.raises(ValueError):
                m.plan(mode='predict')
        finally:
            m.close()


# ---------------------------------------------------------------------------------------------- (a) full size
BASELINE_F32 = [
    ('configs/unet.yaml', 'unet', 1, 8, dict(n_filters_first=3, n_downsample=3, bn=False)),
    ('configs/mulmo_unet.yaml', 'mulmo', 3, 8, dict(n_filters_first=16, n_downsample=4, bn=True)),
    ('configs/unet_big.yaml', 'unet', 1, 4, dict(n_filters_first=64, n_downsample=4, bn=True)),
]


@pytest.mark.parametrize('name, arch, C, B, opts', BASELINE_F32, ids=[c[0].split('/')[1].split('.')[0] for c in BASELINE_F32])
def test_baseline_inference_at_full_size_against_oracle(gpu, name, arch, C, B, opts):
    """The three BASELINE configurations at their full sizes (512 x 512; unet.yaml and mulmo_unet batch 8, unet_big's
    hyper-parameters batch 4, all in dtype f32), inference against the float64 oracle on every pixel: logits, probabilities,
    eval_step's loss and the masks at 0.5 / 0.8.  Perturbed parameters (helpers.perturbed_params: moving mean / variance away from
    0 / 1, every bias non-zero); the head bias is then moved by minus the median of the reference logits, so that half of the pixels
    sit on each side of the 0.5 threshold (as they are, the unet_big reference puts 4e-6 of its pixels above it).  Conditions on
    the inputs, asserted on the reference alone: >= 5 % of the pixels on each side of 0.5, <= 1 % undecided at either threshold.

    Bound: module docstring.  Measured on MI355X (the test prints them: float32-numpy cost / bound / device error):
      unet.yaml   1.24e-8 / 1.24e-7 / 1.19e-8 (0.96 x the float32-numpy cost; max|logit| 0.038)
      mulmo_unet  1.51e-7 / 1.51e-6 / 2.47e-7 (1.63 x; 0.157)
      unet_big    2.21e-7 / 2.21e-6 / 4.86e-7 (2.20 x; 0.133) -- the split-bf16 conv kernels need no more than the 10 x margin.
    Undecided pixels <= 4.1e-5 at 0.5, none at 0.8; CPU oracle 0.8 / 14.9 / 29.1 s."""
    H = W = 512
    spec, dev_opts = _spec(arch, C, opts)
    params = Hp.perturbed_params(spec, np.float64)
    rng = np.random.default_rng(41)
    x = rng.random((B, H, W, C)).astype(np.float32)
    y = (rng.random((B, H, W)) < 0.05).astype(np.float32)
    t0 = time.time()
    raw = _oracle_logits(spec, params, x)
    b0 = params['head.bias']
    params['head.bias'] = (b0 - np.median(raw)).astype(np.float32).astype(np.float64)
    logit_ref = raw + (params['head.bias'] - b0)          # the head bias is added last: the shifted reference, exactly
    l32 = _oracle_logits(spec, params, x, np.float32)
    cpu_s = time.time() - t0
    lmax = float(np.abs(logit_ref).max())
    e32 = float(np.abs(l32.astype(np.float64) - logit_ref).max())
    tol = min(10.0 * e32, LOGIT_TOL * max(1.0, lmax))
    above = float((logit_ref > 0).mean())
    undecided = [float((np.abs(logit_ref - np.log(t / (1 - t))) <= tol).mean()) for t in (0.5, 0.8)]
    print('%s: float32-numpy cost %.3e (%.3e of max|logit| %.3f), bound %.3e (%.3e relative); above 0.5: %.3f, undecided %.2e / %.2e; '
          'oracle %.1f s' % (name, e32, e32 / lmax, lmax, tol, tol / lmax, above, undecided[0], undecided[1], cpu_s))
    assert 0.05 <= above <= 0.95, above
    assert max(undecided) <= 0.01, undecided
    m = gpu.DeviceModel(arch, C, H, W, B, **dev_opts)
    try:
        m.set_params(O.flatten(spec, params))
        if m.n_state:
            m.set_state(O.flatten(spec, params, trainable=False))
        err, _ = _inference_against_oracle(m, spec, params, x, y, name, tol=tol, logit_ref=logit_ref)
        print('%s: device error %.3e = %.2f x the float32-numpy cost' % (name, err, err / max(e32, 1e-300)))
        Hp.record_oracle_plan(m, 'test_baseline_inference_at_full_size_against_oracle', mode='eval', batch=B)
        # the evaluation of a last, smaller batch and predict() on single images launch the B = 1 plan
        _inference_against_oracle(m, spec, params, x[:1], y[:1], name + ' B=1', tol=tol, logit_ref=logit_ref[:1])
        Hp.record_oracle_plan(m, 'test_baseline_inference_at_full_size_against_oracle', mode='eval', batch=1)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------- (c) the 3-channel level
LEVEL3 = [(2, 40, 128, 0.0, False), (8, 16, 256, 0.0, False), (3, 24, 200, 0.0, False), (1, 72, 64, 0.0, False), (2, 64, 256, 0.0, False),
          (2, 64, 256, 0.0, True), (3, 32, 128, 0.0, False), (1, 96, 128, 0.0, False), (9, 32, 256, 0.0, False),
          (2, 64, 256, 0.3, False), (3, 32, 128, 0.3, False), (1, 96, 128, 0.3, False), (9, 32, 256, 0.3, False)]


@pytest.mark.parametrize('B, H, W, leaky, fz_up2', LEVEL3)
def test_inference_of_the_3_channel_level_against_oracle(gpu, monkeypatch, B, H, W, leaky, fz_up2):
    """configs/unet.yaml in inference mode on the shapes where its variants change -- those of
    test_vector_alu_kernels_of_the_3_channel_level_against_oracle and test_block_fused_backward_against_oracle (partial strips, one
    strip, one tile row, more images than XCDs, LeakyReLU 0.3), default switches plus DNNCA_FZ_UP2: the strip / block-fused forward
    kernels without the stored intermediates of a train step, and the conv that feeds the head without its head epilogue."""
    if fz_up2:
        monkeypatch.setenv('DNNCA_FZ_UP2', '1')
    spec, dev_opts = _spec('unet', 1, UNET, leaky)
    params = Hp.perturbed_params(spec, np.float64)
    rng = np.random.default_rng(13)
    x = rng.random((B, H, W, 1)).astype(np.float32)
    y = (rng.random((B, H, W)) < 0.05).astype(np.float32)
    m = gpu.DeviceModel('unet', 1, H, W, B, **dev_opts, **(dict(leaky_alpha=leaky) if leaky else {}))
    try:
        m.set_params(O.flatten(spec, params))
        _inference_against_oracle(m, spec, params, x, y, 'unet.yaml %dx%dx%d leaky %.1f' % (B, H, W, leaky))
        names = set(r[0] for r in m.plan(mode='eval'))
        assert {'g_head_fwd', 'g_loss'} <= names and not any(k.startswith('tail3') for k in names), names
        assert ('fz_up2_6' in names) == bool(fz_up2), names
        Hp.record_oracle_plan(m, 'test_inference_of_the_3_channel_level_against_oracle', mode='eval', batch=B)
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------- (d) ragged and interleaved batches
RAGGED = [
    ('unet', 1, dict(UNET), 64, 256, 0.0),
    ('mulmo', 3, dict(n_filters_first=16, n_downsample=4, bn=True), 64, 64, 0.0),
    ('unet', 1, dict(n_filters_first=64, n_downsample=2, bn=True), 32, 32, 0.0),
]


@pytest.mark.parametrize('arch, C, opts, H, W, alpha', RAGGED, ids=['unet_yaml', 'mulmo_f16', 'unet_f64'])
def test_ragged_batches_against_oracle(gpu, arch, C, opts, H, W, alpha):
    """What engine.eval and the validation between epochs do: one model built for batch 8 runs inference on 8, 3, 1 and 8 images in
    that order (the last batch of a dataset is smaller; the batch decides tile counts, grid sizes and -- for the dense BatchNorm
    models -- whether a conv normalises on load), each against the oracle; then one staged evaluation step on 3 images
    (StagingRing.eval_begin / eval_step / eval_end), whose probabilities (last_prob) and loss meet the same bound."""
    spec, dev_opts = _spec(arch, C, opts, alpha)
    params = Hp.perturbed_params(spec, np.float64)
    rng = np.random.default_rng(29)
    x = rng.random((8, H, W, C)).astype(np.float32)
    y = (rng.random((8, H, W)) < 0.05).astype(np.float32)
    full = _oracle_logits(spec, params, x)
    m = gpu.DeviceModel(arch, C, H, W, 8, **dev_opts)
    try:
        m.set_params(O.flatten(spec, params))
        if m.n_state:
            m.set_state(O.flatten(spec, params, trainable=False))
        for lo, B in ((0, 8), (2, 3), (7, 1), (0, 8)):
            xb, yb = np.ascontiguousarray(x[lo:lo + B]), np.ascontiguousarray(y[lo:lo + B])
            _inference_against_oracle(m, spec, params, xb, yb, '%s B=%d' % (arch, B), logit_ref=full[lo:lo + B])
            Hp.record_oracle_plan(m, 'test_ragged_batches_against_oracle', mode='eval', batch=B)
        # one staged evaluation step on a ragged batch
        lo, B = 4, 3
        xb, yb = np.ascontiguousarray(x[lo:lo + B]), np.ascontiguousarray(y[lo:lo + B])
        ring = m.staging(2)
        px, py = ring.upload(1, xb, yb)
        ring.eval_begin([0.5])
        ring.eval_step(1, px, py, B, m.loss_cfg(**CFG))
        out = ring.out(1)
        (tp, fp, fn, tn), = ring.eval_end()
        prob = m.last_prob(B)[..., None]
        ref = full[lo:lo + B]
        tol = LOGIT_TOL * max(1.0, float(np.abs(ref).max()))
        assert np.abs(prob - _sigmoid(ref)).max() <= tol + PROB_ROUNDING
        assert abs(out.loss - _oracle_loss(spec, params, yb, ref, CFG)) <= 1e-4 * max(1.0, abs(out.loss))
        decided = np.abs(ref) > tol
        assert np.array_equal((prob > 0.5)[decided], (ref > 0)[decided])
        assert tp + fp + fn + tn == B * H * W and tp + fp == int((prob > 0.5).sum())
    finally:
        m.close()


def test_inference_between_train_steps_against_oracle(gpu):
    """train step, inference, train step on a dense BatchNorm model -- the mulmo_unet widths of
    test_dense_configs_at_real_widths_against_oracle (2 x 64 x 64, LeakyReLU(0.99), input seed 121) at that test's tolerances.  The
    inference in the middle reads the MOVING statistics the first step has just updated and must leave nothing behind that the second
    step would find (statistics a conv epilogue claims to have left, an elision decided for another pass, pool positions, staged
    coefficients).  The oracle's two-step sequence: step 1 at learning rate 0 as in the test the model is taken from (the weights
    stay, the moving statistics move), inference on another batch against O.predict on the state after step 1, step 2 at learning
    rate 1e-3 -- loss and gradients against the oracle (batch statistics: those of step 1), the state against the oracle's second
    update of the moving statistics.  Both train steps run on the input of that test: its seed was scanned for max-pool winner flips
    (its docstring; a random batch misses the 1e-4 gradient bound on a handful of tensors by 1e-2 in plain float32 numpy, on the
    generic kernels and on the tuned ones alike, with and without the inference in between -- measured, NOTES.md).  After step 2 the
    weights have moved, so every prepared operand of the inference kernels is stale: a last inference on one image against O.predict
    on the variables read back from the device."""
    arch, C, B, size, alpha = 'mulmo', 3, 2, 64, 0.99
    spec, dev_opts = _spec(arch, C, dict(n_filters_first=16, n_downsample=4, bn=True), alpha)
    params = Hp.perturbed_params(spec, np.float64)
    rng = np.random.default_rng(121)
    x, y = rng.random((B, size, size, C)).astype(np.float32), (rng.random((B, size, size)) < 0.05).astype(np.float32)
    x2, y2 = rng.random((B, size, size, C)).astype(np.float32), (rng.random((B, size, size)) < 0.05).astype(np.float32)
    loss, grads, _, state1 = O.loss_and_grads(spec, params, x.astype(np.float64), y, CFG, training=True)
    p32 = {n: v.astype(np.float32) for n, v in params.items()}
    _, g32, _, _ = O.loss_and_grads(spec, p32, x, y, CFG, training=True)
    gref, g32 = O.flatten(spec, grads), O.flatten(spec, g32).astype(np.float64)
    floor = [10 * np.abs(g32[sl] - gref[sl]).max() for _, sl in Hp.tensor_slices(spec)]
    p1 = dict(params, **state1)
    _, _, _, state2 = O.loss_and_grads(spec, p1, x.astype(np.float64), y, CFG, training=True)
    m = gpu.DeviceModel(arch, C, size, size, B, leaky_alpha=alpha, **dev_opts)

    def step(lr, state_ref, what):
        out = m.train_step(x, y, lr, m.loss_cfg(**CFG))
        assert abs(out.loss - loss) <= 1e-5 * max(1.0, abs(loss)), (what, out.loss, loss)
        Hp.assert_grads_per_tensor(spec, m.get_grads(), gref, 1e-4, floor=floor, what=what)
        assert np.abs(m.get_state() - O.flatten(spec, dict(params, **state_ref), trainable=False)).max() <= 1e-5, what

    try:
        m.set_params(O.flatten(spec, params))
        m.set_state(O.flatten(spec, params, trainable=False))
        step(0.0, state1, 'step 1')
        s1 = m.get_state()
        _inference_against_oracle(m, spec, p1, x2, y2, 'inference after step 1')
        Hp.record_oracle_plan(m, 'test_inference_between_train_steps_against_oracle', mode='eval', batch=B)
        assert np.array_equal(m.get_state(), s1)                                   # inference left the state alone
        step(1e-3, state2, 'step 2')
        p2 = O.unflatten(spec, m.get_params().astype(np.float64))
        O.unflatten(spec, m.get_state().astype(np.float64), trainable=False, into=p2)
        assert np.abs(O.flatten(spec, p2) - O.flatten(spec, params)).max() > 1e-4          # the weights moved
        _inference_against_oracle(m, spec, p2, x2[:1], y2[:1], 'inference after step 2, B=1')
    finally:
        m.close()
