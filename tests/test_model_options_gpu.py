"""-m gpu: off-default model_options (kernel_size 1 / 5 / 7, rate 3, n_conv 1 / 3, first-layer widths 6 and 24) against the float64
oracle: one train step and the inference passes, on a force_generic and on a tuned model.

The launch choice is made per op (conv_supported, ig_conv_supported, fast_pool_supported, fast_tconv_supported, the fused-block
matchers), so a model with such options does not fall to the generic path as a whole: it runs a MIXED plan, tuned and generic
launches side by side, and the hand-offs between them (recorded pool positions against value-compare pool backward, accumulate
flags, need_din, BatchNorms elided by the reader analysis, the head-in-conv decision) are what these cases hold to the oracle.  The
cases are the smallest shapes that still produce the mix (CASES; the plan of every tuned model is pinned in PLANS).

Settings of every case: B = max_batch = 3, parameters helpers.perturbed_params, inputs uniform random and labels `random < 0.05`
from the input seeds 11 and 12 (fixed in advance: in the float32 oracle both are clean for every case -- no healthy tensor is off
by more than 1e-4 of its scale, which _case asserts on the reference alone), loss_cfg(weight_mul=3.0, weight_add=0.25).

Bounds (the project's existing rules, none new):
  train step   |loss - ref| <= 1e-4 max(1, |ref|); every gradient tensor within 2e-5 of its own scale + 10 x the float32 oracle's own
               error on that tensor (tests/test_engine_gpu.py::test_non_square_leaky_l2_tuned_kernels); the moving statistics after
               the step within 1e-5 (tests/test_inference_gpu.py::test_inference_between_train_steps_against_oracle)
  inference    logits and probabilities of forward(training=False) and eval_step within min(10 x the float32 oracle's own error,
               2e-4 max(1, max|logit|)), loss 1e-4, masks (tests/test_inference_gpu.py)
  tuned vs generic   the gradients of the two models per tensor, the train-step bound
Once per case the references are cross-checked as tests/golden/make_golden.py does: oracle against tests/torch_ref.py in float64.

Measured on MI355X (per case in NOTES.md, 2026-10-19): loss within 2.1e-7; worst healthy gradient tensor 3e-7 .. 9e-7 of its scale
without BatchNorm and 2e-6 .. 1.7e-5 with it, never above the float32 oracle's own worst tensor on the same inputs (1e-6 .. 2.5e-6 /
6e-6 .. 2.2e-5); logits at 0.7 .. 3.2 x the float32 oracle's cost; no case is generic throughout on the device, the four n_conv
cases are tuned throughout."""

import numpy as np
import pytest

import helpers as Hp
import test_inference_gpu as TI
import torch_ref
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

B = 3
SEEDS = (11, 12)
CFG = dict(weight_mul=3.0, weight_add=0.25)
# mixed: the plan of the tuned model must hold generic conv / pool / transposed-conv launches AND tuned arithmetic launches (the
# n_conv cases are tuned throughout: the pixel-group, implicit-GEMM and fused-block kernels take every op of theirs)
CASES = {
    'k5_3ch': dict(arch='unet', C=1, H=16, W=24, opts=dict(n_filters_first=3, n_downsample=2, kernel_size=5), mixed=True),
    'k1_bn': dict(arch='unet', C=2, H=16, W=24, opts=dict(n_filters_first=3, n_downsample=2, kernel_size=1, bn=True), mixed=True),
    'k7_3ch': dict(arch='unet', C=1, H=16, W=24, opts=dict(n_filters_first=3, n_downsample=1, kernel_size=7), mixed=True),
    'nconv1': dict(arch='unet', C=1, H=32, W=64, opts=dict(n_filters_first=3, n_downsample=3, n_conv=1), mixed=False),
    'nconv3': dict(arch='unet', C=1, H=32, W=64, opts=dict(n_filters_first=3, n_downsample=3, n_conv=3), mixed=False),
    'f6_c3': dict(arch='unet', C=3, H=24, W=40, opts=dict(n_filters_first=6, n_downsample=1), mixed=True),
    'rate3_3ch': dict(arch='unet', C=1, H=18, W=36, opts=dict(n_filters_first=3, n_downsample=2, rate=3), mixed=True),
    'd_rate3': dict(arch='mulmo', C=2, H=18, W=36, opts=dict(n_filters_first=16, n_downsample=2, rate=3, bn=True), mixed=True),
    'd_k5': dict(arch='unet', C=1, H=24, W=40, opts=dict(n_filters_first=16, n_downsample=2, kernel_size=5, bn=True), mixed=True),
    'd_nconv3': dict(arch='unet', C=1, H=24, W=40, opts=dict(n_filters_first=16, n_downsample=2, n_conv=3, bn=True), mixed=False),
    'd_nconv1': dict(arch='mulmo', C=2, H=24, W=40, opts=dict(n_filters_first=16, n_downsample=2, n_conv=1, bn=True), mixed=False),
    'd_f24': dict(arch='unet', C=1, H=24, W=40, opts=dict(n_filters_first=24, n_downsample=2, bn=True), mixed=True),
}
# one train step of the tuned model as it is planned on MI355X: launch name:count, sorted by name
PLANS = {
    'k5_3ch': 'g_act_bwd:4 g_adam:1 g_conv_dgrad:7 g_conv_fwd:8 g_conv_wgrad:8 g_finalize_scalars:1 g_step_init:1 g_tconv_dgrad:1 g_tconv_fwd:1 g_tconv_wgrad:1 head_train_3:1 label_stats4:1 pg_fold:1 pool2_bwd_3:1 pool2_bwd_6:1 pool2_fwd_3:1 pool2_fwd_6:1 tconv2_fwd_6_3:1 tconv_bwd_6_3:1',
    'k1_bn': 'g_act_bwd:8 g_adam:1 g_bn_apply:12 g_bn_bwd_apply:12 g_bn_bwd_reduce:12 g_bn_finalize:12 g_bn_stats_mean:12 g_bn_stats_var:12 g_conv_dgrad:7 g_conv_fwd:8 g_conv_wgrad:8 g_finalize_scalars:1 g_step_init:1 g_tconv_dgrad:1 g_tconv_fwd:1 g_tconv_wgrad:1 head_train_3:1 label_stats4:1 pg_fold:1 pool2_bwd_3:1 pool2_bwd_6:1 pool2_fwd_3:1 pool2_fwd_6:1 tconv2_fwd_6_3:1 tconv_bwd_6_3:1',
    'k7_3ch': 'g_act_bwd:2 g_adam:1 g_conv_dgrad:3 g_conv_fwd:4 g_conv_wgrad:4 g_finalize_scalars:1 g_step_init:1 g_tconv_dgrad:1 g_tconv_fwd:1 g_tconv_wgrad:1 head_reduce:1 head_train_3:1 label_stats4:1 pool2_bwd_3:1 pool2_fwd_3:1',
    'nconv1': 'g_adam:1 g_finalize_scalars:1 g_step_init:1 head_train_3:1 label_stats4:1 pg_fold:1 pg_prep:1 pgbwd_12x2_12:1 pgbwd_3x1_6:1 pgbwd_3x2_3:1 pgbwd_6x1_12:1 pgbwd_6x2_6:1 pgbwd_w_1x1_3:1 pgfwd_12x2_12:1 pgfwd_1x1_3:1 pgfwd_3x1_6:1 pgfwd_6x1_12:1 pgfwd_6x2_6:1 pool2_bwd_12:1 pool2_bwd_3:1 pool2_bwd_6:1 tconv2_fwd_12_12:1 tconv2_fwd_12_6:1 tconv_bwd_12_12:1 tconv_bwd_12_6:1 tconv_bwd_6_3:1 up3_fwd:1',
    'nconv3': 'g_adam:1 g_finalize_scalars:1 g_step_init:1 label_stats4:1 pg_fold:1 pg_prep:1 pgbwd_12x1_12:4 pgbwd_12x2_12:1 pgbwd_3x1_3:3 pgbwd_3x1_6:1 pgbwd_3x2_3:1 pgbwd_6x1_12:1 pgbwd_6x1_6:4 pgbwd_6x2_6:1 pgbwd_w_1x1_3:1 pgfwd_12x1_12:4 pgfwd_12x2_12:1 pgfwd_1x1_3:1 pgfwd_3x1_3:3 pgfwd_3x1_6:1 pgfwd_6x1_12:1 pgfwd_6x1_6:4 pgfwd_6x2_6:1 pool2_bwd_12:1 pool2_bwd_3:1 pool2_bwd_6:1 tail3_3x1_3:1 tconv2_fwd_12_12:1 tconv2_fwd_12_6:1 tconv_bwd_12_12:1 tconv_bwd_12_6:1 tconv_bwd_6_3:1 up3_fwd:1',
    'f6_c3': 'g_act_bwd:1 g_adam:1 g_finalize_scalars:1 g_head_bwd:1 g_head_fwd:1 g_loss:1 g_step_init:1 g_tconv_dgrad:1 g_tconv_fwd:1 g_tconv_wgrad:1 label_stats4:1 pg_fold:1 pg_prep:1 pgbwd_6x1_6:2 pgbwd_6x2_6:1 pgbwd_w_3x1_6:1 pgfwd_3x1_6:1 pgfwd_6x1_6:2 pgfwd_6x2_6:1 pool2_bwd_6:1',
    'rate3_3ch': 'g_act_bwd:5 g_adam:1 g_conv_dgrad:4 g_conv_fwd:4 g_conv_wgrad:4 g_finalize_scalars:1 g_pool_bwd:2 g_pool_fwd:2 g_step_init:1 g_tconv_dgrad:2 g_tconv_fwd:2 g_tconv_wgrad:2 label_stats4:1 pg_fold:1 pg_prep:1 pgbwd_3x1_3:1 pgbwd_3x2_3:1 pgbwd_w_1x1_3:1 pgfwd_1x1_3:1 pgfwd_3x1_3:1 pgfwd_3x2_3:1 tail3_3x1_3:1',
    'd_rate3': 'bn_apply:3 bn_bwd_apply:9 bn_bwd_reduce:4 bn_stats:3 first_fold:2 first_fwd:2 first_wgrad:2 g_act_bwd:6 g_adam:1 g_bn_apply:9 g_bn_bwd_apply:9 g_bn_bwd_reduce:9 g_bn_finalize:9 g_bn_stats_mean:9 g_bn_stats_var:9 g_finalize_scalars:1 g_pool_bwd:4 g_pool_fwd:4 g_step_init:1 g_tconv_dgrad:2 g_tconv_fwd:2 g_tconv_wgrad:2 head_reduce:1 head_train_16:1 ig3x_conv_dgrad:10 ig3x_conv_fwd:10 ig3x_prep:1 ig3x_wgrad:12 label_stats4:1 wg_fold:12',
    'd_k5': 'bn_apply:10 bn_apply_pool:2 bn_bwd_apply:12 bn_bwd_reduce:12 bn_stats:8 g_adam:1 g_conv_dgrad:7 g_conv_fwd:8 g_conv_wgrad:8 g_finalize_scalars:1 g_step_init:1 head_reduce:1 head_train_16:1 ig_tconv_dgrad:2 ig_tconv_fwd:2 ig_tconv_wgrad2:2 label_stats4:1',
    'd_nconv3': 'bn_apply:3 bn_apply_pool:2 bn_bwd_apply:16 bn_bwd_reduce:7 first_fold:1 first_fwd:1 first_wgrad:1 g_adam:1 g_finalize_scalars:1 g_step_init:1 head_reduce:1 head_train_16:1 ig3x_conv_dgrad:11 ig3x_conv_fwd:11 ig3x_prep:1 ig3x_wgrad:13 ig_tconv_dgrad:2 ig_tconv_fwd:2 ig_tconv_wgrad2:2 label_stats4:1 wg_fold:13',
    'd_nconv1': 'bn_apply:4 bn_apply_pool:4 bn_bwd_apply:12 bn_bwd_reduce:10 first_fold:2 first_fwd:2 first_wgrad:2 g_adam:1 g_finalize_scalars:1 g_step_init:1 head_reduce:1 head_train_16:1 ig3x_conv_dgrad:4 ig3x_conv_fwd:4 ig3x_prep:1 ig3x_wgrad:6 ig_tconv_dgrad:2 ig_tconv_fwd:2 ig_tconv_wgrad2:2 label_stats4:1 wg_fold:6',
    'd_f24': 'g_act_bwd:8 g_adam:1 g_bn_apply:12 g_bn_bwd_apply:12 g_bn_bwd_reduce:12 g_bn_finalize:12 g_bn_stats_mean:12 g_bn_stats_var:12 g_conv_dgrad:4 g_conv_fwd:5 g_conv_wgrad:5 g_finalize_scalars:1 g_head_bwd:1 g_head_fwd:1 g_loss:1 g_pool_bwd:2 g_pool_fwd:2 g_step_init:1 g_tconv_dgrad:1 g_tconv_fwd:1 g_tconv_wgrad:1 ig3x_conv_dgrad:3 ig3x_conv_fwd:3 ig3x_prep:1 ig3x_wgrad:4 ig_tconv_dgrad:1 ig_tconv_fwd:1 ig_tconv_wgrad2:1 label_stats4:1 wg_fold:4',
}
_REF, _DEV = {}, {}


def _spec(name):
    c = CASES[name]
    full = dict(rate=2, kernel_size=3, conv_stride=1, padding='same', bn=False)
    full.update(c['opts'])
    return O.ModelSpec(c['arch'], c['C'], **full)


def _per_tensor_abs(spec, a, b):
    return [float(np.abs(a[sl] - b[sl]).max()) for _, sl in Hp.tensor_slices(spec)]


def _case(name, seed):
    """the references of one (case, input seed), computed once: float64 oracle train step and inference, the same in float32 (the
    cost of the number format), cross-checked against tests/torch_ref.py"""
    if (name, seed) not in _REF:
        c = CASES[name]
        spec = _spec(name)
        params = Hp.perturbed_params(spec, np.float64)
        p32 = {n: v.astype(np.float32) for n, v in params.items()}
        rng = np.random.default_rng(seed)
        x = rng.random((B, c['H'], c['W'], c['C'])).astype(np.float32)
        y = (rng.random((B, c['H'], c['W'])) < 0.05).astype(np.float32)
        x64 = x.astype(np.float64)
        loss, grads, logits, state = O.loss_and_grads(spec, params, x64, y, CFG, training=True)
        _, g32, _, _ = O.loss_and_grads(spec, p32, x, y, CFG, training=True)
        gref, g32 = O.flatten(spec, grads), O.flatten(spec, g32).astype(np.float64)
        cost = _per_tensor_abs(spec, g32, gref)
        logit_ref = O.predict(spec, params, x64)[1]
        logit32 = O.predict(spec, p32, x)[1].astype(np.float64)
        per, _ = O.weighted_crossentropy(y, logit_ref, **CFG)
        loss_eval = float(per.mean(dtype=np.float64)) + O.l2_penalty(spec, params)
        # the two float64 statements agree (tests/golden/make_golden.py's bounds)
        for training, lg in ((True, logits), (False, logit_ref)):
            t = torch_ref.run(spec, params, x64, y, CFG, training=training)
            assert np.abs(lg - t['logits']).max() < 1e-10, (name, seed, training)
            if training:
                assert abs(loss - t['loss']) < 1e-10 * max(1.0, abs(loss)), (name, seed)
                for n, g in grads.items():
                    assert np.abs(g - t['grads'][n]).max() <= 1e-9 * np.abs(t['grads'][n]).max() + 1e-13, (name, seed, n)
                for n, s in t['state'].items():
                    assert np.abs(state[n] - s).max() < 1e-10, (name, seed, n)
        # the float32 oracle is clean on this seed: no healthy tensor is off by more than 1e-4 of its scale (a flipped ReLU mask or
        # max-pool winner would be; its error would then pass into the floor)
        deg = Hp.degenerate_tensors(spec)
        for (n, sl), e in zip(Hp.tensor_slices(spec), cost):
            assert n in deg or e <= 1e-4 * np.abs(gref[sl]).max(), (name, seed, n, e)
        _REF[(name, seed)] = dict(spec=spec, params=params, x=x, y=y, loss=loss, gref=gref, floor=[10 * e for e in cost], cost=cost,
                                  state=O.flatten(spec, dict(params, **state), trainable=False) if state else None,
                                  logit_ref=logit_ref, logit_cost=float(np.abs(logit32 - logit_ref).max()), loss_eval=loss_eval)
    return _REF[(name, seed)]


def _model(gpu, name, generic):
    c = CASES[name]
    r = _case(name, SEEDS[0])
    m = gpu.DeviceModel(**Hp.device_kwargs(r['spec'], c['H'], c['W'], B, force_generic=generic))
    m.set_params(O.flatten(r['spec'], r['params']))
    return m


def _reset_state(m, r):
    if m.n_state:
        m.set_state(O.flatten(r['spec'], r['params'], trainable=False))


def _worst(spec, g, gref):
    deg = Hp.degenerate_tensors(spec)          # rounding noise in any float32 implementation: judged by their floor, not reported
    errs = {n: e for n, e in Hp.per_tensor_err(spec, g, gref).items() if n not in deg}
    n = max(errs, key=errs.get)
    return n, errs[n]


def _train_step(gpu, name, generic):
    """{seed: (loss, gradients, state after the step)} of one train step per input seed on the device -- run once per (case, model)"""
    if (name, generic) not in _DEV:
        m = _model(gpu, name, generic)
        try:
            out = {}
            for seed in SEEDS:
                r = _case(name, seed)
                _reset_state(m, r)
                step = m.train_step(r['x'], r['y'], 0.0, m.loss_cfg(**CFG))
                out[seed] = (step.loss, m.get_grads().astype(np.float64), m.get_state() if m.n_state else None)
            plan = ([k for k, _, _ in m.plan()], [k for k, _, _ in m.plan(variants=True)])
        finally:
            m.close()
        _DEV[(name, generic)] = (out, plan)
    return _DEV[(name, generic)]


def _arith(k):
    """a launch that computes a conv, a pool or a transposed conv (tuned or generic), as opposed to loss, optimizer, BatchNorm
    bookkeeping and copies"""
    return any(s in k for s in ('conv', 'pool', 'pg', 'ig_', 'ig3x', 'fz', 'strip', 'tail', 'blk', 'up'))


@pytest.mark.parametrize('generic', [True, False], ids=['generic', 'tuned'])
@pytest.mark.parametrize('name', list(CASES))
def test_train_step_against_oracle(gpu, name, generic):
    out, (plan, variants) = _train_step(gpu, name, generic)
    what = '%s %s' % (name, 'generic' if generic else 'tuned')
    counts = {k: plan.count(k) for k in sorted(set(plan))}
    print('%s plan: %s' % (what, ' '.join('%s x%d' % kv for kv in counts.items())))
    failed = []
    for seed in SEEDS:
        r = _case(name, seed)
        spec = r['spec']
        loss, g, state = out[seed]
        wn, we = _worst(spec, g, r['gref'])
        c32 = max(e / (np.abs(r['gref'][sl]).max() + 1e-300) for (n, sl), e in zip(Hp.tensor_slices(spec), r['cost'])
                  if n not in Hp.degenerate_tensors(spec))
        serr = float(np.abs(state - r['state']).max()) if state is not None else 0.0
        print('%s seed %d: loss %.9g ref %.9g (err %.2e of bound 1e-4); worst gradient tensor %s %.3e of its scale (float32 oracle: '
              'worst healthy tensor %.3e; bound 2e-5 + 10 x its own float32 cost); moving statistics err %.2e (bound 1e-5)' % (
                  what, seed, loss, r['loss'], abs(loss - r['loss']) / max(1.0, abs(r['loss'])), wn, we, c32, serr))
        if not abs(loss - r['loss']) <= 1e-4 * max(1.0, abs(r['loss'])):
            failed.append((seed, 'loss', loss, r['loss']))
        try:
            Hp.assert_grads_per_tensor(spec, g, r['gref'], 2e-5, floor=r['floor'], what='%s seed %d gradient' % (what, seed))
        except AssertionError as e:
            failed.append((seed, str(e)))
        if not serr <= 1e-5:
            failed.append((seed, 'moving statistics', serr))
    assert not failed, failed
    Hp.record_oracle_plan(variants, 'test_train_step_against_oracle')
    if not generic:
        generic_kernels = [k for k in counts if k.startswith(('g_conv', 'g_pool', 'g_tconv'))]
        tuned_kernels = [k for k in counts if not k.startswith('g_') and _arith(k)]
        print('%s: generic conv / pool / tconv launches %s; tuned arithmetic launches %s' % (what, generic_kernels, tuned_kernels))
        if CASES[name]['mixed']:
            assert generic_kernels and tuned_kernels, (name, counts)
        assert ' '.join('%s:%d' % kv for kv in counts.items()) == PLANS[name], (name, counts)
    else:
        assert all(k.startswith('g_') for k in counts), counts


@pytest.mark.parametrize('name', list(CASES))
def test_tuned_against_generic(gpu, name):
    tuned, _ = _train_step(gpu, name, False)
    plain, _ = _train_step(gpu, name, True)
    failed = []
    for seed in SEEDS:
        r = _case(name, seed)
        wn, we = _worst(r['spec'], tuned[seed][1], plain[seed][1])
        print('%s seed %d: tuned vs generic worst gradient tensor %s %.3e of its scale, loss %.9g vs %.9g' % (
            name, seed, wn, we, tuned[seed][0], plain[seed][0]))
        try:
            Hp.assert_grads_per_tensor(r['spec'], tuned[seed][1], plain[seed][1], 2e-5, floor=r['floor'],
                                       what='%s seed %d tuned vs generic' % (name, seed))
        except AssertionError as e:
            failed.append((seed, str(e)))
        if not abs(tuned[seed][0] - plain[seed][0]) <= 1e-4 * max(1.0, abs(plain[seed][0])):
            failed.append((seed, 'loss', tuned[seed][0], plain[seed][0]))
    assert not failed, failed


@pytest.mark.parametrize('generic', [True, False], ids=['generic', 'tuned'])
@pytest.mark.parametrize('name', list(CASES))
def test_inference_against_oracle(gpu, name, generic):
    m = _model(gpu, name, generic)
    what = '%s %s' % (name, 'generic' if generic else 'tuned')
    try:
        for seed in SEEDS:
            r = _case(name, seed)
            _reset_state(m, r)
            lmax = float(np.abs(r['logit_ref']).max())
            tol = min(10.0 * r['logit_cost'], TI.LOGIT_TOL * max(1.0, lmax))
            print('%s seed %d: float32 oracle cost %.3e, bound %.3e' % (what, seed, r['logit_cost'], tol))
            prob, logits = m.forward(r['x'], training=False, return_logits=True)
            step, prob_e = m.eval_step(r['x'], r['y'], m.loss_cfg(**CFG), return_prob=True)
            TI._assert_inference('%s seed %d forward' % (what, seed), logits, prob, None, r['logit_ref'], r['loss_eval'], tol)
            TI._assert_inference('%s seed %d eval_step' % (what, seed), logits, prob_e, step.loss, r['logit_ref'], r['loss_eval'], tol)
        Hp.record_oracle_plan(m, 'test_inference_against_oracle', mode='eval', batch=B)
    finally:
        m.close()
