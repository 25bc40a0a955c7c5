"""-m gpu: the device at three operating points that training reaches and the other oracle tests do not (cases, inputs and
transforms: tests/operating_points.py; what each case contains and that a wrong rule fails it: tests/test_operating_points.py).

  exact zeros    a zero background under zero biases: act'(0) and the element of a tied max-pool window decide the gradient
  saturated head logits of -30 .. 30: the log(1 + e) and sigmoid tails of every head / loss kernel
  shifted bias   a transposed-conv bias 16 sigma off in front of its BatchNorm: the raw-moment statistics

Every case runs the tuned plan (whose launches it asserts from the dry plan) and force_generic.  Bounds, for every train step:
loss within 1e-4 max(1, |loss|) (the 'agree' labels of the saturated head: 1e-4 |loss|, the loss is below 1 there); every
gradient tensor within 2e-5 max|g_ref| + 10 x the float32 oracle's error on that tensor (operating_points.allowance, the rule of
test_block_fused_backward_against_oracle), degenerate tensors against their sibling.  Every test prints its figures before it
asserts.

Measured on an MI355X (NOTES.md 2026-10-20), worst tensor error over its allowance: exact zeros 0.016 .. 0.093; saturated head
0.03 .. 0.31 ('agree' loss within 2.0e-6 relative); shifted bias at 16 sigma 0.05 .. 0.09 tuned and 0.13 .. 0.26 generic (tuned
before k_ig_tconv_fwd2 summed the moments of z - bias: 1.47 on c16, 0.56, 0.53); probabilities 8.6e-8, tails 1.7e-7 relative; the
attribution map 1.36e-7 relative L2 against a float32 cost of 1.16e-7."""

import re

import numpy as np
import pytest

import attr_cases as AC
import attr_ref
import helpers as Hp
import operating_points as OP
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

# the launches of the tuned plan that a case is meant to hold (from the dry plan, DeviceModel.plan())
BN_POOL = ('bn_apply_pool', 'bn_bwd_reduce', 'bn_bwd_apply')        # k_bn_apply_pool_fast records the window positions ...
WANT_ZERO = {
    # whole 128 x 32 tiles at every level: the strip kernels and all four block-fused backward launches
    ('u3_3x32x128', 'relu'): ('first3_fwd', 'up3_fwd', 'tail3_3x1_3', 'first3_bwd', 'fzb_up_6', 'fzb_up_12', 'fzb_down_6_12', 'fzb_down_3_6'),
    # LeakyReLU: the pool fold keeps the per-layer kernels (its tie rule is ReLU's), so k_pool2_bwd runs at all three levels
    ('u3_3x32x128', 'leaky'): ('tail3_3x1_3', 'fzb_up_6', 'fzb_up_12', 'pool2_bwd_12', 'pool2_bwd_6', 'pool2_bwd_3', 'bwd3v_3x1_3'),
    ('u3_2x40x128', 'relu'): ('tail3_3x1_3', 'pgbwd_tc_3x2_3', 'pool2_bwd_12', 'pool2_bwd_6', 'first3_bwd'),
    ('u3_2x40x128', 'leaky'): ('tail3_3x1_3', 'pgbwd_tc_3x2_3', 'pool2_bwd_12', 'pool2_bwd_6', 'pool2_bwd_3', 'bwd3v_3x1_3'),
    ('c3', 'relu'): ('tail3_3x1_3', 'pool2_bwd_12', 'pool2_bwd_6', 'first3_bwd', 'g_act_bwd'),
    ('c3', 'leaky'): ('tail3_3x1_3', 'pool2_bwd_12', 'pool2_bwd_6', 'pool2_bwd_3', 'pgbwd_3x1_3', 'g_act_bwd'),
    ('c64', 'relu'): ('head_train_64', 'ig3x_conv_dgrad', 'g_pool_bwd', 'g_act_bwd'),
    ('c64', 'leaky'): ('head_train_64', 'ig3x_conv_dgrad', 'g_pool_bwd', 'g_act_bwd'),
}
WANT_HEAD = {('c3', False): ('tail3_3x1_3',), ('c3', True): ('head_region_fwd_3', 'head_region_train_3'),
             ('c16', False): ('head_train_16',), ('c16', True): ('head_region_fwd_16', 'head_region_train_16'),
             ('c64', False): ('head_train_64',), ('c64', True): ('head_region_fwd_64', 'head_region_train_64')}
LOGITS_ARM = ('region_sums', 'region_loss_finish', 'region_loss_grad')


def _model(gpu, case, generic):
    spec, params, x, y, region = OP.build(case)
    act = case[2] if case[0] == 'zero' else 'relu'
    m = gpu.DeviceModel(**OP.device_kwargs(case[1], act, force_generic=generic))
    m.set_params(O.flatten(spec, params))
    if m.n_state:
        m.set_state(O.flatten(spec, params, trainable=False))
    if region:
        m.set_region_loss({})
    return m


def _step(m, case, what):
    """one train step at lr 0 against the float64 oracle: (|loss error|, {tensor: error / allowed}), printed"""
    spec, params, x, y, region = OP.build(case)
    ref = OP.reference(case)
    out = m.train_step(x, y, 0.0, m.loss_cfg(**OP.LOSS))
    e = OP.errors_over_allowance(spec, m.get_grads(), ref['grads'], ref['allowed'])
    worst = max(e, key=e.get)
    err_loss = abs(out.loss - ref['loss'])
    print('%s %s: loss %.9g ref %.9g (err %.2e, relative %.2e); worst tensor %s at %.3f of its allowance, %d of %d over' % (
        OP.case_id(case), what, out.loss, ref['loss'], err_loss, err_loss / abs(ref['loss']), worst, e[worst],
        sum(v > 1.0 for v in e.values()), len(e)))
    return err_loss, e, ref


def _assert_grads(e):
    bad = {n: round(v, 3) for n, v in e.items() if not v <= 1.0}
    assert not bad, '%d of %d tensors over their allowance: %s' % (len(bad), len(e), bad)


def _names(m, case):
    return [r[0] for r in m.plan(batch=OP.SHAPES[case[1]]['B'])]


@pytest.mark.parametrize('generic', [False, True], ids=['tuned', 'generic'])
@pytest.mark.parametrize('case', OP.zero_cases(), ids=[OP.case_id(c) for c in OP.zero_cases()])
def test_exact_zeros_and_ties(gpu, case, generic):
    """a zero background under zero biases, ReLU and LeakyReLU(0.3): every backward kernel's restatement of act'(0) = slope and of
    the first-maximum pool rule against the oracle's.  Without BatchNorm a LeakyReLU case holds both rules and a ReLU case the
    activation rule; under BatchNorm a case holds the activation rule (test_operating_points.py says why and proves each)"""
    m = _model(gpu, case, generic)
    try:
        names = _names(m, case)
        spec = OP.build(case)[0]
        if not generic:
            want = BN_POOL if spec.bn else WANT_ZERO[(case[1], case[2])]
            assert set(want) <= set(names), (want, names)
            if spec.bn:         # ... and the BatchNorm's backward passes route the pooled gradient by them (variant p1 / p2)
                variants = [r[0] for r in m.plan(variants=True, batch=OP.SHAPES[case[1]]['B'])]
                assert any(re.match(r'bn_bwd_apply#.*p[12]', n) for n in variants), variants
        err_loss, e, ref = _step(m, case, 'generic' if generic else 'tuned')
        assert err_loss <= 1e-4 * max(1.0, abs(ref['loss']))
        _assert_grads(e)
        if not generic:
            Hp.record_oracle_plan(m, 'test_exact_zeros_and_ties', batch=OP.SHAPES[case[1]]['B'])
    finally:
        m.close()


@pytest.mark.parametrize('generic', [False, True], ids=['tuned', 'generic'])
@pytest.mark.parametrize('case', OP.saturate_cases(), ids=[OP.case_id(c) for c in OP.saturate_cases()])
def test_saturated_head(gpu, case, generic):
    """logits of -30 .. 30 through every head and loss kernel of a train step: the fused heads (tail3, head_train_16 / 64,
    head_region_*) and the from-logits arms (g_loss, region_sums / region_loss_grad).  'agree' labels leave a loss made of
    log(1 + e) terms alone, held relatively"""
    _, shape, labels, region = case
    m = _model(gpu, case, generic)
    try:
        names = _names(m, case)
        if generic:
            assert [n for n in names if 'region' in n or n == 'g_loss'] == (list(LOGITS_ARM) if region else ['g_loss']), names
        else:
            assert set(WANT_HEAD[(shape, region)]) <= set(names), names
        err_loss, e, ref = _step(m, case, 'generic' if generic else 'tuned')
        assert err_loss <= (1e-4 * abs(ref['loss']) if labels == 'agree' else 1e-4 * max(1.0, abs(ref['loss'])))
        _assert_grads(e)
        if not generic and not region:
            Hp.record_oracle_plan(m, 'test_saturated_head', batch=OP.SHAPES[shape]['B'])
    finally:
        m.close()


@pytest.mark.parametrize('generic', [False, True], ids=['tuned', 'generic'])
@pytest.mark.parametrize('shape', OP.SATURATE_SHAPES)
def test_saturated_probabilities(gpu, shape, generic):
    """forward(training=False) with the saturated head: probabilities finite and in [0, 1], within 2^-22 of the float64 sigmoid
    of the device's own logits, and within 1e-5 relative wherever that sigmoid is below 1e-3 (one float32 exp and one divide cost
    about 3e-7: a tail that flushes to 0 or loses digits fails)"""
    case = ('saturate', shape, 'disagree', False)
    spec, _, x, _, _ = OP.build(case)
    m = _model(gpu, case, generic)
    try:
        if spec.bn:         # the inference pass normalises with the moving statistics: the head is scaled on ITS logits
            m.set_params(O.flatten(spec, OP.saturate_head(spec, Hp.perturbed_params(spec, np.float64), x, training=False)))
        names = [r[0] for r in m.plan(mode='forward', batch=len(x))]
        prob, logits = m.forward(x, training=False, return_logits=True)
        want = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
        tail = want < 1e-3
        err = np.abs(prob - want)
        rel = float((err[tail] / want[tail]).max()) if tail.any() else 0.0
        print('saturated probabilities %s %s: logits %.3f .. %.3f, %d of %d pixels in the tail; max error %.3e (2^-22 = %.3e), tail '
              'relative error %.3e; head launches %s' % (shape, 'generic' if generic else 'tuned', logits.min(), logits.max(), int(tail.sum()),
                                                         tail.size, err.max(), 2.0 ** -22, rel, [n for n in names if 'head' in n or 'sigmoid' in n]))
        assert np.isfinite(logits).all() and np.abs(logits).max() > 17.0 and tail.any()
        assert np.isfinite(prob).all() and prob.min() >= 0.0 and prob.max() <= 1.0
        assert err.max() <= 2.0 ** -22
        assert rel <= 1e-5
    finally:
        m.close()


def _worst_relative(spec, g, gref):
    """(tensor, error of its scale) of the worst tensor, a degenerate one against its sibling's scale"""
    sl = dict(Hp.tensor_slices(spec))
    deg = Hp.degenerate_tensors(spec)
    e = {n: float(np.abs(g[s] - gref[s]).max() / np.abs(gref[sl[Hp.sibling_of(n)] if n in deg else s]).max()) for n, s in sl.items()}
    worst = max(e, key=e.get)
    return worst, e[worst]


@pytest.mark.parametrize('generic', [False, True], ids=['tuned', 'generic'])
@pytest.mark.parametrize('shape', OP.SHIFT_SHAPES)
def test_shifted_transposed_conv_bias_under_batchnorm(gpu, shape, generic):
    """every *.tconv.bias 16 sigma off, sign alternating by channel: loss, every gradient tensor and the moving variances (1e-5)
    against the oracle on the shifted parameters.  The statistics of the tuned plan are raw moments of float32 partial sums.
    The worst tensor at 4, 16 and 64 sigma is printed (NOTES.md); the assertion stands at 16"""
    case = ('shift', shape, OP.SHIFT_SIGMAS)
    spec, params, x, y, _ = OP.build(case)
    what = 'generic' if generic else 'tuned'
    m = _model(gpu, case, generic)
    try:
        names = _names(m, case)
        if not generic:
            assert {'ig_tconv_fwd', 'bn_apply', 'bn_bwd_reduce', 'bn_bwd_apply'} <= set(names), names
        before = m.get_state().copy()
        err_loss, e, ref = _step(m, case, what)
        state = dict(params)
        state.update(ref['state'])
        want = O.flatten(spec, state, trainable=False)
        got = m.get_state().astype(np.float64)
        err_var = max(float(np.abs(got[s] - want[s]).max()) for n, s in Hp.tensor_slices(spec, trainable=False) if n.endswith('moving_variance'))
        print('shift %s %s: moving variances off by %.3e' % (shape, what, err_var))
        for sig in (4.0, 64.0):
            other = ('shift', shape, sig)
            p2 = OP.build(other)[1]
            m.set_params(O.flatten(spec, p2))
            m.set_state(before)
            out = m.train_step(x, y, 0.0, m.loss_cfg(**OP.LOSS))
            r2 = OP.reference(other, with_float32=False)
            print('shift %s %s at %g sigma: loss err %.2e, worst tensor %s %.3e of its scale' % (
                (shape, what, sig, abs(out.loss - r2['loss'])) + _worst_relative(spec, m.get_grads().astype(np.float64), r2['grads'])))
        print('shift %s %s at 16 sigma: loss err %.2e, worst tensor %s %.3e of its scale' % (
            (shape, what, err_loss) + _worst_relative(spec, _grads_again(m, case, before), ref['grads'])))
        assert err_loss <= 1e-4 * max(1.0, abs(ref['loss']))
        _assert_grads(e)
        assert err_var <= 1e-5
        if not generic:
            Hp.record_oracle_plan(m, 'test_shifted_transposed_conv_bias_under_batchnorm', batch=OP.SHAPES[shape]['B'])
    finally:
        m.close()


def _grads_again(m, case, state):
    spec, params, x, y, _ = OP.build(case)
    m.set_params(O.flatten(spec, params))
    m.set_state(state)
    m.train_step(x, y, 0.0, m.loss_cfg(**OP.LOSS))
    return m.get_grads().astype(np.float64)


@pytest.mark.parametrize('generic', [False, True], ids=['tuned', 'generic'])
def test_attribution_map_on_a_zero_background(gpu, generic):
    """the per-pixel integrated-gradients map shows which pixel of a tied window received the gradient: behind the first BatchNorm
    the background is a constant and every window of it a four-way tie.  From the 'mean' baseline the background of every path
    image is a non-zero constant and the map there is (x - x0) times the gradient, so a gradient routed to another element of a
    tied window moves the map (test_operating_points.py: the last-maximum rule moves it by far more than the bound); from the
    'black' baseline the path keeps the background at exactly 0.0 and the first conv's output there, and the map must be 0
    wherever x is.  The rule of tests/test_attr_gpu.py: the map within 10 x the float32 cost of the same statement, relative L2;
    torch routes a tied window's gradient to its first maximum and differentiates LeakyReLU at 0 with the slope, as the oracle"""
    a = OP.attribution_case()
    m = gpu.DeviceModel(**dict(a['kw'], force_generic=generic))
    try:
        m.set_params(O.flatten(a['spec'], a['params']))
        m.set_state(O.flatten(a['spec'], a['params'], trainable=False))
        background = (a['x'] == 0)
        failed = []
        for bl in attr_ref.BASELINES:
            got = m.integrated_gradients(a['x'], steps=OP.ATTR_STEPS, baseline=bl, return_map=True)
            e, cost = AC.errors(got, a['ref'][bl]), a['cost'][bl]
            print('attribution on a zero background %s %s: map L2 error %.3e (float32 cost %.3e, bound %.3e), max-abs %.3e (cost %.3e)' % (
                'generic' if generic else 'tuned', bl, e['map_l2'], cost['map_l2'], 10 * cost['map_l2'], e['map_max'], cost['map_max']))
            assert np.isfinite(got.map).all()
            if bl == 'black':
                assert not got.map[background].any()
            else:
                assert np.abs(got.map[background]).max() > 0
            if not e['map_l2'] <= 10 * cost['map_l2']:
                failed.append((bl, e['map_l2'], cost['map_l2']))
        assert not failed, failed
    finally:
        m.close()
