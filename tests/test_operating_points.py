"""CPU only: the cases of tests/operating_points.py on the oracle alone.  Every case is decidable by the reference (the float32
oracle takes the float64 oracle's decisions), every exact-zero case contains the zeros and ties it claims, each of the two wrong
rules moves it by more than ten times what the device is allowed, the saturated cases are saturated, and the float64 oracle does
not see the transposed-conv bias shift."""

import numpy as np
import pytest

import helpers as Hp
import operating_points as OP

IDS = [OP.case_id(c) for c in OP.all_cases()]


@pytest.mark.parametrize('case', OP.all_cases(), ids=IDS)
def test_every_case_is_decidable_by_the_reference_alone(case):
    """the float32 oracle within 1e-4 of every non-degenerate tensor's scale and of the loss: clean inputs cost 2e-6 .. 7e-5, an
    input on which float32 flips a ReLU mask or a pool argmax >= 3.8e-4.  A case that fails gets another seed in
    operating_points.ZERO_SEED, never a wider bound"""
    spec = OP.build(case)[0]
    ref = OP.reference(case)
    cost = OP.float32_cost(spec, ref['grads'], ref['grads32'])
    worst = max(cost, key=cost.get)
    print('%s: loss %.9g float32 oracle: loss err %.2e worst tensor %s %.2e' % (
        OP.case_id(case), ref['loss'], abs(ref['loss32'] - ref['loss']) / max(1.0, abs(ref['loss'])), worst, cost[worst]))
    assert np.isfinite(ref['grads']).all() and np.isfinite(ref['loss'])
    assert abs(ref['loss32'] - ref['loss']) <= 1e-4 * max(1.0, abs(ref['loss']))
    bad = {n: e for n, e in cost.items() if not e <= 1e-4}
    assert not bad, bad
    assert all(np.abs(ref['grads'][sl]).max() > 0 for n, sl in Hp.tensor_slices(spec) if n in cost)


@pytest.mark.parametrize('case', OP.zero_cases(), ids=[OP.case_id(c) for c in OP.zero_cases()])
def test_exact_zero_case_contains_ties_and_zeros_and_has_teeth(case):
    """at the first encoder level there are tied pool windows and exactly-zero values; act'(0) = 1 moves at least one tensor by
    more than 10 x its allowed error in every case, the last-maximum pool rule in every LeakyReLU case (under ReLU a tie at 0 is
    killed by act'(0) = 0: a ReLU case claims only the activation rule, and the figure is printed).

    Under BatchNorm the tied windows are those of a constant region: a window is tied only where the second conv's output is
    constant, so its input is constant one pixel further out and the first conv's two pixels further out -- every activation
    that the gradient of any of the four elements reaches is the same constant, and each weight, bias and BatchNorm gradient is a
    sum that does not depend on which element was taken (the same holds level by level).  The pool rule therefore cannot show in
    a parameter gradient there (asserted: the last-maximum oracle agrees to rounding); a BatchNorm case claims the activation rule
    alone, and the pool rule under BatchNorm is held by the per-pixel attribution map of test_operating_points_gpu.py"""
    spec, params, x, y, _ = OP.build(case)
    tied, windows, zeros, values = OP.first_level_counts(spec, params, x)
    ref = OP.reference(case)
    moved = {}
    for rule in OP.WRONG_RULES:
        e = OP.errors_over_allowance(spec, OP.wrong_rule_grads(case, rule), ref['grads'], ref['allowed'])
        moved[rule] = (max(e.values()), sum(v > 10.0 for v in e.values()), len(e))
    print('%s: %d of %d windows tied, %d of %d values exactly zero; act\'(0) = 1: worst %.3g x allowed, %d of %d tensors off; '
          'last maximum: worst %.3g x allowed, %d of %d tensors off' % ((OP.case_id(case), tied, windows, zeros, values) +
                                                                        moved['act'] + moved['pool']))
    assert tied > 0 and zeros > 0
    assert moved['act'][0] > 10.0
    if case[2] == 'leaky' and not spec.bn:
        assert moved['pool'][0] > 10.0
    if spec.bn:
        assert moved['pool'][0] <= 1e-6


@pytest.mark.parametrize('shape', OP.SATURATE_SHAPES)
def test_saturated_head_is_saturated(shape):
    """the transformed logits span -30 .. 30 (to the float32 rounding of the head), 'agree' labels leave a loss of log1p terms
    only (0.2 .. 0.4) and the case's own labels a loss above 8"""
    for region in (False, True):
        dis, agr = (OP.reference(('saturate', shape, lab, region)) for lab in ('disagree', 'agree'))
        L = dis['logits']
        print('%s region=%d: logits %.4f .. %.4f, loss disagree %.6g agree %.6g' % (shape, region, L.min(), L.max(), dis['loss'], agr['loss']))
        assert abs(L.min() + 30.0) <= 1e-3 and abs(L.max() - 30.0) <= 1e-3
        assert np.array_equal(L, agr['logits'])
        # at least 1 % of the pixels where float32 1 + e is exactly 1, and 1 % where log(1 + e) computed from 1 + e has lost digits
        assert (np.abs(L) > 17.0).mean() >= 0.01 and ((np.abs(L) > 10.0) & (np.abs(L) <= 17.0)).mean() >= 0.01
    dis, agr = (OP.reference(('saturate', shape, lab, False)) for lab in ('disagree', 'agree'))
    assert dis['loss'] > 8.0 and 0.2 <= agr['loss'] <= 0.4, (dis['loss'], agr['loss'])


@pytest.mark.parametrize('shape', OP.SHIFT_SHAPES)
def test_shift_is_invariant_in_the_float64_oracle(shape):
    """moving every transposed-conv bias under BatchNorm by +-16 sigma changes neither the loss nor any gradient of the float64
    oracle by more than 1e-10 (of the tensor's scale; a degenerate tensor: of its sibling's), so the shifted case asks the
    device for exactly what the unshifted one asks -- and the shifted channel really has |mean| = 16 sigma"""
    case = ('shift', shape, OP.SHIFT_SIGMAS)
    spec, shifted, x, y, _ = OP.build(case)
    plain = Hp.perturbed_params(spec, np.float64)
    loss0, g0, _, _ = OP.oracle_run(spec, plain, x, y, False, np.float64)
    ref = OP.reference(case)
    sl = dict(Hp.tensor_slices(spec))
    deg = Hp.degenerate_tensors(spec)
    worst = 0.0
    for n, s in sl.items():
        scale = np.abs(g0[sl[Hp.sibling_of(n)] if n in deg else s]).max()
        worst = max(worst, float(np.abs(ref['grads'][s] - g0[s]).max() / scale))
    print('%s: shift moves the float64 loss by %.2e and the worst tensor by %.2e of its scale' % (shape, abs(ref['loss'] - loss0), worst))
    assert abs(ref['loss'] - loss0) <= 1e-10 and worst <= 1e-10
    sd = OP.tconv_sigmas(spec, plain, x)
    for p, s in sd.items():
        moved = np.abs(shifted[p + '.tconv.bias'] - plain[p + '.tconv.bias'])
        assert np.allclose(moved, OP.SHIFT_SIGMAS * s, rtol=1e-6, atol=0), p
        assert np.allclose(OP.tconv_sigmas(spec, shifted, x)[p], s, rtol=1e-9, atol=0)
    assert any(n.endswith('.tconv.bias') for n in deg)


def test_attribution_case_shows_the_pool_rule_from_the_mean_baseline_only():
    """the last-maximum rule moves the float64 map from the 'mean' baseline by more than 100 x the bound of the device test (10 x
    the float32 cost, relative L2) and leaves the map from the 'black' baseline alone: there (x - x0) is 0 on every tied pixel"""
    import attr_cases as AC
    a = OP.attribution_case()
    moved = {bl: AC.errors(OP.attribution_with_last_maximum(bl), a['ref'][bl])['map_l2'] for bl in ('black', 'mean')}
    print('attribution case: float32 cost %.3e (black) %.3e (mean); the last maximum moves the map by %.3e (black) %.3e (mean)' % (
        a['cost']['black']['map_l2'], a['cost']['mean']['map_l2'], moved['black'], moved['mean']))
    assert a['cost']['mean']['map_l2'] <= 1e-5 and a['cost']['black']['map_l2'] <= 1e-5        # float32 flips no decision
    assert moved['mean'] > 1000 * a['cost']['mean']['map_l2']
    assert moved['black'] == 0.0
    assert (a['x'] == 0).mean() > 0.5
    # the reference's convolutions are written out term by term (operating_points.position_independent_convs): the same statement
    # as tests/attr_ref.py's library calls, to rounding, where no tie of a constant region can show
    import attr_ref
    import torch
    plain = attr_ref.integrated_gradients(a['spec'], a['params'], a['x'], OP.ATTR_STEPS, 'black', torch.float64)
    same = AC.errors(plain, a['ref']['black'])
    print('attribution case: term-by-term convolutions against the library ones: %s' % same)
    assert same['map_l2'] <= 1e-12 and same['endpoints'] <= 1e-10
