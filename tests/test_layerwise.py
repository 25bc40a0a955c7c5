"""The per-launch checker (tests/layerwise.py) on the oracle alone: no GPU.

A fake device whose op table and stored tensors come from the bf16-emulating statements themselves (tests/fake_layerwise_device.py)
runs every case of tests/layerwise_case.py.  The checker must reproduce it -- error exactly 0 on every bf16-stored tensor, float64
noise on the others -- and the float32 cost term of every launch must stay below 1e-4 of its tensor's scale, or the case could not
decide anything on the device.  Then seven planted defects must each fail by at least ten allowances on the tensor they hit."""

import functools

import numpy as np
import pytest

import layerwise as L
import layerwise_case as LC
from fake_layerwise_device import MUTANTS, FakeDense
from oracle import unet_oracle as O


@functools.lru_cache(maxsize=None)
def _run(name, mutant=None):
    case = LC.CASES[name]
    spec, params, x, y = LC.inputs(case)
    fake = FakeDense(spec, case['H'], case['W'], case['max_batch'], case['dtype'], mutant)
    flat, state0 = O.flatten(spec, params), O.flatten(spec, params, trainable=False)
    fake.set_params(flat)
    fake.set_state(state0)
    return LC.check_model(case, fake.ops_text, fake.forward, lambda xv, yv: fake.train_step(xv, yv, LC.LOSS), fake.tensor, fake.bn_coef,
                          fake.get_grads, fake.get_state, flat, state0, x, y, lambda: False), fake


# float32 coefficients against their float64 definition: one float32 rounding (6e-8) of the mean or of inv, in units of the
# statistics bound (1e-5 of the standard deviation / of inv) -- far below one allowance, and never zero
COEF_KINDS = ('bn_mean', 'bn_inv', 'bn_infer_mean', 'bn_infer_inv', 'bn_coef')


@pytest.mark.parametrize('name', list(LC.CASES))
def test_checker_reproduces_the_emulating_oracle_and_every_case_can_decide(name):
    (r_eval, r_train), fake = _run(name)
    case = LC.CASES[name]
    kinds = set(r['kind'] for r in r_eval + r_train)
    print(name, {k: ('%.2e' % v[0], '%.1e' % v[2]) for k, v in L.summarise(r_eval + r_train).items()})
    for r in r_eval + r_train:
        if r['kind'].endswith('/bf16-stored'):
            assert r['ratio'] == 0.0, r
        elif r['kind'].startswith(COEF_KINDS):
            assert r['ratio'] <= 0.5, r
        else:
            assert r['ratio'] <= 1e-6, r
        assert r['cost'] < L.DECIDABLE, 'the float32 reference costs %.2e of the scale of %s (%s): the case cannot decide' % (r['cost'], r['name'], r['kind'])
    # the case builds what it is there for
    stored = [o['name'] for o in fake.ops if o['out'] and o['out']['hd']]
    if case['dtype'] == 'bf16':
        assert 'conv_fwd[bf16]' in kinds or 'conv_fwd[bf16]/bf16-stored' in kinds
        assert any(k.startswith('dgrad[') for k in kinds) and 'conv_wgrad[bf16]' in kinds
    if case['dtype'] == 'bf16' and case['bn'] and case['f0'] == 64:
        assert {'conv_fwd[bf16]/bf16-stored', 'tconv_fwd[bf16]/bf16-stored', 'bn_apply/bf16-stored', 'dgrad[conv+pool]/bf16-stored',
                'dgrad[bn]/bf16-stored', 'pool', 'bn_mean', 'bn_inv', 'bn_moving_mean', 'bn_moving_variance'} <= kinds, kinds
        assert 'decoder.up0.tconv' in stored
    if not case['bn'] or case['dtype'] == 'f32':
        assert not any(k.endswith('/bf16-stored') for k in kinds) or case['bn'], kinds


def test_a_case_that_cannot_decide_fails_loudly(monkeypatch):
    """the float32-cost condition has teeth of its own: with a float32 statement that is off by 2e-4 of the scale, the assertion above trips"""
    exact = L.conv_out

    def noisy(x, w, b, alpha, bf16, ft):
        out = exact(x, w, b, alpha, bf16, ft)
        return out if ft is np.float64 else out + np.float32(2e-4) * np.abs(out).max()
    monkeypatch.setattr(L, 'conv_out', noisy)
    _run.cache_clear()
    try:
        (r_eval, _), _ = _run('bn64_2x16x16')
    finally:
        _run.cache_clear()
    assert any(r['cost'] >= L.DECIDABLE for r in r_eval if r['kind'].startswith('conv_fwd'))


# mutant -> (case, pass, the result it must trip: kind prefix, name)
TEETH = {
    'halo_column': ('bn64_3of4x24x40', 'train', 'conv_fwd[bf16]', 'decoder.up1.conv0'),
    'dropped_k_chunk': ('bn64_3of4x24x40', 'train', 'conv_fwd[bf16]', 'decoder.up1.conv0'),
    'ragged_next_image': ('bn64_3of4x24x40', 'eval', 'conv_fwd[bf16]', 'decoder.up1.conv0'),
    'skip_overwritten': ('bn64_3of4x24x40', 'train', 'dgrad[conv+pool]', 'd(encoder.down0.bn1.out)'),
    'stale_coefficients': ('bn64_2x16x16', 'train', 'bn_apply', 'encoder.down1.bn0'),
    'stats_unrounded': ('bn64_2x16x16', 'train', 'bn_', 'decoder.up0.tconv_bn'),
    'tconv_mean_without_bias': ('bn64_2x16x16', 'train', 'bn_mean', 'decoder.up0.tconv_bn'),
}


@pytest.mark.parametrize('mutant', MUTANTS)
def test_planted_defects_fail_by_ten_allowances(mutant):
    name, which, kind, tensor = TEETH[mutant]
    (r_eval, r_train), _ = _run(name, mutant)
    res = r_eval if which == 'eval' else r_train
    hit = [r for r in res if r['kind'].startswith(kind) and r['name'] == tensor]
    assert hit, (kind, tensor, sorted(set((r['kind'], r['name']) for r in res))[:8])
    worst = max(r['ratio'] for r in hit)
    print('%s: %s %s off by %.3g allowances' % (mutant, kind, tensor, worst))
    assert worst >= 10.0, hit
    # and the launch that is wrong is the one that is named: nothing upstream of it moves
    (c_eval, c_train), _ = _run(name)
    clean = {(r['kind'], r['name']) for r in (c_eval if which == 'eval' else c_train)}
    assert {(r['kind'], r['name']) for r in res if r['ratio'] > 1.0} <= clean


def test_the_interval_rule_is_the_rounding_of_a_value_within_the_allowance():
    ref = np.array([1.0, 1.00390625 - 1e-7, -3.0, 0.0])      # the second sits just below a tie between two bf16 values
    a = 1e-6
    up = L.to_bf16(ref + a)
    assert L.smallest_multiple(L.to_bf16(ref), [(ref, a, None)], True) == 0.0
    assert up[1] != L.to_bf16(ref)[1]
    t = L.smallest_multiple(up, [(ref, a, None)], True)
    assert 0.0 < t <= 1.0
    off = L.to_bf16(ref).copy()
    off[0] += 2.0 ** -7                                        # one bf16 step: half a step (2^-8) away from any value near ref
    assert L.smallest_multiple(off, [(ref, a, None)], True) > 1000.0


def test_parse_round_trip():
    case = LC.CASES['bn64_2x16x16']
    fake = FakeDense(LC.spec_of(case), 16, 16, 2)
    ops = L.parse_ops(fake.ops_text())
    assert [o['type'] for o in ops[:4]] == ['CONV', 'BN', 'CONV', 'BN'] and ops[-1]['type'] == 'HEAD'
    T = L.tensor_table(ops)
    skip = ops[3]['out'].id
    assert sorted(ops[r]['type'] for r, _ in T[skip]['readers']) == ['CONV', 'POOL']
    assert ops[4]['accA'] == 1 and ops[1]['maskA'] == 1 and ops[0]['premasked'] == 1
