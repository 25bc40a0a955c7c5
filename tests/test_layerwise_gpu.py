"""-m gpu: every launch of the dtype-bf16 dense plans against the float64 statement of that one operation on the device's OWN stored
inputs (tests/layerwise.py), in a child process per case with DNNCA_IGB_NW = 4 / 8 (tests/layerwise_case.py; the library reads the
switch once per process).  Bounds, none of them new: per tensor 2e-5 of its scale + 10 x what the float32 statement costs on the same
stored inputs; bf16-stored tensors element by element inside [to_bf16(ref - a), to_bf16(ref + a)]; BatchNorm mean within 1e-5 of the
channel's standard deviation, inv within 1e-5 relative (each + 10 x the float32 cost), moving statistics within 1e-5.

This is the bound the whole-step comparison (tests/test_engine_gpu.py::test_bf16_kernels_against_bf16_emulating_oracle) cannot
give: there bf16 rounding flips cascade through the layers (2e-2 per tensor at 16 x 16, 'worst tensor <= 0.8' with BatchNorm over
two levels); here device and reference differ by one fp32 accumulation, at any size.  Measured on an MI355X (NOTES.md, 2026-10-20,
per-launch bound): every launch kind of every case at 0 .. 0.08 of its allowance, both wave variants; the float32 cost term is
1e-7 .. 4e-6 of a tensor's scale (tests/test_layerwise.py proves on the CPU that it stays below 1e-4 for every case)."""

import json
import os
import subprocess
import sys

import pytest

import helpers as Hp
import layerwise_case as LC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _child(name, nw, **env):
    r = subprocess.run([sys.executable, os.path.join(HERE, 'layerwise_case.py'), name], env=dict(os.environ, DNNCA_IGB_NW=str(nw), **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _print(o, nw):
    for which in ('eval', 'train'):
        for kind, (ratio, name, cost) in sorted(o[which].items()):
            print('%-20s w%d %-5s %-32s worst %.3g of its allowance (%s), float32 cost %.1e of scale' % (o['case'], nw, which, kind, ratio, name, cost))


@pytest.mark.parametrize('nw', [4, 8])
@pytest.mark.parametrize('name', [n for n, c in LC.CASES.items() if not c.get('shift')])
def test_every_launch_against_its_own_stored_inputs(gpu, name, nw):
    case = LC.CASES[name]
    o = _child(name, nw)
    _print(o, nw)
    assert not o['fail_eval'], o['fail_eval']
    assert not o['fail_train'], o['fail_train']
    # the read-back aids refuse batch > max_batch, a wrong n and a view without a buffer: DNNCA_EINVAL and a message
    assert [rc for rc, _ in o['refusals']] == [-1, -1, -1] and all(msg for _, msg in o['refusals']), o['refusals']
    assert 'batch' in o['refusals'][0][1] and 'floats expected' in o['refusals'][1][1] and 'no data buffer' in o['refusals'][2][1], o['refusals']
    plan, kinds = set(o['plan']), set(o['train']) | set(o['eval'])
    Hp.record_oracle_plan(plan, 'test_every_launch_against_its_own_stored_inputs')
    Hp.record_oracle_plan(set(o['plan_eval']), 'test_every_launch_against_its_own_stored_inputs', mode='eval')
    if case['dtype'] == 'f32':          # the control: the split-bf16 / fp32 kernels through the same checker
        assert not any(n.startswith('igb_') for n in plan) and 'ig_tconv_fwd' in plan, plan
        assert not o['bf16_stored'] and {'conv_fwd[f32]', 'tconv_fwd[f32]', 'conv_wgrad[f32]', 'tconv_wgrad[f32]'} <= kinds
        return
    suffix = '_w%d' % nw
    a16 = '_a16' if case['bn'] else ''
    assert any(n.startswith('igb_conv_fwd' + suffix) for n in plan) and any(n.startswith('igb_conv_dgrad' + suffix) for n in plan), plan
    assert not any(n.startswith('igb_conv') and n.split('#')[0].endswith('_w%d' % (12 - nw)) for n in plan), plan      # the variant under test ran
    if case['f0'] == 64:
        assert {'igb_conv_fwd' + suffix + a16, 'igb_conv_dgrad' + suffix + a16, 'igb_wgrad64', 'igb_tconv_fwd', 'igb_tconv_dgrad', 'igb_tconv_wgrad'} <= plan, plan
        assert 'ig_tconv_fwd' not in plan
    if case['bn']:
        assert 'bn_apply_pool' in plan and o['bf16_stored'], plan
        assert {'conv_fwd[bf16]/bf16-stored', 'tconv_fwd[bf16]/bf16-stored', 'bn_apply/bf16-stored', 'dgrad[conv+pool]/bf16-stored', 'dgrad[bn]/bf16-stored',
                'dgrad[tconv]/bf16-stored', 'bn_mean', 'bn_inv', 'bn_moving_mean', 'bn_moving_variance', 'pool'} <= kinds, kinds
    else:
        assert not o['bf16_stored'] and {'conv_fwd[bf16]', 'tconv_fwd[bf16]', 'dgrad[conv+pool+act]'} <= kinds, kinds
    if case['f0'] == 32:                # mixed: the 32-channel level stays in f32, the 64-channel level stores bf16
        assert {'bn_apply', 'bn_apply/bf16-stored', 'tconv_fwd[f32]', 'tconv_fwd[bf16]/bf16-stored', 'igb_wgrad'} <= kinds | plan
    if case['cin'] == 1:
        assert 'first_fwd' in plan and 'conv_fwd[f32]' in kinds, plan


@pytest.mark.parametrize('nw,z_f32', [(4, False), (8, False), (4, True)])
def test_transposed_conv_bias_16_sigma_off_in_front_of_its_batchnorm(gpu, nw, z_f32):
    """every *.tconv.bias of the first case's network moved by +-16 sigma of its channel (tests/operating_points.py): the BatchNorm
    behind the bf16 transposed conv is held to its statistics bound.  Before k_igb_tconv_fwd / k_igb_tconv_fwd2 took their moments
    from (stored z) - bias this failed: inv of decoder.up1.tconv_bn at 1.4 allowances (raw float32 moments of values 16 sigma from 0
    lose 256 x their digits in sumsq / n - mean^2); every other launch of the case was inside its bound.  z_f32: DNNCA_NO_HALF_Z
    keeps z in f32, which is how the first-generation kernel (k_igb_tconv_fwd) comes to carry the statistics."""
    o = _child('bn64_2x16x16_shift', nw, **(dict(DNNCA_NO_HALF_Z='1') if z_f32 else {}))
    _print(o, nw)
    assert ('igb_tconv_fwd#h1' if z_f32 else 'igb_tconv_fwd#2h1') in o['plan'], o['plan']
    assert ('decoder.up1.tconv.out' in o['bf16_stored']) == (not z_f32), o['bf16_stored']
    assert not o['fail_eval'], o['fail_eval']
    assert not o['fail_train'], o['fail_train']
