"""-m gpu: the first-layer kernels of the input-sensitivity and integrated-gradients passes (sens_first_tile in csrc/sens_first_dev.h,
shared by k_sens_first and k_attr_first) at the shapes tests/test_sensitivity_gpu.py and tests/test_attr_gpu.py do not reach: the
kernel size is a run-time argument up to kSensMaxK = 7, the tile body loops over chunks of 16 output channels and the kernels over
`tpb` tiles per block, and every case of those files has K = 3, at most 16 first filters and tpb == 1.

  s_k5    unet C=3 f0=3 L=2 K=5 BatchNorm, 3 x 24 x 40: the K = 5 halo across the 16 + 8 tile split
  s_k7    unet C=5 f0=3 L=1 K=7, 2 x 24 x 40: kSensMaxK, two input-channel chunks (4 + 1)
  s_f24   unet C=3 f0=24 L=1 BatchNorm, 2 x 24 x 40: the output-channel loop, 16 + a partial chunk of 8
  s_f40m  mulmo C=2 f0=40 L=1 BatchNorm, 2 x 24 x 40: three chunks, one first conv per encoder
  s_tpb   unet C=17 f0=3 L=1, 8 x 112 x 144: 63 tiles x 8 slices x 5 descriptors = 2520 > 2048 blocks, so tpb = 2: 32 blocks per
          (slice, descriptor), the last of one tile; input-channel chunks 4, 4, 4, 4, 1

References: tests/sens_ref.py and tests/attr_ref.py in float64.  Bound: 10 x the same statement in float32 (the rules of
tests/test_sensitivity_gpu.py and tests/test_attr_gpu.py); for the attribution steps = 4, both baselines, the cost of a quantity
pooled over the baselines, the map in relative L2 norm.  Parameters helpers.perturbed_params (seed 2), input seed 11.  Every case runs
on a force_generic and on a tuned model; two calls must give equal bits; every test prints device error, cost and bound first.

Measured on MI355X (NOTES.md 2026-10-19, off-default model_options): sensitivity sums off by 1.7e-7 .. 1.1e-6 at float32 costs of
7.7e-7 .. 3.8e-6 on sums of 6 .. 34; attribution sums 1.7e-7 .. 6.2e-7 and the map 1.5e-7 .. 4.4e-7 of its norm on the four small
cases, generic and tuned alike (at 3, 24 and 40 first filters and at K = 5, 7 every launch of these passes but the first-layer
kernel is a generic one on both models).  s_tpb's path images decide a ReLU mask or a max-pool winner within a
rounding error somewhere on 8 x 112 x 144 x 17 inputs (tests/test_attr_gpu.py, case (c)): its float32 attribution cost is 2.6e-4 on
the sums and 1.1e-3 on the map (device 5.6e-4 / 3.1e-3), so there the attribution only shows that no tile is lost and the
sensitivity sums (cost 3.8e-6, device 1.7e-7) hold the tile loop tightly."""

import numpy as np
import pytest
import torch

import attr_cases as AC
import attr_ref
import helpers as Hp
import sens_ref
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

SEED = 11
STEPS = 4
CASES = {
    's_k5': dict(arch='unet', C=3, B=3, H=24, W=40, opts=dict(n_filters_first=3, n_downsample=2, kernel_size=5, bn=True)),
    's_k7': dict(arch='unet', C=5, B=2, H=24, W=40, opts=dict(n_filters_first=3, n_downsample=1, kernel_size=7, bn=False)),
    's_f24': dict(arch='unet', C=3, B=2, H=24, W=40, opts=dict(n_filters_first=24, n_downsample=1, bn=True)),
    's_f40m': dict(arch='mulmo', C=2, B=2, H=24, W=40, opts=dict(n_filters_first=40, n_downsample=1, bn=True)),
    's_tpb': dict(arch='unet', C=17, B=8, H=112, W=144, opts=dict(n_filters_first=3, n_downsample=1, bn=False)),
}
BOTH = [(n, g) for n in CASES for g in (True, False)]
IDS = ['%s-%s' % (n, 'generic' if g else 'tuned') for n, g in BOTH]
_SPEC, _SENS, _ATTR = {}, {}, {}


def _spec_of(name, **over):
    """(spec, device kwargs, params {name: float64 array}, x)"""
    key = (name, tuple(sorted(over.items())))
    if key not in _SPEC:
        c = CASES[name]
        full = dict(rate=2, kernel_size=3, conv_stride=1, padding='same')
        full.update(c['opts'])
        full.update(over)
        spec = O.ModelSpec(c['arch'], c['C'], **full)
        x = np.random.default_rng(SEED).random((c['B'], c['H'], c['W'], c['C'])).astype(np.float32)
        _SPEC[key] = (spec, Hp.device_kwargs(spec, c['H'], c['W'], c['B']), Hp.perturbed_params(spec, np.float64), x)
    return _SPEC[key]


def _sens(name):
    """(float64 reference sums, float32 cost), computed once"""
    if name not in _SENS:
        spec, kw, params, x = _spec_of(name)
        ref = sens_ref.sums(spec, params, x, torch.float64)
        _SENS[name] = (ref, float(np.abs(sens_ref.sums(spec, params, x, torch.float32) - ref).max()))
    return _SENS[name]


def _attr(name, baseline):
    """(float64 reference (signed, absolute, endpoints, map), {quantity: float32 cost}), computed once"""
    if (name, baseline) not in _ATTR:
        spec, kw, params, x = _spec_of(name)
        ref, f32 = (attr_ref.integrated_gradients(spec, params, x, STEPS, baseline, dt) for dt in (torch.float64, torch.float32))
        _ATTR[(name, baseline)] = (ref, AC.errors(f32, ref))
    return _ATTR[(name, baseline)]


def _model(gpu, name, generic, **over):
    spec, kw, params, x = _spec_of(name, **over)
    m = gpu.DeviceModel(**dict(kw, force_generic=generic))
    m.set_params(O.flatten(spec, params))
    if m.n_state:
        m.set_state(O.flatten(spec, params, trainable=False))
    return m


def test_the_tile_loop_case_has_two_tiles_per_block():
    """the grid arithmetic of sens_first_grid (csrc/kernels_sens.hip) restated: s_tpb is the smallest case of this file's shapes at
    which a block walks more than one tile and the last block is short"""
    c = CASES['s_tpb']
    ntiles = -(-c['H'] // 16) * -(-c['W'] // 16)
    nz = -(-c['C'] // 4)
    tpb = max(1, -(-ntiles * c['B'] * nz // 2048))
    assert (ntiles, nz, ntiles * c['B'] * nz, tpb, -(-ntiles // tpb), ntiles % tpb) == (63, 5, 2520, 2, 32, 1)
    for name in ('s_k5', 's_k7', 's_f24', 's_f40m'):
        c = CASES[name]
        assert -(-c['H'] // 16) * -(-c['W'] // 16) * c['B'] * max(1, -(-c['C'] // 4)) <= 2048, name


@pytest.mark.parametrize('name,generic', BOTH, ids=IDS)
def test_sensitivity_sums_against_float64_autograd(gpu, name, generic):
    spec, kw, params, x = _spec_of(name)
    ref, cost = _sens(name)
    m = _model(gpu, name, generic)
    try:
        s = m.input_sensitivity(x)
        again = m.input_sensitivity(x)
        plan = [r[0] for r in m.plan(mode='sensitivity', batch=len(x))]
    finally:
        m.close()
    err = float(np.abs(s - ref).max())
    print('case %s %s: device err %.3e, float32 cost %.3e (bound %.3e), sums %.4e .. %.4e, launches: %s' % (
        name, 'generic' if generic else 'tuned', err, cost, 10 * cost, float(ref.min()), float(ref.max()), ' '.join(sorted(set(plan)))))
    assert s.shape == ref.shape == (len(x), CASES[name]['C']) and s.dtype == np.float64
    assert np.isfinite(s).all() and (ref > 0).all()
    assert err <= 10 * cost, (name, err, cost)
    assert np.array_equal(s, again), 'two runs differ'
    assert plan.count('sens_first') == 1 and plan.count('sens_head') == 1
    assert ('bn_infer_bwd' in plan) == bool(spec.bn)


@pytest.mark.parametrize('name,generic', BOTH, ids=IDS)
def test_attribution_against_float64_autograd(gpu, name, generic):
    spec, kw, params, x = _spec_of(name)
    m = _model(gpu, name, generic)
    worst = {q: (0.0, None) for q in AC.QUANTITIES}
    try:
        for bl in attr_ref.BASELINES:
            got = m.integrated_gradients(x, steps=STEPS, baseline=bl, return_map=True)
            again = m.integrated_gradients(x, steps=STEPS, baseline=bl, return_map=True)
            plan = [r[0] for r in m.plan(mode='attribution', batch=len(x))]
            assert got.signed.shape == got.absolute.shape == (len(x), x.shape[3]) and got.endpoints.shape == (len(x), 2)
            assert got.map.shape == x.shape and all(np.isfinite(v).all() for v in got)
            for a, b in zip(got, again):
                assert np.array_equal(a, b), 'two runs differ'
            assert plan.count('attr_first') == STEPS and plan.count('sens_head') == STEPS and 'sens_first' not in plan, plan
            for q, e in AC.errors(got, _attr(name, bl)[0]).items():
                if e >= worst[q][0]:
                    worst[q] = (e, bl)
    finally:
        m.close()
    cost = {q: max(_attr(name, bl)[1][q] for bl in attr_ref.BASELINES) for q in AC.QUANTITIES}
    failed = []
    for q in AC.QUANTITIES:
        e, where = worst[q]
        held = q in AC.QUANTITIES[:4]
        print('case %s %s %-9s device err %.3e  float32 cost %.3e  bound %.3e  at baseline %s%s' % (
            name, 'generic' if generic else 'tuned', q, e, cost[q], 10 * cost[q], where, '' if held else '  (not held)'))
        if held and not e <= 10 * cost[q]:
            failed.append((q, e, cost[q], where))
    assert not failed, (name, generic, failed)


def _live_launches(m, run):
    m.profile_reset()
    m.profile_enable(1)
    try:
        run()
    finally:
        m.sync()
        counts = {r[0]: r[1] for r in m.profile()}
        m.profile_enable(0)
        m.profile_reset()
    return counts


def test_kernel_size_9_is_refused_and_nothing_is_launched(gpu):
    """kernel_size 9 is above kSensMaxK: both passes answer DNNCA_EINVAL (-1) before any launch; the model's parameters, state and
    the probabilities of the last forward are what they were"""
    from dnncancerannotator_amd import _lib
    spec, kw, params, x = _spec_of('s_k7', kernel_size=9)
    m = _model(gpu, 's_k7', False, kernel_size=9)
    try:
        m.forward(x, training=False, return_prob=False)
        before = [m.get_params(), m.last_prob(len(x)).copy()]
        for call in (lambda: m.input_sensitivity(x), lambda: m.input_sensitivity(batch=len(x)),
                     lambda: m.integrated_gradients(x, steps=STEPS), lambda: m.integrated_gradients(batch=len(x), steps=STEPS, baseline='mean')):
            def refused():
                with pytest.raises(_lib.DnncaError) as e:
                    call()
                assert e.value.code == -1 and 'kernel_size 9' in str(e.value), str(e.value)
            assert _live_launches(m, refused) == {}
            assert np.array_equal(m.get_params(), before[0]) and np.array_equal(m.last_prob(len(x)), before[1])
        # the model still works: the same forward gives the same probabilities
        m.forward(x, training=False, return_prob=False)
        assert np.array_equal(m.last_prob(len(x)), before[1])
    finally:
        m.close()
