"""-m gpu: the integrated-gradients pass (dnnca_integrated_gradients, DeviceModel.integrated_gradients, `annotator evaluate
--visualize_attribution`) against the float64 torch-CPU autograd statement tests/attr_ref.py.  Cases, panel and references:
tests/attr_cases.py.

Bound (the project's rule): the device must lie within 10 x the float32-vs-float64 cost of the same statement -- max-abs error for
`signed`, `absolute` and `endpoints`, relative L2 error for the map; per case and quantity the cost is the largest over the panel
of 8 input seeds, both baselines and the step counts 1, 4, 16 (a flipped ReLU mask is part of that cost, attr_cases.py).  Case (e)
(LeakyReLU 0.999: no flip can hide a wrong mask) holds the map in max-abs norm as well.  Every test prints device error, cost and
bound per case before it asserts."""

import csv
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import attr_cases as AC
import attr_ref
from dnncancerannotator_amd import casewise as CW
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = AC.PANEL[0]


def _model(gpu, name, params=None, **extra):
    spec, kw, p = AC.spec_of(name)
    p = p if params is None else params
    m = gpu.DeviceModel(**dict(kw, **extra))
    m.set_params(O.flatten(spec, p))
    m.set_state(O.flatten(spec, p, trainable=False))
    return m


def _worst(gpu, name, generic, steps, panel):
    """the largest device error per quantity over panel x baselines x steps, with where it occurred"""
    m = _model(gpu, name, force_generic=generic)
    worst = {q: (0.0, None) for q in AC.QUANTITIES}
    for seed in panel:
        x = AC.input_of(name, seed)
        for st in steps:
            for bl in attr_ref.BASELINES:
                got = m.integrated_gradients(x, steps=st, baseline=bl, return_map=True)
                assert got.signed.dtype == got.absolute.dtype == got.endpoints.dtype == np.float64 and got.map.dtype == np.float32
                assert got.signed.shape == got.absolute.shape == (len(x), x.shape[3]) and got.endpoints.shape == (len(x), 2)
                assert got.map.shape == x.shape and all(np.isfinite(v).all() for v in got)
                for q, e in AC.errors(got, AC.reference(name, seed, st, bl)[0]).items():
                    if e >= worst[q][0]:
                        worst[q] = (e, (seed, st, bl))
    m.close()
    return worst


def _report_and_check(name, generic, worst, cost, quantities):
    failed = []
    for q in AC.QUANTITIES:
        e, where = worst[q]
        held = q in quantities
        print('case %s %s %-9s device err %.3e  float32 cost %.3e  bound %.3e  at (seed, steps, baseline) %s%s' % (
            name, 'generic' if generic else 'tuned', q, e, cost[q], 10 * cost[q], where, '' if held else '  (not held)'))
        if held and not e <= 10 * cost[q]:
            failed.append((q, e, cost[q], where))
    assert not failed, (name, generic, failed)


@pytest.mark.parametrize('name,generic', [('a', True), ('a', False), ('b', True), ('b', False), ('d', True), ('d', False),
                                          ('e', True), ('e', False)])
def test_attribution_against_float64_autograd(gpu, name, generic):
    worst = _worst(gpu, name, generic, AC.STEPS, AC.PANEL)
    held = AC.QUANTITIES if name == 'e' else AC.QUANTITIES[:4]          # (e): the map in max-abs norm as well
    _report_and_check(name, generic, worst, AC.pooled_cost(name), held)


def test_attribution_at_full_width(gpu):
    """(c): configs/unet.yaml's network at 512 x 512, B = 1, steps = 2, the panel, both baselines.  At this size a decision a
    rounding error away from a tie (a ReLU mask, a max-pool argmax: the low-contrast path images of the mean baseline have many
    near-ties) flips in some input of the panel, on the device or in the float32 statement, and moves the map by 1e-4 .. 1e-3 of
    its norm around one spot; without one the map agrees to 1e-7 (NOTES.md)"""
    worst = _worst(gpu, 'c', False, (2,), AC.PANEL)
    _report_and_check('c', False, worst, AC.pooled_cost('c', steps=(2,)), AC.QUANTITIES[:4])


@pytest.mark.parametrize('name,generic', [('a', False), ('b', False), ('d', True)])
def test_two_calls_give_identical_bits_and_the_map_is_optional(gpu, name, generic):
    x = AC.input_of(name, SEED)
    m = _model(gpu, name, force_generic=generic)
    for bl in attr_ref.BASELINES:
        one = m.integrated_gradients(x, steps=4, baseline=bl, return_map=True)
        two = m.integrated_gradients(x, steps=4, baseline=bl, return_map=True)
        bare = m.integrated_gradients(x, steps=4, baseline=bl)
        for a, b in zip(one, two):
            assert np.array_equal(a, b), 'two runs differ'
        assert bare.map is None
        for a, b in zip(one[:3], bare[:3]):
            assert np.array_equal(a, b), 'the sums depend on return_map'
        # the sums are those of the map that came back
        assert np.allclose(one.signed, one.map.astype(np.float64).sum((1, 2)), rtol=0, atol=1e-9 * np.abs(one.map).sum())
    m.close()


def _snapshot(m):
    mo, vo, it = m.get_opt_state()
    return [m.get_params(), m.get_state(), mo, vo, np.array([it])]


@pytest.mark.parametrize('name,generic', [('a', True), ('a', False), ('b', False)])
def test_pass_leaves_the_model_and_the_next_train_step_alone(gpu, name, generic):
    x = AC.input_of(name, SEED)
    y = (np.random.default_rng(SEED + 1).random(x.shape[:3]) < 0.1).astype(np.float32)
    m, plain = _model(gpu, name, force_generic=generic), _model(gpu, name, force_generic=generic)
    cfg = m.loss_cfg(weight_mul=3.0)
    m.train_step(x, y, 1e-3, cfg)          # optimizer slots and an iteration count that are not the initial ones
    before = _snapshot(m)
    plain.set_params(before[0])
    plain.set_state(before[1])
    plain.set_opt_state(before[2], before[3], int(before[4][0]))
    m.forward(x, training=False, return_prob=False)
    ig = m.integrated_gradients(batch=len(x), steps=4, baseline='mean', return_map=True)      # the slices the forward left
    for a, b in zip(ig, m.integrated_gradients(x, steps=4, baseline='mean', return_map=True)):
        assert np.array_equal(a, b)
    s = m.input_sensitivity(batch=len(x))          # the staged slices are still the forward's
    assert np.array_equal(s, m.input_sensitivity(x)) and np.array_equal(s, plain.input_sensitivity(x))
    prob = m.last_prob(len(x))
    after = _snapshot(m)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(prob, plain.forward(x, training=False)[..., 0].reshape(prob.shape)), 'the pass touched the probabilities'
    la, lb = m.train_step(x, y, 1e-3, cfg).loss, plain.train_step(x, y, 1e-3, cfg).loss
    ga, gb = m.get_grads(), plain.get_grads()
    m.close()
    plain.close()
    assert la == lb, (la, lb)
    # two identical steps differ by float-atomics noise only: the rule of tests/test_sensitivity_gpu.py
    assert np.abs(ga - gb).max() <= 4 * 7e-7 * np.abs(gb).max(), (np.abs(ga - gb).max(), np.abs(gb).max())


def test_zeroed_head_gives_zero_sums_equal_endpoints_and_nan_shares(gpu):
    spec, kw, params = AC.spec_of('a')
    p = dict(params)
    p['head.kernel'] = np.zeros_like(p['head.kernel'])
    m = _model(gpu, 'a', params=p)
    x = AC.input_of('a', SEED)
    for bl in attr_ref.BASELINES:
        ig = m.integrated_gradients(x, steps=4, baseline=bl, return_map=True)
        assert (ig.signed == 0).all() and (ig.absolute == 0).all() and (ig.map == 0).all()
        assert np.array_equal(ig.endpoints[:, 0], ig.endpoints[:, 1])
        assert np.isnan(CW.attribution_shares(ig.absolute)).all()
        gap, rel = CW.attribution_gap(ig.signed, ig.endpoints)
        assert (gap == 0).all() and np.isnan(rel).all()
    m.close()


@pytest.mark.parametrize('name', ['a', 'd'])
def test_mean_baseline_of_constant_planes_gives_exactly_zero(gpu, name):
    c = AC.CASES[name]
    # values whose plane sums are exact in double and whose mean is the value itself
    consts = np.random.default_rng(SEED).random((c['B'], 1, 1, c['C'])).astype(np.float32)
    x = np.ascontiguousarray(np.broadcast_to(consts, (c['B'], c['H'], c['W'], c['C'])))
    m = _model(gpu, name)
    ig = m.integrated_gradients(x, steps=4, baseline='mean', return_map=True)
    m.close()
    assert (ig.map == 0).all() and (ig.signed == 0).all() and (ig.absolute == 0).all()
    assert np.array_equal(ig.endpoints[:, 0], ig.endpoints[:, 1])


def test_argument_errors_and_refusals(gpu):
    import ctypes as C
    from dnncancerannotator_amd import _lib
    spec, kw, params = AC.spec_of('a')
    m = _model(gpu, 'a')
    dp = C.POINTER(C.c_double)
    s, a, e = (np.zeros((4, 3), np.float64) for _ in range(3))
    sp, ap, ep = (v.ctypes.data_as(dp) for v in (s, a, e))
    xx = np.zeros((4, 32, 48, 3), np.float32)
    call = m.lib.dnnca_integrated_gradients
    assert call(None, _lib.fptr(xx), 2, 4, 0, sp, ap, ep, None) == -1          # handle
    assert call(m.handle, _lib.fptr(xx), 0, 4, 0, sp, ap, ep, None) == -1      # batch
    assert call(m.handle, _lib.fptr(xx), 5, 4, 0, sp, ap, ep, None) == -1
    assert call(m.handle, _lib.fptr(xx), 2, 0, 0, sp, ap, ep, None) == -1      # steps
    assert call(m.handle, _lib.fptr(xx), 2, 257, 0, sp, ap, ep, None) == -1
    assert call(m.handle, _lib.fptr(xx), 2, 4, 2, sp, ap, ep, None) == -1      # baseline
    assert call(m.handle, _lib.fptr(xx), 2, 4, -1, sp, ap, ep, None) == -1
    assert call(m.handle, _lib.fptr(xx), 2, 4, 0, None, ap, ep, None) == -1    # outputs
    assert call(m.handle, _lib.fptr(xx), 2, 4, 0, sp, None, ep, None) == -1
    assert call(m.handle, _lib.fptr(xx), 2, 4, 0, sp, ap, None, None) == -1
    m.forward(xx[:2], training=False, return_prob=False)
    assert call(m.handle, None, 3, 4, 0, sp, ap, ep, None) == -4               # not the batch the last forward left
    assert call(m.handle, None, 2, 4, 0, sp, ap, ep, None) == 0
    assert call(m.handle, None, 2, 256, 1, sp, ap, ep, None) == 0              # the largest step count
    with pytest.raises(ValueError):
        m.integrated_gradients(xx[:2], baseline='grey')
    m.close()
    x = AC.input_of('a', SEED)
    h = gpu.DeviceModel(**dict(kw, dtype='bf16'))
    with pytest.raises(_lib.DnncaError) as err:
        h.integrated_gradients(x)
    h.close()
    assert err.value.code == -1 and 'bf16' in str(err.value)
    from dnncancerannotator_amd import models
    r = models.MultiResUnet(n_channels=5, n_filters_first=4).build([1, 32, 32, 5], seed=0)
    with pytest.raises(_lib.DnncaError) as err:
        r.integrated_gradients(np.zeros((1, 32, 32, 5), np.float32))
    r.close()
    assert err.value.code == -1 and 'MultiResUnet' in str(err.value)


@pytest.mark.parametrize('name,generic', [('a', True), ('b', False), ('d', False)])
def test_plan_lists_the_launches_of_one_call(gpu, name, generic):
    spec, kw, params = AC.spec_of(name)
    x = AC.input_of(name, SEED)
    m = _model(gpu, name, force_generic=generic)
    before = {mode: m.plan(variants=True, mode=mode, batch=len(x)) for mode in ('train', 'eval', 'forward', 'sensitivity')}
    for steps, bl in ((1, 'black'), (4, 'mean'), (3, 'black')):
        ig = m.integrated_gradients(x, steps=steps, baseline=bl)
        plan = [r[0] for r in m.plan(mode='attribution', batch=len(x))]
        assert plan.count('attr_path_in') == steps and plan.count('attr_first') == steps and plan.count('sens_head') == steps
        assert plan.count('attr_finish') == 1 and plan.count('attr_prob_sum') == 2
        assert plan.count('attr_baseline') == (1 if bl == 'mean' else 0)
        assert plan.count('g_head_fwd') == steps + 2           # steps + 2 forwards, steps backward passes
        assert 'sens_first' not in plan
        assert not [k for k in plan if 'wgrad' in k or 'adam' in k or k.startswith('g_bn_bwd') or k.startswith('g_bn_stats')]
        assert ('bn_infer_bwd' in plan) == bool(spec.bn)
        # a dry run: the same call gives the same bits afterwards
        for a, b in zip(ig[:3], m.integrated_gradients(x, steps=steps, baseline=bl)[:3]):
            assert np.array_equal(a, b)
    if name == 'b':
        assert any(k.endswith('conv_dgrad') and k != 'g_conv_dgrad' for k in plan), plan      # the dense data-gradient kernels
    for mode, p in before.items():
        assert m.plan(variants=True, mode=mode, batch=len(x)) == p, mode
    m.close()


# ---------------------------------------------------------------------------------------------------------------- end to end
def _run(args, env, timeout=600):
    r = subprocess.run([sys.executable, '-m', 'annotator'] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]


def _files(d):
    return sorted(os.path.relpath(os.path.join(a, f), d) for a, _, fs in os.walk(d) for f in fs)


def test_cli_evaluate_writes_attribution_files(gpu, tmp_path):
    import yaml
    from dnncancerannotator_amd import engine, load
    from dnncancerannotator_amd.runs.train import make_dataset
    data = 'synthetic:32x32x3'
    cfgs = {
        'unet.yaml': dict(model='UNetAnnotator', model_options=dict(n_filters_first=3, n_downsample=2, rate=2, kernel_size=3,
                                                                     conv_stride=1, bn=True, padding='same')),
        'deploy.yaml': {'deploy_options': {'optimizer': 'adam',
                                           'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}},
                                           'enable_multigpu': False}},
        'data.yaml': {'data_options': {'train': {'batch_size': 4}, 'eval': {'batch_size': 4}}},
    }
    paths = []
    for name, obj in cfgs.items():
        p = tmp_path / name
        p.write_text(yaml.safe_dump(obj))
        paths.append(str(p))
    save = str(tmp_path / 'run')
    env = dict(os.environ, PYTHONPATH=ROOT)
    _run(['train', '--config'] + paths + ['--save_path', save, '--data_path', data, '--max_steps', '4', '--save_freq', '4'], env)
    ev = ['evaluate', '--save_path', save, '--data_path', data, '--export_csv', '--export_images']
    _run(ev + ['--tag', 'attr', '--visualize_attribution', '--attribution_steps', '4'], env)
    _run(ev + ['--tag', 'plain'], env)
    tfe = os.path.join(save, 'tfevents')
    with_flag, without = _files(os.path.join(tfe, 'attr')), _files(os.path.join(tfe, 'plain'))
    extra = [f for f in with_flag if '_attribution.' in f]
    assert not [f for f in without if 'attribution' in f]
    assert sorted(set(with_flag) - set(extra) - {'attribution_results.csv'}) == without      # without the flag: the file set of before
    assert 'attribution_results.csv' in with_flag
    for f in without:                                                                         # ... and the same bytes
        assert open(os.path.join(tfe, 'attr', f), 'rb').read() == open(os.path.join(tfe, 'plain', f), 'rb').read(), f

    config = load.load_config(os.path.join(save, 'options.yaml'))['config']
    m = engine.TFKerasModel(config)
    ds = make_dataset([data], config['data_options']['eval'], training=False, include_meta=True)
    m._build(ds)
    m.load(os.path.join(save, 'checkpoints', 'ckpt-4'))
    names, n, shares_all, rel_all = ['ch0', 'ch1', 'ch2'], 0, [], []
    for x, y, tpaths, ids in ds:
        ig = m.device_model.integrated_gradients(np.asarray(x, np.float32), steps=4, baseline='black', return_map=True)
        shares = CW.attribution_shares(ig.absolute)
        shares_all += list(shares)
        rel_all += list(CW.attribution_gap(ig.signed, ig.endpoints)[1])
        for b, (p, k) in enumerate(zip(tpaths, ids)):
            tag = CW.tag_of(p, k)
            text = open(CW.attribution_path(os.path.join(tfe, 'attr'), tag, 4, 'csv')).read()
            assert text == CW.attribution_csv(names, shares[b], ig.signed[b], ig.absolute[b], ig.endpoints[b])
            table = list(csv.reader(io.StringIO(text)))
            assert [r[0] for r in table] == ['modality'] + names + ['f_x', 'f_baseline', 'gap', 'relative_gap']
            png = open(CW.attribution_path(os.path.join(tfe, 'attr'), tag, 4, 'images'), 'rb').read()
            assert png == CW.encode_png(CW.attribution_image(ig.map[b], names))
            n += 1
    m.device_model.close()
    assert n > 0 and len(extra) == 2 * n
    table = list(csv.reader(open(os.path.join(tfe, 'attr', 'attribution_results.csv'))))
    assert table[0] == ['step'] + CW.ATTRIBUTION_RESULT_COLUMNS + ['share_%s' % c for c in names] + ['mean_relative_gap', 'max_relative_gap']
    assert len(table) == 2 and table[1] == [str(v) for v in [4] + CW.attribution_summary(4, 'black', shares_all, rel_all)]
