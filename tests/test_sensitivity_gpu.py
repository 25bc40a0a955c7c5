"""-m gpu: the input-sensitivity pass (dnnca_input_sensitivity, DeviceModel.input_sensitivity, `annotator evaluate
--visualize_sensitivity`) against the float64 torch-CPU autograd statement tests/sens_ref.py.

Cases (the smallest shapes at which the pass can still go wrong):
  (a) unet, 3 input channels, 3 first filters, 2 levels, BatchNorm, 32 x 48, max_batch 4 run at B = 3 (non-square, ragged batch)
  (b) mulmo, 3 input channels, 16 first filters, 2 levels, BatchNorm, 40 x 48, B = 2 (dense path, one first conv per encoder)
  (c) configs/unet.yaml's hyper-parameters with 3 input channels, B = 1, 512 x 512, once: the first-layer reduction's block and
      ticket structure at full width
(a) and (b) run on a force_generic and on a tuned model.  BatchNorm moving statistics, gammas, betas and biases are perturbed
(helpers.perturbed_params), inputs are uniform random; seeds: parameters helpers.PARAM_SEED, inputs SEED below.

Bound: the same torch statement in float32 against float64 on the same inputs is the cost of the number format; the device's
raw sums must lie within 10 x that cost (max over the [B, C] entries), the rule tests/test_inference_gpu.py uses for logits."""

import csv
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as Hp
import sens_ref
from dnncancerannotator_amd import casewise as CW
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11
CASES = {
    'a': dict(arch='unet', C=3, H=32, W=48, max_batch=4, B=3, opts=dict(n_filters_first=3, n_downsample=2, bn=True)),
    'b': dict(arch='mulmo', C=3, H=40, W=48, max_batch=2, B=2, opts=dict(n_filters_first=16, n_downsample=2, bn=True)),
    'c': dict(arch='unet', C=3, H=512, W=512, max_batch=1, B=1, opts=dict(n_filters_first=3, n_downsample=3, bn=False)),
}
_REF = {}


def _case(name):
    """(spec, device kwargs, params {name: float64 array}, x, float64 reference sums, float32 cost) -- computed once per case"""
    if name not in _REF:
        c = CASES[name]
        full = dict(rate=2, kernel_size=3, conv_stride=1, padding='same')
        full.update(c['opts'])
        spec = O.ModelSpec(c['arch'], c['C'], **full)
        params = Hp.perturbed_params(spec, np.float64)
        x = np.random.default_rng(SEED).random((c['B'], c['H'], c['W'], c['C'])).astype(np.float32)
        ref = sens_ref.sums(spec, params, x, torch.float64)
        cost = float(np.abs(sens_ref.sums(spec, params, x, torch.float32) - ref).max())
        _REF[name] = (spec, Hp.device_kwargs(spec, c['H'], c['W'], c['max_batch']), params, x, ref, cost)
    return _REF[name]


def _model(gpu, name, **extra):
    spec, kw, params, x, ref, cost = _case(name)
    m = gpu.DeviceModel(**dict(kw, **extra))
    m.set_params(O.flatten(spec, params))
    m.set_state(O.flatten(spec, params, trainable=False))
    return m


@pytest.mark.parametrize('name,generic', [('a', True), ('a', False), ('b', True), ('b', False), ('c', False)])
def test_raw_sums_against_float64_autograd(gpu, name, generic):
    spec, kw, params, x, ref, cost = _case(name)
    m = _model(gpu, name, force_generic=generic)
    s = m.input_sensitivity(x)
    again = m.input_sensitivity(x)
    plan = [r[0] for r in m.plan(mode='sensitivity', batch=len(x))]
    m.close()
    err = float(np.abs(s - ref).max())
    print('case %s %s: device err %.3e, float32 cost %.3e (bound %.3e), max sum %.4e, launches: %s' % (
        name, 'generic' if generic else 'tuned', err, cost, 10 * cost, float(ref.max()), ' '.join(sorted(set(plan)))))
    assert s.shape == ref.shape == (len(x), CASES[name]['C']) and s.dtype == np.float64
    assert np.isfinite(s).all() and (ref > 0).all()
    assert err <= 10 * cost, (name, err, cost)
    assert np.array_equal(s, again), 'two runs differ'
    assert np.allclose(CW.normalise_sensitivity(s).sum(1), 1.0, rtol=0, atol=1e-12)
    # data gradients only, the first layer in its own launch, BatchNorm on the moving statistics
    assert plan.count('sens_first') == 1 and plan.count('sens_head') == 1
    assert not [k for k in plan if 'wgrad' in k or 'adam' in k or k.startswith('g_bn_bwd') or k.startswith('g_bn_stats')]
    assert ('bn_infer_bwd' in plan) == bool(spec.bn)
    if name == 'b' and not generic:
        assert any(k.endswith('conv_dgrad') and k != 'g_conv_dgrad' for k in plan), plan      # the dense data-gradient kernels


def _snapshot(m):
    mo, vo, it = m.get_opt_state()
    return [m.get_params(), m.get_state(), mo, vo, np.array([it])]


@pytest.mark.parametrize('name,generic', [('a', True), ('a', False), ('b', False)])
def test_pass_leaves_the_model_and_the_next_train_step_alone(gpu, name, generic):
    spec, kw, params, x, ref, cost = _case(name)
    y = (np.random.default_rng(SEED + 1).random(x.shape[:3]) < 0.1).astype(np.float32)
    m, plain = _model(gpu, name, force_generic=generic), _model(gpu, name, force_generic=generic)
    cfg = m.loss_cfg(weight_mul=3.0)
    m.train_step(x, y, 1e-3, cfg)          # optimizer slots and an iteration count that are not the initial ones
    before = _snapshot(m)
    plain.set_params(before[0])
    plain.set_state(before[1])
    plain.set_opt_state(before[2], before[3], int(before[4][0]))
    m.forward(x, training=False, return_prob=False)
    s = m.input_sensitivity(batch=len(x))          # the slices the forward left on the device
    assert np.array_equal(s, m.input_sensitivity(x))
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
    # two identical steps differ by float-atomics noise only (NOTES.md 2026-10-16, train metrics; run-to-run spread <= 7e-7 of
    # the largest entry, NOTES.md round 5): four times that
    assert np.abs(ga - gb).max() <= 4 * 7e-7 * np.abs(gb).max(), (np.abs(ga - gb).max(), np.abs(gb).max())


def test_zeroed_head_gives_zero_sums_and_nan_rows(gpu):
    spec, kw, params, x, ref, cost = _case('a')
    m = _model(gpu, 'a')
    p = dict(params)
    p['head.kernel'] = np.zeros_like(p['head.kernel'])
    m.set_params(O.flatten(spec, p))
    s = m.input_sensitivity(x)
    m.close()
    assert (s == 0).all()
    assert np.isnan(CW.normalise_sensitivity(s)).all()


def test_argument_errors_and_bf16(gpu):
    import ctypes as C
    from dnncancerannotator_amd import _lib
    spec, kw, params, x, ref, cost = _case('a')
    m = _model(gpu, 'a')
    out = np.zeros((4, 3), np.float64)
    outp = out.ctypes.data_as(C.POINTER(C.c_double))
    xx = np.zeros((4, 32, 48, 3), np.float32)
    assert m.lib.dnnca_input_sensitivity(m.handle, _lib.fptr(xx), 0, outp) == -1
    assert m.lib.dnnca_input_sensitivity(m.handle, _lib.fptr(xx), 5, outp) == -1
    assert m.lib.dnnca_input_sensitivity(m.handle, _lib.fptr(xx), 2, None) == -1
    assert m.lib.dnnca_input_sensitivity(None, _lib.fptr(xx), 2, outp) == -1
    m.forward(xx[:2], training=False, return_prob=False)
    assert m.lib.dnnca_input_sensitivity(m.handle, None, 3, outp) == -4          # not the batch the last forward left
    assert m.lib.dnnca_input_sensitivity(m.handle, None, 2, outp) == 0
    m.close()
    h = gpu.DeviceModel(**dict(kw, dtype='bf16'))
    with pytest.raises(_lib.DnncaError) as e:
        h.input_sensitivity(x)
    h.close()
    assert e.value.code == -1 and 'bf16' in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- end to end
def _run(args, env, timeout=600):
    r = subprocess.run([sys.executable, '-m', 'annotator'] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]


def _files(d):
    return sorted(os.path.relpath(os.path.join(a, f), d) for a, _, fs in os.walk(d) for f in fs)


def test_cli_evaluate_writes_sensitivity_files(gpu, tmp_path):
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
    _run(ev + ['--tag', 'sens', '--visualize_sensitivity'], env)
    _run(ev + ['--tag', 'plain'], env)
    tfe = os.path.join(save, 'tfevents')
    with_flag, without = _files(os.path.join(tfe, 'sens')), _files(os.path.join(tfe, 'plain'))
    extra = [f for f in with_flag if '_sensitivity.' in f]
    assert not [f for f in without if 'sensitivity' in f]
    assert sorted(set(with_flag) - set(extra)) == without          # without the flag: exactly the file set of before
    for f in without:                                              # ... and the same bytes
        assert open(os.path.join(tfe, 'sens', f), 'rb').read() == open(os.path.join(tfe, 'plain', f), 'rb').read(), f

    config = load.load_config(os.path.join(save, 'options.yaml'))['config']
    m = engine.TFKerasModel(config)
    ds = make_dataset([data], config['data_options']['eval'], training=False, include_meta=True)
    m._build(ds)
    m.load(os.path.join(save, 'checkpoints', 'ckpt-4'))
    n = 0
    for x, y, tpaths, ids in ds:
        sens = CW.normalise_sensitivity(m.device_model.input_sensitivity(np.asarray(x, np.float32)))
        assert np.isfinite(sens).all()
        for row, p, k in zip(sens, tpaths, ids):
            tag = CW.tag_of(p, k)
            text = open(CW.sensitivity_path(os.path.join(tfe, 'sens'), tag, 4, 'csv')).read()
            assert text == CW.sensitivity_csv(['ch0', 'ch1', 'ch2'], row)
            table = list(csv.reader(io.StringIO(text)))
            assert table[0] == ['', '0'] and [r[0] for r in table[1:]] == ['ch0', 'ch1', 'ch2']
            png = open(CW.sensitivity_path(os.path.join(tfe, 'sens'), tag, 4, 'images'), 'rb').read()
            assert png == CW.encode_png(CW.sensitivity_chart(row))
            n += 1
    m.device_model.close()
    assert n > 0 and len(extra) == 2 * n
