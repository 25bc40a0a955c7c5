"""-m gpu: MultiResUnet (configs/multiresunet.yaml) on the device against its float64 reference statement (tests/multires_ref.py).

All cases: f32, 5 input channels, labels that are discs with some positives in every image.  Tolerances:
  inference   logits within min(10 x the float32 reference's own error against float64 on the same inputs, 2e-4 max(1, max|logit|))
              (the rule of tests/test_inference_gpu.py), probabilities the same + 2^-22, masks at 0.5 bit-exact wherever the reference
              logit is farther than the logit tolerance from the threshold
  train step  loss 1e-4 relative; gradients PER VARIABLE max|g - g_ref| <= 2e-5 max|g_ref| + 10 x what the float32 reference costs on
              that variable; moving statistics 1e-5; the Adam update against oracle.adam_step on the device's gradient within 1e-5 lr
ReLU is fixed in this network, so the flip lottery of DESIGN section 2 applies: the input seeds of the train-step cases were picked
on the CPU with the reference alone (tools/multires_seed_scan.py, multires_ref.decision_safety), so that the float64 and the
float32 run take every ReLU and max-pool decision the same way, with the most room to spare.  n_filters_first 4, seeds 0 .. 159:
seed 2 has the largest ratio of a tensor's smallest decision margin to the float32 run's largest deviation on that tensor, 4.7 --
no float32 arithmetic of that accuracy can flip a decision there.  n_filters_first 32 has 1.3 M decisions and no such seed (best
0.4): of the seeds 0 .. 127, 28 are clean for the single-threaded float32 run, 4 for all three float32 summation orders the scan
tries (one thread, all threads, the non-oneDNN convolutions), and seed 122 has the most room over the three (every decision's margin
at least 1.7 x the run's deviation at that element).  The test asserts on the CPU side that the float32 reference of the machine it
runs on is itself within the bounds for the seeds, so a seed that drifts fails loudly instead of loosening anything."""

import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import multires_ref as R
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

PARAM_SEED, PERTURB = 7, 0.1          # seeded glorot kernels; betas, gammas and moving statistics off their symmetric start
TRAIN_SEEDS = {4: 2, 32: 122}         # n_filters_first -> input seed (see above)
LR = 0.05                             # one float32 rounding of a weight in [1, 2) is 6e-8: the 1e-5 lr bound must stay above it
LOGIT_TOL = 2e-4
PROB_ROUNDING = 2.0 ** -22
GRAD_TOL = 2e-5
# what a float32 run of the reference may cost per variable for its seed to count as clean: the clean seeds of the scan cost at most
# 1e-4 of a variable's scale (tools/multires_seed_scan.py, 'worst tensor'), a seed with a flipped decision 5e-3 and more; the floor is for
# the variables whose gradient is analytically zero (block9.out_bn.beta: a shift in front of conv 1x1 + BatchNorm; float32 noise 1e-8)
F32_COST, F32_FLOOR = 3e-4, 1e-7


def _model(gpu, nff, B, H, W):
    from dnncancerannotator_amd import models
    dm = models.MultiResUnet(n_channels=5, n_filters_first=nff).build([B, H, W, 5], seed=0)
    p, s = R.init(5, nff, PARAM_SEED, PERTURB)
    dm.set_params(p)
    dm.set_state(s)
    return dm, p, s


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def test_variables_match_the_reference_statement(gpu):
    dm, _, _ = _model(gpu, 4, 1, 16, 16)
    try:
        lay, (nt, ns) = R.layout(5, 4)
        infos = dm.param_infos()
        assert [(n, s, t) for n, s, t, off in infos] == R.param_specs(5, 4)
        assert [off for n, s, t, off in infos] == [lay[n][0] for n, s, t, off in infos]
        assert (dm.n_trainable, dm.n_state) == (nt, ns)
    finally:
        dm.close()


@pytest.mark.parametrize('B,H,W', [(2, 32, 32), (1, 16, 16), (2, 32, 48)])
def test_inference_at_reference_widths(gpu, B, H, W):
    """moving statistics, betas and gammas at non-trivial values; 1 x 16 x 16: the bottom level is 1 x 1"""
    dm, p, s = _model(gpu, 32, B, H, W)
    try:
        x = np.random.default_rng(11 + H + W).standard_normal((B, H, W, 5)).astype(np.float32)
        ref = R.run(p, s, x, n_filters_first=32)['logits']
        ref32 = R.run(p, s, x, n_filters_first=32, dtype=torch.float32)['logits']
        lmax = float(np.abs(ref).max())
        e32 = float(np.abs(ref32 - ref).max())
        tol = min(10.0 * e32, LOGIT_TOL * max(1.0, lmax))
        prob, logits = dm.forward(x, training=False, return_logits=True)
        err = float(np.abs(logits - ref).max())
        perr = float(np.abs(prob - _sigmoid(ref)).max())
        print('inference %dx%dx%d: |logit|max %.3f float32 reference %.2e tol %.2e device %.2e prob %.2e' % (B, H, W, lmax, e32, tol, err, perr))
        assert err <= tol, (err, tol)
        assert perr <= tol + PROB_ROUNDING, (perr, tol)
        decided = np.abs(ref) > tol
        assert np.array_equal((prob > 0.5)[decided], (ref > 0)[decided]), 'mask flip away from the threshold'
        # the dry plan of the inference pass: every join is one join_infer launch
        names = [k for k, _, _ in dm.plan(mode='forward')]
        assert names.count('join_infer') == 19 and 'join_fwd' not in names and 'g_join_fwd' not in names
    finally:
        dm.close()


@functools.lru_cache(maxsize=None)
def _train_reference(nff):
    """float64 and float32 reference of one train step of the case (computed once, shared, never modified)"""
    seed = TRAIN_SEEDS[nff]
    p, s = R.init(5, nff, PARAM_SEED, PERTURB)
    x = np.random.default_rng(seed).standard_normal((2, 32, 32, 5)).astype(np.float32)
    y = R.discs(2, 32, 32, seed + 1000)
    r64 = R.run(p, s, x, y, nff, training=True)
    r32 = R.run(p, s, x, y, nff, training=True, dtype=torch.float32)
    for r in (r64, r32):
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return x, y, r64, r32


def _device_step(gpu, nff):
    x, y, _, _ = _train_reference(nff)
    dm, p, s = _model(gpu, nff, 2, 32, 32)
    try:
        out = dm.train_step(x, y, LR, dm.loss_cfg())
        names = [k for k, _, _ in dm.plan()]
        return dict(loss=out.loss, grads=dm.get_grads().astype(np.float64), params=dm.get_params(), state=dm.get_state(), p0=p,
                    it=dm.get_opt_state()[2], plan=names)
    finally:
        dm.close()


@functools.lru_cache(maxsize=None)
def _device_step_cached(gpu, nff):
    return _device_step(gpu, nff)


def _assert_step(nff, dev, what):
    x, y, r64, r32 = _train_reference(nff)
    lay = r64['lay']
    by_tensor, by_element = R.decision_safety(r64, r32)
    print('%s: seed %d: float32 reference takes the float64 decisions: %s; safety by tensor %.2f, by element %.2f' % (
        what, TRAIN_SEEDS[nff], R.same_decisions(r64['decisions'], r32['decisions']), by_tensor, by_element))
    assert R.same_decisions(r64['decisions'], r32['decisions']), \
        'seed %d: the float32 reference takes a ReLU / max-pool decision the float64 reference does not' % TRAIN_SEEDS[nff]
    print('%s: loss %.7f reference %.7f' % (what, dev['loss'], r64['loss']))
    bad, worst = [], 0.0
    for name, (off, shape, tr) in lay.items():
        if not tr:
            continue
        sl = slice(off, off + int(np.prod(shape)))
        scale = float(np.abs(r64['grads'][sl]).max())
        cost = float(np.abs(r32['grads'][sl] - r64['grads'][sl]).max())
        err = float(np.abs(dev['grads'][sl] - r64['grads'][sl]).max())
        allowed = GRAD_TOL * scale + 10.0 * cost
        if name in ('block1.conv3.kernel', 'block1.conv5.kernel', 'block1.shortcut.kernel', 'head.kernel'):
            print('   %-24s scale %.2e float32 reference %.1e device %.1e allowed %.1e' % (name, scale, cost, err, allowed))
        worst = max(worst, err / allowed)
        if not err <= allowed:
            bad.append((name, scale, cost, err, allowed))
    print('   %d of %d gradient tensors out of bounds; worst error / allowed %.3f' % (len(bad), sum(t for _, _, t in lay.values()), worst))
    # the CPU side first: plain float32 on THIS machine is itself within the bounds for the seed (a seed whose float32 run flips a
    # ReLU or max-pool decision costs 5e-3 .. 4e-1 of a tensor's scale and would loosen the 10 x term above: it fails here instead)
    for name, (off, shape, tr) in lay.items():
        if tr:
            sl = slice(off, off + int(np.prod(shape)))
            cost = float(np.abs(r32['grads'][sl] - r64['grads'][sl]).max())
            assert cost <= F32_COST * float(np.abs(r64['grads'][sl]).max()) + F32_FLOOR, \
                'seed %d: the float32 reference is off by %.2e on %s' % (TRAIN_SEEDS[nff], cost, name)
    assert abs(r32['loss'] - r64['loss']) <= 1e-4 * abs(r64['loss'])
    assert np.abs(r32['state'] - r64['state']).max() <= 1e-5
    assert np.isfinite(dev['loss']) and abs(dev['loss'] - r64['loss']) <= 1e-4 * abs(r64['loss']), (dev['loss'], r64['loss'])
    assert not bad, '%s: %d gradient tensors out of bounds (name, scale, float32 cost, error, allowed): %s' % (what, len(bad), bad[:6])
    serr = float(np.abs(dev['state'] - r64['state']).max())
    assert serr <= 1e-5, serr
    # k_adam on the device's own gradient, first step
    named_p = R.unflatten(lay, dev['p0'].astype(np.float64))
    named_g = R.unflatten(lay, dev['grads'])
    want = R.flatten(lay, O.adam_step(named_p, named_g, {}, {}, 1, LR))
    assert dev['it'] == 1
    uerr = float(np.abs((dev['params'].astype(np.float64) - dev['p0']) - (want - dev['p0'])).max())
    assert uerr <= 1e-5 * LR, uerr


@pytest.mark.parametrize('nff', [4, 32])
def test_train_step_against_the_reference(gpu, nff):
    dev = _device_step_cached(gpu, nff)
    _assert_step(nff, dev, 'train step n_filters_first %d' % nff)
    assert dev['plan'].count('join_fwd') == 19 and dev['plan'].count('join_bwd') == 19
    assert 'g_join_fwd' not in dev['plan'] and 'g_join_bwd' not in dev['plan']


@pytest.mark.parametrize('nff', [4, 32])
def test_slices_of_the_concat_accumulate_their_two_gradients(gpu, nff):
    """slices b and c of a block's concat tensor receive gradient from the concat BatchNorm AND from the next conv: accumulation
    flags keyed on the base pointer would let conv7's backward overwrite slice b's gradient, which shows in the kernels of the
    convs that produce a and b"""
    dev = _device_step_cached(gpu, nff)
    _, _, r64, r32 = _train_reference(nff)
    for name in ('block1.conv5.kernel', 'block1.conv3.kernel', 'block5.conv5.kernel', 'block9.conv3.kernel'):
        off, shape, _ = r64['lay'][name]
        sl = slice(off, off + int(np.prod(shape)))
        scale = float(np.abs(r64['grads'][sl]).max())
        allowed = GRAD_TOL * scale + 10.0 * float(np.abs(r32['grads'][sl] - r64['grads'][sl]).max())
        err = float(np.abs(dev['grads'][sl] - r64['grads'][sl]).max())
        assert err <= allowed, 'gradient of %s: error %.3e of scale %.3e, allowed %.3e (the gradient of a concat slice was overwritten?)' % (
            name, err, scale, allowed)


def test_no_join_switch_gives_the_same_step(gpu, monkeypatch):
    monkeypatch.setenv('DNNCA_NO_JOIN', '1')          # read once per model, at creation
    dev = _device_step(gpu, 4)
    monkeypatch.delenv('DNNCA_NO_JOIN')
    _assert_step(4, dev, 'DNNCA_NO_JOIN train step')
    assert dev['plan'].count('g_join_fwd') == 19 and dev['plan'].count('g_join_bwd') == 19
    assert not any(k in dev['plan'] for k in ('join_fwd', 'join_bwd', 'join_infer'))
    with_join = _device_step_cached(gpu, 4)
    assert 'join_fwd' in with_join['plan'] and 'join_bwd' in with_join['plan']


# ---- the join kernels alone ------------------------------------------------------------------------------------------------
_FP, _DP = C.POINTER(C.c_float), C.POINTER(C.c_double)


def _debug_join(dm, what, B, H, W, Cn, ps, c0, grid, generic, in0, in1, io0, io1=None, coef=None, sums=None, acc=(0, 0)):
    fn = dm.lib.dnnca_debug_join
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [C.c_int] * 9 + [_FP, _FP, _FP, _FP, _FP, _DP, C.c_int, C.c_int]
    ptr = lambda a, t=_FP: None if a is None else a.ctypes.data_as(t)          # noqa: E731
    rc = fn(dm.handle, what, B, H, W, Cn, ps, c0, grid, generic, ptr(in0), ptr(in1), ptr(io0), ptr(io1), ptr(coef), ptr(sums, _DP), acc[0], acc[1])
    assert rc == 0, dm.lib.dnnca_last_error().decode()


# (B, H, W, C, ps, c0): dense with 4 | n (float4 walk, no tail); dense with n % 4 == 1 (float4 walk + scalar tail); one channel; a
# channel slice (17 channels at offset 8 of a 51-channel tensor: the strided walk)
JOIN_SHAPES = [(2, 16, 16, 51, 51, 0), (1, 3, 5, 51, 51, 0), (2, 16, 16, 1, 1, 0), (2, 16, 16, 17, 51, 8)]


@pytest.fixture(scope='module')
def join_model(gpu):
    dm, _, _ = _model(gpu, 4, 1, 16, 16)
    yield dm
    dm.close()


@pytest.mark.parametrize('shape', JOIN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('grid', [0, 37])          # the streaming rule's grid; many blocks for the tensor: the fold order
def test_join_forward_kernels_against_numpy(join_model, shape, grid):
    B, H, W, Cn, ps, c0 = shape
    rng = np.random.default_rng(5)
    a = rng.standard_normal((B * H * W, ps)).astype(np.float32)
    b = rng.standard_normal((B * H * W, ps)).astype(np.float32)
    keep = rng.standard_normal((B * H * W, ps)).astype(np.float32)
    view = slice(c0, c0 + Cn)
    want = keep.copy()
    want[:, view] = np.maximum(a[:, view] + b[:, view], np.float32(0))
    runs = []
    for _ in range(2):
        out, sums = keep.copy(), np.full(Cn, np.nan)
        _debug_join(join_model, 0, B, H, W, Cn, ps, c0, grid, 0, a, b, out, sums=sums)
        assert np.array_equal(out, want)                       # the same float32 add; channels outside the view untouched
        ref = want[:, view].astype(np.float64).sum(0)
        assert np.all(np.abs(sums - ref) <= 1e-6 * np.abs(ref)), (sums, ref)          # every channel on its own sum
        runs.append(sums)
    assert np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64))          # block partials folded in block order
    # without the sums (the kernel's other instantiation) and the generic cross-check
    for generic in (0, 1):
        out = keep.copy()
        _debug_join(join_model, 0, B, H, W, Cn, ps, c0, grid, generic, a, b, out)
        assert np.array_equal(out, want)
    # inference: add, ReLU and the BatchNorm's affine in one pass
    coef = np.concatenate([rng.uniform(0.5, 2.0, Cn), rng.standard_normal(Cn)]).astype(np.float32)
    out = keep.copy()
    _debug_join(join_model, 1, B, H, W, Cn, ps, c0, grid, 0, a, b, out, coef=coef)
    y = want[:, view].astype(np.float64) * coef[:Cn] + coef[Cn:]
    assert np.array_equal(out[:, :c0], keep[:, :c0]) and np.array_equal(out[:, c0 + Cn:], keep[:, c0 + Cn:])
    assert np.abs(out[:, view] - y).max() <= 2.0 ** -22 * max(1.0, float(np.abs(y).max()))          # one fused multiply-add in float32


@pytest.mark.parametrize('shape', JOIN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('acc', [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_join_backward_kernels_against_numpy(join_model, shape, acc):
    B, H, W, Cn, ps, c0 = shape
    rng = np.random.default_rng(6)
    dr = rng.standard_normal((B * H * W, ps)).astype(np.float32)
    r = np.maximum(rng.standard_normal((B * H * W, ps)), 0).astype(np.float32)
    da0 = rng.standard_normal((B * H * W, ps)).astype(np.float32)
    db0 = rng.standard_normal((B * H * W, ps)).astype(np.float32)
    view = slice(c0, c0 + Cn)
    d = np.where(r[:, view] > 0, dr[:, view], np.float32(0))
    wa, wb = da0.copy(), db0.copy()
    wa[:, view] = da0[:, view] + d if acc[0] else d
    wb[:, view] = db0[:, view] + d if acc[1] else d
    for generic, grid in ((0, 0), (0, 37), (1, 0)):
        da, db = da0.copy(), db0.copy()
        _debug_join(join_model, 2, B, H, W, Cn, ps, c0, grid, generic, dr, r, da, db, acc=acc)
        assert np.array_equal(da, wa) and np.array_equal(db, wb), (generic, grid)


# ---- the engine ------------------------------------------------------------------------------------------------------------
def _config(**deploy):
    d = {'optimizer': 'adam', 'enable_multigpu': False,
         'metrics': [{'Precision': {'thresholds': 0.5, 'name': 'pixel/precision'}}, {'Recall': {'thresholds': 0.5, 'name': 'pixel/recall'}}]}
    d.update(deploy)
    return {'model': 'MultiResUnet', 'model_options': {'height': None, 'width': None, 'n_channels': 5}, 'deploy_options': d,
            'data_options': {'train': {'batch_size': 4}, 'eval': {'batch_size': 4}}}


def test_engine_train_eval_checkpoint_predict(gpu, tmp_path):
    from dnncancerannotator_amd import data, engine
    from dnncancerannotator_amd.runs.train import make_dataset
    cfg = _config(train_metrics='device')
    save = str(tmp_path / 'run')
    m = engine.TFKerasModel(cfg)
    res = m.train(data.SyntheticDataset(4, 32, 32, 5, n_batches=2, seed=3), save_path=save, max_steps=3, save_freq=3)
    assert len(res.history['loss']) == 3 and np.all(np.isfinite(res.history['loss']))
    assert len(res.history['pixel/precision']) == 3 and len(res.history['pixel/recall']) == 3          # train_metrics: device
    ev = lambda: data.SyntheticDataset(4, 32, 32, 5, n_batches=2, seed=11, repeat=False)               # noqa: E731
    rows = m.eval(ev(), save_path=save, tag='a', export_csv=True)
    assert list(rows) == [3] and set(rows[3]) == {'loss', 'pixel/precision', 'pixel/recall'} and np.isfinite(rows[3]['loss'])
    # the checkpoint in a fresh model: the same evaluation, bit for bit
    fresh = engine.TFKerasModel(cfg)
    again = fresh.eval(ev(), save_path=save, tag='b')
    assert again[3]['loss'] == rows[3]['loss']
    assert np.array_equal(fresh.device_model.get_params(), m.device_model.get_params())
    assert np.array_equal(fresh.device_model.get_state(), m.device_model.get_state())
    # annotator predict: lesion tables from the device
    ds = make_dataset(['synthetic:32x32x5'], cfg['data_options']['eval'], training=False, include_meta=True, labels=False)
    out = str(tmp_path / 'out')
    info = fresh.annotate(ds, save, out, threshold=0.5, filter_size=3)
    assert info['step'] == 3 and info['slices'] > 0
    assert sorted(os.listdir(out)) == ['lesions.csv', 'slices.csv']
    with pytest.raises(NotImplementedError):
        fresh.eval(ev(), save_path=save, tag='c', visualize_sensitivity=True)
    with pytest.raises(Exception, match='MultiResUnet'):
        fresh.device_model.input_sensitivity(np.zeros((1, 32, 32, 5), np.float32))          # refused by the library too, before any launch


def test_loss_goes_down_over_twenty_steps(gpu):
    from dnncancerannotator_amd import models
    dm = models.MultiResUnet(n_channels=5, n_filters_first=8).build([4, 32, 32, 5], seed=0)
    try:
        x = np.random.default_rng(1).standard_normal((4, 32, 32, 5)).astype(np.float32)
        y = R.discs(4, 32, 32, 2)
        x[..., 0] += 2.0 * y                                    # something to learn
        losses = [dm.train_step(x, y, 1e-3, dm.loss_cfg()).loss for _ in range(20)]
        print('losses', ' '.join('%.4f' % v for v in losses))
        assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]
        assert np.mean(losses[-5:]) < np.mean(losses[:5])
    finally:
        dm.close()
