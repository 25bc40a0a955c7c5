"""-m gpu: gradient accumulation (dnnca_model_set_accumulation) -- the kernel alone against numpy float32 addition bit for bit, cycles
against the sequential float32 sum of the device's own gradients and the float64 optimizer recurrences of tests/optim_oracle.py,
planted gradients through apply_gradients, the fused arm of the pixel-group plan, the equivalence with one large batch against the
float64 oracle, off means off, the refusals, the data-parallel arm on a one-rank communicator, and the engine end to end."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as Hp
import optim_oracle as OO
from oracle import unet_oracle as O
from test_optimizer_gpu import CASES, LR, UNET3, Session, _unet3

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL, ESTATE = -1, -4
ADAMW_CLIP_EMA = 'adamw_global_clipnorm_ema'


@pytest.fixture(scope='module')
def sessions(gpu):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Session(gpu, name)
        return made[name]
    yield get
    for s in made.values():
        s.m.close()


def _batches(S, n, seed):
    rng = np.random.default_rng(seed)
    return [(rng.random(S.x.shape).astype(np.float32), (rng.random(S.y.shape) < 0.1).astype(np.float32)) for _ in range(n)]


def _profiled(m, fn):
    """fn() with every launch counted -> (its result, {launch name: (launches, bytes per launch)})"""
    m.sync()
    m.profile_reset()
    m.profile_enable(1)
    try:
        out = fn()
        return out, {name: (k, by) for name, k, _, by, _ in m.profile()}
    finally:
        m.profile_enable(0)
        m.profile_reset()


# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38, 1e30, -1e30, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan,
                     1.0, -1.0, 16777216.0, 1.0000001], np.float32)


def _special_pairs(n, seed):
    """acc, g of n elements: every pair of SPECIALS first (as far as n reaches: +-0, denormals, 1e30 / -1e30 pairs, overflow to inf,
    inf - inf, NaN), then normal values over many binades"""
    rng = np.random.default_rng(seed)
    acc = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(np.float32)
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(np.float32)
    a, b = np.meshgrid(SPECIALS, SPECIALS)
    k = min(n, a.size)
    at = rng.permutation(n)[:k]          # anywhere in the vector: body and tail
    acc[at], g[at] = a.ravel()[:k], b.ravel()[:k]
    return acc, g


@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 4097, 2048 * 256 * 4 + 5])
def test_kernel_alone_is_float32_addition_bit_for_bit(sessions, n, first):
    m = sessions('unet3_2x64x256').m
    acc, g = _special_pairs(n, n + first)
    with np.errstate(all='ignore'):
        want = g.copy() if first else acc + g
    got = m.grad_accumulate_of(None if first and n % 2 else acc, g, first)
    assert got.dtype == np.float32 and got.shape == (n,)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)                                            # NaN by position
    assert got[~nan].tobytes() == want[~nan].tobytes()                                   # everything else bit for bit (signed zeros too)
    if n >= SPECIALS.size ** 2:
        assert nan.any() and np.isinf(want).any() and np.any((want == 0) & np.signbit(want))
        if not first:
            tiny = np.float32(1.1754942e-38)
            assert np.any((want != 0) & (np.abs(want) < tiny))                           # denormal sums survive


# ---- 2. cycles against the device's own gradients ---------------------------------------------------------------------------------
@pytest.mark.parametrize('arm', ['adam', ADAMW_CLIP_EMA])
@pytest.mark.parametrize('k', [2, 3])
@pytest.mark.parametrize('name', sorted(CASES))
def test_cycle_against_the_devices_own_gradients(sessions, name, k, arm):
    S = sessions(name)
    m = S.m
    ema = arm == ADAMW_CLIP_EMA
    spec = OO.spec('adam')
    if ema:          # half the norm of one gradient: the clip is active on a mean of such gradients
        spec = OO.spec('adamw', weight_decay=0.05, global_clipnorm=0.5 * float(np.linalg.norm(S.g0.astype(np.float64))))
    S.reset(spec)
    if ema:
        m.set_ema(0.9, warmup=False)
    m.set_accumulation(k)
    batches = _batches(S, 2 * k, 40 + k)
    worst = {}
    try:
        for cycle in range(2):
            p, mm, vv, it = S.state()
            avg, nup = m.get_ema() if ema else (None, 0)
            acc = None
            for j in range(1, k + 1):
                x, y = batches[cycle * k + j - 1]
                out = m.train_step(x, y, LR, S.cfg)
                assert np.isfinite(out.loss)
                g = m.get_grads()
                acc = g.copy() if j == 1 else acc + g                      # the second cycle starts with a = g again
                a, steps, pos = m.get_accumulation()
                assert a.tobytes() == acc.tobytes(), (name, cycle, j)
                assert steps == k and pos == (j if j < k else 0)
                assert m.get_grads().tobytes() == g.tobytes()              # g is never overwritten by the sum
                if j < k:
                    p1, m1, v1, it1 = S.state()
                    assert p1.tobytes() == p.tobytes() and m1.tobytes() == mm.tobytes() and v1.tobytes() == vv.tobytes() and it1 == it
                    if ema:
                        avg1, nup1 = m.get_ema()
                        assert avg1.tobytes() == avg.tobytes() and nup1 == nup
            want = OO.step(spec, S.slices, S.decay, p, mm, vv, acc, it + 1, LR, gscale=1.0 / k)
            p1, m1, v1, it1 = S.state()
            assert it1 == it + 1
            w = OO.check(p1, m1, v1, want)
            if ema:
                total, _ = m.last_grad_norm()
                w['norm'] = float(abs(total - want['norm']) / OO.norm_tol(want['norm'], m.n_trainable))
                assert m.get_ema()[1] == nup + 1
                assert np.abs(m.get_ema()[0] - avg).max() > 0
            assert np.abs(p1 - p).max() > 1e-5
            worst = {key: max(v, worst.get(key, 0.0)) for key, v in w.items()}
        print(name, 'k', k, arm, 'worst error / bound:', ' '.join('%s %.3f' % kv for kv in sorted(worst.items())))
        assert all(v <= 1.0 for v in worst.values()), worst
    finally:
        m.set_accumulation(1)
        m.set_ema(0)


# ---- 3. planted gradients through apply_gradients ---------------------------------------------------------------------------------
PLANTED = ('unet3_2x64x256', 'unet64_f32_10x14')
PLANTED_SPECS = {'adam': OO.spec('adam'), 'adamw_clip': OO.spec('adamw', weight_decay=0.05, global_clipnorm=1.0), 'sgd_nesterov': OO.spec('sgd', momentum=0.9, nesterov=True)}


def _planted(S, spec, vectors, k):
    """the vectors through apply_gradients from the session's start, with accumulation k (1: off) -> (p, m, v, iterations)"""
    S.reset(spec)
    S.m.set_accumulation(k)
    try:
        for g in vectors:
            S.m.apply_gradients(g, LR)
        if k > 1:
            assert S.m.get_accumulation()[2] == len(vectors) % k
        return S.state()
    finally:
        S.m.set_accumulation(1)


@pytest.mark.parametrize('kind', sorted(PLANTED_SPECS))
@pytest.mark.parametrize('name', PLANTED)
def test_planted_gradients_pin_the_mean_the_order_and_gscale(sessions, name, kind):
    S = sessions(name)
    spec = PLANTED_SPECS[kind]
    rng = np.random.default_rng(12)
    c = (rng.standard_normal(S.m.n_trainable) * 10.0 ** rng.integers(-4, 3, S.m.n_trainable)).astype(np.float32)
    # +c, +c, -c, -c: c + c, 2c - c and c - c are exact, the update sees zeros
    zero = _planted(S, spec, [np.zeros_like(c)], 1)
    got = _planted(S, spec, [c, c, -c, -c], 4)
    assert got[3] == zero[3] == 7
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], zero[:3]))
    # four times v: v + v, 2v + v (rounds to even) + v and (4v) * 0.25 give v again -- one update, identical to apply_gradients(v)
    v = (S.g0 * np.float32(3.0)).astype(np.float32)
    s = v + v
    s = s + v
    s = s + v
    assert s.tobytes() == (np.float32(4.0) * v).tobytes() and (s * np.float32(0.25)).tobytes() == v.tobytes()
    once = _planted(S, spec, [v], 1)
    got = _planted(S, spec, [v, v, v, v], 4)
    assert got[3] == once[3] == 7
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], once[:3]))
    assert np.abs(once[0] - S.p0).max() > 1e-5
    # three of the four: nothing has moved
    S.reset(spec)
    before = S.state()
    part = _planted(S, spec, [v, v, v], 4)
    assert part[3] == before[3] and all(a.tobytes() == b.tobytes() for a, b in zip(part[:3], before[:3]))


# ---- 4. the fused arm and the deferred fold ---------------------------------------------------------------------------------------
def _names(m):
    return [r[0] for r in m.plan(mode='train')]


def test_fused_arm_and_the_deferred_fold(gpu, sessions, monkeypatch):
    S = sessions('unet3_2x64x256')
    m, k = S.m, 3
    batches = _batches(S, k, 7)
    unfused = None
    S.reset(OO.spec('adam'))
    n = m.n_trainable
    try:
        # the same batches with accumulation off and lr 0: the step outputs every micro-step must report
        plain = [m.train_step(x, y, 0.0, S.cfg) for x, y in batches]
        S.reset(OO.spec('adam'))                              # (lr 0 has moved the slots and the iteration count)
        monkeypatch.setenv('DNNCA_NO_FOLD_ACC', '1')          # read once per model, where the other step switches are read
        unfused = _unet3(gpu, 2, 64, 256)
        monkeypatch.delenv('DNNCA_NO_FOLD_ACC')
        unfused.set_params(S.p0)
        unfused.set_opt_state(S.m0, S.v0, 6)
        m.set_accumulation(k)
        unfused.set_accumulation(k)
        for j in range(1, k + 1):
            plan, plan_u = _names(m), _names(unfused)
            if j < k:
                assert 'pg_fold_acc' in plan and not {'pg_fold_adam', 'grad_accumulate', 'pg_fold', 'g_adam', 'g_finalize_scalars'} & set(plan), plan
                assert len(plan) == len([r for r in S.plain_plan if r[0] not in ('g_finalize_scalars', 'g_adam')])     # pg_fold -> pg_fold_acc
                assert plan_u[-3:] == ['pg_fold', 'g_finalize_scalars', 'grad_accumulate'] and 'pg_fold_acc' not in plan_u, plan_u
                assert ('pg_fold_acc', (4.0 if j == 1 else 8.0) * n, (0.0 if j == 1 else 1.0) * n) in m.plan(mode='train')
            else:
                for pl in (plan, plan_u):
                    assert [q for q in pl if q in ('pg_fold', 'grad_accumulate', 'g_adam', 'pg_fold_acc', 'pg_fold_adam')] == ['pg_fold', 'grad_accumulate', 'g_adam'], pl
                assert ('grad_accumulate', 12.0 * n, 1.0 * n) in m.plan(mode='train')
            x, y = batches[j - 1]
            out, rows = _profiled(m, lambda: m.train_step(x, y, LR, S.cfg))
            out_u, rows_u = _profiled(unfused, lambda: unfused.train_step(x, y, LR, S.cfg))
            if j < k:
                assert rows['pg_fold_acc'][0] == 1 and not {'pg_fold', 'grad_accumulate', 'g_adam', 'pg_fold_adam', 'g_finalize_scalars'} & set(rows), rows
                assert rows_u['pg_fold'][0] == 1 and rows_u['grad_accumulate'] == (1, (8.0 if j == 1 else 12.0) * n), rows_u
                assert not {'pg_fold_acc', 'g_adam', 'pg_fold_adam', 'g_finalize_scalars'} & set(rows_u), rows_u
                assert sum(r[0] for r in rows.values()) + 1 == sum(r[0] for r in rows_u.values())
            else:
                for r in (rows, rows_u):
                    assert r['pg_fold'][0] == 1 and r['grad_accumulate'] == (1, 12.0 * n) and r['g_adam'][0] == 1, r
                    assert not {'pg_fold_acc', 'pg_fold_adam', 'g_finalize_scalars'} & set(r), r
            # the accumulators of the two arms: bit-identical on the same batch and state
            a, a_u = m.get_accumulation()[0], unfused.get_accumulation()[0]
            print('micro-step', j, 'gradients identical:', m.get_grads().tobytes() == unfused.get_grads().tobytes(),
                  'max |a - a_unfused|', float(np.abs(a - a_u).max()))
            assert a.tobytes() == a_u.tobytes(), j
            for o in (out, out_u):
                for field in ('loss', 'positive_rate', 'weight', 'label_min', 'label_max'):
                    assert getattr(o, field) == getattr(plain[j - 1], field), (j, field)
        assert m.get_params().tobytes() == unfused.get_params().tobytes()
        # conditions of the deferred fold unmet: the generic model accumulates in a launch of its own on every micro-step
        G = sessions('unet3_generic')
        G.reset(OO.spec('adam'))
        G.m.set_accumulation(2)
        try:
            for j in (1, 2):
                plan = _names(G.m)
                assert 'grad_accumulate' in plan and 'pg_fold_acc' not in plan and ('g_adam' in plan) == (j == 2), plan
                G.m.train_step(G.x, G.y, LR, G.cfg)
        finally:
            G.m.set_accumulation(1)
    finally:
        m.set_accumulation(1)
        if unfused is not None:
            unfused.close()


# ---- 5. equivalence with one large batch ------------------------------------------------------------------------------------------
def test_two_micro_batches_are_one_large_batch_against_the_oracle(gpu):
    """unet3 without BatchNorm, a fixed loss weight, no label smoothing: the loss is a mean over the batch's pixels, so the mean of
    the gradients of two micro-batches of 2 is the gradient of the batch of 4.  a / 2 and the large step's own gradient are each
    held to the float64 oracle's gradient of the batch of 4 with the per-tensor bound of the one-step oracle tests (2e-5 of the
    tensor's largest entry: tests/test_engine_gpu.py, test_label_smoothing_loss_matches_oracle)."""
    spec = O.ModelSpec('unet', 1, **UNET3)
    params = Hp.perturbed_params(spec, np.float64)
    B, H, W = 4, 64, 256
    rng = np.random.default_rng(21)
    x = rng.random((B, H, W, 1)).astype(np.float32)
    y = (rng.random((B, H, W)) < 0.1).astype(np.float32)
    cfg = dict(weight=5.0, weight_mul=3.0)
    _, grads, _, _ = O.loss_and_grads(spec, params, x.astype(np.float64), y, cfg, training=True)
    gref = O.flatten(spec, grads)
    m = gpu.DeviceModel('unet', 1, H, W, B, **UNET3)
    try:
        m.set_params(O.flatten(spec, params))
        dcfg = m.loss_cfg(**cfg)
        m.train_step(x, y, 0.0, dcfg)
        large = m.get_grads()
        m.set_accumulation(2)
        m.train_step(x[:2], y[:2], 0.0, dcfg)
        m.train_step(x[2:], y[2:], 0.0, dcfg)
        a, steps, pos = m.get_accumulation()
        assert (steps, pos) == (2, 0)
        mean = a.astype(np.float64) / 2
        e_large = Hp.per_tensor_err(spec, large, gref)
        e_mean = Hp.per_tensor_err(spec, mean, gref)
        print('worst per-tensor error: one step of 4 %.3g, mean of two steps of 2 %.3g' % (max(e_large.values()), max(e_mean.values())))
        Hp.assert_grads_per_tensor(spec, large, gref, 2e-5, what='gradient of the batch of 4')
        Hp.assert_grads_per_tensor(spec, mean, gref, 2e-5, what='mean of the two micro-batch gradients')
    finally:
        m.close()


# ---- 6. off means off -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['unet3_2x64x256', 'unet64_f32_10x14'])
def test_off_means_off(gpu, sessions, name):
    S = sessions(name)
    m = S.m
    S.reset(OO.spec('adam'))
    never = CASES[name][0](gpu)
    try:
        with pytest.raises(Exception, match='accumulation is off') as e:          # a model that never asked holds no accumulator
            never.get_accumulation()
        assert e.value.code == ESTATE
        assert m.plan(variants=True, mode='train') == S.plain_plan == never.plan(variants=True, mode='train')
        m.set_accumulation(3)
        assert m.plan(variants=True, mode='train') != S.plain_plan
        for mode in ('eval', 'forward'):
            assert m.plan(variants=True, mode=mode) == never.plan(variants=True, mode=mode)
        m.train_step(S.x, S.y, LR, S.cfg)
        m.set_accumulation(1)
        assert m.plan(variants=True, mode='train') == S.plain_plan
        with pytest.raises(Exception, match='accumulation is off'):
            m.get_accumulation()
        # a step is then the step of a model that never had it: the planted one bit for bit on both plans, the trained one bit for
        # bit where the gradient itself is (the dense plan; the 3-channel plan's weight gradients go through float atomics)
        never.set_params(S.p0)
        if never.n_state:
            never.set_state(S.s0)
        S.reset(OO.spec('adam'))
        for q in (m, never):
            q.set_opt_state(S.m0, S.v0, 6)
            q.apply_gradients(S.g0, LR)
        assert m.get_params().tobytes() == never.get_params().tobytes()
        outs = [_profiled(q, lambda: q.train_step(S.x, S.y, LR, S.cfg)) for q in (m, never)]
        assert set(outs[0][1]) == set(outs[1][1]) and not {'grad_accumulate', 'pg_fold_acc'} & set(outs[0][1]), outs[0][1]
        assert outs[0][0].loss == outs[1][0].loss
        if name == 'unet64_f32_10x14':
            assert m.get_params().tobytes() == never.get_params().tobytes()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(m.get_opt_state()[:2], never.get_opt_state()[:2]))
    finally:
        m.set_accumulation(1)
        never.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(sessions):
    S = sessions('unet3_2x64x256')
    m = S.m
    S.reset(OO.spec('adam'))
    try:
        for bad in (0, -1, 4097):
            with pytest.raises(Exception, match='dnnca_model_set_accumulation') as e:
                m.set_accumulation(bad)
            assert e.value.code == EINVAL
            with pytest.raises(Exception, match='accumulation is off') as e:          # nothing changed: still off
                m.get_accumulation()
            assert e.value.code == ESTATE
        m.set_accumulation(4096)
        m.set_accumulation(3)
        m.train_step(S.x, S.y, LR, S.cfg)
        a1 = m.get_accumulation()
        assert a1[1:] == (3, 1)
        for bad in (0, -1, 4097):
            with pytest.raises(Exception, match='dnnca_model_set_accumulation'):
                m.set_accumulation(bad)
            a = m.get_accumulation()
            assert a[1:] == (3, 1) and a[0].tobytes() == a1[0].tobytes()
        m.set_params(S.p0)                                    # new weights mid-cycle: the partial cycle is dropped
        assert m.get_accumulation()[2] == 0
        m.train_step(S.x, S.y, LR, S.cfg)
        assert m.get_accumulation()[2] == 1
        m.set_opt_state(S.m0, S.v0, 6)
        assert m.get_accumulation()[2] == 0
        m.train_step(S.x, S.y, LR, S.cfg)
        m.set_optimizer('sgd', momentum=0.9)                  # these two keep the position
        m.set_ema(0.9)
        assert m.get_accumulation()[2] == 1
        m.set_accumulation(3)                                 # setting it again discards the partial cycle
        assert m.get_accumulation()[2] == 0
        m.exchange_ema()
        with pytest.raises(Exception, match='averaged weights are in use') as e:
            m.set_accumulation(2)
        assert e.value.code == ESTATE
        m.exchange_ema()
        assert m.get_accumulation()[1] == 3
        with pytest.raises(ValueError, match='grad_accumulate_of'):
            m.grad_accumulate_of(np.zeros(3, np.float32), np.zeros(4, np.float32), False)
    finally:
        m.set_ema(0)
        m.set_optimizer('adam')
        m.set_accumulation(1)


# ---- 8. the data-parallel arm -----------------------------------------------------------------------------------------------------
def test_communicator_arm_in_a_child_process(gpu):
    """a k = 2 cycle behind a one-rank communicator (DNNCA_FORCE_RCCL=1): one collective per micro-step, the loss slot alone and then
    the accumulator with the loss slot behind it; no bucketing; weights, slots and accumulator bit-identical to the single-replica cycle"""
    env = dict(os.environ, DNNCA_FORCE_RCCL='1')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'accumulate_comm_case.py')], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    o = json.loads(r.stdout.strip().splitlines()[-1])
    print(o)
    assert o['collectives'] == [1, 1] and o['floats'] == [1, o['n'] + 1]
    assert o['positions'] == [[1, 0], [1, 0]] and o['iterations'] == [7, 7] and o['moved'] > 1e-5
    assert o['launches'] == dict(grad_accumulate=2, pg_fold=2, pg_fold_acc=0, g_adam=1, g_finalize_scalars=2)
    assert o['losses'][0] == o['losses'][1]
    assert all(o['same'].values()), o


# ---- 9. the engine end to end -----------------------------------------------------------------------------------------------------
def _arrays(path):
    with np.load(path + '.data-00000-of-00001') as z:
        return {k: z[k].copy() for k in z.files}


# Bit equality across runs can only be asked of a model whose train step is itself reproducible.  Measured on the parent's step as on
# this one (k = 1 and k = 2, 8 steps, twice each): unet3 at 32 x 32 and a 16-filter BatchNorm U-Net at 16 x 16 give the same bytes
# every run, so there a resumed run must equal the uninterrupted one bit for bit.  unet3 at 64 x 64 does not -- its conv weight
# gradients are float atomic sums over more blocks than slabs; two runs differ by 6e-8 in the weights with or without accumulation
# -- so there the comparison is the loss history, to the 1e-5 this file's neighbours hold a float32 loss to, and the launch counts
# of the fused arm through the staged feeder
UNET16 = dict(n_filters_first=16, n_downsample=2, rate=2, kernel_size=3, conv_stride=1, bn=True, padding='same')
ENGINE_MODELS = {'dense_unet16_bn_16x16': (UNET16, 16, True), 'pixel_group_unet3_32x32': (UNET3, 32, True),
                 'pixel_group_unet3_64x64': (UNET3, 64, False)}


@pytest.mark.parametrize('name', sorted(ENGINE_MODELS))
def test_engine_end_to_end(gpu, tmp_path, monkeypatch, name):
    """synthetic data through the staged feeder, k = 2, save_freq 4, max_steps 8: checkpoints at 4 and 8 whose iterations are 2 and
    4, one train_log.csv line per micro-step, a run resumed from step 4 and a run with DNNCA_NO_FEEDER=1 against the uninterrupted one"""
    from dnncancerannotator_amd import data, engine, load
    root = os.path.dirname(HERE)
    options, size, exact = ENGINE_MODELS[name]
    cfg = {'model': 'UNetAnnotator', 'model_options': options,
           'deploy_options': {'optimizer': 'adam', 'enable_multigpu': False,
                              'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}}},
           'data_options': {'eval': {'batch_size': 4}}}
    cfg = load._apply_config(cfg, load.load_config(os.path.join(root, 'configs', 'additionals', 'accumulate_batch64.yaml')))
    assert cfg['deploy_options']['gradient_accumulation_steps'] == 8
    cfg['deploy_options']['gradient_accumulation_steps'] = 2

    def run(tag, stops, feeder=True):
        if feeder:
            monkeypatch.delenv('DNNCA_NO_FEEDER', raising=False)
        else:
            monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
        path, losses = str(tmp_path / tag), []
        for stop in stops:
            e = engine.TFKerasModel(cfg)
            e.learning_rate = 0.01
            res = e.train(data.SyntheticDataset(4, size, size, 1, n_batches=2, seed=3), save_path=path, max_steps=stop, save_freq=4,
                          profile=True)
            losses += res.history['loss']
            rows = {r[0]: r[1] for r in e.device_model.profile()}
            steps = len(res.history['loss'])
            assert rows.get('pg_fold_acc', 0) + rows.get('grad_accumulate', 0) == steps, rows          # one or the other on every micro-step
            if name == 'pixel_group_unet3_64x64':          # the fused arm on the micro-steps that end in no update
                assert rows.get('pg_fold_acc') == steps // 2 and rows.get('grad_accumulate') == steps // 2, rows
            assert e.device_model.get_accumulation()[1:] == (2, 0)
            e.device_model.close()
        return path, np.asarray(losses, np.float32)
    whole, losses = run('whole', [8])
    assert losses.shape == (8,) and np.isfinite(losses).all()
    for step, iterations in ((4, 2), (8, 4)):
        ck = os.path.join(whole, 'checkpoints', 'ckpt-%d' % step)
        index = json.load(open(ck + '.index'))
        assert index['step'] == step and index['iterations'] == iterations
        assert list(index) == ['format', 'step', 'iterations', 'learning_rate', 'variables']        # the files keep their format
        assert list(_arrays(ck)) == ['params', 'state', 'adam_m', 'adam_v']
    with open(os.path.join(whole, 'tfevents', 'train_log.csv')) as f:
        lines = f.read().splitlines()
    assert [int(line.split(',')[0]) for line in lines] == list(range(1, 9))                          # one line per micro-step
    want = _arrays(os.path.join(whole, 'checkpoints', 'ckpt-8'))
    assert np.abs(want['params'] - _arrays(os.path.join(whole, 'checkpoints', 'ckpt-4'))['params']).max() > 1e-4
    for tag, stops, feeder in (('resumed', [4, 8], True), ('unfed', [8], False)):
        path, got_losses = run(tag, stops, feeder)
        got = _arrays(os.path.join(path, 'checkpoints', 'ckpt-8'))
        print(name, tag, 'max difference from the uninterrupted run:',
              {k: float(np.abs(got[k].astype(np.float64) - want[k]).max()) if want[k].size else 0.0 for k in want},
              'losses', float(np.abs(got_losses - losses).max()))
        if exact:
            assert all(got[k].tobytes() == want[k].tobytes() for k in want), tag
            assert got_losses.tobytes() == losses.tobytes(), tag
        else:
            assert np.all(np.abs(got_losses - losses) <= 1e-5 * np.abs(losses)), tag
