"""-m gpu: the configurable optimizers (dnnca_model_set_optimizer) -- every optimizer x clip arm against the float64 recurrences of
tests/optim_oracle.py on the device's own state and gradients, planted gradients through apply_gradients, the bit identities
(opt_adam == g_adam, run to run), off means off, the data-parallel arm on a one-rank communicator, and the engine end to end."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import optim_oracle as OO

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T, LR = 5, 1e-2
UNET3 = dict(n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')
UNET64 = dict(n_filters_first=64, n_downsample=1, rate=2, kernel_size=3, conv_stride=1, bn=True, padding='same')


def _unet3(gpu, B, H, W, **kw):
    return gpu.DeviceModel('unet', 1, H, W, B, **dict(UNET3, **kw))


def _multires(gpu):
    from dnncancerannotator_amd import models
    return models.MultiResUnet(n_channels=5, n_filters_first=4).build([1, 16, 16, 5], seed=0)


# name -> (builder, batch fed): the small shapes of tests/test_ema_gpu.py, which reach every arm of the step
CASES = {
    'unet3_2x64x256': (lambda g: _unet3(g, 2, 64, 256), 2),                    # pixel-group plan: the deferred fold must be declined
    'unet3_ragged_3_of_4x40x24': (lambda g: _unet3(g, 4, 40, 24), 3),
    'unet3_generic': (lambda g: _unet3(g, 2, 64, 256, force_generic=True), 2),
    'mulmo16_bn_12x20x3': (lambda g: g.DeviceModel('mulmo', 3, 12, 20, 2, n_filters_first=16, n_downsample=2, rate=2, kernel_size=3,
                                                    conv_stride=1, bn=True, padding='same'), 2),
    # the 64 -> 128 kernel spans 72 chunks, the biases are smaller than one
    'unet64_f32_10x14': (lambda g: g.DeviceModel('unet', 1, 10, 14, 2, **UNET64), 2),
    'unet64_bf16_10x14': (lambda g: g.DeviceModel('unet', 1, 10, 14, 2, dtype='bf16', **UNET64), 2),
    'multires4_1x16x16': (_multires, 1),
}
KINDS = {
    'adam': OO.spec('adam'),
    'adamw': OO.spec('adamw', weight_decay=0.05),
    'sgd_momentum': OO.spec('sgd', momentum=0.9),
    'sgd_nesterov': OO.spec('sgd', momentum=0.9, nesterov=True),
}
LAUNCH = {'adam': 'opt_adam', 'adamw': 'opt_adamw', 'sgd': 'opt_sgd'}


class Session:
    """one model per case, shared by the tests: a batch, starting weights, one real gradient, and planted slots at iteration 6 scaled
    to that gradient (as test_adam_kernel_with_history plants them), so that a step depends on gradient magnitudes"""

    def __init__(self, gpu, name):
        builder, fed = CASES[name]
        self.name, self.m = name, builder(gpu)
        m = self.m
        m.init_glorot(seed=5)
        rng = np.random.default_rng(6)
        m.set_params((m.get_params() + rng.uniform(-0.05, 0.05, m.n_trainable)).astype(np.float32))      # non-zero biases
        self.p0, self.s0 = m.get_params(), m.get_state()
        self.x = rng.random((fed,) + m.in_shape).astype(np.float32)
        self.y = (rng.random((fed,) + m.in_shape[:2]) < 0.1).astype(np.float32)
        self.cfg = m.loss_cfg(weight_mul=3.0)
        self.slices = OO.variable_slices(m.param_infos())
        self.decay = m.decay_mask()
        self.plain_plan = m.plan(variants=True, mode='train')
        m.train_step(self.x, self.y, 0.0, self.cfg)          # lr 0: the weights stay
        self.g0 = m.get_grads()
        scale = np.abs(self.g0) + 1e-6
        self.m0 = (rng.standard_normal(m.n_trainable) * scale).astype(np.float32)
        self.v0 = (rng.random(m.n_trainable) * scale ** 2).astype(np.float32)
        self.unclipped = {}

    def reset(self, spec=None, slots=True):
        m = self.m
        m.set_ema(0)
        m.set_params(self.p0)
        if m.n_state:
            m.set_state(self.s0)
        if slots:          # SGD's accumulator is a weight change, lr times a gradient: planted on that scale
            sgd = spec is not None and spec.kind == 'sgd'
            m.set_opt_state(self.m0 * np.float32(LR) if sgd else self.m0, self.v0, 6)
        else:
            m.set_opt_state(np.zeros_like(self.m0), np.zeros_like(self.v0), 0)
        if spec is not None:
            m.set_optimizer(decay_mask=self.decay, **OO.device_kwargs(spec))

    def state(self):
        mm, vv, it = self.m.get_opt_state()
        return self.m.get_params(), mm, vv, it


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


def _train_run(S, spec, steps=T):
    """`steps` train steps of one arm from the session's start; after every step the device's weights, slots and norms against one
    oracle step from the device's previous state and its get_grads().  -> per step dict(worst, want, out)"""
    m = S.m
    S.reset(spec)
    by_norm = bool(spec.clipnorm or spec.global_clipnorm)
    recs = []
    for k in range(steps):
        p, mm, vv, it = S.state()
        out = m.train_step(S.x, S.y, LR, S.cfg)
        g = m.get_grads()
        want = OO.step(spec, S.slices, S.decay, p, mm, vv, g, it + 1, LR)
        p1, m1, v1, it1 = S.state()
        assert it1 == it + 1 == 7 + k
        worst = OO.check(p1, m1, v1, want)
        if by_norm:
            total, per = m.last_grad_norm()
            worst['norm'] = float(abs(total - want['norm']) / OO.norm_tol(want['norm'], m.n_trainable))
            sizes = np.array([sl.stop - sl.start for _, sl in S.slices])
            worst['norms'] = float((np.abs(per - want['norms']) / OO.norm_tol(want['norms'], sizes)).max())
        assert np.isfinite(out.loss)
        assert np.abs(p1 - p).max() > 1e-5                                   # and the step did something
        recs.append(dict(worst=worst, want=want, g=g, out=out))
    return recs


def _assert_within(name, arm, recs):
    worst = {k: max(r['worst'][k] for r in recs) for k in recs[0]['worst']}
    print(name, arm, 'worst error / bound:', ' '.join('%s %.3f' % kv for kv in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), (name, arm, worst)


# ---- 1. every optimizer arm against the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', sorted(KINDS))
@pytest.mark.parametrize('name', sorted(CASES))
def test_every_arm_against_the_oracle(sessions, name, kind):
    S = sessions(name)
    base = KINDS[kind]
    # no clip: also the run the clip values come from
    free = _train_run(S, base)
    _assert_within(name, kind, free)
    launch = LAUNCH[base.kind]
    plan = [r[0] for r in S.m.plan(mode='train')]
    if kind == 'adam':          # Adam with nothing else is the model as it was: the oracle has just been held against g_adam
        assert [r[0].split('#')[0] for r in S.plain_plan] == plan and 'g_adam' in plan and launch not in plan, plan
    else:
        assert launch in plan and 'g_adam' not in plan, plan
    assert 'pg_fold_adam' not in plan and 'grad_sqnorm' not in plan, plan
    norms = np.array([r['want']['norm'] for r in free])
    per = np.array([r['want']['norms'] for r in free])
    # clipvalue: the median magnitude of the first gradient -- on every step some elements are clipped and some are not
    cv = float(np.median(np.abs(free[0]['g'][free[0]['g'] != 0])))
    recs = _train_run(S, base._replace(clipvalue=cv))
    _assert_within(name, kind + ' clipvalue', recs)
    for r in recs:
        frac = float(np.mean(np.abs(r['g'][r['g'] != 0]) > np.float32(cv)))          # of the non-zero elements
        assert 0.0 < frac < 1.0, frac
    # by norm: half the smallest observed norm (active on every step), twice the largest (never active).  Per variable, the
    # variables whose gradient is numerically nothing (a conv bias in front of a BatchNorm: 1e-6 of the largest norm or less) are
    # left out of "smallest": a clip down there would only test the arithmetic of zero
    arms = {'clipnorm': ('clipnorm', 0.5 * float(per[per > 1e-6 * per.max()].min()), 2.0 * float(per.max())),
            'global_clipnorm': ('global_clipnorm', 0.5 * float(norms.min()), 2.0 * float(norms.max()))}
    for arm, (key, active, never) in arms.items():
        recs = _train_run(S, base._replace(**{key: active}))
        _assert_within(name, '%s %s=%.3g (active)' % (kind, key, active), recs)
        for r in recs:
            scales = r['want']['scales']
            assert scales.min() < 1.0 if key == 'clipnorm' else np.all(scales < 1.0), scales
        plan = [r[0] for r in S.m.plan(mode='train')]
        assert [k for k in plan if k in ('pg_fold', 'grad_sqnorm', 'grad_clip_scale', launch)][-3:] == ['grad_sqnorm', 'grad_clip_scale', launch]
        recs = _train_run(S, base._replace(**{key: never}))
        _assert_within(name, '%s %s=%.3g (never active)' % (kind, key, never), recs)
        for r in recs:
            assert np.all(r['want']['scales'] == 1.0)


def test_the_pixel_group_plan_declines_the_deferred_fold(sessions):
    """unet3 2 x 64 x 256 runs fold + Adam + outputs as one launch (pg_fold_adam); with an optimizer set the live step runs pg_fold
    and the optimizer's launches, which also write the step outputs (no g_finalize_scalars)"""
    S = sessions('unet3_2x64x256')
    m = S.m

    def rows(spec):
        S.reset(spec)
        m.sync()
        m.profile_reset()
        m.profile_enable(1)
        try:
            outs = [m.train_step(S.x, S.y, LR, S.cfg) for _ in range(2)]
            return {name: (k, by) for name, k, _, by, _ in m.profile()}, outs
        finally:
            m.profile_enable(0)
            m.profile_reset()
    plain, outs0 = rows(OO.spec('adam'))
    assert plain['pg_fold_adam'][0] == 2 and not [k for k in plain if k.startswith(('opt_', 'grad_'))], plain
    n = m.n_trainable
    on, outs1 = rows(OO.spec('adamw', weight_decay=0.05, global_clipnorm=1.0))
    assert on['pg_fold'][0] == 2 and on['opt_adamw'] == (2, 28.0 * n) and on['grad_sqnorm'] == (2, 4.0 * n) and on['grad_clip_scale'][0] == 2
    assert 'pg_fold_adam' not in on and 'g_adam' not in on and 'g_finalize_scalars' not in on, on
    # the first step's outputs come from the same weights: the optimizer launch wrote what pg_fold_adam writes
    a, b = outs0[0], outs1[0]
    for field in ('loss', 'positive_rate', 'weight', 'label_min', 'label_max'):
        assert abs(getattr(a, field) - getattr(b, field)) <= 1e-5 * abs(getattr(a, field)), field
    sgd, _ = rows(OO.spec('sgd', momentum=0.9))
    assert sgd['opt_sgd'] == (2, 20.0 * n) and 'grad_sqnorm' not in sgd
    S.reset(OO.spec('sgd'))
    assert ('opt_sgd', 12.0 * n, 4.0 * n) in m.plan(mode='train')


# ---- 2. planted gradients through apply_gradients -------------------------------------------------------------------------------
PLANTED = ('unet3_2x64x256', 'unet64_f32_10x14')


def _apply(S, spec, g, slots=False, lr=LR):
    S.reset(spec, slots=slots)
    S.m.apply_gradients(g, lr)
    return S.state()


@pytest.mark.parametrize('name', PLANTED)
def test_planted_zero_gradient_moves_only_by_decay(sessions, name):
    S = sessions(name)
    spec = OO.spec('adamw', weight_decay=0.05, global_clipnorm=1.0)
    p1, m1, v1, it = _apply(S, spec, np.zeros_like(S.p0))
    assert it == 1 and not np.any(m1) and not np.any(v1)
    lrwd = np.float32(float(np.float32(LR)) * float(np.float32(0.05)))
    assert np.finfo(np.longdouble).nmant >= 63          # p - lrwd p exactly (59 bits at most), then the one rounding of the device's fma
    for (vname, sl), d in zip(S.slices, S.decay):
        p = S.p0[sl].astype(np.longdouble)
        want = p - np.longdouble(lrwd) * p if d else p               # a scale of 0 / 0 would have made every weight NaN
        assert p1[sl].tobytes() == want.astype(np.float32).tobytes(), vname
    total, per = S.m.last_grad_norm()
    assert total == 0.0 and not np.any(per)
    assert any(S.decay) and not all(S.decay)


@pytest.mark.parametrize('name', PLANTED)
def test_planted_1e30_entries_have_a_finite_double_norm(sessions, name):
    S = sessions(name)
    g = np.zeros_like(S.p0)
    g[::7] = np.float32(1e30)
    g[3::11] = np.float32(-1e30)
    assert not np.isfinite(np.float32(1e30) * np.float32(1e30))          # the squares overflow float
    spec = OO.spec('sgd', global_clipnorm=1.0)
    S.reset(spec, slots=False)
    want = OO.step(spec, S.slices, S.decay, S.p0, np.zeros_like(S.p0), np.zeros_like(S.p0), g, 1, LR)
    S.m.apply_gradients(g, LR)
    p1, m1, v1, _ = S.state()
    total, per = S.m.last_grad_norm()
    count = int(np.count_nonzero(g))
    assert np.isfinite(total) and abs(total - float(np.float32(1e30)) * np.sqrt(count)) <= OO.norm_tol(total, S.m.n_trainable)
    assert abs(total - want['norm']) <= OO.norm_tol(total, S.m.n_trainable)
    worst = OO.check(p1, m1, v1, want)
    print(name, worst, 'norm %.6g' % total)
    assert max(worst.values()) <= 1.0 and np.all(np.isfinite(p1))
    moved = np.abs(p1 - S.p0)[g != 0]
    assert np.all(moved > 0) and np.allclose(moved, LR / np.sqrt(count), rtol=1e-3)


@pytest.mark.parametrize('name', PLANTED)
def test_planted_one_variable_over_its_clip(sessions, name):
    S = sessions(name)
    c = 0.5
    rng = np.random.default_rng(8)
    g = np.zeros_like(S.p0)
    big = max(range(len(S.slices)), key=lambda k: S.slices[k][1].stop - S.slices[k][1].start)          # spans the most chunks
    for k, (_, sl) in enumerate(S.slices):
        v = rng.standard_normal(sl.stop - sl.start)
        g[sl] = (v / np.linalg.norm(v) * (10 * c if k == big else 0.9 * c * rng.random())).astype(np.float32)
    free = _apply(S, OO.spec('sgd'), g)
    spec = OO.spec('sgd', clipnorm=c)
    clipped = _apply(S, spec, g)
    total, per = S.m.last_grad_norm()
    want = OO.step(spec, S.slices, S.decay, S.p0, np.zeros_like(S.p0), np.zeros_like(S.p0), g, 1, LR)
    assert [k for k, s in enumerate(want['scales']) if s < 1.0] == [big] and abs(want['scales'][big] - 0.1) < 1e-6
    for k, (vname, sl) in enumerate(S.slices):
        if k != big:
            assert clipped[0][sl].tobytes() == free[0][sl].tobytes(), vname          # bit for bit elsewhere
    sl = S.slices[big][1]
    assert np.abs(clipped[0][sl] - free[0][sl]).max() > 1e-5
    assert max(OO.check(clipped[0], clipped[1], clipped[2], want).values()) <= 1.0
    sizes = np.array([s.stop - s.start for _, s in S.slices])
    assert np.all(np.abs(per - want['norms']) <= OO.norm_tol(want['norms'], sizes)) and abs(per[big] - 10 * c) < 1e-5


@pytest.mark.parametrize('name', PLANTED)
def test_planted_norm_equal_to_the_clip_passes_bit_for_bit(sessions, name):
    S = sessions(name)
    c = 0.75
    g = np.zeros_like(S.p0)
    g[S.m.n_trainable // 2] = c
    for kind in ('adam', 'sgd_nesterov'):
        free = _apply(S, KINDS[kind], g, slots=True)
        for key in ('clipnorm', 'global_clipnorm'):
            got = _apply(S, KINDS[kind]._replace(**{key: c}), g, slots=True)
            total, per = S.m.last_grad_norm()
            assert total == c and per.max() == c
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], free[:3])), (kind, key)


# ---- 3. bit identities ----------------------------------------------------------------------------------------------------------
def _applied(S, spec, g, ema):
    m = S.m
    S.reset(spec)
    if ema:
        m.set_ema(0.9, warmup=False)
    m.sync()
    m.profile_reset()
    m.profile_enable(1)
    try:
        m.apply_gradients(g, LR)
        m.apply_gradients(S.g0, LR)
        rows = {name: k for name, k, _, _, _ in m.profile()}
    finally:
        m.profile_enable(0)
        m.profile_reset()
    out = S.state()[:3] + ((m.get_ema()[0],) if ema else ())
    m.set_ema(0)
    return out, rows


@pytest.mark.parametrize('ema', [False, True], ids=['plain', 'ema'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_opt_adam_with_scale_one_is_g_adam_bit_for_bit(sessions, name, ema):
    S = sessions(name)
    g = (S.g0 * np.float32(3.0)).astype(np.float32)
    suffix = '_ema' if ema else ''
    ref, rows = _applied(S, OO.spec('adam'), g, ema)
    assert rows.get('g_adam' + suffix) == 2 and not [k for k in rows if k.startswith(('opt_', 'grad_'))], rows
    for spec in (OO.spec('adam', global_clipnorm=1e30), OO.spec('adam', clipnorm=1e30), OO.spec('adam', clipvalue=1e30)):
        got, rows = _applied(S, spec, g, ema)
        assert rows.get('opt_adam' + suffix) == 2 and 'g_adam' + suffix not in rows, rows
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref)), spec
    assert np.abs(ref[0] - S.p0).max() > 1e-3 and (not ema or np.abs(ref[3] - S.p0).max() > 1e-4)


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_arm_is_bit_identical_from_run_to_run(sessions, name):
    S = sessions(name)
    g = (S.g0 * np.float32(3.0)).astype(np.float32)
    norm = float(np.linalg.norm(g.astype(np.float64)))
    for kind, base in sorted(KINDS.items()):
        for clip in ({}, dict(clipvalue=float(np.abs(g).max()) / 4), dict(clipnorm=norm / 8), dict(global_clipnorm=norm / 2)):
            spec = base._replace(**clip)
            runs = []
            for _ in range(2):
                out, _ = _applied(S, spec, g, ema=True)
                runs.append(out + ((S.m.last_grad_norm()[1],) if (spec.clipnorm or spec.global_clipnorm) else ()))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs)), (kind, clip)


# ---- 4. off means off -----------------------------------------------------------------------------------------------------------
def test_off_means_off(gpu):
    never = _unet3(gpu, 2, 64, 256)
    toggled = _unet3(gpu, 2, 64, 256)
    try:
        before = never.plan(variants=True, mode='train')
        assert toggled.plan(variants=True, mode='train') == before
        n = toggled.n_trainable
        toggled.set_optimizer('sgd', momentum=0.9, clipnorm=1.0)
        on = toggled.plan(variants=True, mode='train')
        assert [r for r in on if r[0] not in ('grad_sqnorm', 'grad_clip_scale', 'opt_sgd')] == [r for r in before if r[0] != 'g_adam']
        assert [r[0] for r in on][-3:] == ['grad_sqnorm', 'grad_clip_scale', 'opt_sgd'] and ('opt_sgd', 20.0 * n, 4.0 * n) in on
        for mode in ('eval', 'forward'):
            assert toggled.plan(variants=True, mode=mode) == never.plan(variants=True, mode=mode)
        toggled.set_optimizer('adam')                     # Adam with nothing else: the tables are freed
        assert toggled.plan(variants=True, mode='train') == before
        rng = np.random.default_rng(3)
        x = rng.random((2, 64, 256, 1)).astype(np.float32)
        y = (rng.random((2, 64, 256)) < 0.1).astype(np.float32)
        cfg = never.loss_cfg(weight_mul=3.0)
        for m in (never, toggled):
            m.sync()
            m.profile_reset()
            m.profile_enable(1)
            for _ in range(2):
                m.train_step(x, y, LR, cfg)
            rows = {name: k for name, k, _, _, _ in m.profile()}
            m.profile_enable(0)
            m.profile_reset()
            assert rows['pg_fold_adam'] == 2 and not [k for k in rows if k.startswith(('opt_', 'grad_')) or k == 'pg_fold'], rows
            with pytest.raises(Exception, match='no clipping by norm'):
                m.last_grad_norm()
        # the betas of a plain Adam mapping reach the launch the model always ran
        toggled.set_optimizer('adam', beta1=0.5, beta2=0.9, epsilon=1e-3)
        never.set_adam(0.5, 0.9, 1e-3)
        for m in (never, toggled):
            m.init_glorot(seed=4)
            m.set_opt_state(np.zeros(n, np.float32), np.zeros(n, np.float32), 0)
            m.apply_gradients(np.full(n, 0.25, np.float32), LR)
        assert toggled.get_params().tobytes() == never.get_params().tobytes()
        bad = [dict(kind='adam', clipnorm=1.0, global_clipnorm=1.0), dict(kind='adam', clipvalue=-1.0), dict(kind='adam', clipnorm=float('nan')),
               dict(kind='adam', global_clipnorm=float('inf')), dict(kind='adam', momentum=0.5), dict(kind='adam', weight_decay=0.1),
               dict(kind='adamw', weight_decay=-0.1), dict(kind='adamw', weight_decay=float('nan')), dict(kind='sgd', momentum=1.0),
               dict(kind='sgd', momentum=-0.1), dict(kind='sgd', weight_decay=0.1), dict(kind='adam', beta1=1.0), dict(kind='adam', beta2=-0.1),
               dict(kind='adam', epsilon=-1.0), dict(kind='sgd', clipnorm=1.0, decay_mask=[1, 0])]
        for kw in bad:
            with pytest.raises(Exception, match='dnnca_model_set_optimizer'):
                never.set_optimizer(**kw)
        assert never.plan(variants=True, mode='train') == before          # a refusal changes nothing
        with pytest.raises(Exception, match='dnnca_apply_gradients'):
            never.apply_gradients(np.zeros(n - 1, np.float32), LR)
        toggled.set_ema(0.9)
        toggled.set_optimizer('adamw', weight_decay=0.01)
        assert [r[0] for r in toggled.plan(mode='train')][-1] == 'opt_adamw_ema'
        toggled.exchange_ema()
        with pytest.raises(Exception, match='averaged weights are in use'):
            toggled.set_optimizer('sgd')
        with pytest.raises(Exception, match='averaged weights are in use'):
            toggled.apply_gradients(np.zeros(n, np.float32), LR)
        toggled.exchange_ema()
    finally:
        never.close()
        toggled.close()


# ---- 5. the data-parallel arm ---------------------------------------------------------------------------------------------------
def test_communicator_arm_in_a_child_process(gpu):
    """opt_adamw without finalize, gscale = 1 / world, behind the all-reduce of a one-rank communicator (DNNCA_FORCE_RCCL=1)"""
    env = dict(os.environ, DNNCA_FORCE_RCCL='1')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'optimizer_comm_case.py')], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    o = json.loads(r.stdout.strip().splitlines()[-1])
    print(o)
    assert o['launches'] == dict(opt_adamw=T, grad_sqnorm=T, grad_clip_scale=T, g_finalize_scalars=T) and o['plain'] == 0
    assert o['collectives'] >= 1 and o['iterations'] == 6 + T
    assert max(o['worst'].values()) <= 1.0 and o['clipped_steps'] == T and o['moved'] > 1e-4


# ---- 6. the engine end to end ---------------------------------------------------------------------------------------------------
def _engine_cfg(optimizer, **deploy):
    d = {'optimizer': optimizer, 'enable_multigpu': False, 'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}}}
    d.update(deploy)
    return {'model': 'UNetAnnotator', 'model_options': UNET3, 'deploy_options': d, 'data_options': {'eval': {'batch_size': 4}}}


def _arrays(path):
    with np.load(path + '.data-00000-of-00001') as z:
        return {k: z[k].copy() for k in z.files}


def _resumed_state_and_next_step(engine, data, cfg, ck, spec):
    """a new engine loaded from `ck`: its device state is the checkpoint's bit for bit, and its next step meets the oracle"""
    ds = data.SyntheticDataset(4, 64, 64, 1, n_batches=2, seed=3)
    e = engine.TFKerasModel(cfg)
    e._build(ds)
    e.load(ck)
    dm = e.device_model
    saved, index = _arrays(ck), json.load(open(ck + '.index'))
    p, (mm, vv, it) = dm.get_params(), dm.get_opt_state()
    assert p.tobytes() == saved['params'].tobytes() and mm.tobytes() == saved['adam_m'].tobytes() and vv.tobytes() == saved['adam_v'].tobytes()
    assert it == index['iterations']
    if 'ema' in saved:
        avg, n = dm.get_ema()
        assert avg.tobytes() == saved['ema'].tobytes() and n == index['ema']['num_updates']
    x, y = next(iter(ds))
    dm.train_step(x, y, e.learning_rate, dm.loss_cfg(weight_mul=3.0))
    want = OO.step(spec, OO.variable_slices(dm.param_infos()), dm.decay_mask(), p, mm, vv, dm.get_grads(), it + 1, e.learning_rate)
    m1, v1, it1 = dm.get_opt_state()
    worst = OO.check(dm.get_params(), m1, v1, want)
    print(index.get('optimizer', {}).get('class_name'), 'resumed step, worst error / bound:', worst)
    assert it1 == it + 1 and max(worst.values()) <= 1.0
    return e


def test_engine_adamw_clip_ema_trains_checkpoints_resumes_and_evaluates(gpu, tmp_path):
    from dnncancerannotator_amd import data, engine, load
    root = os.path.dirname(HERE)
    cfg = _engine_cfg('adam')
    for overlay in ('adamw.yaml', 'clip_global_norm.yaml', 'ema.yaml'):
        cfg = load._apply_config(cfg, load.load_config(os.path.join(root, 'configs', 'additionals', overlay)))
    opt = {'class_name': 'AdamW', 'config': {'learning_rate': 0.01, 'weight_decay': 0.05, 'global_clipnorm': 0.05}}
    assert cfg['deploy_options']['optimizer']['class_name'] == 'Adam'          # the later overlay replaced the whole mapping
    cfg['deploy_options']['optimizer'] = opt
    run = str(tmp_path / 'run')
    ds = data.SyntheticDataset(4, 64, 64, 1, n_batches=2, seed=3)
    val = data.SyntheticDataset(4, 64, 64, 1, n_batches=1, seed=9, repeat=False)
    e = engine.TFKerasModel(cfg)
    res = e.train(ds, save_path=run, max_steps=12, save_freq=6, val_data=val)
    assert len(res.history['loss']) == 12 and np.all(np.isfinite(res.history['loss'])) and len(res.history['val_loss']) == 2
    assert res.history['lr'] == [0.01] * 12
    total, per = e.device_model.last_grad_norm()
    assert total > 0 and np.isfinite(total) and per.shape == (len(e.device_model.trainable_names()),)
    plan = [r[0] for r in e.device_model.plan(mode='train')]
    assert plan[-3:] == ['grad_sqnorm', 'grad_clip_scale', 'opt_adamw_ema']
    ck6 = os.path.join(run, 'checkpoints', 'ckpt-6')
    index = json.load(open(ck6 + '.index'))
    assert index['optimizer']['class_name'] == 'AdamW' and index['optimizer']['config']['global_clipnorm'] == 0.05
    assert index['optimizer']['config']['weight_decay'] == 0.05 and index['iterations'] == 6 and index['ema']['num_updates'] == 6
    assert sorted(_arrays(ck6)) == ['adam_m', 'adam_v', 'ema', 'params', 'state']
    e.device_model.close()
    spec = OO.spec('adamw', weight_decay=0.05, global_clipnorm=0.05)
    e2 = _resumed_state_and_next_step(engine, data, cfg, ck6, spec)
    rows = e2.eval(val, save_path=run, tag='t')
    assert sorted(rows) == [6, 12] and all(np.isfinite(r['loss']) for r in rows.values())
    e2.device_model.close()


def test_engine_sgd_nesterov_trains_and_resumes(gpu, tmp_path):
    from dnncancerannotator_amd import data, engine, load
    root = os.path.dirname(HERE)
    cfg = load._apply_config(_engine_cfg('adam'), load.load_config(os.path.join(root, 'configs', 'additionals', 'sgd_nesterov.yaml')))
    run = str(tmp_path / 'run')
    ds = data.SyntheticDataset(4, 64, 64, 1, n_batches=2, seed=3)
    e = engine.TFKerasModel(cfg)
    res = e.train(ds, save_path=run, max_steps=12, save_freq=6)
    assert np.all(np.isfinite(res.history['loss'])) and res.history['loss'][-2] < res.history['loss'][0]          # the same batch
    assert [r[0] for r in e.device_model.plan(mode='train')][-1] == 'opt_sgd'
    ck = os.path.join(run, 'checkpoints', 'ckpt-12')
    arrays = _arrays(ck)
    assert np.abs(arrays['adam_m']).max() > 0 and not np.any(arrays['adam_v'])          # the accumulator; v untouched
    assert json.load(open(ck + '.index'))['optimizer']['class_name'] == 'SGD'
    e.device_model.close()
    e2 = _resumed_state_and_next_step(engine, data, cfg, ck, OO.spec('sgd', momentum=0.9, nesterov=True))
    adam = engine.TFKerasModel(_engine_cfg('adam'))
    adam.device_model = e2.device_model
    with pytest.raises(ValueError, match='optimizer slots of SGD'):
        adam.load(ck)
    e2.device_model.close()


def test_engine_string_adam_writes_what_it_wrote(gpu, tmp_path):
    """optimizer: adam -- the index keys and the data arrays of the checkpoint are those of the parent behaviour and the plan is the
    plan it was; a plain Adam mapping (which frees the tables again) adds the index entry and nothing else"""
    from dnncancerannotator_amd import data, engine
    got = {}
    for tag, optimizer in (('string', 'adam'), ('mapping', {'class_name': 'Adam', 'config': {}})):
        run = str(tmp_path / tag)
        e = engine.TFKerasModel(_engine_cfg(optimizer))
        e.train(data.SyntheticDataset(4, 64, 64, 1, n_batches=2, seed=3), save_path=run, max_steps=4, save_freq=4)
        plan = [r[0] for r in e.device_model.plan(mode='train')]          # (the dry plan never defers: pg_fold, g_adam)
        assert plan[-1] == 'g_adam' and not [k for k in plan if k.startswith(('opt_', 'grad_'))]
        ck = os.path.join(run, 'checkpoints', 'ckpt-4')
        got[tag] = (json.load(open(ck + '.index')), _arrays(ck))
        e.device_model.close()
    index, arrays = got['string']
    assert list(index) == ['format', 'step', 'iterations', 'learning_rate', 'variables'] and index['learning_rate'] == 0.001
    assert list(arrays) == ['params', 'state', 'adam_m', 'adam_v'] and np.any(arrays['adam_v'])
    index_m, arrays_m = got['mapping']
    assert list(index_m) == list(index) + ['optimizer'] and {k: index_m[k] for k in index} == index
    assert list(arrays_m) == list(arrays) and all(arrays_m[k].shape == arrays[k].shape and arrays_m[k].dtype == arrays[k].dtype for k in arrays)
