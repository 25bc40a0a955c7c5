"""-m gpu: the exponential moving average of the weights (dnnca_model_set_ema) -- every Adam arm against the float64 recurrence of
tests/ema_oracle.py on the weights the device itself produced, the exact exchange and the forward behind it, off means off, the
engine with checkpoints / resume / `predict --weights`, and determinism."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ema_oracle as EO

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T, LR = 5, 1e-2
UNET3 = dict(n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')
MODES = {'fixed': (0.5, False), 'warmup': (0.999, True)}          # warm-up: effective decays 2/11, 3/12, ...


def _unet3(gpu, B, H, W, **kw):
    return gpu.DeviceModel('unet', 1, H, W, B, **dict(UNET3, **kw))


def _multires(gpu):
    from dnncancerannotator_amd import models
    return models.MultiResUnet(n_channels=5, n_filters_first=4).build([1, 16, 16, 5], seed=0)


# name -> (builder, batch fed, environment of the build, the Adam launch of a live step)
CASES = {
    'unet3_2x64x256': (lambda g: _unet3(g, 2, 64, 256), 2, {}, 'pg_fold_adam_ema'),
    'unet3_ragged_3_of_4x40x24': (lambda g: _unet3(g, 4, 40, 24), 3, {}, 'g_adam_ema'),
    'unet3_no_fold_adam': (lambda g: _unet3(g, 2, 64, 256), 2, {'DNNCA_NO_FOLD_ADAM': '1'}, 'g_adam_ema'),
    'mulmo16_bn_12x20x3': (lambda g: g.DeviceModel('mulmo', 3, 12, 20, 2, n_filters_first=16, n_downsample=2, rate=2, kernel_size=3,
                                                    conv_stride=1, bn=True, padding='same'), 2, {}, 'g_adam_ema'),
    'unet64_bf16_10x14': (lambda g: g.DeviceModel('unet', 1, 10, 14, 2, n_filters_first=64, n_downsample=1, rate=2, kernel_size=3,
                                                   conv_stride=1, bn=True, padding='same', dtype='bf16'), 2, {}, 'g_adam_ema'),
    'multires4_1x16x16': (_multires, 1, {}, 'g_adam_ema'),
    'unet3_generic': (lambda g: _unet3(g, 2, 64, 256, force_generic=True), 2, {}, 'g_adam_ema'),
}


def _build(gpu, name):
    builder, _, env, _ = CASES[name]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)          # the switches are read once per model, when it is built
    try:
        return builder(gpu)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _batch(m, B, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((B,) + m.in_shape).astype(np.float32)
    y = (rng.random((B,) + m.in_shape[:2]) < 0.1).astype(np.float32)
    return x, y


def _steps(m, x, y, n=T):
    """n train steps under the launch profile -> (the weights after every step, {launch name: (launches, bytes per launch)})"""
    cfg = m.loss_cfg(weight_mul=3.0)
    m.sync()
    m.profile_reset()
    m.profile_enable(1)
    try:
        thetas = []
        for _ in range(n):
            m.train_step(x, y, LR, cfg)
            thetas.append(m.get_params())
        rows = {name: (k, by) for name, k, _, by, _ in m.profile()}
    finally:
        m.profile_enable(0)
        m.profile_reset()
    return thetas, rows


class Session:
    """one model per case: T steps under each mode of MODES (set_ema restarts the average from the weights), shared by the tests"""

    def __init__(self, gpu, name):
        self.name, self.m = name, _build(gpu, name)
        m = self.m
        m.init_glorot(seed=5)
        rng = np.random.default_rng(6)
        m.set_params((m.get_params() + rng.uniform(-0.05, 0.05, m.n_trainable)).astype(np.float32))      # non-zero biases
        self.x, self.y = _batch(m, CASES[name][1], 7)
        self.plain_plan = [r[0] for r in m.plan(mode='train')]
        self.runs = {}
        for mode, (decay, warmup) in MODES.items():
            m.set_ema(decay, warmup)
            e0, n0 = m.get_ema()
            assert n0 == 0 and np.array_equal(e0, m.get_params())          # switching on copies the weights
            plan = [r[0] for r in m.plan(mode='train')]
            thetas, rows = _steps(m, self.x, self.y)
            eT, nT = m.get_ema()
            self.runs[mode] = dict(e0=e0, thetas=thetas, eT=eT, n=nT, rows=rows, plan=plan)


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


def test_the_cases_cover_every_adam_arm():
    assert {c[3] for c in CASES.values()} >= {'pg_fold_adam_ema', 'g_adam_ema'}      # (the communicator arm: its own test below)


# ---- 1. every Adam arm against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('name', sorted(CASES))
def test_average_against_the_oracle(sessions, name, mode):
    s = sessions(name)
    r = s.runs[mode]
    decay, warmup = MODES[mode]
    m = s.m
    # which arm ran: the dry plan shows the separate Adam launch, the live profile the launch that really ran
    assert 'g_adam_ema' in r['plan'] and 'g_adam' not in r['plan'] and 'g_adam' in s.plain_plan, r['plan']
    ran = sorted(k for k in r['rows'] if k.endswith('_ema'))
    print(name, mode, 'live Adam launch:', ran, 'n_trainable', m.n_trainable)
    assert len(ran) == 1 and r['rows'][ran[0]] == (T, 36.0 * m.n_trainable), r['rows']
    assert 'g_adam' not in r['rows'] and 'pg_fold_adam' not in r['rows']
    assert 'g_finalize_scalars' not in r['rows']          # single replica: the Adam launch also writes the step outputs (finalize form)
    assert ran == [CASES[name][3]], (ran, CASES[name][3])
    assert r['n'] == T
    want = EO.run(r['thetas'], r['e0'], decay, warmup)
    tol = EO.bound(r['thetas'], r['e0'])
    err = np.abs(r['eT'].astype(np.float64) - want)
    print(name, mode, 'max error / bound: %.3f' % float((err / tol).max()))
    assert np.all(err <= tol), (float((err / tol).max()), int(np.argmax(err / tol)))
    # the head tensors: k_pg_fold's extra blocks own them
    for pname, shape, trainable, off in m.param_infos():
        if trainable and pname.startswith('head.'):
            sl = slice(off, off + int(np.prod(shape)))
            assert np.all(err[sl] <= tol[sl]), pname
            assert np.abs(r['thetas'][-1][sl] - r['e0'][sl]).max() > 1e-3, pname          # and they moved
    # the test can tell: a stale p, a wrong index or a skipped element is off by about om * 1e-2
    assert np.abs(r['eT'] - r['thetas'][-1]).max() > 1e-3
    assert np.abs(r['eT'] - r['e0']).max() > 1e-3


def test_communicator_arm_in_a_child_process(gpu):
    """g_adam without finalize, gscale = 1 / world, behind the all-reduce of a one-rank communicator (DNNCA_FORCE_RCCL=1)"""
    env = dict(os.environ, DNNCA_FORCE_RCCL='1')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'ema_comm_case.py')], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    for mode in MODES:
        o = out[mode]
        assert o['ran'] == ['g_adam_ema'] and o['launches'] == T and o['finalize_launches'] == T      # the form without finalize
        assert o['collectives'] >= 1 and o['n'] == T
        assert o['worst'] <= 1.0 and o['moved'] > 1e-3


# ---- 2. the exchange is exact and reaches every plan ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_exchange_is_exact_and_the_forward_reads_the_average(gpu, sessions, name):
    s = sessions(name)
    m = s.m
    p0, (e0, n0) = m.get_params(), m.get_ema()
    state0, opt0 = m.get_state(), m.get_opt_state()
    raw = m.forward(s.x, training=False)
    m.exchange_ema()
    assert m.get_params().tobytes() == e0.tobytes() and m.get_ema()[0].tobytes() == p0.tobytes()
    m.exchange_ema()
    assert m.get_params().tobytes() == p0.tobytes() and m.get_ema()[0].tobytes() == e0.tobytes()
    with m.averaged_weights() as inside:
        assert inside is m
        averaged = m.forward(s.x, training=False)
        cfg = m.loss_cfg(weight_mul=3.0)
        for refused in (lambda: m.train_step(s.x, s.y, LR, cfg), lambda: m.set_params(p0), lambda: m.set_opt_state(*opt0),
                        lambda: m.set_ema(0.9), lambda: m.set_ema_state(e0, 0)):
            with pytest.raises(Exception, match='averaged weights are in use'):
                refused()
        m.eval_step(s.x, s.y, cfg)                                   # evaluation is what the exchange is for
        assert m.get_params().tobytes() == e0.tobytes()
    assert m.get_params().tobytes() == p0.tobytes() and m.get_ema()[0].tobytes() == e0.tobytes() and m.get_ema()[1] == n0
    fresh = _build(gpu, name)
    try:
        fresh.set_params(e0)
        if fresh.n_state:
            fresh.set_state(state0)
        want = fresh.forward(s.x, training=False)
    finally:
        fresh.close()
    assert averaged.tobytes() == want.tobytes()                      # operands rebuilt from the exchanged weights, in every plan
    assert np.abs(averaged - raw).max() > 1e-4
    assert m.forward(s.x, training=False).tobytes() == raw.tobytes()
    # Adam's slots, its iteration count and the BatchNorm statistics: untouched by any of it
    opt1 = m.get_opt_state()
    assert opt1[0].tobytes() == opt0[0].tobytes() and opt1[1].tobytes() == opt0[1].tobytes() and opt1[2] == opt0[2] == 2 * T
    assert m.get_state().tobytes() == state0.tobytes()
    # the context exchanges back when the block raises
    with pytest.raises(RuntimeError, match='boom'):
        with m.averaged_weights():
            raise RuntimeError('boom')
    assert m.get_params().tobytes() == p0.tobytes()
    m.train_step(s.x, s.y, 0.0, m.loss_cfg(weight_mul=3.0))          # and training goes on (lr 0: the session's weights stay)


# ---- 3. off means off -------------------------------------------------------------------------------------------------------------
def test_off_means_off(gpu):
    never = _unet3(gpu, 2, 64, 256)
    toggled = _unet3(gpu, 2, 64, 256)
    try:
        before = {mode: never.plan(variants=True, mode=mode) for mode in ('train', 'eval', 'forward')}
        assert {mode: toggled.plan(variants=True, mode=mode) for mode in before} == before
        toggled.set_ema(0.999)
        on = toggled.plan(variants=True, mode='train')
        assert [r for r in on if r[0] == 'g_adam_ema'] == [('g_adam_ema', 36.0 * toggled.n_trainable, 13.0 * toggled.n_trainable)]
        assert [r for r in on if not r[0].endswith('_ema')] == [r for r in before['train'] if r[0] != 'g_adam']
        for mode in ('eval', 'forward'):
            assert toggled.plan(variants=True, mode=mode) == before[mode]
        toggled.set_ema(0)
        x, y = _batch(never, 2, 3)
        for m in (never, toggled):
            for mode, plan in before.items():
                assert m.plan(variants=True, mode=mode) == plan
                assert not [r[0] for r in plan if r[0].endswith('_ema')]
            _, rows = _steps(m, x, y, n=2)
            assert rows['pg_fold_adam'][0] == 2 and not [k for k in rows if k.endswith('_ema') or k == 'ema_exchange'], rows
            with pytest.raises(Exception, match='no weight average'):
                m.get_ema()
            with pytest.raises(Exception, match='no weight average'):
                m.exchange_ema()
        for bad in (1.0, -0.5, 1.5, float('nan')):
            with pytest.raises(Exception, match='decay'):
                never.set_ema(bad)
    finally:
        never.close()
        toggled.close()


# ---- 4. the engine on the 3-channel plan ------------------------------------------------------------------------------------------
def _texts(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            with open(os.path.join(d, f), 'rb') as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_engine_validation_checkpoints_resume_and_predict(gpu, tmp_path):
    import yaml
    from dnncancerannotator_amd import __main__ as cli, data, engine, load
    root = os.path.dirname(HERE)
    cfg = {'model': 'UNetAnnotator', 'model_options': UNET3,
           'deploy_options': {'optimizer': 'adam', 'enable_multigpu': False,
                              'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}}},
           'data_options': {'eval': {'batch_size': 4}}}
    cfg = load._apply_config(cfg, load.load_config(os.path.join(root, 'configs', 'additionals', 'ema.yaml')))
    assert cfg['deploy_options']['ema'] == dict(decay=0.999, warmup=True, validate='ema')
    run = str(tmp_path / 'run')
    ds = data.SyntheticDataset(4, 64, 64, 1, n_batches=2, seed=3)
    val = data.SyntheticDataset(4, 64, 64, 1, n_batches=1, seed=9, repeat=False)
    e = engine.TFKerasModel(cfg)
    e.learning_rate = 0.01          # large enough for the average to lag the weights visibly after three steps (asserted below)
    res = e.train(ds, save_path=run, max_steps=6, save_freq=3, val_data=val)
    assert len(res.history['val_loss']) == 2
    val3 = res.history['val_loss'][0]
    ck3, ck6 = (os.path.join(run, 'checkpoints', 'ckpt-%d' % k) for k in (3, 6))
    index = json.load(open(ck3 + '.index'))
    assert index['ema'] == dict(decay=0.999, warmup=True, num_updates=3)
    with np.load(ck3 + '.data-00000-of-00001') as z:
        saved, raw = z['ema'].copy(), z['params'].copy()
    assert np.abs(saved - raw).max() > 1e-3          # written with the raw weights in place
    e.device_model.close()

    # the logged validation loss is that of the averaged weights, not of the raw ones
    e2 = engine.TFKerasModel(cfg)
    loss_ema = e2.eval(val, save_path=run, tag='ema', step_range=(3, 3), weights='ema')[3]['loss']
    loss_raw = e2.eval(val, save_path=run, tag='raw', step_range=(3, 3))[3]['loss']
    tol = 1e-5 * max(1.0, abs(val3))
    print('val_loss logged %.8g, --weights ema %.8g, raw %.8g' % (val3, loss_ema, loss_raw))
    assert abs(val3 - loss_ema) <= tol
    assert abs(val3 - loss_raw) > tol
    e2.device_model.close()

    # a new engine resumed from ckpt-3 has the average and its count bit for bit, and its next step meets the oracle from its own weights
    e3 = engine.TFKerasModel(cfg)
    e3._build(ds)
    e3.load(ck3)
    dm = e3.device_model
    e0, n0 = dm.get_ema()
    assert e0.tobytes() == saved.tobytes() and n0 == 3 and dm.get_params().tobytes() == raw.tobytes()
    x, y = next(iter(ds))
    dm.train_step(x, y, 0.01, dm.loss_cfg(weight_mul=3.0))
    theta = dm.get_params()
    got, n1 = dm.get_ema()
    assert n1 == 4
    want = EO.run([theta], e0, 0.999, True, first_update=4)
    assert np.all(np.abs(got - want) <= EO.bound([theta], e0))
    assert np.abs(got - e0).max() > 1e-4
    # predict: the averaged checkpoint gives other tables; without the flag the files are those of --weights raw, byte for byte
    with open(os.path.join(run, 'options.yaml'), 'w') as f:
        yaml.safe_dump({'config': cfg}, f)
    e3.load(ck6)
    xb = next(iter(data.SyntheticDataset(4, 64, 64, 1, n_batches=2, repeat=False)))[0]
    thr = float(np.median(dm.forward(xb, training=False)))
    dm.close()
    texts = {}
    for name, flags in (('bare', []), ('raw', ['--weights', 'raw']), ('ema', ['--weights', 'ema'])):
        out = str(tmp_path / name)
        assert cli.main(['predict', '--save_path', run, '--data_path', 'synthetic:64x64', '--output', out, '--step', '6',
                         '--threshold', repr(thr), '--filter_size', '1'] + flags) == 0
        texts[name] = _texts(out)
    assert texts['bare'] == texts['raw'] and sorted(texts['bare']) == ['lesions.csv', 'slices.csv']
    assert texts['ema']['lesions.csv'] != texts['raw']['lesions.csv'] or texts['ema']['slices.csv'] != texts['raw']['slices.csv']


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------------
def test_the_update_is_bit_identical_from_run_to_run(gpu):
    m = _unet3(gpu, 2, 64, 256)
    try:
        m.init_glorot(seed=1)
        m.set_ema(0.9, warmup=False)
        x, y = _batch(m, 2, 2)
        cfg = m.loss_cfg(weight_mul=3.0)
        p = m.get_params()
        e0 = np.random.default_rng(3).normal(0.0, 0.3, m.n_trainable).astype(np.float32)
        results = []
        for _ in range(2):
            m.set_ema_state(e0, 0)
            for _ in range(2):
                m.train_step(x, y, 0.0, cfg)          # lr 0: the weights stay, the average moves towards them
            results.append(m.get_ema())
            assert m.get_params().tobytes() == p.tobytes()
        assert results[0][0].tobytes() == results[1][0].tobytes() and results[0][1] == results[1][1] == 2
        want = EO.run([p, p], e0, 0.9, False)
        assert np.all(np.abs(results[0][0] - want) <= EO.bound([p, p], e0)) and np.abs(results[0][0] - e0).max() > 1e-3
    finally:
        m.close()
