"""CPU: deploy_options.optimizer -- the float64 oracle (tests/optim_oracle.py) against an independent statement (torch.optim in
float64), the parsing of the mapping and its refusals, and the engine over tests/fake_optimizer_device.py: one set_optimizer call per
built model and one after growth, the decay mask, what a checkpoint's index holds, the refused resume across slot families, and the
shipped overlays."""

import json
import os

import numpy as np
import pytest

import optim_oracle as OO
from fake_optimizer_device import install
from oracle import unet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = dict(n_filters_first=3, n_downsample=2, rate=2, kernel_size=3, conv_stride=1, bn=True, padding='same')
LOSS = {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}}


def config(optimizer='adam', **deploy):
    d = {'optimizer': optimizer, 'loss': LOSS, 'enable_multigpu': False, 'metrics': []}
    d.update(deploy)
    return {'model': 'UNetAnnotator', 'model_options': OPTS, 'deploy_options': d, 'data_options': {'eval': {'batch_size': 2}}}


def mapping(class_name, **cfg):
    return {'class_name': class_name, 'config': cfg}


# ---- 1. the oracle against torch.optim ------------------------------------------------------------------------------------------
SIZES = (7, 1, 12)          # three "variables"
SLICES = [('a.kernel', slice(0, 7)), ('a.bias', slice(7, 8)), ('b.kernel', slice(8, 20))]
LR, STEPS = 3e-3, 6


def _run_torch(make, grads, p0, clip=None):
    import torch
    ps = [torch.tensor(p0[sl], dtype=torch.float64, requires_grad=True) for _, sl in SLICES]
    opt = make(ps)
    for g in grads:
        for p, (_, sl) in zip(ps, SLICES):
            p.grad = torch.tensor(g[sl], dtype=torch.float64)
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(ps, clip)
        opt.step()
    return np.concatenate([p.detach().numpy() for p in ps])


def _run_oracle(s, grads, p0, decay=(1, 1, 1)):
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t, g in enumerate(grads, 1):
        r = OO.step(s, SLICES, decay, p, m, v, g, t, LR, round32=False)
        p, m, v = r['p'], r['m'], r['v']
    return p


def _problem():
    # gradient norms of 4 .. 40: PyTorch's clip_grad_norm_ adds 1e-6 to the norm, a relative 1e-6 / norm on the scale, and a relative
    # change of the gradient moves Adam's step by about lr times as much -- far inside the 1e-8 asked of that comparison
    rng = np.random.default_rng(11)
    return rng.standard_normal(20), [rng.standard_normal(20) * 10.0 ** rng.integers(0, 2) for _ in range(STEPS)]


def test_oracle_against_torch_optim():
    import torch
    p0, grads = _problem()
    cases = {
        'adam': (OO.spec('adam', epsilon=0.0), lambda ps: torch.optim.Adam(ps, lr=LR, eps=0.0)),
        'adamw': (OO.spec('adamw', epsilon=0.0, weight_decay=0.05), lambda ps: torch.optim.AdamW(ps, lr=LR, eps=0.0, weight_decay=0.05)),
        'sgd': (OO.spec('sgd'), lambda ps: torch.optim.SGD(ps, lr=LR)),
        'sgd_momentum': (OO.spec('sgd', momentum=0.9), lambda ps: torch.optim.SGD(ps, lr=LR, momentum=0.9)),
        'sgd_nesterov': (OO.spec('sgd', momentum=0.9, nesterov=True), lambda ps: torch.optim.SGD(ps, lr=LR, momentum=0.9, nesterov=True)),
    }
    for name, (s, make) in cases.items():
        err = np.abs(_run_oracle(s, grads, p0) - _run_torch(make, grads, p0)).max()
        print(name, 'oracle - torch.optim: %.3g' % err)
        assert err <= 1e-12, name
    # global-norm clipping: PyTorch adds 1e-6 to the norm
    c = 0.5 * min(np.linalg.norm(g) for g in grads)
    err = np.abs(_run_oracle(OO.spec('adam', epsilon=0.0, global_clipnorm=c), grads, p0) -
                 _run_torch(lambda ps: torch.optim.Adam(ps, lr=LR, eps=0.0), grads, p0, clip=c)).max()
    print('adam + clip_grad_norm_: %.3g' % err)
    assert err <= 1e-8


def test_oracle_transforms_and_decay_mask():
    g = np.zeros(20, np.float32)
    g[:7] = 3.0
    g[7] = -40.0
    g[8:] = 0.25
    # clipvalue first, then the norms of what is left
    gh, total, per, scales = OO.transforms(OO.spec('adam', clipvalue=5.0, clipnorm=2.0), SLICES, g)
    assert gh[7] == -5.0 and np.allclose(per, [3.0 * np.sqrt(7), 5.0, 0.25 * np.sqrt(12)], rtol=1e-15)
    assert scales[2] == 1.0 and scales[1] == OO.f32(2.0 / 5.0) and abs(total - np.sqrt(63 + 25 + 0.75)) < 1e-14
    # zero gradient: scale exactly 1, never 0 / 0; norm == c: exactly 1
    assert np.all(OO.transforms(OO.spec('adam', global_clipnorm=1.0), SLICES, np.zeros(20))[3] == 1.0)
    one = np.zeros(20, np.float32)
    one[3] = 0.75
    assert np.all(OO.transforms(OO.spec('adam', global_clipnorm=0.75), SLICES, one)[3] == 1.0)
    # AdamW's decay reaches only the flagged variables: with a zero gradient nothing else moves
    p = np.linspace(-1, 1, 20).astype(np.float32)
    r = OO.step(OO.spec('adamw', weight_decay=0.1), SLICES, (1, 0, 1), p, np.zeros(20), np.zeros(20), np.zeros(20), 1, 0.5)
    assert r['p'][7] == p[7] and np.allclose(r['p'][:7], p[:7] * (1 - OO.f32(OO.f32(0.5) * OO.f32(0.1))))


# ---- 2. parsing -----------------------------------------------------------------------------------------------------------------
def test_config_parsing_accepts():
    from dnncancerannotator_amd import engine
    e = engine.TFKerasModel(config())
    assert e.optimizer is None and e.learning_rate == 0.001 and e.adam == dict(beta1=0.9, beta2=0.999, epsilon=1e-7)
    o = engine.TFKerasModel(config(mapping('Adam'))).optimizer
    assert o['device'] == dict(kind='adam', clipvalue=0.0, clipnorm=0.0, global_clipnorm=0.0, beta1=0.9, beta2=0.999, epsilon=1e-7)
    assert o['learning_rate'] == 0.001 and o['config']['amsgrad'] is False and o['config']['clipnorm'] is None
    e = engine.TFKerasModel(config(mapping('Adam', learning_rate=0.01, beta_1=0.8, beta_2=0.99, epsilon=1e-8, clipvalue=0.5, clipnorm=2)))
    assert e.learning_rate == 0.01 and e.adam == dict(beta1=0.8, beta2=0.99, epsilon=1e-8)
    assert e.optimizer['device']['clipvalue'] == 0.5 and e.optimizer['device']['clipnorm'] == 2.0
    o = engine.TFKerasModel(config(mapping('AdamW', weight_decay=0.05, global_clipnorm=1.0))).optimizer
    assert o['device']['kind'] == 'adamw' and o['device']['weight_decay'] == 0.05 and o['device']['global_clipnorm'] == 1.0
    assert o['exclude'] == ('bias', 'beta', 'gamma')
    assert engine.TFKerasModel(config(mapping('AdamW', exclude_from_weight_decay=['head']))).optimizer['exclude'] == ('head',)
    assert engine.TFKerasModel(config(mapping('AdamW', weight_decay=0))).optimizer['device']['weight_decay'] == 0.0
    o = engine.TFKerasModel(config(mapping('SGD', momentum=0.9, nesterov=True))).optimizer
    assert o['device'] == dict(kind='sgd', clipvalue=0.0, clipnorm=0.0, global_clipnorm=0.0, momentum=0.9, nesterov=True)
    assert o['learning_rate'] == 0.01                                              # Keras' SGD default
    assert engine.TFKerasModel(config('sgd')).optimizer['device']['kind'] == 'sgd'   # Keras' string identifiers
    assert engine.TFKerasModel(config('AdamW')).optimizer['config']['weight_decay'] == 0.004
    assert engine.TFKerasModel(config({'class_name': 'SGD'})).optimizer['device']['momentum'] == 0.0
    # the saved config keeps the key as it was given
    assert engine.TFKerasModel(config(mapping('SGD', momentum=0.5))).model_config['deploy_options']['optimizer'] == mapping('SGD', momentum=0.5)


@pytest.mark.parametrize('bad, match', [
    (mapping('Adam', amsgrad=True), 'amsgrad'),
    (mapping('AdamW', amsgrad=True), 'amsgrad'),
    (mapping('Adam', amsgrad='no'), 'amsgrad'),
    (mapping('Adam', clipnorm=1.0, global_clipnorm=1.0), 'exclude each other'),
    (mapping('Adam', clipnorm=-1.0), 'clipnorm'),
    (mapping('Adam', clipnorm=0.0), 'clipnorm'),
    (mapping('Adam', clipvalue=float('nan')), 'clipvalue'),
    (mapping('SGD', global_clipnorm=float('inf')), 'global_clipnorm'),
    (mapping('Adam', learning_rate=-0.1), 'learning_rate'),
    (mapping('Adam', learning_rate=float('nan')), 'learning_rate'),
    (mapping('Adam', learning_rate='0.1'), 'learning_rate'),
    (mapping('Adam', beta_1=1.0), 'beta_1'),
    (mapping('Adam', beta_2=-0.1), 'beta_2'),
    (mapping('Adam', epsilon=-1e-7), 'epsilon'),
    (mapping('AdamW', weight_decay=-0.01), 'weight_decay'),
    (mapping('AdamW', weight_decay=float('nan')), 'weight_decay'),
    (mapping('AdamW', weight_decay=True), 'weight_decay'),
    (mapping('AdamW', exclude_from_weight_decay='bias'), 'exclude_from_weight_decay'),
    (mapping('SGD', momentum=1.0), 'momentum'),
    (mapping('SGD', momentum=-0.5), 'momentum'),
    (mapping('SGD', nesterov=1), 'nesterov'),
    (mapping('Adam', momentum=0.9), 'unknown keys'),
    (mapping('SGD', beta_1=0.9), 'unknown keys'),
    (mapping('Adam', weight_decay=0.1), 'unknown keys'),
    (mapping('Adam', lr=0.1), 'unknown keys'),
    (mapping('RMSprop'), 'unknown class_name'),
    ('rmsprop', 'unknown optimizer'),
    ({'class_name': 'Adam', 'config': {}, 'extra': 1}, 'mapping'),
    ({'config': {}}, 'mapping'),
    ({'class_name': 'Adam', 'config': [1]}, 'config must be a mapping'),
    (None, 'mapping'),
    (7, 'mapping'),
])
def test_config_parsing_refuses(bad, match, monkeypatch):
    from dnncancerannotator_amd import device, engine
    monkeypatch.setattr(device, 'init_device', lambda *a: pytest.fail('a device call before the refusal'))
    with pytest.raises(ValueError, match=match):
        engine.TFKerasModel(config(bad))


# ---- 3. the engine over the fake device -----------------------------------------------------------------------------------------
def _data():
    from dnncancerannotator_amd import data
    x, y = O.synthetic_batch(8, 16, 16, 1, seed_x=3, seed_y=4)
    return x, y, data.ArrayDataset(x, y, 4, repeat=True)


def _trained(tmp_path, monkeypatch, optimizer, steps=4, name='run'):
    from dnncancerannotator_amd import engine
    built = install(monkeypatch.setattr)
    monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
    _, _, ds = _data()
    e = engine.TFKerasModel(config(optimizer))
    e.train(ds, save_path=str(tmp_path / name), max_steps=steps, save_freq=2)
    return e, built, str(tmp_path / name)


def _set_calls(dm):
    return [c for c in dm.calls if c[0] == 'set_optimizer']


def test_set_optimizer_once_per_model_again_after_growth_and_the_decay_mask(tmp_path, monkeypatch):
    from dnncancerannotator_amd import engine
    built = install(monkeypatch.setattr)
    _, _, ds = _data()
    e = engine.TFKerasModel(config(mapping('AdamW', weight_decay=0.05, global_clipnorm=1.0)))
    e._build(ds)
    dm = e.device_model
    (call,) = _set_calls(dm)
    assert call[1] == 'adamw' and call[2]['weight_decay'] == 0.05 and call[2]['global_clipnorm'] == 1.0
    names = dm.trainable_names()
    excluded = [n for n, flag in zip(names, call[3]) if not flag]
    assert excluded == [n for n in names if n.endswith(('.bias', '.beta', '.gamma'))] and excluded
    assert {n.rsplit('.', 1)[1] for n in excluded} == {'bias', 'beta', 'gamma'}
    assert all(n.endswith('.kernel') for n, flag in zip(names, call[3]) if flag)
    assert e._ensure_capacity(6) and e.device_model is built[-1] and e.device_model is not dm
    assert _set_calls(e.device_model) == [call] and e.device_model.max_batch == 6      # the same call on the bigger model
    assert e._build(ds) is None and len(_set_calls(e.device_model)) == 1               # a second _build makes none
    # the string adam: no call at all
    plain = engine.TFKerasModel(config())
    plain._build(ds)
    assert _set_calls(plain.device_model) == []
    # a custom exclusion list
    only = engine.TFKerasModel(config(mapping('AdamW', exclude_from_weight_decay=['head', 'gamma'])))
    only._build(ds)
    mask = _set_calls(only.device_model)[0][3]
    assert [n for n, f in zip(names, mask) if not f] == [n for n in names if 'head' in n or 'gamma' in n]


def test_checkpoint_index_gains_the_entry_only_for_a_mapping(tmp_path, monkeypatch):
    opt = mapping('SGD', learning_rate=0.05, momentum=0.9, nesterov=True)
    e, _, run = _trained(tmp_path, monkeypatch, opt)
    index = json.load(open(os.path.join(run, 'checkpoints', 'ckpt-4.index')))
    assert index['optimizer']['class_name'] == 'SGD'
    assert index['optimizer']['config'] == dict(learning_rate=0.05, momentum=0.9, nesterov=True, clipvalue=None, clipnorm=None,
                                                global_clipnorm=None)
    assert index['learning_rate'] == 0.05 and index['iterations'] == 4
    with np.load(os.path.join(run, 'checkpoints', 'ckpt-4.data-00000-of-00001')) as z:
        assert z.files == ['params', 'state', 'adam_m', 'adam_v']                  # the data file keeps its arrays
        assert np.abs(z['adam_m']).max() > 0 and not np.any(z['adam_v'])           # the accumulator; SGD's adam_v is zeros
    _, _, run0 = _trained(tmp_path, monkeypatch, 'adam', name='plain')
    index0 = json.load(open(os.path.join(run0, 'checkpoints', 'ckpt-4.index')))
    assert list(index0) == ['format', 'step', 'iterations', 'learning_rate', 'variables']      # exactly what it was
    with np.load(os.path.join(run0, 'checkpoints', 'ckpt-4.data-00000-of-00001')) as z:
        assert z.files == ['params', 'state', 'adam_m', 'adam_v'] and np.any(z['adam_v'])


def test_resume_across_slot_families_is_refused(tmp_path, monkeypatch):
    from dnncancerannotator_amd import engine
    _, _, run_adam = _trained(tmp_path, monkeypatch, 'adam', name='adam')
    _, _, run_w = _trained(tmp_path, monkeypatch, mapping('AdamW'), name='adamw')
    e_sgd, _, run_sgd = _trained(tmp_path, monkeypatch, mapping('SGD', momentum=0.9), name='sgd')
    _, _, ds = _data()
    ck = {k: os.path.join(r, 'checkpoints', 'ckpt-2') for k, r in (('adam', run_adam), ('adamw', run_w), ('sgd', run_sgd))}

    def fresh(optimizer):
        e = engine.TFKerasModel(config(optimizer))
        e._build(ds)
        return e
    sgd = fresh(mapping('SGD', momentum=0.9))
    before = sgd.device_model.get_params()
    for other in ('adam', 'adamw'):
        with pytest.raises(ValueError, match='optimizer slots of Adam'):
            sgd.load(ck[other])
    assert np.array_equal(sgd.device_model.get_params(), before)          # refused from the index, before any data is read
    for own in ('adam', mapping('AdamW'), mapping('Adam', global_clipnorm=1.0)):
        with pytest.raises(ValueError, match='optimizer slots of SGD'):
            fresh(own).load(ck['sgd'])
    # inside a family everything loads: a checkpoint without the entry into Adam / AdamW, AdamW's into Adam, SGD's into SGD
    fresh(mapping('AdamW')).load(ck['adam'])
    fresh('adam').load(ck['adamw'])
    fresh(mapping('Adam', clipnorm=1.0)).load(ck['adam'])
    sgd.load(ck['sgd'])
    with np.load(ck['sgd'] + '.data-00000-of-00001') as z:
        assert np.array_equal(sgd.device_model.get_opt_state()[0], z['adam_m']) and sgd.device_model.get_opt_state()[2] == 2
    # and auto-resume goes through the same door
    again = engine.TFKerasModel(config(mapping('Adam')))
    with pytest.raises(ValueError, match='optimizer slots of SGD'):
        again.train(ds, save_path=run_sgd, max_steps=6, save_freq=2)


def test_fake_steps_follow_the_oracle_and_the_schedule_starts_at_learning_rate(tmp_path, monkeypatch):
    from dnncancerannotator_amd import engine
    install(monkeypatch.setattr)
    monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
    _, _, ds = _data()
    e = engine.TFKerasModel(config(mapping('SGD', learning_rate=0.04, momentum=0.5),
                                   LearningRateScheduler='lambda epoch, current_lr: current_lr * 0.5'))
    res = e.train(ds, max_steps=3, save_freq=100)
    assert res.history['lr'] == [0.02, 0.01, 0.005]


@pytest.mark.parametrize('overlay, want', [
    ('adamw.yaml', ('AdamW', 'adamw')), ('clip_global_norm.yaml', ('Adam', 'adam')), ('sgd_nesterov.yaml', ('SGD', 'sgd'))])
def test_overlays_merge_over_the_base_config(overlay, want):
    from dnncancerannotator_amd import engine, load
    base = config()
    assert base['deploy_options']['optimizer'] == 'adam'
    cfg = load._apply_config(base, load.load_config(os.path.join(ROOT, 'configs', 'additionals', overlay)))
    assert isinstance(cfg['deploy_options']['optimizer'], dict)          # the mapping replaces the string
    assert cfg['deploy_options']['loss'] == LOSS                          # and nothing else
    o = engine.TFKerasModel(cfg).optimizer
    assert (o['class_name'], o['device']['kind']) == want
    if overlay == 'clip_global_norm.yaml':
        assert o['device']['global_clipnorm'] == 1.0
    if overlay == 'sgd_nesterov.yaml':
        assert o['device']['nesterov'] is True and o['device']['momentum'] == 0.9
    if overlay == 'adamw.yaml':
        assert o['device']['weight_decay'] == 0.004 and o['exclude'] == ('bias', 'beta', 'gamma')
