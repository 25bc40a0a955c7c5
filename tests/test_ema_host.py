"""CPU: deploy_options.ema -- parsing, what a checkpoint holds with and without the option, the three resume cases, `--weights ema`
refused from the index files alone, and validation inside the exchange (tests/fake_ema_device.py stands in for the device)."""

import json
import logging
import os

import numpy as np
import pytest

import ema_oracle as EO
from fake_ema_device import install
from oracle import unet_oracle as O

OPTS = dict(n_filters_first=3, n_downsample=2, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')
EMA = dict(decay=0.5, warmup=False)


def config(**deploy):
    d = {'optimizer': 'adam', 'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}}, 'enable_multigpu': False,
         'metrics': [{'Precision': {'thresholds': 0.5, 'name': 'pixel/precision'}}]}
    d.update(deploy)
    return {'model': 'UNetAnnotator', 'model_options': OPTS, 'deploy_options': d, 'data_options': {'eval': {'batch_size': 2}}}


def _data():
    from dnncancerannotator_amd import data
    x, y = O.synthetic_batch(8, 16, 16, 1, seed_x=3, seed_y=4)
    return x, y, data.ArrayDataset(x, y, 4, repeat=True)


def _trained(tmp_path, monkeypatch, ema, steps=4, name='run', **kw):
    from dnncancerannotator_amd import data, engine
    install(monkeypatch.setattr)
    monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
    x, y, ds = _data()
    e = engine.TFKerasModel(config(**({} if ema is None else dict(ema=ema))))
    e.learning_rate = 0.05
    res = e.train(ds, save_path=str(tmp_path / name), max_steps=steps, save_freq=2, val_data=data.ArrayDataset(x[:4], y[:4], 4), **kw)
    return e, res, str(tmp_path / name)


def test_key_parsing():
    from dnncancerannotator_amd import engine
    assert engine.TFKerasModel(config()).ema is None
    assert engine.TFKerasModel(config(ema={})).ema == dict(decay=0.999, warmup=True, validate='ema')
    assert engine.TFKerasModel(config(ema=dict(decay=0.9, warmup=False, validate='raw'))).ema == dict(decay=0.9, warmup=False, validate='raw')
    for bad in (0.0, 1.0, -0.1, 1.5, float('nan'), float('inf'), '0.9', None, True):
        with pytest.raises(ValueError, match='decay'):
            engine.TFKerasModel(config(ema=dict(decay=bad)))
    with pytest.raises(ValueError, match='unknown keys'):
        engine.TFKerasModel(config(ema=dict(decay=0.9, momentum=0.1)))
    for bad in ('EMA', 'both', True, None):
        with pytest.raises(ValueError, match='validate'):
            engine.TFKerasModel(config(ema=dict(validate=bad)))
    with pytest.raises(ValueError, match='warmup'):
        engine.TFKerasModel(config(ema=dict(warmup='yes')))
    with pytest.raises(ValueError, match='mapping'):
        engine.TFKerasModel(config(ema=0.999))
    assert engine.TFKerasModel(config(ema=dict(EMA))).model_config['deploy_options']['ema'] == EMA      # the saved config keeps the key


def test_shipped_overlay_parses():
    from dnncancerannotator_amd import engine, load
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load._apply_config(config(), load.load_config(os.path.join(root, 'configs', 'additionals', 'ema.yaml')))
    assert engine.TFKerasModel(cfg).ema == dict(decay=0.999, warmup=True, validate='ema')


def test_checkpoint_contents_with_and_without_the_option(tmp_path, monkeypatch):
    e, _, run = _trained(tmp_path, monkeypatch, dict(EMA))
    path = os.path.join(run, 'checkpoints', 'ckpt-4')
    index = json.load(open(path + '.index'))
    assert index['ema'] == dict(decay=0.5, warmup=False, num_updates=4) and index['format'] == 'dnnca-ckpt-1'
    with np.load(path + '.data-00000-of-00001') as z:
        assert sorted(z.files) == ['adam_m', 'adam_v', 'ema', 'params', 'state']
        average, raw = z['ema'], z['params']
    assert np.array_equal(average, e.device_model.get_ema()[0]) and np.array_equal(raw, e.device_model.get_params())
    assert average.dtype == np.float32 and np.abs(average - raw).max() > 1e-3          # written with the raw weights in place
    plain, _, run0 = _trained(tmp_path, monkeypatch, None, name='plain')
    index0 = json.load(open(os.path.join(run0, 'checkpoints', 'ckpt-4.index')))
    assert list(index0) == ['format', 'step', 'iterations', 'learning_rate', 'variables']               # exactly what it was
    with np.load(os.path.join(run0, 'checkpoints', 'ckpt-4.data-00000-of-00001')) as z:
        assert z.files == ['params', 'state', 'adam_m', 'adam_v']
    assert not [c for c in plain.device_model.calls if c[0] in ('set_ema', 'exchange_ema', 'set_ema_state')]


def test_resume_cases(tmp_path, monkeypatch, caplog):
    from dnncancerannotator_amd import engine
    e, _, run = _trained(tmp_path, monkeypatch, dict(EMA))
    _, _, run0 = _trained(tmp_path, monkeypatch, None, name='plain')
    _, _, ds = _data()
    ck, ck0 = os.path.join(run, 'checkpoints', 'ckpt-2'), os.path.join(run0, 'checkpoints', 'ckpt-2')
    with np.load(ck + '.data-00000-of-00001') as z:
        saved, raw = z['ema'].copy(), z['params'].copy()
    # both have one: restored bit for bit, with the count
    a = engine.TFKerasModel(config(ema=dict(EMA)))
    a._build(ds)
    a.load(ck)
    got, n = a.device_model.get_ema()
    assert np.array_equal(got, saved) and n == 2 and np.array_equal(a.device_model.get_params(), raw)
    # the model has one, the file does not: e <- p, count 0, one warning
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        a.load(ck0)
    assert len([r for r in caplog.records if 'weight average' in r.getMessage()]) == 1
    got, n = a.device_model.get_ema()
    assert np.array_equal(got, a.device_model.get_params()) and n == 0
    # the file has one, the model does not: ignored
    b = engine.TFKerasModel(config())
    b._build(ds)
    b.load(ck)
    assert np.array_equal(b.device_model.get_params(), raw)
    assert not [c for c in b.device_model.calls if c[0] in ('set_ema', 'set_ema_state')]
    # weights='ema': the file's average becomes the parameters, with or without a device average
    b.load(ck, weights='ema')
    assert np.array_equal(b.device_model.get_params(), saved) and not [c for c in b.device_model.calls if c[0] == 'set_ema_state']
    with pytest.raises(ValueError, match='no weight average'):
        b.load(ck0, weights='ema')
    with pytest.raises(ValueError, match='--weights'):
        b.load(ck, weights='mean')


def test_average_follows_the_oracle_and_survives_growth(tmp_path, monkeypatch):
    """the engine's own steps: the saved average is the recurrence over the weights the device wrote; _ensure_capacity carries it"""
    from dnncancerannotator_amd import engine
    built = install(monkeypatch.setattr)
    x, y, ds = _data()
    e = engine.TFKerasModel(config(ema=dict(decay=0.999, warmup=True)))
    e._build(ds)
    dm = e.device_model
    e0 = dm.get_ema()[0]
    assert np.array_equal(e0, dm.get_params()) and dm.get_ema()[1] == 0
    thetas = []
    for _ in range(3):
        dm.train_step(x[:4], y[:4], 0.05, dm.loss_cfg(weight_mul=3.0))
        thetas.append(dm.get_params())
    want = EO.run(thetas, e0, 0.999, True)
    assert np.abs(dm.get_ema()[0] - want).max() <= 1e-6 and dm.get_ema()[1] == 3
    assert float(EO.om_of(1, 0.999, True)) == float(np.float32(1 - 2 / 11))
    before = dm.get_ema()
    assert e._ensure_capacity(6) and e.device_model is built[-1] and e.device_model is not dm
    after = e.device_model.get_ema()
    assert np.array_equal(after[0], before[0]) and after[1] == 3 and e.device_model.max_batch == 6


def test_validation_runs_inside_the_exchange(tmp_path, monkeypatch):
    from dnncancerannotator_amd import engine
    e, res, _ = _trained(tmp_path, monkeypatch, dict(EMA))
    calls = e.device_model.calls
    kinds = [c[0] if c[0] != 'eval_in_use' else ('eval', c[1]) for c in calls if c[0] in ('exchange_ema', 'eval_in_use', 'train')]
    assert kinds == ['train', 'train', 'exchange_ema', ('eval', True), 'exchange_ema'] * 2
    assert len(res.history['val_loss']) == 2 and not e.device_model.in_use
    # validate: raw -- no exchange, validation on the raw weights
    r, res_raw, _ = _trained(tmp_path, monkeypatch, dict(EMA, validate='raw'), name='raw')
    assert not [c for c in r.device_model.calls if c[0] == 'exchange_ema']
    assert [c[1] for c in r.device_model.calls if c[0] == 'eval_in_use'] == [False, False]
    assert res_raw.history['loss'] == res.history['loss'] and res_raw.history['val_loss'] != res.history['val_loss']
    # the exchange is undone when _evaluate raises
    install(monkeypatch.setattr)

    def boom(self, dataset, **kw):
        assert self.device_model.in_use
        raise RuntimeError('validation failed')
    monkeypatch.setattr(engine.TFKerasModel, '_evaluate', boom)
    x, y, ds = _data()
    f = engine.TFKerasModel(config(ema=dict(EMA)))
    with pytest.raises(RuntimeError, match='validation failed'):
        f.train(ds, max_steps=2, save_freq=2, val_data=ds)
    assert not f.device_model.in_use and [c[0] for c in f.device_model.calls].count('exchange_ema') == 2
    assert f._averaged_in_use is False
    f.device_model.train_step(x[:4], y[:4], 0.05, f.device_model.loss_cfg(weight_mul=3.0))        # and training goes on


def test_weights_ema_is_refused_from_the_index_before_any_data_is_opened(tmp_path, monkeypatch):
    import yaml
    from dnncancerannotator_amd import __main__ as cli, engine
    from dnncancerannotator_amd.runs import evaluate as run_evaluate, predict as run_predict
    _, _, run0 = _trained(tmp_path, monkeypatch, None, name='plain')
    _, _, run = _trained(tmp_path, monkeypatch, dict(EMA))
    for r, cfg in ((run0, config()), (run, config(ema=dict(EMA)))):
        with open(os.path.join(r, 'options.yaml'), 'w') as f:
            yaml.safe_dump({'config': cfg}, f)
    opened, seen = [], []
    monkeypatch.setattr(run_evaluate, 'make_dataset', lambda *a, **k: opened.append('evaluate') or 'ds')
    monkeypatch.setattr(run_predict, 'make_dataset', lambda *a, **k: opened.append('predict') or 'ds')
    monkeypatch.setattr(engine.TFKerasModel, 'eval', lambda self, dataset, **kw: seen.append(kw) or {})
    monkeypatch.setattr(engine.TFKerasModel, 'annotate', lambda self, dataset, **kw: seen.append(kw) or {})
    ev = ['evaluate', '--data_path', 'synthetic:16x16x2', '--tag', 't', '--skip_visualization', '--save_path']
    pr = ['predict', '--data_path', 'synthetic:16x16x2', '--output', str(tmp_path / 'o'), '--save_path']
    for base in (ev, pr):
        with pytest.raises(ValueError, match=r'ckpt-\d+ holds no weight average'):
            cli.main(base + [run0, '--weights', 'ema'])
    with pytest.raises(ValueError, match='ckpt-4 holds no weight average'):
        cli.main(pr + [run0, '--weights', 'ema', '--step', '4'])
    assert opened == [] and seen == []
    # a run with averages passes the check; the keyword travels only with the flag
    assert cli.main(ev + [run, '--weights', 'ema']) == 0 and cli.main(pr + [run, '--weights', 'ema']) == 0
    assert cli.main(ev + [run]) == 0 and cli.main(pr + [run, '--weights', 'raw']) == 0
    assert [kw.get('weights') for kw in seen] == ['ema', 'ema', None, None]
    # one checkpoint of the run without an average: named, unless the step range leaves it out
    index = os.path.join(run, 'checkpoints', 'ckpt-2.index')
    entry = json.load(open(index))
    del entry['ema']
    json.dump(entry, open(index, 'w'))
    with pytest.raises(ValueError, match='ckpt-2 holds no weight average'):
        cli.main(ev + [run, '--weights', 'ema'])
    assert cli.main(ev + [run, '--weights', 'ema', '--step_range', '3', '9']) == 0 and cli.main(pr + [run, '--weights', 'ema']) == 0
    with pytest.raises(SystemExit):
        cli.main(ev + [run, '--weights', 'mean'])


def test_engine_eval_and_annotate_read_the_averaged_checkpoint(tmp_path, monkeypatch):
    """engine level: eval(weights='ema') loads every checkpoint's average; without the keyword the load is today's call"""
    from dnncancerannotator_amd import data, engine
    e, _, run = _trained(tmp_path, monkeypatch, dict(EMA))
    x, y, _ = _data()
    ev = data.ArrayDataset(x[:4], y[:4], 4)
    loads = []
    real = engine.TFKerasModel.load
    monkeypatch.setattr(engine.TFKerasModel, 'load', lambda self, path, **kw: loads.append((os.path.basename(path), kw)) or real(self, path, **kw))
    rows_raw = e.eval(ev, run, tag='raw')
    rows_ema = e.eval(ev, run, tag='ema', weights='ema')
    assert loads == [('ckpt-2', {}), ('ckpt-4', {}), ('ckpt-2', dict(weights='ema')), ('ckpt-4', dict(weights='ema'))]
    assert list(rows_raw) == list(rows_ema) == [2, 4] and rows_raw[4]['loss'] != rows_ema[4]['loss']
    with np.load(os.path.join(run, 'checkpoints', 'ckpt-4.data-00000-of-00001')) as z:
        assert np.array_equal(e.device_model.get_params(), z['ema'])
    with pytest.raises(ValueError, match='--weights'):
        e.eval(ev, run, tag='bad', weights='mean')
