"""CPU: deploy_options.gradient_accumulation_steps -- what check_accumulation accepts and refuses, the configurations train() refuses
before it reads any data, the dropped partial cycle, the setting carried over to a regrown model, no call without the key, the
shipped overlays, and two gloo ranks that call the same sequence (tests/fake_accumulate_device.py in place of the HIP device)."""

import json
import logging
import os

import numpy as np
import pytest

from fake_accumulate_device import install
from oracle import unet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = dict(n_filters_first=3, n_downsample=2, rate=2, kernel_size=3, conv_stride=1, bn=True, padding='same')
LOSS = {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}}
KEY = 'gradient_accumulation_steps'


def config(k=None, **deploy):
    d = {'optimizer': 'adam', 'loss': LOSS, 'enable_multigpu': False, 'metrics': []}
    if k is not None:
        d[KEY] = k
    d.update(deploy)
    return {'model': 'UNetAnnotator', 'model_options': OPTS, 'deploy_options': d, 'data_options': {'eval': {'batch_size': 2}}}


def _data(repeat=True, n=8):
    from dnncancerannotator_amd import data
    x, y = O.synthetic_batch(n, 16, 16, 1, seed_x=3, seed_y=4)
    return data.ArrayDataset(x, y, 4, repeat=repeat)


class Unread:
    """a data set that may be asked for its element shape and nothing else"""

    def __init__(self):
        self.element_spec = _data().element_spec

    def __iter__(self):
        pytest.fail('the data set was read before the refusal')


def _set_calls(dm):
    return [c for c in dm.calls if c[0] == 'set_accumulation']


@pytest.mark.parametrize('value, want', [(None, 1), (1, 1), (2, 2), (7, 7), (4096, 4096)])
def test_check_accumulation_accepts(value, want):
    from dnncancerannotator_amd import engine
    assert engine.check_accumulation(value) == want
    got = engine.TFKerasModel(config(value)).accumulation
    assert got == want and type(got) is int


@pytest.mark.parametrize('bad', [0, -1, 4097, True, False, 2.0, 1.5, '2', 'two', [2], {'steps': 2}, float('nan')])
def test_check_accumulation_refuses_with_the_key_in_the_message(bad, monkeypatch):
    from dnncancerannotator_amd import device, engine
    monkeypatch.setattr(device, 'init_device', lambda *a: pytest.fail('a device call before the refusal'))
    with pytest.raises(ValueError, match='deploy_options.gradient_accumulation_steps') as e:
        engine.check_accumulation(bad)
    assert repr(bad) in str(e.value)
    with pytest.raises(ValueError, match='deploy_options.gradient_accumulation_steps'):
        engine.TFKerasModel(config(bad))


@pytest.mark.parametrize('kw, numbers', [(dict(save_freq=5, max_steps=10), ('2', 'save_freq 5')),
                                         (dict(save_freq=2, max_steps=7), ('2', 'max_steps 7'))])
def test_train_refuses_a_schedule_that_cuts_a_cycle_before_reading_data(kw, numbers, tmp_path, monkeypatch):
    from dnncancerannotator_amd import engine
    built = install(monkeypatch.setattr)
    monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
    e = engine.TFKerasModel(config(2))
    with pytest.raises(ValueError, match=KEY) as err:
        e.train(Unread(), save_path=str(tmp_path / 'run'), **kw)
    assert all(n in str(err.value) for n in numbers), str(err.value)
    assert built == [] and not os.path.exists(tmp_path / 'run')          # before anything was built or written
    # the same numbers are fine without the key, and max_steps may be left open
    engine.check_accumulation_schedule(1, kw['save_freq'], kw['max_steps'], 3)
    engine.check_accumulation_schedule(2, 4, None, 6)


def test_train_refuses_a_resumed_step_inside_a_cycle_before_reading_data(tmp_path, monkeypatch):
    from dnncancerannotator_amd import engine
    install(monkeypatch.setattr)
    monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
    run = str(tmp_path / 'run')
    engine.TFKerasModel(config()).train(_data(), save_path=run, max_steps=3, save_freq=3)
    assert os.path.exists(os.path.join(run, 'checkpoints', 'ckpt-3.index'))
    e = engine.TFKerasModel(config(2))
    with pytest.raises(ValueError, match=KEY) as err:
        e.train(Unread(), save_path=run, max_steps=6, save_freq=2)
    assert 'resumed step 3' in str(err.value) and ' 2 ' in str(err.value)
    assert [c for c in e.device_model.calls if c[0] == 'train'] == []
    # three divides it: that run goes on, one update per three steps
    e3 = engine.TFKerasModel(config(3))
    res = e3.train(_data(), save_path=run, max_steps=6, save_freq=3)
    assert len(res.history['loss']) == 3 and e3.device_model.iterations == 3 + 1
    assert json.load(open(os.path.join(run, 'checkpoints', 'ckpt-6.index')))['iterations'] == 4


def test_partial_cycle_is_dropped_with_one_warning_when_the_data_ends(monkeypatch, caplog):
    from dnncancerannotator_amd import engine
    install(monkeypatch.setattr)
    monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
    e = engine.TFKerasModel(config(2))
    with caplog.at_level(logging.WARNING):
        res = e.train(_data(repeat=False, n=12), save_freq=100)          # three batches, no max_steps: the second cycle stays open
    dm = e.device_model
    assert len(res.history['loss']) == 3 and dm.iterations == 1
    assert len([r for r in caplog.records if 'partial cycle' in r.getMessage()]) == 1
    assert _set_calls(dm) == [('set_accumulation', 2)] * 2                # once when built, once to reset the counter
    assert dm.get_accumulation()[1:] == (2, 0)
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        e2 = engine.TFKerasModel(config(2))
        e2.train(_data(repeat=False, n=8), save_freq=100)                 # two batches: the data ends between cycles
    assert not [r for r in caplog.records if 'partial cycle' in r.getMessage()]
    assert _set_calls(e2.device_model) == [('set_accumulation', 2)]


def test_one_call_per_built_model_again_after_growth_and_none_without_the_key(monkeypatch):
    from dnncancerannotator_amd import engine
    built = install(monkeypatch.setattr)
    ds = _data()
    e = engine.TFKerasModel(config(4))
    e._build(ds)
    dm = e.device_model
    assert _set_calls(dm) == [('set_accumulation', 4)]
    assert e._ensure_capacity(6) and e.device_model is built[-1] and e.device_model is not dm
    assert _set_calls(e.device_model) == [('set_accumulation', 4)] and e.device_model.max_batch == 6
    assert e.device_model.get_accumulation()[1:] == (4, 0)
    assert e._build(ds) is None and len(_set_calls(e.device_model)) == 1
    for k in (None, 1):                                                   # without the key, or with 1: no call at all
        plain = engine.TFKerasModel(config(k))
        plain._build(ds)
        monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
        plain.train(ds, max_steps=2, save_freq=100)
        assert _set_calls(plain.device_model) == [] and plain.device_model.iterations == 2
        assert plain._ensure_capacity(6) and _set_calls(plain.device_model) == []


def test_steps_stay_micro_steps_and_iterations_count_cycles(tmp_path, monkeypatch):
    from dnncancerannotator_amd import engine
    install(monkeypatch.setattr)
    monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
    run = str(tmp_path / 'run')
    e = engine.TFKerasModel(config(2, LearningRateScheduler='lambda epoch, current_lr: 0.001 * (epoch + 1)'))
    res = e.train(_data(), save_path=run, max_steps=8, save_freq=4)
    assert res.history['lr'] == [pytest.approx(0.001 * (s + 1)) for s in range(8)]          # the scheduler sees micro-steps
    lines = open(os.path.join(run, 'tfevents', 'train_log.csv')).read().splitlines()
    assert [int(line.split(',')[0]) for line in lines] == list(range(1, 9))
    for step, iterations in ((4, 2), (8, 4)):
        index = json.load(open(os.path.join(run, 'checkpoints', 'ckpt-%d.index' % step)))
        assert index['step'] == step and index['iterations'] == iterations
        assert list(index) == ['format', 'step', 'iterations', 'learning_rate', 'variables']
        with np.load(os.path.join(run, 'checkpoints', 'ckpt-%d.data-00000-of-00001' % step)) as z:
            assert z.files == ['params', 'state', 'adam_m', 'adam_v']                        # the accumulator never enters a checkpoint


@pytest.mark.parametrize('overlay, k, batch', [('accumulate_batch64.yaml', 8, None), ('accumulate_batch28.yaml', 7, 4)])
def test_overlays_merge_over_the_base_config(overlay, k, batch):
    from dnncancerannotator_amd import engine, load
    base = config()
    base['data_options']['train'] = {'batch_size': 8}
    cfg = load._apply_config(base, load.load_config(os.path.join(ROOT, 'configs', 'additionals', overlay)))
    assert cfg['deploy_options'][KEY] == k and cfg['deploy_options']['loss'] == LOSS
    assert cfg['data_options']['train']['batch_size'] == (batch or 8)
    assert engine.TFKerasModel(cfg).accumulation == k


def test_two_ranks_call_the_same_sequence(tmp_path):
    from test_dp_gloo import _spawn
    r, _ = _spawn('dp_accumulate_worker.py', tmp_path)
    r0, r1 = r
    n = r0['n']
    # per cycle: the loss alone, then the accumulator with the loss behind it; one update per cycle
    want = [['set_accumulation', 2]] + [['train', 2], ['allreduce', 1], ['train', 2], ['allreduce', n + 1]] * 2
    assert r0['calls'] == want and r1['calls'] == want
    assert r0['iterations'] == r1['iterations'] == 2
    assert r0['params'] == r1['params'] and r0['loss'] == r1['loss'] and len(r0['loss']) == 4
