"""CPU: bench.py's control flow with a counting stand-in for the device model (no kernels run).  A plain run does exactly
--warmup + settle + --steps train steps and prints the headline fields alone; --full adds the rest; the last step of every timed
region starts from the initial model; --dump-outputs writes the state right after the last timed step, within its size bound.
What the numbers mean is test_engine_gpu.py's subject."""

import json
import sys

import numpy as np
import pytest

import bench


class _StepOut:
    def __init__(self, steps):
        self.loss, self.positive_rate, self.weight, self.label_min, self.label_max = float(steps), 0.25, 3.0, 0.0, 1.0


class CountingModel:
    """DeviceModel's surface as bench.py uses it; `loss` of the step outputs is the Adam step count (train steps since the last
    set_opt_state)."""
    made = []

    def __init__(self, arch, C, H, W, B, force_generic=False, dtype='f32', **opts):
        self.n_trainable = 3 * bench.DUMP_MAX_ELEMS if opts['n_filters_first'] == 64 else 1000
        self.steps, self.iterations, self.restarts = 0, 0, 0
        self.params = np.arange(self.n_trainable, dtype=np.float32)
        CountingModel.made.append(self)

    def init_glorot(self, seed=None):
        pass

    def loss_cfg(self, **kw):
        return kw

    def train_step_dev(self, xb, yb, batch, lr, cfg):
        self.steps += 1
        self.iterations += 1
        self.params = self.params + 1

    def sync(self):
        pass

    def last_step_out(self):
        return _StepOut(self.iterations)

    def get_params(self):
        return self.params.copy()

    def set_params(self, flat):
        self.params = np.array(flat, np.float32)

    def get_grads(self):
        return np.full(self.n_trainable, 0.5, np.float32)

    def get_state(self):
        return np.zeros(0, np.float32)

    def set_state(self, flat):
        assert len(flat) == 0

    def get_opt_state(self):
        return np.zeros(self.n_trainable, np.float32), np.ones(self.n_trainable, np.float32), self.iterations

    def set_opt_state(self, m, v, iterations):
        assert not np.any(m) and not np.any(v)
        self.iterations = iterations
        self.restarts += 1

    def profile_reset(self):
        pass

    def profile_enable(self, mode=1, focus=None, period=1):
        pass

    def profile(self):
        return [('k_big', 10, 1.0, 1e8, 1e9), ('k_small', 5, 0.5, 1e6, 1e6)]

    def timer_start(self):
        pass

    def timer_stop(self):
        return 1.0

    def staging(self):
        class Ring:
            slots = 2

            def upload(self, slot, x, y, wait=True):
                return 0, 0

            def train_step(self, *a):
                pass

            def out(self, slot):
                pass
        return Ring()

    def close(self):
        pass


@pytest.fixture
def run_bench(monkeypatch, capsys):
    monkeypatch.setattr(bench.dev, 'DeviceModel', CountingModel)
    monkeypatch.setattr(bench.dev, 'DeviceBuffer', lambda a: a)
    monkeypatch.setattr(bench.dev, 'init_device', lambda ordinal: None)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'DNNCA_FORCE_COMM'):
        monkeypatch.delenv(k, raising=False)

    def run(*args):
        del CountingModel.made[:]
        monkeypatch.setattr(sys, 'argv', ['bench.py'] + [str(a) for a in args])
        bench.main()
        return json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return run


def test_plain_run_times_exactly_the_given_steps(run_bench, tmp_path):
    line = run_bench('--gpus', 1, '--steps', 7, '--warmup', 3, '--dump-outputs', tmp_path / 'd')
    settle = line['settle_steps']
    assert settle >= bench.SETTLE_MIN_STEPS
    assert [m.steps for m in CountingModel.made] == [3 + settle + 7]          # one model, no other leg, no extra steps
    assert CountingModel.made[0].restarts == 1
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in line, k
    assert line['steps'] == 7 and line['warmup'] == 3
    for k in ('repeats', 'region_ms', 'roofline', 'roofline_all', 'roofline_step', 'hip_event_ms_per_step', 'from_host_memory',
              'other_workloads', 'cpu_baseline'):
        assert k not in line, k
    d = tmp_path / 'd'
    assert float(np.load(d / 'loss.npy')[0]) == 1                             # one step from the initial model
    assert not (d / 'state.npy').exists()                                       # empty vectors are skipped
    for name in ('params', 'grads', 'adam_m', 'adam_v'):
        a = np.load(d / (name + '.npy'))
        assert a.dtype == np.float32 and a.shape == (1000,)
    np.testing.assert_array_equal(np.load(d / 'params.npy'), np.arange(1000, dtype=np.float32) + 1)


def test_full_run_keeps_every_figure(run_bench, tmp_path):
    line = run_bench('--steps', 4, '--warmup', 2, '--full', '--no-cpu-baseline', '--dump-outputs', tmp_path / 'd')
    for k in ('repeats', 'region_ms', 'roofline', 'roofline_all', 'roofline_step', 'hip_event_ms_per_step', 'from_host_memory',
              'other_workloads'):
        assert k in line, k
    assert line['repeats'] == 3 and len(line['region_ms']) == 3 and 'cpu_baseline' not in line
    assert sorted(line['other_workloads']) == ['mulmo_unet', 'unet_big']
    # the last step of every region starts from the initial model; the dump is the same step as a plain run's
    assert CountingModel.made[0].restarts == 3
    assert CountingModel.made[0].steps == 2 + bench.PROF_STEPS + line['settle_steps'] + 3 * 4
    assert float(np.load(tmp_path / 'd' / 'loss.npy')[0]) == 1
    np.testing.assert_array_equal(np.load(tmp_path / 'd' / 'params.npy'), np.arange(1000, dtype=np.float32) + 1)


@pytest.mark.parametrize('steps', [1, 2])
def test_short_regions_restart_once(run_bench, steps):
    run_bench('--steps', steps, '--warmup', 1)
    assert CountingModel.made[0].restarts == 1 and CountingModel.made[0].iterations == 1


def test_dump_of_a_large_model_is_a_fixed_sample(run_bench, tmp_path):
    for tag in ('a', 'b'):
        run_bench('--workload', 'unet_big', '--steps', 2, '--warmup', 1, '--dump-outputs', tmp_path / tag)
    total = sum(p.stat().st_size for p in (tmp_path / 'a').iterdir())
    assert total <= 64 << 20
    a, b = np.load(tmp_path / 'a' / 'params.npy'), np.load(tmp_path / 'b' / 'params.npy')
    assert a.shape == (bench.DUMP_MAX_ELEMS,) and (np.diff(a) > 0).all()      # sorted positions of arange + 1: distinct, in order
    np.testing.assert_array_equal(a, b)
