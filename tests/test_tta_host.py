"""CPU: the host side of test-time augmentation (`predict --tta`, `evaluate --tta`).  The numpy oracle of the views
(tests/tta_oracle.py) against the written formula and numpy's own flips; tta.mask_of; engine.annotate and engine.eval on a fake device
that records its forwards (tests/fake_tta_device.py); the command line."""

import inspect
import os

import numpy as np
import pytest

import tta_oracle as TO
from dnncancerannotator_amd import tta
from dnncancerannotator_amd.__main__ import build_parser
from fake_link_device import Slices
from fake_match_device import LabelledSlices
from fake_tta_device import fake_engine


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def test_invert_undoes_apply_for_all_eight_views():
    p = np.arange(3 * 4 * 4, dtype=np.float32).reshape(3, 4, 4)           # distinct values
    seen = set()
    for k in range(8):
        v = TO.apply_view(p[..., None], k)[..., 0]
        assert np.array_equal(TO.invert_view(v, k), p)
        seen.add(v.tobytes())
    assert len(seen) == 8                                                   # eight different views


def _by_formula(x, k):
    """section by section what include/dnnca.h writes: the flips, then the transpose"""
    t, v, h = k >> 2 & 1, k >> 1 & 1, k & 1
    B, H, W, C = x.shape
    xf = np.empty_like(x)
    for i in range(H):
        for j in range(W):
            xf[:, i, j] = x[:, H - 1 - i if v else i, W - 1 - j if h else j]
    if not t:
        return xf
    xk = np.empty((B, W, H, C), x.dtype)
    for i in range(W):
        for j in range(H):
            xk[:, i, j] = xf[:, j, i]
    return xk


def test_formula_agrees_with_numpy_flips():
    x = np.arange(2 * 3 * 5, dtype=np.float32).reshape(2, 3, 5, 1)
    for k in range(4):
        want = x
        if k & 2:
            want = np.flip(want, 1)
        if k & 1:
            want = np.flip(want, 2)
        assert np.array_equal(_by_formula(x, k), want) and np.array_equal(TO.apply_view(x, k), want)
    sq = np.arange(2 * 4 * 4 * 2, dtype=np.float32).reshape(2, 4, 4, 2)
    for k in range(4, 8):                                                   # the transposed ones on a square
        assert np.array_equal(TO.apply_view(sq, k), _by_formula(sq, k))
        assert np.array_equal(TO.apply_view(sq, k), np.swapaxes(TO.apply_view(sq, k - 4), 1, 2))


def test_mean_of_sums_in_float32_in_ascending_order():
    rng = np.random.default_rng(5)
    planes = rng.random((3, 2, 4, 4)).astype(np.float32)
    got = TO.mean_of(planes, 0x07)
    back = [TO.invert_view(planes[i], k) for i, k in enumerate((0, 1, 2))]
    want = ((back[0] + back[1]).astype(np.float32) + back[2]).astype(np.float32) / np.float32(3)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(TO.mean_of(planes[:1], 0x20), TO.invert_view(planes[0], 5))
    assert TO.views_of(0xB4) == [2, 4, 5, 7]


# ---- the modes -------------------------------------------------------------------------------------------------------------------
def test_mask_of():
    assert tta.MODES == ('none', 'flips', 'd4')
    assert tta.mask_of('none', 16, 32) is None and tta.mask_of('none', 16, 16) is None
    assert tta.mask_of('flips', 16, 32) == 0x0F and tta.mask_of('flips', 16, 16) == 0x0F
    assert tta.mask_of('d4', 16, 16) == 0xFF
    with pytest.raises(ValueError, match='flips'):
        tta.mask_of('d4', 16, 32)
    with pytest.raises(ValueError, match='unknown mode'):
        tta.mask_of('rot90', 16, 16)


# ---- annotate on the fake device -------------------------------------------------------------------------------------------------
def _drawn():
    """7 slices of 12 x 12 of exams a (4 slices) and b (3), as tests/test_surface_host.py draws them"""
    prob, y = np.zeros((7, 12, 12), np.float32), np.zeros((7, 12, 12), np.float32)
    y[0:6, 2:6, 2:6] = 1.0
    prob[0:5, 3:7, 2:6] = 0.75
    prob[2:4, 9:11, 1:4] = 0.55
    return prob, y


def _texts(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            with open(os.path.join(d, f), 'rb') as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def _forwards(e):
    return [c for c in e.device_model.calls if c[0] in ('forward', 'forward_tta')]


def _annotate_setup(tmp_path, monkeypatch):
    prob, _ = _drawn()
    e = fake_engine(monkeypatch, 3)
    ds = Slices(prob, ['a'] * 4 + ['b'] * 3, [0, 1, 2, 3, 0, 1, 2], 4)
    e._build(ds)
    e.current_step = 1
    run = str(tmp_path / 'run')
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    return e, ds, run


def test_annotate_flips_calls_forward_tta_once_per_chunk(tmp_path, monkeypatch):
    e, ds, run = _annotate_setup(tmp_path, monkeypatch)
    res = e.annotate(ds, run, str(tmp_path / 'tta'), filter_size=1, export_images=True, tta='flips')
    # data set batches of 4 and 3 on a device of 3 slices per call: chunks of 3, 1, 3
    assert _forwards(e) == [('forward_tta', 3, 0x0F), ('forward_tta', 1, 0x0F), ('forward_tta', 3, 0x0F)]
    assert res['slices'] == 7
    # the fake network is the identity on channel 0, and four equal values average to themselves: the files are the plain ones
    e.device_model.calls.clear()
    e.annotate(ds, run, str(tmp_path / 'plain'), filter_size=1, export_images=True)
    assert _texts(str(tmp_path / 'tta')) == _texts(str(tmp_path / 'plain'))
    e.device_model.calls.clear()
    e.annotate(ds, run, str(tmp_path / 'd4'), filter_size=1, tta='d4', link_slices=True)
    assert _forwards(e) == [('forward_tta', 3, 0xFF), ('forward_tta', 1, 0xFF), ('forward_tta', 3, 0xFF)]


def test_annotate_without_a_mode_calls_only_forward(tmp_path, monkeypatch):
    e, ds, run = _annotate_setup(tmp_path, monkeypatch)
    e.annotate(ds, run, str(tmp_path / 'a'), filter_size=1, export_images=True)
    first = _forwards(e)
    e.device_model.calls.clear()
    e.annotate(ds, run, str(tmp_path / 'b'), filter_size=1, export_images=True, tta='none')
    assert first == _forwards(e) == [('forward', 3), ('forward', 1), ('forward', 3)]
    a, b = _texts(str(tmp_path / 'a')), _texts(str(tmp_path / 'b'))
    assert a == b and 'lesions.csv' in a and len(a) == 2 + 7
    with pytest.raises(ValueError, match='unknown mode'):
        e.annotate(ds, run, str(tmp_path / 'c'), tta='rot90')


# ---- eval on the fake device -----------------------------------------------------------------------------------------------------
class _Probe:
    """a pixel metric that notes which device call came last before it read the probabilities"""
    name = 'probe'

    def reset_state(self):
        self.seen = []

    def update_state(self, dm, y):
        self.seen.append(dm.calls[-1][0])

    def result(self):
        return 0.0


class _Pairs:
    """the (x, y) batches of a LabelledSlices: what the evaluation itself reads"""

    def __init__(self, ds):
        self.ds, self.element_spec = ds, ds.element_spec

    def __iter__(self):
        for x, y, _, _ in self.ds:
            yield x, y


def test_eval_flips_uses_forward_tta_everywhere_and_not_the_ring(tmp_path, monkeypatch, caplog):
    from dnncancerannotator_amd import engine
    prob, y = _drawn()
    e = fake_engine(monkeypatch, 3)
    ds = LabelledSlices(prob, y, ['a'] * 4 + ['b'] * 3, [0, 1, 2, 3, 0, 1, 2], 4)
    e._build(ds)
    e.current_step = 1
    run = str(tmp_path / 'run')
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    probe = _Probe()
    e.metrics = [probe]
    staged = []
    monkeypatch.setattr(engine.TFKerasModel, '_staged_eval_possible', lambda self: True)
    monkeypatch.setattr(engine.TFKerasModel, '_evaluate_staged',
                        lambda self, dataset, cfg_kw, shard, region_groups=(): staged.append(1) or (0.0, 0, []))
    kw = dict(exam_ds=ds, exam_lesions=True, exam_filter_size=1, surface_ds=ds, surface_distances=True, surface_filter_size=1)
    with caplog.at_level('INFO'):
        rows = e.eval(_Pairs(ds), run, tag='t', export_csv=True, tta='flips', **kw)
    assert not staged and [r.getMessage() for r in caplog.records if '--tta flips' in r.getMessage()]
    calls = [c for c in e.device_model.calls if c[0] in ('eval', 'forward', 'forward_tta')]
    # the per-batch step: batches of 4 and 3 in chunks of 3, 1, 3, each a test step and then the augmented forward ...
    step = [('eval', 3), ('forward_tta', 3, 0x0F), ('eval', 1), ('forward_tta', 1, 0x0F), ('eval', 3), ('forward_tta', 3, 0x0F)]
    # ... then the exam-lesion pass and the surface pass, one augmented forward per chunk each
    assert calls == step + [('forward_tta', 3, 0x0F), ('forward_tta', 1, 0x0F), ('forward_tta', 3, 0x0F)] * 2
    assert probe.seen == ['forward_tta'] * 3                               # the metrics read behind it
    assert list(rows) == [1] and 'loss' in rows[1]
    with_tta = _texts(os.path.join(run, 'tfevents', 't'))
    # without a mode: the staged path is taken, every pass uses the plain forward, and the files are the same (identity network)
    e.device_model.calls.clear()
    monkeypatch.setattr(engine.TFKerasModel, '_evaluate_staged',
                        lambda self, dataset, cfg_kw, shard, region_groups=(): staged.append(1) or (0.0, 0, dataset))
    e.eval(_Pairs(ds), run, tag='u', export_csv=True, **kw)
    assert staged == [1] and not [c for c in e.device_model.calls if c[0] == 'forward_tta']
    assert [c for c in e.device_model.calls if c[0] == 'forward'] == [('forward', 3), ('forward', 1), ('forward', 3)] * 2
    plain = _texts(os.path.join(run, 'tfevents', 'u'))
    assert sorted(plain) == sorted(with_tta) and all(plain[k] == with_tta[k] for k in plain if k != 'results.csv')
    with pytest.raises(ValueError, match='flips'):
        e.eval(LabelledSlices(np.zeros((2, 16, 32), np.float32), np.zeros((2, 16, 32), np.float32), ['a'] * 2, [0, 1], 2), run, tag='v',
               tta='d4')


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_and_signatures():
    from dnncancerannotator_amd import engine
    from dnncancerannotator_amd.runs.evaluate import evaluate
    from dnncancerannotator_amd.runs.predict import predict
    p = build_parser()
    for base, fn, method in ((['predict', '--save_path', 's', '--data_path', 'd', '--output', 'o'], predict, engine.TFKerasModel.annotate),
                             (['evaluate', '--save_path', 's', '--data_path', 'd', '--tag', 't'], evaluate, engine.TFKerasModel.eval)):
        assert 'tta' not in vars(p.parse_args(base))                        # the default is that of the run function
        assert inspect.signature(fn).parameters['tta'].default == 'none'
        assert inspect.signature(method).parameters['tta'].default == 'none'
        for mode in tta.MODES:
            assert vars(p.parse_args(base + ['--tta', mode]))['tta'] == mode
        with pytest.raises(SystemExit):
            p.parse_args(base + ['--tta', 'rot90'])


def test_run_functions_forward_the_mode_only_when_given(monkeypatch, tmp_path):
    import yaml
    from dnncancerannotator_amd import __main__ as cli, engine
    seen = []
    monkeypatch.setattr(engine.TFKerasModel, 'eval', lambda self, dataset, **kw: seen.append(kw) or {})
    monkeypatch.setattr(engine.TFKerasModel, 'annotate', lambda self, dataset, **kw: seen.append(kw) or {})
    monkeypatch.setattr(engine.TFKerasModel, '__init__', lambda self, config: None)
    save = tmp_path / 'run'
    save.mkdir()
    (save / 'options.yaml').write_text(yaml.safe_dump({'config': {'data_options': {'eval': {'batch_size': 2}}}}))
    ev = ['evaluate', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--tag', 't', '--skip_visualization']
    pr = ['predict', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--output', str(tmp_path / 'o')]
    for base in (ev, pr):
        assert cli.main(base) == 0 and cli.main(base + ['--tta', 'none']) == 0 and cli.main(base + ['--tta', 'flips']) == 0
    assert ['tta' in kw for kw in seen] == [False, False, True] * 2 and seen[2]['tta'] == seen[5]['tta'] == 'flips'
    assert seen[0] == seen[1] and {k: v for k, v in seen[4].items() if k != 'dataset'} == {k: v for k, v in seen[3].items() if k != 'dataset'}


def test_predict_d4_on_non_square_slices_ends_before_any_checkpoint(monkeypatch, tmp_path):
    import yaml
    from dnncancerannotator_amd import __main__ as cli, engine
    touched = []
    monkeypatch.setattr(engine.TFKerasModel, 'load', lambda self, path: touched.append(('load', path)))
    monkeypatch.setattr(engine.TFKerasModel, 'get_ckpts', lambda self, path: touched.append(('get_ckpts', path)) or {})
    monkeypatch.setattr(engine.TFKerasModel, '_build', lambda self, dataset, *a, **k: touched.append(('build',)))
    cfg = {'model': 'UNetAnnotator', 'data_options': {'eval': {'batch_size': 2}},
           'model_options': dict(n_filters_first=2, n_downsample=1, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same'),
           'deploy_options': {'optimizer': 'adam', 'enable_multigpu': False}}
    save = tmp_path / 'run'
    save.mkdir()
    (save / 'options.yaml').write_text(yaml.safe_dump({'config': cfg}))
    base = ['predict', '--save_path', str(save), '--output', str(tmp_path / 'o'), '--tta', 'd4', '--data_path']
    with pytest.raises(ValueError, match='flips'):
        cli.main(base + ['synthetic:16x32x2'])
    assert touched == []
    with pytest.raises(ValueError, match='no checkpoint'):                   # square slices get as far as the checkpoints
        cli.main(base + ['synthetic:16x16x2'])
    assert [t[0] for t in touched] == ['build', 'get_ckpts']
