"""CPU: the host side of `annotator evaluate --visualize_attribution` -- casewise's arithmetic, CSV text and image on hand-made
arrays, the flag's checks before anything is read, engine.eval on a fake device (tests/fake_attr_device.py: the files, the order
of the calls, what runs without the flag), the C declaration and the build list -- and one property of the oracle itself
(tests/attr_ref.py): the completeness gap of the float64 statement is smaller at 64 path points than at 4."""

import inspect
import os
import re

import numpy as np
import pytest

from dnncancerannotator_amd import casewise as CW
from dnncancerannotator_amd.__main__ import build_parser
from fake_attr_device import attribution_of, fake_engine
from fake_match_device import LabelledSlices
from test_spread_host import EXAMS, IDS, _Pairs, _drawn, _texts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = 'path:/data/p0/exam7/mri,sliceID:3'


# ---- casewise: hand-made -----------------------------------------------------------------------------------------------------------
def test_shares_and_gap():
    absolute = np.array([[1.0, 3.0], [0.0, 0.0], [2.0, 2.0]])
    shares = CW.attribution_shares(absolute)
    assert shares[0].tolist() == [0.25, 0.75] and shares[2].tolist() == [0.5, 0.5] and np.isnan(shares[1]).all()
    signed = np.array([[1.0, -3.0], [0.0, 0.0], [2.0, 2.5]])
    ends = np.array([[5.0, 6.0], [7.0, 7.0], [4.0, 0.0]])
    gap, rel = CW.attribution_gap(signed, ends)
    assert gap.tolist() == [-1.0, 0.0, 0.5] and rel[0] == -1.0 and np.isnan(rel[1]) and rel[2] == 0.125
    one_gap, one_rel = CW.attribution_gap(signed[2], ends[2])          # one slice
    assert float(one_gap) == 0.5 and float(one_rel) == 0.125


def test_csv_text_and_paths():
    text = CW.attribution_csv(['DWI', 'A,DC'], [0.25, 0.75], [1.0, -3.0], [1.0, 3.0], [5.0, 6.0])
    assert text == ('modality,share,signed,absolute\nDWI,0.25,1.0,1.0\n"A,DC",0.75,-3.0,3.0\n'
                    'f_x,5.0\nf_baseline,6.0\ngap,-1.0\nrelative_gap,-1.0\n')
    nan = float('nan')
    text = CW.attribution_csv(['a'], [nan], [0.0], [0.0], [7.0, 7.0])
    assert text.splitlines() == ['modality,share,signed,absolute', 'a,,0.0,0.0', 'f_x,7.0', 'f_baseline,7.0', 'gap,0.0', 'relative_gap,']
    assert CW.attribution_csv(['a'], [1.0], [1e-20], [1e-20], [0.1, 0.0]).splitlines()[1] == 'a,1.0,1e-20,1e-20'
    root = '/out/tag'
    assert CW.attribution_path(root, TAG, 12, 'csv') == '/out/tag/csv/p0/exam7/mri/03/step_00000012_attribution.csv'
    assert CW.attribution_path(root, TAG, 12, 'images') == '/out/tag/images/p0/exam7/mri/03/step_00000012_attribution.png'
    assert os.path.dirname(CW.attribution_path(root, TAG, 12, 'csv')) == os.path.dirname(CW.csv_path(root, TAG, 12))
    with pytest.raises(KeyError):
        CW.attribution_path(root, TAG, 12, 'tfevents')


def test_image_shape_and_colours_of_a_known_map():
    amap = np.zeros((3, 4, 2), np.float32)
    amap[0, 0, 0] = 2.0              # the slice's largest |attr|: full red
    amap[1, 1, 0] = -1.0             # half blue
    amap[2, 3, 1] = -2.0             # full blue, in the second panel
    amap[0, 2, 1] = 0.5              # a quarter red
    img = CW.attribution_image(amap, ['DWI', 'ADC'])
    g = CW.ATTRIBUTION_GAP
    assert img.shape == (3, 2 * 4 + g, 3) and img.dtype == np.uint8
    assert img[0, 0].tolist() == [255, 0, 0] and img[1, 1].tolist() == [128, 128, 255]
    assert img[2, 4 + g + 3].tolist() == [0, 0, 255] and img[0, 4 + g + 2].tolist() == [255, 191, 191]
    white = np.ones(img.shape[:2], bool)
    for y, x in ((0, 0), (1, 1), (2, 4 + g + 3), (0, 4 + g + 2)):
        white[y, x] = False
    assert (img[white] == 255).all()                          # zero attribution and the gap between the panels
    # one common scale: the same value in the other panel has the same colour
    amap[1, 1, 1] = -1.0
    assert CW.attribution_image(amap, ['DWI', 'ADC'])[1, 4 + g + 1].tolist() == [128, 128, 255]
    assert (CW.attribution_image(np.zeros((3, 4, 2)), ['a', 'b']) == 255).all()
    assert (CW.attribution_image(np.full((2, 2, 1), np.nan)) == 255).all()
    with pytest.raises(ValueError):
        CW.attribution_image(amap, ['only one'])
    png = CW.encode_png(img)
    assert png[:8] == b'\x89PNG\r\n\x1a\n'


def test_summary_line():
    shares = np.array([[0.25, 0.75], [np.nan, np.nan], [0.75, 0.25]])
    line = CW.attribution_summary(8, 'mean', shares, [0.5, np.nan, -0.25])
    assert line == [8, 'mean', 3, '0.5', '0.5', '0.375', '0.5']
    assert CW.attribution_summary(4, 'black', np.zeros((0, 2)), []) == [4, 'black', 0, '', '', '', '']


# ---- the flag's checks ------------------------------------------------------------------------------------------------------------
def test_parser_and_signatures():
    from dnncancerannotator_amd import engine
    from dnncancerannotator_amd.runs.evaluate import evaluate
    p = build_parser()
    ev = ['evaluate', '--save_path', 's', '--data_path', 'd', '--tag', 't']
    got = vars(p.parse_args(ev))
    assert not [k for k in got if 'attribution' in k]                # absent unless given
    got = vars(p.parse_args(ev + ['--visualize_attribution', '--attribution_steps', '8', '--attribution_baseline', 'mean']))
    assert got['visualize_attribution'] is True and got['attribution_steps'] == 8 and got['attribution_baseline'] == 'mean'
    with pytest.raises(SystemExit):
        p.parse_args(ev + ['--visualize_attribution', '--attribution_baseline', 'grey'])
    with pytest.raises(SystemExit):
        p.parse_args(['predict', '--save_path', 's', '--data_path', 'd', '--output', 'o', '--visualize_attribution'])
    for fn in (evaluate, engine.TFKerasModel.eval):
        sig = inspect.signature(fn).parameters
        assert sig['visualize_attribution'].default is False and sig['attribution_steps'].default is None
        assert sig['attribution_baseline'].default is None
    assert engine.check_attribution(False, None, None, False, False) is None
    assert engine.check_attribution(True, None, None, True, False) == (CW.ATTRIBUTION_STEPS, 'black') == (32, 'black')
    assert engine.check_attribution(True, '256', 'mean', False, True) == (256, 'mean')


def test_cli_checks_the_flag_before_anything_is_read(monkeypatch, tmp_path):
    import yaml
    from dnncancerannotator_amd import __main__ as cli, engine
    touched, seen = [], []
    monkeypatch.setattr(engine.TFKerasModel, '__init__', lambda self, config: touched.append('init'))
    monkeypatch.setattr(engine.TFKerasModel, 'load', lambda self, path: touched.append('load'))
    monkeypatch.setattr(engine.TFKerasModel, 'eval', lambda self, dataset, **kw: seen.append(kw) or {})
    save = tmp_path / 'run'
    save.mkdir()                                     # no options.yaml yet: reading it first would raise another error
    ev = ['evaluate', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--tag', 't']
    with pytest.raises(ValueError, match='--visualize_attribution'):
        cli.main(ev + ['--visualize_attribution'])                                       # neither --export_csv nor --export_images
    for steps in ('0', '257', '-3'):
        with pytest.raises(ValueError, match='--attribution_steps'):
            cli.main(ev + ['--export_csv', '--visualize_attribution', '--attribution_steps', steps])
    with pytest.raises(ValueError, match='--visualize_attribution'):
        cli.main(ev + ['--export_csv', '--attribution_steps', '8'])                      # the option without the flag
    assert touched == [] and seen == []
    monkeypatch.undo()
    monkeypatch.setattr(engine.TFKerasModel, '__init__', lambda self, config: None)
    monkeypatch.setattr(engine.TFKerasModel, 'eval', lambda self, dataset, **kw: seen.append(kw) or {})
    (save / 'options.yaml').write_text(yaml.safe_dump({'config': {'data_options': {'eval': {'batch_size': 2}}}}))
    assert cli.main(ev + ['--export_images', '--visualize_attribution']) == 0
    assert cli.main(ev + ['--export_csv', '--visualize_attribution', '--attribution_steps', '8', '--attribution_baseline', 'mean',
                          '--visualize_sensitivity']) == 0
    assert cli.main(ev + ['--export_csv']) == 0
    assert (seen[0]['visualize_attribution'], seen[0]['attribution_steps'], seen[0]['attribution_baseline']) == (True, 32, 'black')
    assert (seen[1]['visualize_attribution'], seen[1]['attribution_steps'], seen[1]['attribution_baseline']) == (True, 8, 'mean')
    assert seen[1]['visualize_sensitivity'] is True and seen[0]['viz_ds'] is not None
    assert not [k for k in seen[2] if 'attribution' in k]            # without the flag engine.eval gets no new keyword


# ---- engine.eval on the fake device -----------------------------------------------------------------------------------------------
def _engine(tmp_path, monkeypatch, batch=4, max_batch=3):
    prob, y = _drawn()
    e = fake_engine(monkeypatch, max_batch)
    ds = LabelledSlices(prob, y, EXAMS, IDS, batch)
    e._build(ds)
    e.current_step = 1
    run = str(tmp_path / 'run')
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    e.metrics = []
    return e, ds, run, prob


def test_evaluate_writes_the_attribution_files_and_nothing_else_changes(tmp_path, monkeypatch):
    e, ds, run, prob = _engine(tmp_path, monkeypatch)
    e.eval(_Pairs(ds), run, viz_ds=ds, tag='p', export_csv=True, export_images=True)
    plain_calls = list(e.device_model.calls)
    e.device_model.calls.clear()
    e.eval(_Pairs(ds), run, viz_ds=ds, tag='a', export_csv=True, export_images=True, visualize_attribution=True, attribution_steps=4,
           attribution_baseline='mean')
    calls = e.device_model.calls
    own = [c for c in calls if c[0] == 'integrated_gradients']
    assert own == [('integrated_gradients', n, 4, 'mean', True) for n in (3, 1, 3)]          # batches of 4 on a model of 3
    assert [c for c in calls if c[0] != 'integrated_gradients'] == plain_calls
    # ... each on the slices its forward left, behind the composite
    names = [c[0] for c in calls]
    assert all(names[i - 1] == 'render_composite' for i, n in enumerate(names) if n == 'integrated_gradients')
    plain, with_flag = _texts(os.path.join(run, 'tfevents', 'p')), _texts(os.path.join(run, 'tfevents', 'a'))
    new = sorted(set(with_flag) - set(plain))
    assert all(with_flag[k] == v for k, v in plain.items())                                   # byte for byte what it was
    assert len(new) == 2 * 7 + 1 and 'attribution_results.csv' in new
    assert not [k for k in plain if 'attribution' in k]
    root = os.path.join(run, 'tfevents', 'a')
    want = attribution_of(prob, 4, 'mean', True)
    shares = CW.attribution_shares(want.absolute)
    for b, (exam, k) in enumerate(zip(EXAMS, IDS)):
        tag = CW.tag_of(exam, k)
        text = with_flag[os.path.relpath(CW.attribution_path(root, tag, 1, 'csv'), root)].decode()
        assert text == CW.attribution_csv(['ch0', 'ch1'], shares[b], want.signed[b], want.absolute[b], want.endpoints[b])
        png = with_flag[os.path.relpath(CW.attribution_path(root, tag, 1, 'images'), root)]
        assert png == CW.encode_png(CW.attribution_image(want.map[b], ['ch0', 'ch1']))
    rel = CW.attribution_gap(want.signed, want.endpoints)[1]
    assert with_flag['attribution_results.csv'].decode().splitlines() == [
        'step,steps,baseline,slices,share_ch0,share_ch1,mean_relative_gap,max_relative_gap',
        ','.join(str(v) for v in [1] + CW.attribution_summary(4, 'mean', shares, rel))]
    assert np.isnan(shares[6]).all() and with_flag['attribution_results.csv'].decode().splitlines()[1].startswith('1,4,mean,7,')


def test_the_map_leaves_the_device_only_for_images_and_the_sensitivity_runs_beside_it(tmp_path, monkeypatch):
    e, ds, run, prob = _engine(tmp_path, monkeypatch)
    e.eval(_Pairs(ds), run, viz_ds=ds, tag='c', export_csv=True, visualize_attribution=True, visualize_sensitivity=True, tta='flips')
    calls = e.device_model.calls
    assert [c for c in calls if c[0] == 'integrated_gradients'] == [('integrated_gradients', n, 32, 'black', False) for n in (3, 1, 3)]
    names = [c[0] for c in calls]
    assert names.count('input_sensitivity') == 3 and 'forward_tta' in names
    files = _texts(os.path.join(run, 'tfevents', 'c'))
    assert len([k for k in files if k.endswith('_attribution.csv')]) == 7 and not [k for k in files if k.endswith('.png')]
    # no Visualizer, no attribution: a rank other than 0, --skip_visualization
    e.device_model.calls.clear()
    e.eval(_Pairs(ds), run, viz_ds=None, tag='n', export_csv=True, visualize_attribution=True)
    assert not [c for c in e.device_model.calls if c[0] == 'integrated_gradients']
    assert 'attribution_results.csv' not in _texts(os.path.join(run, 'tfevents', 'n'))


def test_bad_arguments_are_refused_before_anything_is_read(tmp_path, monkeypatch):
    from dnncancerannotator_amd import engine
    e, ds, run, prob = _engine(tmp_path, monkeypatch)
    touched = []
    monkeypatch.setattr(engine.TFKerasModel, 'load', lambda self, path: touched.append(path))
    monkeypatch.setattr(engine.TFKerasModel, 'get_ckpts', lambda self, path: touched.append(path) or {})
    for kw in (dict(), dict(export_csv=True, attribution_steps=0), dict(export_csv=True, attribution_steps=257),
               dict(export_images=True, attribution_baseline='grey')):
        with pytest.raises(ValueError, match='--visualize_attribution|--attribution_'):
            e.eval(_Pairs(ds), run, viz_ds=ds, tag='t', visualize_attribution=True, **kw)
    assert touched == [] and e.device_model.calls == []
    e.model.supports_sensitivity = False                          # MultiResUnet
    with pytest.raises(NotImplementedError, match='--visualize_attribution'):
        e.eval(_Pairs(ds), run, viz_ds=ds, tag='t', export_csv=True, visualize_attribution=True)
    assert touched == []


# ---- the library's surface, read from the sources -----------------------------------------------------------------------------------
def test_header_build_list_and_binding_name_the_pass():
    from dnncancerannotator_amd import build, device
    header = open(os.path.join(ROOT, 'include', 'dnnca.h')).read()
    decl = re.search(r'int dnnca_integrated_gradients\((.*?)\);', header, re.S).group(1)
    decl = re.sub(r'/\*.*?\*/', '', decl, flags=re.S)
    assert [' '.join(a.split()) for a in decl.split(',')] == [
        'void* model', 'const float* x_nhwc', 'int batch', 'int steps', 'int baseline', 'double* signed_sums', 'double* abs_sums',
        'double* endpoints', 'float* map']
    assert 'DNNCA_PLAN_ATTRIBUTION = 8' in header
    assert 'kernels_attr.hip' in build.SOURCES
    assert device.DeviceModel.PLAN_PASSES['attribution'] == 8 and device.DeviceModel.PLAN_PASSES['sensitivity'] == 3
    sig = inspect.signature(device.DeviceModel.integrated_gradients).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [('x', None), ('batch', None), ('steps', 32), ('baseline', 'black'),
                                                            ('return_map', False)]
    assert device.Attribution._fields == ('signed', 'absolute', 'endpoints', 'map')
    # nothing of the pass is named ig_*: that prefix is the implicit-GEMM code's
    src = open(os.path.join(ROOT, 'dnncancerannotator_amd', 'csrc', 'kernels_attr.hip')).read()
    assert not re.search(r'\b[gk]?_?ig_', src) and 'atomic' not in src.replace('No atomics', '').replace('an atomic', '')


# ---- the oracle's own property ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['a', 'b', 'd', 'e'])
def test_oracle_gap_shrinks_from_4_to_64_path_points(name):
    """completeness: the attributions sum to F(x) - F(baseline) up to the quadrature's error.  That error is not monotonic from one
    step count to the next, so only |gap(64)| < |gap(4)| is asserted, for every slice and both baselines (float64 statement)"""
    import attr_cases as AC
    import attr_ref
    spec, kw, params = AC.spec_of(name)
    x = AC.input_of(name, AC.PANEL[0])
    for baseline in attr_ref.BASELINES:
        gaps = {}
        for m in (4, 64):
            signed, absolute, ends, amap = attr_ref.integrated_gradients(spec, params, x, m, baseline)
            gaps[m] = np.abs(attr_ref.gap(signed, ends))
            assert np.allclose(signed, amap.sum((1, 2))) and (absolute >= np.abs(signed)).all()
        print('case %s %-5s |gap| at m = 4: %s  at m = 64: %s' % (name, baseline, gaps[4], gaps[64]))
        assert (gaps[64] < gaps[4]).all(), (name, baseline, gaps)
