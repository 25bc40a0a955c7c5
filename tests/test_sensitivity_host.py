"""CPU: the host side of `annotator evaluate --visualize_sensitivity` (dnncancerannotator_amd/casewise.py): the CSV bytes of
pandas.Series.to_csv, file names, modality names, the bar chart, and the flag's way from the command line to engine.eval."""

import io
import os
import struct
import zlib

import numpy as np
import pytest

from dnncancerannotator_amd import casewise as CW

TAG = 'path:/data/p0/exam7/mri,sliceID:3'


@pytest.mark.parametrize('n', [1, 3, 5])
def test_sensitivity_csv_is_pandas_text(n):
    pd = pytest.importorskip('pandas')
    rng = np.random.default_rng(n)
    names = ['TRA', 'ADC', 'DWI', 'DCEE', 'DCEL'][:n]
    raw = rng.random((3, n)) * np.array([1e-7, 1.0, 3e4])[:, None]
    raw[1] = 0.0                                            # an all-zero slice: 0 / 0
    sens = CW.normalise_sensitivity(raw)
    assert np.isnan(sens[1]).all() and np.allclose(sens[[0, 2]].sum(1), 1.0)
    for row in sens:
        assert CW.sensitivity_csv(names, row) == pd.Series(row, index=names).to_csv()
    assert CW.sensitivity_csv(names, sens[0]).splitlines()[0] == ',0'
    # a name the csv module has to quote, a value with an exponent
    assert CW.sensitivity_csv(['a,b'], [1e-20]) == pd.Series([1e-20], index=['a,b']).to_csv()


def test_sensitivity_paths():
    root = '/out/tag'
    assert CW.sensitivity_path(root, TAG, 12, 'csv') == '/out/tag/csv/p0/exam7/mri/03/step_00000012_sensitivity.csv'
    assert CW.sensitivity_path(root, TAG, 12, 'images') == '/out/tag/images/p0/exam7/mri/03/step_00000012_sensitivity.png'
    assert os.path.dirname(CW.sensitivity_path(root, TAG, 12, 'csv')) == os.path.dirname(CW.csv_path(root, TAG, 12))
    assert os.path.dirname(CW.sensitivity_path(root, TAG, 12, 'images')) == os.path.dirname(CW.image_path(root, TAG, 12))
    with pytest.raises(KeyError):
        CW.sensitivity_path(root, TAG, 12, 'tfevents')


def test_modality_names():
    assert CW.modality_names(['TRA', 'ADC', 'label', 'DWI'], 3) == ['TRA', 'ADC', 'DWI']
    assert CW.modality_names(None, 3) == ['ch0', 'ch1', 'ch2']
    assert CW.modality_names([], 1) == ['ch0']
    assert CW.modality_names(['TRA', 'label'], 2) == ['ch0', 'ch1']          # names that do not match the model's channels


def _decode_png(data):
    """8-bit RGB PNG, filter 0 rows (what encode_png writes), with zlib alone"""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, shape = 8, b'', None
    while pos < len(data):
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        if kind == b'IHDR':
            w, h, depth, colour = struct.unpack('>IIBB', body[:10])
            assert (depth, colour) == (8, 2)
            shape = (h, w)
        elif kind == b'IDAT':
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(shape[0], 1 + 3 * shape[1])
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(shape[0], shape[1], 3)


@pytest.mark.parametrize('values', [[1.0], [0.5, 0.25, 0.25], [0.0, 0.013, 0.987, 0.0, 0.0], [float('nan')] * 3])
def test_chart_png_decodes_to_the_bar_heights(values):
    png = CW.encode_png(CW.sensitivity_chart(values))
    img = _decode_png(png)
    try:
        from PIL import Image
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(png)).convert('RGB')), img)
    except ImportError:
        pass
    n = len(values)
    assert img.shape == (CW.CHART_PLOT_H + 2 * CW.CHART_MARGIN + 2, n * CW.CHART_SLOT + 2 * CW.CHART_MARGIN + 2, 3)
    bar = (img == np.array(CW.CHART_BAR_RGB, np.uint8)).all(-1)
    bottom = CW.CHART_MARGIN + CW.CHART_PLOT_H + 1          # the frame's bottom line: y = 0
    cols = CW.chart_bar_columns(n)
    assert len(cols) == n and all(b[0] >= a[1] for a, b in zip(cols, cols[1:]))
    covered = np.zeros(img.shape[1], bool)
    for (x0, x1), v in zip(cols, values):
        want = 0 if v != v else int(round(v * CW.CHART_PLOT_H))
        heights = bar[:, x0:x1].sum(0)
        assert (heights == want).all(), (v, heights)
        if want:                                            # the bar stands on y = 0 and is solid
            assert bar[bottom - want:bottom, x0:x1].all()
        covered[x0:x1] = True
    assert not bar[:, ~covered].any()
    # y = 1 is the frame's top line: a bar of 1.0 reaches it and no higher
    assert (img[CW.CHART_MARGIN, CW.CHART_MARGIN:-CW.CHART_MARGIN] == 0).all() and (img[bottom, CW.CHART_MARGIN:-CW.CHART_MARGIN] == 0).all()
    assert (img[:CW.CHART_MARGIN] == 255).all()


def test_chart_clips_to_the_y_range():
    assert CW.chart_bar_height(1.7) == CW.CHART_PLOT_H and CW.chart_bar_height(-0.2) == 0 and CW.chart_bar_height(float('nan')) == 0


def test_cli_flag_reaches_engine_eval(monkeypatch, tmp_path):
    """`annotator evaluate --visualize_sensitivity` -> runs.evaluate -> TFKerasModel.eval(visualize_sensitivity=True)"""
    import yaml
    from dnncancerannotator_amd import __main__ as cli, engine
    seen = []

    def fake_eval(self, dataset, **kw):
        seen.append(kw)
        return {}
    monkeypatch.setattr(engine.TFKerasModel, 'eval', fake_eval)
    monkeypatch.setattr(engine.TFKerasModel, '__init__', lambda self, config: None)
    save = tmp_path / 'run'
    save.mkdir()
    (save / 'options.yaml').write_text(yaml.safe_dump({'config': {'data_options': {'eval': {'batch_size': 2}}}}))
    base = ['evaluate', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--tag', 't']
    for extra, want in ((['--visualize_sensitivity'], True), ([], False)):
        assert cli.main(base + extra) == 0
        assert seen[-1]['visualize_sensitivity'] is want
    assert seen[0]['viz_ds'] is not None


def test_engine_eval_no_longer_warns_that_the_flag_is_ignored():
    import inspect
    from dnncancerannotator_amd import engine
    assert 'ignored' not in inspect.getsource(engine.TFKerasModel.eval)
