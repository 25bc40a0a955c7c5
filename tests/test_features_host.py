"""CPU tests of `predict --lesion_features`: the arithmetic of casewise on hand-made records, tests/features_oracle.py on hand-counted
drawings, engine.annotate on a fake device that keeps its staged batch (tests/fake_features_device.py), and the command line."""

import inspect
import math
import os

import numpy as np
import pytest

import features_oracle as FO
import lesion_oracle as LO
from dnncancerannotator_amd import casewise as CW
from dnncancerannotator_amd.__main__ import build_parser
from fake_features_device import FeatureSlices, fake_engine


# ---- casewise on hand-made records -----------------------------------------------------------------------------------------------
def _records(pixels, values=None, ring_values=None, bins=4, slice_=0, row=0):
    """the records of one lesion from its pixels [(x, y)] and their values (one channel): (row, shape, body [1], ring [1] or None,
    hist [1, bins]); the outline counts are not made here"""
    xs, ys = [p[0] for p in pixels], [p[1] for p in pixels]
    values = np.asarray([0.5] * len(pixels) if values is None else values, np.float32)
    r = np.zeros(1, LO.ROW_DTYPE)[0]
    r['slice'], r['row'], r['area'], r['x0'], r['y0'], r['x1'], r['y1'] = slice_, row, len(pixels), min(xs), min(ys), max(xs), max(ys)
    r['sum_x'], r['sum_y'] = sum(xs), sum(ys)
    s = np.zeros(1, FO.SHAPE_DTYPE)[0]
    s['slice'], s['row'], s['area'], s['boundary'], s['edges'] = slice_, row, len(pixels), len(pixels), 2 * len(pixels) + 2
    s['sum_xx'], s['sum_yy'], s['sum_xy'] = sum(x * x for x in xs), sum(y * y for y in ys), sum(x * y for x, y in zip(xs, ys))
    body = np.array([FO.intensity(slice_, row, 0, values)], FO.INTENSITY_DTYPE)
    ring = None if ring_values is None else np.array([FO.intensity(slice_, row, 0, np.asarray(ring_values, np.float32))], FO.INTENSITY_DTYPE)
    hist = np.bincount(FO.bin_of(values, bins), minlength=bins).astype(np.uint32)[None]
    return r, s, body, ring, hist


def _cells(names, values):
    cols = CW.lesion_feature_columns(names)
    assert len(cols) == len(values)
    return dict(zip(cols, values))


def test_one_pixel_lesion():
    c = _cells(['t2'], CW.lesion_feature_values('e', 3, *_records([(5, 7)], [0.25], [0.75, 0.25])))
    assert (c['exam'], c['slice'], c['lesion'], c['boundary_px'], c['edge_len']) == ('e', 3, 0, 1, 4)
    assert [float(c[k]) for k in ('extent', 'major_axis', 'minor_axis', 'eccentricity', 'orientation_deg')] == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert (c['mean_t2'], c['std_t2'], c['min_t2'], c['max_t2']) == ('0.25', '0.0', '0.25', '0.25')
    assert c['p10_t2'] == c['p50_t2'] == c['p90_t2'] == '0.25'              # clipped to [min, max]
    assert (c['ring_px_t2'], c['ring_mean_t2'], c['ring_std_t2'], c['contrast_t2']) == (2, '0.5', '0.25', '-0.25')


def test_horizontal_bar_and_diagonal():
    c = _cells(['a'], CW.lesion_feature_values('e', 0, *_records([(x, 4) for x in range(2, 11)])))
    var = sum((x - 6) ** 2 for x in range(2, 11)) / 9                        # 60 / 9
    assert float(c['major_axis']) == 4 * math.sqrt(var) and float(c['minor_axis']) == 0.0
    assert float(c['eccentricity']) == 1.0 and float(c['orientation_deg']) == 0.0 and float(c['extent']) == 1.0
    c = _cells(['a'], CW.lesion_feature_values('e', 0, *_records([(3 + i, 1 + i) for i in range(5)])))
    assert float(c['orientation_deg']) == 45.0 and float(c['eccentricity']) == 1.0 and float(c['extent']) == 5 / 25
    assert float(c['major_axis']) == 4 * math.sqrt(2 * 2.0) and float(c['minor_axis']) == 0.0
    c = _cells(['a'], CW.lesion_feature_values('e', 0, *_records([(3 + i, 9 - i) for i in range(5)])))
    assert float(c['orientation_deg']) == -45.0
    c = _cells(['a'], CW.lesion_feature_values('e', 0, *_records([(x, y) for x in range(4) for y in range(4)])))
    assert float(c['eccentricity']) == 0.0 and float(c['major_axis']) == float(c['minor_axis']) == 4 * math.sqrt(1.25)
    # large coordinates: the central moments are differences of products near 2^50 -- exact in integers, lost in float64 products
    far = [(60000 + x, 65000) for x in range(3)]
    c = _cells(['a'], CW.lesion_feature_values('e', 0, *_records(far)))
    assert float(c['major_axis']) == 4 * math.sqrt(2 / 3) and float(c['minor_axis']) == 0.0


def test_percentiles_on_a_known_histogram():
    hist = [2, 0, 6, 2]                                                      # n = 10, bins of width 0.25
    assert CW.feature_percentile(hist, 0.1, 0.0, 1.0) == (0 + 1 / 2) / 4     # t = 1: half way through bin 0
    assert CW.feature_percentile(hist, 0.2, 0.0, 1.0) == (0 + 2 / 2) / 4     # t = 2 sits on the edge: bin 0 reaches it, its upper edge
    assert CW.feature_percentile(hist, 0.5, 0.0, 1.0) == (2 + 3 / 6) / 4     # t = 5: past the empty bin 1, 3 of 6 into bin 2
    assert CW.feature_percentile(hist, 0.9, 0.0, 1.0) == (3 + 1 / 2) / 4
    assert CW.feature_percentile(hist, 0.9, 0.0, 0.8) == 0.8 and CW.feature_percentile(hist, 0.1, 0.2, 1.0) == 0.2
    assert [CW.feature_percentile([7], f, 0.0, 1.0) for f in (0.1, 0.5, 0.9)] == [0.1, 0.5, 0.9]     # one bin: a straight line
    assert CW.feature_percentile([7], 0.5, 0.25, 0.375) == 0.375
    with pytest.raises(ValueError):
        CW.feature_percentile([0, 0], 0.5, 0.0, 1.0)


def test_blank_cells():
    row, shape, body, ring, hist = _records([(1, 1), (2, 1)], [0.25, 0.75], [])
    c = _cells(['m'], CW.lesion_feature_values('e', 0, row, shape, body, ring, None))          # --feature_bins 0, an empty ring
    assert c['p10_m'] == c['p50_m'] == c['p90_m'] == '' and c['mean_m'] == '0.5' and c['std_m'] == '0.25'
    assert (c['ring_px_m'], c['ring_mean_m'], c['ring_std_m'], c['contrast_m']) == (0, '', '', '')
    c = _cells(['m'], CW.lesion_feature_values('e', 0, row, shape, body, None, hist))          # --feature_ring 0
    assert (c['ring_px_m'], c['ring_mean_m'], c['ring_std_m'], c['contrast_m']) == ('', '', '', '') and c['p50_m'] != ''
    shape['area'] += 1
    with pytest.raises(ValueError):
        CW.lesion_feature_values('e', 0, row, shape, body, None, hist)


def test_exam_pooling_equals_the_values_of_the_concatenated_pixels():
    rng = np.random.default_rng(3)
    va, vb, ra, rb = rng.random(7), rng.random(30) * 0.5, rng.random(11), rng.random(0)
    a = _records([(x, 0) for x in range(7)], va, ra, bins=8)
    b = _records([(x, 1) for x in range(30)], vb, rb, bins=8, slice_=1)
    both = _records([(x, 0) for x in range(37)], np.concatenate([va, vb]), np.concatenate([ra, rb]), bins=8)
    pooled = CW.exam_lesion_feature_values('e', 4, [a[1:], b[1:]])
    cols = CW.exam_lesion_feature_columns(['m'])
    assert len(cols) == len(pooled) and pooled[:3] == ['e', 4, int(a[1]['edges']) + int(b[1]['edges'])]
    assert pooled[3:] == CW.lesion_feature_values('e', 0, *both)[3 + len(CW.FEATURE_SHAPE_COLUMNS):]
    means = [float(CW.lesion_feature_values('e', 0, *r)[3 + len(CW.FEATURE_SHAPE_COLUMNS)]) for r in (a, b)]
    assert float(pooled[3]) != sum(means) / 2                               # not the mean of the parts' means
    assert pooled[cols.index('ring_px_m')] == 11


def test_check_features():
    assert CW.check_features(False) == (None, None) and CW.check_features(True) == (32, 3) and CW.check_features(True, 0, 0) == (0, 0)
    assert CW.check_features(True, 256, 8) == (256, 8)
    for kw in (dict(bins=8), dict(ring=2)):
        with pytest.raises(ValueError, match='--lesion_features'):
            CW.check_features(False, **kw)
    for kw in (dict(bins=257), dict(bins=-1), dict(ring=9), dict(ring=-1)):
        with pytest.raises(ValueError, match='outside'):
            CW.check_features(True, **kw)


# ---- the oracle on a hand-counted drawing ----------------------------------------------------------------------------------------
def test_oracle_by_hand():
    prob = np.zeros((1, 8, 10), np.float32)
    prob[0, 2:4, 2:5] = 1.0                                                  # 2 x 3 block
    prob[0, 2, 6] = 1.0                                                      # a pixel two columns to its right
    x = np.zeros((1, 8, 10, 1), np.float32)
    x[0, 2:4, 2:5, 0] = [[0.0, 0.25, 0.5], [0.75, 1.0, 2.0]]
    x[0, 2, 5, 0] = 0.5                                                      # between the two: within 1 pixel of both, row 0's
    shape, body, ring, hist = FO.lesion_features(prob, x, k=1, bins=4, ring=1)
    assert shape['area'].tolist() == [6, 1] and shape['boundary'].tolist() == [6, 1] and shape['edges'].tolist() == [10, 4]
    assert shape['sum_xx'].tolist() == [2 * (4 + 9 + 16), 36] and shape['sum_xy'].tolist() == [9 * 2 + 9 * 3, 12]
    assert body['sum_q16'][:, 0].tolist() == [int(3.5 * 65536), 0] and body['max'][:, 0].tolist() == [1.0, 0.0]
    assert body['sum_sq_q16'][0, 0] == (1 + 4 + 9 + 16 + 16) * (1 << 28)
    assert hist[0, 0].tolist() == [1, 1, 1, 3]                               # 0.75, 1 and the clamped 2 share the last bin
    assert ring['n'][:, 0].tolist() == [4 * 5 - 6, 9 - 1 - 3] and ring['sum_q16'][:, 0].tolist() == [1 << 15, 0]


# ---- annotate on the fake device -------------------------------------------------------------------------------------------------
EXAMS, IDS = ['a'] * 4 + ['b'] * 3, [0, 1, 2, 3, 0, 1, 2]
KW = dict(threshold=0.5, filter_size=1, max_lesions=8)


def _drawn():
    """7 slices of 12 x 12 x 3 of exams a (4 slices) and b (3): the drawing of tests/test_spread_host.py in channel 0 (slice 6 has
    no lesion, slice 5 is a checkerboard of 72 single-pixel lesions), random values in the others"""
    x = np.random.default_rng(5).random((7, 12, 12, 3)).astype(np.float32)
    prob = np.zeros((7, 12, 12), np.float32)
    prob[0:5, 3:7, 2:6] = 0.75
    prob[2:4, 9:11, 1:4] = 0.625
    yy, xx = np.mgrid[0:12, 0:12]
    prob[5] = np.where((yy + xx) % 2 == 0, 0.875, 0.0)
    x[..., 0] = prob
    return x


def _texts(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            with open(os.path.join(d, f), 'rb') as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def _setup(tmp_path, monkeypatch, slice_types=None):
    e = fake_engine(monkeypatch, 3)
    ds = FeatureSlices(_drawn(), EXAMS, IDS, 4, slice_types)
    e._build(ds)
    e.current_step = 1
    run = str(tmp_path / 'run')
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    return e, ds, run


def _expected(names, bins, ring, probs=None):
    """lesion_features.csv from the oracle alone, slice by slice"""
    x = _drawn()
    probs = x[..., 0] if probs is None else probs
    s = (KW['threshold'], 1.0, KW['filter_size'], 0, KW['max_lesions'])
    lines = []
    for i, (exam, k) in enumerate(zip(EXAMS, IDS)):
        rows, _, _ = LO.lesion_table(probs[i:i + 1], *s)
        sh, bd, rg, hs = FO.lesion_features(probs[i:i + 1], x[i:i + 1], *s, bins=bins, ring=ring)
        lines += [CW.lesion_feature_values(exam, k, r, sh[j], bd[j], None if rg is None else rg[j], None if hs is None else hs[j])
                  for j, r in enumerate(rows)]
    return CW.plain_csv(CW.lesion_feature_columns(names), lines)


@pytest.mark.parametrize('link', [False, True])
def test_annotate_feature_files(tmp_path, monkeypatch, link):
    e, ds, run = _setup(tmp_path, monkeypatch, ['t2', 'adc', 'dwi', 'label'])
    e.annotate(ds, run, str(tmp_path / 'plain'), export_images=True, link_slices=link, **KW)
    plain_calls = list(e.device_model.calls)
    e.device_model.calls.clear()
    res = e.annotate(ds, run, str(tmp_path / 'feat'), export_images=True, link_slices=link, lesion_features=True, **KW)
    calls = e.device_model.calls
    assert [c for c in calls if c[0].startswith('forward')] == [c for c in plain_calls if c[0].startswith('forward')]
    if link:                         # the linked table runs exactly as without the flag; the feature records come from a second call
        assert [c for c in calls if c[0] == 'lesion_table_linked'] == [c for c in plain_calls if c[0] == 'lesion_table_linked']
        assert [c for c in calls if c[0] == 'lesion_table_features'] == [('lesion_table_features', n, False, 32, 3) for n in (3, 1, 3)]
    else:                            # one call serves the table and the records
        assert [c for c in calls if c[0] == 'lesion_table_features'] == [('lesion_table_features', n, True, 32, 3) for n in (3, 1, 3)]
        assert not [c for c in calls if c[0] == 'lesion_table']
    with_flag, without = _texts(str(tmp_path / 'feat')), _texts(str(tmp_path / 'plain'))
    new = ['lesion_features.csv'] + (['exam_lesion_features.csv'] if link else [])
    assert sorted(set(with_flag) - set(without)) == sorted(new)
    assert all(with_flag[k] == v for k, v in without.items()) and 'lesions.csv' in without and 'slices.csv' in without
    names = ['t2', 'adc', 'dwi']
    text = with_flag['lesion_features.csv'].decode()
    assert text == _expected(names, 32, 3)
    assert text.splitlines()[0].split(',') == CW.lesion_feature_columns(names) and 'contrast_dwi' in text.splitlines()[0]
    key = lambda t, n: [l.split(',')[:n] for l in t.decode().splitlines()[1:]]
    assert key(with_flag['lesion_features.csv'], 3) == key(with_flag['lesions.csv'], 3) and res['lesions'] == len(key(with_flag['lesions.csv'], 3))
    if link:
        lines = with_flag['exam_lesion_features.csv'].decode().splitlines()
        assert lines[0].split(',') == CW.exam_lesion_feature_columns(names)
        assert key(with_flag['exam_lesion_features.csv'], 2) == key(with_flag['exam_lesions.csv'], 2)
        # exam a's first lesion is the block of 16 pixels in slices 0..3: its pooled mean of channel 0 is the probability there,
        # its surface four outlines of 16 faces, and its ring the four slices' rings
        first = dict(zip(lines[0].split(','), lines[1].split(',')))
        per_slice = [dict(zip(text.splitlines()[0].split(','), l.split(','))) for l in text.splitlines()[1:]]
        parts = [d for d in per_slice if d['exam'] == 'a' and d['lesion'] == '0']
        assert (first['exam'], first['exam_lesion'], first['surface_px']) == ('a', '0', '64') and float(first['mean_t2']) == 0.75
        assert int(first['ring_px_adc']) == sum(int(d['ring_px_adc']) for d in parts) and len(parts) == 4
        x = _drawn()
        assert np.float32(first['max_dwi']) == x[0:4, 3:7, 2:6, 2].max()        # 9 digits give the float32 back


def test_annotate_features_beside_uncertainty_and_without_names(tmp_path, monkeypatch):
    import tta_oracle as TO
    e, ds, run = _setup(tmp_path, monkeypatch)
    e.annotate(ds, run, str(tmp_path / 'unc'), tta='flips', uncertainty=True, **KW)
    e.device_model.calls.clear()
    e.annotate(ds, run, str(tmp_path / 'both'), tta='flips', uncertainty=True, lesion_features=True, feature_bins=0, feature_ring=0, **KW)
    calls = e.device_model.calls
    assert [c for c in calls if c[0] == 'lesion_table_features'] == [('lesion_table_features', n, False, 0, 0) for n in (3, 1, 3)]
    assert [c[:2] for c in calls if c[0] == 'lesion_table_spread'] == [('lesion_table_spread', n) for n in (3, 1, 3)]
    both, unc = _texts(str(tmp_path / 'both')), _texts(str(tmp_path / 'unc'))
    assert sorted(set(both) - set(unc)) == ['lesion_features.csv'] and all(both[k] == v for k, v in unc.items())
    x = _drawn()
    planes = np.stack([(TO.apply_view(x[..., :1], k)[..., 0] * np.float32(1 - k / 32)).astype(np.float32) for k in TO.views_of(0x0F)])
    # the table is that of the views' mean, the channels are the untransformed batch's
    assert both['lesion_features.csv'].decode() == _expected(['ch0', 'ch1', 'ch2'], 0, 0, TO.mean_of(planes, 0x0F))


def test_feature_flags_are_checked_before_load(tmp_path, monkeypatch):
    from dnncancerannotator_amd import engine
    e, ds, run = _setup(tmp_path, monkeypatch)
    touched = []
    monkeypatch.setattr(engine.TFKerasModel, 'load', lambda self, path: touched.append(path))
    monkeypatch.setattr(engine.TFKerasModel, 'get_ckpts', lambda self, path: touched.append(path) or {})
    for kw in (dict(feature_bins=8), dict(feature_ring=2), dict(lesion_features=True, feature_bins=257),
               dict(lesion_features=True, feature_ring=9)):
        with pytest.raises(ValueError, match='feature_'):
            e.annotate(ds, run, str(tmp_path / 'o'), **kw)
    assert touched == [] and not os.path.exists(str(tmp_path / 'o'))


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_and_signatures():
    from dnncancerannotator_amd import engine
    from dnncancerannotator_amd.runs.predict import predict
    p = build_parser()
    base = ['predict', '--save_path', 's', '--data_path', 'd', '--output', 'o']
    got = vars(p.parse_args(base))
    assert not {'lesion_features', 'feature_bins', 'feature_ring'} & set(got)            # the defaults are those of the run function
    for fn in (predict, engine.TFKerasModel.annotate):
        par = inspect.signature(fn).parameters
        assert par['lesion_features'].default is False and par['feature_bins'].default is None and par['feature_ring'].default is None
    got = vars(p.parse_args(base + ['--lesion_features', '--feature_bins', '64', '--feature_ring', '5']))
    assert (got['lesion_features'], got['feature_bins'], got['feature_ring']) == (True, 64, 5)
    with pytest.raises(SystemExit):
        p.parse_args(['evaluate', '--save_path', 's', '--data_path', 'd', '--tag', 't', '--lesion_features'])


def test_cli_checks_the_feature_flags_before_anything_is_read(monkeypatch, tmp_path):
    import yaml
    from dnncancerannotator_amd import __main__ as cli, engine
    touched, seen = [], []
    monkeypatch.setattr(engine.TFKerasModel, '__init__', lambda self, config: touched.append('init'))
    monkeypatch.setattr(engine.TFKerasModel, 'load', lambda self, path: touched.append('load'))
    monkeypatch.setattr(engine.TFKerasModel, 'annotate', lambda self, dataset, **kw: seen.append(kw) or {})
    save = tmp_path / 'run'
    pr = ['predict', '--save_path', str(save), '--data_path', 'synthetic:16x16x2', '--output', str(tmp_path / 'o')]
    for flags in (['--feature_bins', '8'], ['--feature_ring', '2'], ['--lesion_features', '--feature_bins', '300'],
                  ['--lesion_features', '--feature_ring', '-1']):
        with pytest.raises(ValueError, match='feature_'):
            cli.main(pr + flags)                 # options.yaml does not even exist yet
    assert touched == [] and seen == []
    save.mkdir()
    (save / 'options.yaml').write_text(yaml.safe_dump({'config': {'data_options': {'eval': {'batch_size': 2}}}}))
    assert cli.main(pr + ['--lesion_features', '--feature_ring', '0']) == 0 and cli.main(pr) == 0
    assert seen[0]['lesion_features'] is True and seen[0]['feature_ring'] == 0 and seen[0]['feature_bins'] is None
    assert not {'lesion_features', 'feature_bins', 'feature_ring'} & set(seen[1])
