"""CPU: the region-metric oracle (tests/region_oracle.py) on the reference's scenarios (annotator/tests/test_region_metrics.py,
restated in tests/region_cases.py: expected counts known by construction), its connected components against scipy.ndimage.label,
the metric classes' float32 formulas, the spec grouping, and the `deploy_options.region_metrics: device` switch."""

import logging

import numpy as np
import pytest

import region_cases as RC
import region_oracle as O
from dnncancerannotator_amd import metrics as M
from dnncancerannotator_amd import region_metrics as R

METRICS_YAML_REGION = [
    {'RegionBasedPrecision': dict(thresholds=0.80, IoU_threshold=0.30, resize_factor=0.5, name='region/precision')},
    {'RegionBasedRecall': dict(thresholds=0.80, IoU_threshold=0.30, resize_factor=0.5, name='region/recall')},
    {'RegionBasedTruePositives': dict(thresholds=0.80, IoU_threshold=0.30, resize_factor=0.5, name='region/TP')},
    {'RegionBasedFalsePositives': dict(thresholds=0.80, IoU_threshold=0.30, resize_factor=0.5, name='region/FP')},
    {'RegionBasedFalseNegatives': dict(thresholds=0.80, IoU_threshold=0.30, resize_factor=0.5, name='region/FN')},
    {'RegionBasedFBetaScore': dict(thresholds=0.80, IoU_threshold=0.30, resize_factor=0.5, beta=1.0, name='region/F1-score')},
    {'RegionBasedFBetaScore': dict(thresholds=0.80, IoU_threshold=0.30, resize_factor=0.5, beta=2.0, name='region/F2-score')},
]


@pytest.mark.parametrize('rf', [1.0, 0.5])
@pytest.mark.parametrize('thr', [RC.THRESHOLDS_1, RC.THRESHOLDS_10], ids=['T1', 'T10'])
def test_oracle_on_the_reference_scenarios(rf, thr):
    for name, y, p, expected in RC.scenarios(seed=11):
        got = O.region_counts(p, y, thr, 0.30, rf, 5)
        assert [tuple(r) for r in got] == [expected] * len(thr), (name, rf, got.tolist())


def test_oracle_threshold_consistency():
    """test_region_metrics.py test_consistency_multithresholds: T thresholds at once = T single-threshold runs"""
    y, p = RC.random_slices(5, n=6)
    many = O.region_counts(p, y, RC.THRESHOLDS_10, 0.3, 0.5, 5)
    one = np.concatenate([O.region_counts(p, y, [t], 0.3, 0.5, 5) for t in RC.THRESHOLDS_10])
    assert np.array_equal(many, one)
    assert many[:, 0].sum() > 0 and many[:, 1].sum() > 0 and many[:, 3].sum() > 0      # matches and misses both occur


def test_oracle_components_match_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(4)
    masks = [rng.random((37, 53)) < d for d in (0.3, 0.5, 0.6)]
    spiral = np.zeros((41, 41), bool)
    y0, x0, y1, x1 = 0, 0, 40, 40
    while y0 <= y1 and x0 <= x1:
        spiral[y0, x0:x1 + 1] = spiral[y0:y1 + 1, x1] = spiral[y1, x0:x1 + 1] = True
        spiral[y0 + 2:y1 + 1, x0] = True
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
        if y0 <= y1:
            spiral[y0, x0 - 1] = False
    masks += [spiral, np.eye(30, dtype=bool), np.ones((16, 9), bool), np.zeros((5, 5), bool)]
    four = ndimage.generate_binary_structure(2, 1)
    for m in masks:
        lab, n = ndimage.label(m, structure=four)
        par = O.ccl(m)
        assert len(np.unique(par[m])) == n
        # same partition: a component of one is a component of the other, and its root is its smallest flat index
        for c in range(1, n + 1):
            roots = np.unique(par[lab == c])
            assert roots.size == 1 and roots[0] == np.flatnonzero((lab == c).ravel())[0]


def test_oracle_resize_and_opening_pieces():
    assert O.out_size(200, 200, 0.5) == (100, 100)
    assert O.out_size(512, 512, 0.5) == (256, 256)
    assert O.out_size(97, 161, 0.3) == (int(np.float16(97) * np.float16(0.3)), int(np.float16(161) * np.float16(0.3)))
    x = np.arange(16, dtype=np.float32).reshape(4, 4)
    assert np.array_equal(O.resize(x, 4, 4), x)
    assert O.resize(x, 2, 2).tolist() == [[2.5, 4.5], [10.5, 12.5]]
    m = np.zeros((9, 9), bool)
    m[1:8, 1:8] = True
    m[4, 0] = True                                          # a one-pixel spur: removed by the opening
    o = O.morph_open(m, 3)
    assert o[1:8, 1:8].all() and o.sum() == 49
    full = np.ones((6, 7), bool)
    assert O.morph_open(full, 5).all()                     # out-of-bounds pixels are ignored, not zeros
    assert not O.morph_open(np.eye(8, dtype=bool), 3).any()


def test_iou_threshold_range():
    y = np.zeros((1, 8, 8), np.float32)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            O.region_counts(y, y, [0.5], bad)
        with pytest.raises(ValueError):
            R.RegionBasedRecall(0.5, IoU_threshold=bad)
    with pytest.raises(ValueError):
        R.RegionBasedRecall([-0.5])
    with pytest.raises(ValueError):
        R.RegionBasedRecall(np.linspace(0, 1, 65))


def test_metric_formulas_in_float32():
    counts = np.array([[3, 2, 4, 5], [0, 0, 0, 0], [7, 1, 6, 0]], np.int64)
    eps = np.float32(1e-7)
    kw = dict(thresholds=[0.2, 0.5, 0.9], IoU_threshold=0.3)
    ms = {c: getattr(R, c)(**(dict(kw, beta=2.0) if c == 'RegionBasedFBetaScore' else kw)) for c in R._REGISTRY}
    for m in ms.values():
        m.add_counts(counts)
    f32 = lambda v: np.float32(v)
    rec = counts[:, 0].astype(np.float32) / ((counts[:, 0] + counts[:, 1]).astype(np.float32) + eps)
    pre = counts[:, 2].astype(np.float32) / ((counts[:, 2] + counts[:, 3]).astype(np.float32) + eps)
    assert ms['RegionBasedRecall'].result() == rec.tolist()
    assert ms['RegionBasedPrecision'].result() == pre.tolist()
    assert ms['RegionBasedTruePositives'].result() == [3, 0, 7]
    assert ms['RegionBasedFalseNegatives'].result() == [2, 0, 1]
    assert ms['RegionBasedFalsePositives'].result() == [5, 0, 0]
    f2 = (f32(5.0) * pre * rec / (f32(4.0) * pre + rec + eps)).tolist()
    assert ms['RegionBasedFBetaScore'].result() == f2
    cm = ms['RegionBasedConfusionMatrix']
    assert np.isnan(cm.result())
    d = cm.result_dict()
    assert d['true_positive_counts'] == [3, 0, 7] and d['false_positive_counts'] == [5, 0, 0]
    assert d['recall'] == rec.tolist()
    assert d['precision'] == (counts[:, 0].astype(np.float32) / ((counts[:, 0] + counts[:, 3]).astype(np.float32) + eps)).tolist()
    one = R.RegionBasedTruePositives(0.5)                  # T = 1 squeezes to a scalar
    one.add_counts([[4, 1, 2, 3]])
    assert one.result() == 4
    r1 = R.RegionBasedRecall(0.5)
    r1.add_counts([[4, 1, 2, 3]])
    assert r1.result() == float(np.float32(4) / (np.float32(5) + eps))


def test_metrics_yaml_region_entries_share_one_spec():
    ms = [R.solve_region_metric(s) for s in METRICS_YAML_REGION]
    assert all(m is not None for m in ms)
    groups = R.group_by_spec(ms)
    assert len(groups) == 1 and len(groups[0][1]) == 7
    assert groups[0][0] == ((float(np.float32(0.8)),), float(np.float32(0.3)), 0.5, 5)
    other = R.RegionBasedRecall([0.8], IoU_threshold=0.5, resize_factor=0.5)
    assert len(R.group_by_spec(ms + [other])) == 2
    assert R.solve_region_metric({'Precision': {'thresholds': 0.8}}) is None


def _engine(metrics, region=None):
    from dnncancerannotator_amd.engine import TFKerasModel
    deploy = dict(optimizer='adam', metrics=metrics)
    if region is not None:
        deploy['region_metrics'] = region
    cfg = dict(model='UNetAnnotator', model_options=dict(n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False,
                                                padding='same'), deploy_options=deploy)
    return TFKerasModel(cfg)


def test_region_metrics_device_switch(caplog):
    pixel = [{'Precision': dict(thresholds=0.8, name='pixel/precision')}]
    with caplog.at_level(logging.WARNING):
        e = _engine(pixel + METRICS_YAML_REGION)
    assert [m.name for m in e.metrics] == ['pixel/precision'] and e.region_metrics == []
    assert 'skipped' in caplog.text                         # unchanged default: the region entries are skipped with a warning
    assert M.solve_metric(METRICS_YAML_REGION[0]) is None
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        e = _engine(pixel + METRICS_YAML_REGION, region='device')
    assert [m.name for m in e.metrics] == ['pixel/precision']
    assert [m.name for m in e.region_metrics] == [list(s.values())[0]['name'] for s in METRICS_YAML_REGION]
    assert 'skipped' not in caplog.text
    with pytest.raises(ValueError):
        _engine(pixel, region='cpu')
