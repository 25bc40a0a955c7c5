"""CPU: losses.TverskyCrossentropy / DiceCrossentropy -- the float64 reference of tests/region_loss_ref.py against central differences
and the textbook soft Dice, the registry and its checks, and the engine's one call of DeviceModel.set_region_loss."""

import numpy as np
import pytest

import fake_train_metrics
import region_loss_ref as R
from oracle import unet_oracle as O


def _case():
    """2 x 6 x 5, random logits, image 0 without positives"""
    rng = np.random.default_rng(11)
    logits = rng.normal(0.0, 1.5, (2, 6, 5, 1))
    y = np.zeros((2, 6, 5))
    y[1, 1:4, 2:5] = 1.0
    return y, logits


@pytest.mark.parametrize('cfg', [
    dict(),
    dict(alpha=0.3, beta=0.7, smooth=0.1, weight_mul=3.0),
    dict(crossentropy_weight=0.0, region_weight=2.0),
    dict(alpha=0.0, beta=1.0, weight=4.0, crossentropy_weight=0.5),
])
def test_analytic_gradient_matches_central_differences(cfg):
    """d(sum_b L_b)/dlogit against (f(x + h) - f(x - h)) / 2h in float64, h = 1e-6: truncation ~ h^2 f''' / 6 = 2e-13 and rounding
    ~ eps |f| / h = 1e-9 absolute on gradient entries of 1e-2 and more relative to the largest one, so 1e-7 of the largest entry"""
    y, logits = _case()
    per, dper = R.tversky_crossentropy(y, logits, **cfg)
    assert per.shape == (2,) and dper.shape == logits.shape
    h = 1e-6
    num = np.zeros_like(logits)
    for idx in np.ndindex(*logits.shape):
        lp, lm = logits.copy(), logits.copy()
        lp[idx] += h
        lm[idx] -= h
        num[idx] = (R.tversky_crossentropy(y, lp, **cfg)[0].sum() - R.tversky_crossentropy(y, lm, **cfg)[0].sum()) / (2 * h)
    assert np.abs(dper).max() > 1e-3
    assert np.abs(num - dper).max() <= 1e-7 * np.abs(dper).max()
    # an image's loss does not depend on the other image's logits beyond the shared positive-class weight, which is a label statistic
    lp = logits.copy()
    lp[0] += 0.5
    assert R.tversky_crossentropy(y, lp, **cfg)[0][1] == per[1]


def test_half_half_is_soft_dice():
    y, logits = _case()
    for s in (1.0, 0.1):
        per, _ = R.tversky_crossentropy(y, logits, crossentropy_weight=0.0, smooth=s)
        I, P, Y = R.region_sums(y, logits).T
        dice = (2 * I + 2 * s) / (P + Y + 2 * s)
        assert np.abs(per - (1.0 - dice)).max() <= 1e-15
    # a label-free image: T = s / (alpha P + s)
    t = R.tversky_index(R.region_sums(y, logits), 0.3, 0.7, 0.5)
    P0 = R.region_sums(y, logits)[0, 1]
    assert abs(t[0] - 0.5 / (0.3 * P0 + 0.5)) <= 1e-15


def test_label_smoothing_blurs_the_region_labels_too():
    y, logits = _case()
    y = y.astype(np.float32)                 # the labels' dtype in every step: the blurred ones are rounded to it
    cfg = dict(label_smoothing=True, label_smoothing_filter_size=3, label_smoothing_sigma=1.0)
    per, _ = R.tversky_crossentropy(y, logits, crossentropy_weight=0.0, **cfg)
    ys = R.loss_labels(y, cfg)
    assert np.abs(ys - O.gaussian_filter2d(y, 3, 1.0)).max() <= 1e-7 and ys.max() <= 1.0 and (ys > 0).sum() > (y > 0).sum()
    assert np.abs(per - (1.0 - R.tversky_index(R.region_sums(ys, logits), 0.5, 0.5, 1.0))).max() <= 1e-15


def test_registry_and_validation():
    from dnncancerannotator_amd import losses
    base = losses.WeightedCrossentropy()
    assert base.get_config() == dict(weight=None, weight_add=0.0, weight_mul=1.0, label_smoothing=False,
                                     label_smoothing_filter_size=6, label_smoothing_sigma=3)
    assert not hasattr(base, 'region_cfg')
    t = losses.get({'class_name': 'TverskyCrossentropy', 'config': dict(alpha=0.3, beta=0.7, weight_mul=3.0, smooth=0.5)})
    assert type(t) is losses.TverskyCrossentropy and isinstance(t, losses.WeightedCrossentropy)
    assert t.region_cfg() == dict(region_weight=1.0, crossentropy_weight=1.0, alpha=0.3, beta=0.7, smooth=0.5)
    assert t.device_cfg() == losses.WeightedCrossentropy(weight_mul=3.0).device_cfg()
    assert t.get_config()['alpha'] == 0.3 and t.get_config()['weight_mul'] == 3.0
    d = losses.get('DiceCrossentropy')
    assert isinstance(d, losses.TverskyCrossentropy) and d.region_cfg() == dict(region_weight=1.0, crossentropy_weight=1.0, alpha=0.5,
                                                                                beta=0.5, smooth=1.0)
    assert losses.get(d) is d
    assert losses.get({'class_name': 'DiceCrossentropy', 'config': {'label_smoothing': True}}).device_cfg()['label_smoothing'] is True
    for bad in (dict(region_weight=0.0), dict(region_weight=-1.0), dict(crossentropy_weight=-0.1), dict(alpha=-0.1), dict(beta=-1.0),
                dict(alpha=0.0, beta=0.0), dict(smooth=0.0), dict(smooth=-1.0), dict(smooth=float('nan')), dict(alpha=float('inf')),
                dict(region_weight='1'), dict(label_smoothing=True, label_smoothing_filter_size=99)):
        with pytest.raises(ValueError):
            losses.TverskyCrossentropy(**bad)
    with pytest.raises(ValueError):
        losses.DiceCrossentropy(alpha=0.3)
    with pytest.raises(ValueError):
        losses.get('FocalLoss')
    losses.TverskyCrossentropy(crossentropy_weight=0.0, alpha=0.0, beta=1.0)       # the edges that are allowed


def test_overlays_select_the_classes():
    import os
    from dnncancerannotator_amd import load, losses
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = {'deploy_options': {'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}}}}
    for name, cls, ab in (('dice_loss.yaml', losses.DiceCrossentropy, (0.5, 0.5)), ('tversky_recall.yaml', losses.TverskyCrossentropy, (0.3, 0.7))):
        over = load._load_config_single(os.path.join(root, 'configs', 'additionals', name))
        cfg = load._apply_config({'deploy_options': {'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}}}}, over)
        loss = losses.get(cfg['deploy_options']['loss'])
        assert type(loss) is cls and (loss.alpha, loss.beta) == ab and loss.weight_mul == 3.0
    assert base['deploy_options']['loss']['class_name'] == 'WeightedCrossentropy'


OPTS = dict(n_filters_first=3, n_downsample=2, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')


def _config(loss):
    return {'model': 'UNetAnnotator', 'model_options': OPTS,
            'deploy_options': {'optimizer': 'adam', 'loss': loss, 'enable_multigpu': False, 'metrics': []}}


class _RegionFake(fake_train_metrics.FakeTrainMetricsDevice):
    def set_region_loss(self, cfg=None, **kw):
        self.region_calls = getattr(self, 'region_calls', []) + [dict(cfg or {}, **kw)]


def test_engine_sets_the_region_loss_once_and_only_for_the_new_class(tmp_path, monkeypatch):
    from dnncancerannotator_amd import data, engine
    x, y = O.synthetic_batch(8, 16, 16, 1, seed_x=3, seed_y=4)
    monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
    # the old class on a device without the method: nothing is called
    built = fake_train_metrics.install(monkeypatch.setattr)
    assert not hasattr(fake_train_metrics.FakeTrainMetricsDevice, 'set_region_loss')
    res = engine.TFKerasModel(_config({'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}})).train(
        data.ArrayDataset(x, y, 4, repeat=True), save_path=str(tmp_path / 'a'), max_steps=2, save_freq=100)
    assert len(res.history['loss']) == 2 and len(built) == 1
    # ... and on a device with it: still nothing
    monkeypatch.setattr(fake_train_metrics, 'FakeTrainMetricsDevice', _RegionFake)
    built = fake_train_metrics.install(monkeypatch.setattr)
    engine.TFKerasModel(_config({'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}})).train(
        data.ArrayDataset(x, y, 4, repeat=True), save_path=str(tmp_path / 'b'), max_steps=2, save_freq=100)
    assert len(built) == 1 and not hasattr(built[0], 'region_calls')
    # the new class: once per device model, with the five values
    built = fake_train_metrics.install(monkeypatch.setattr)
    m = engine.TFKerasModel(_config({'class_name': 'TverskyCrossentropy', 'config': {'weight_mul': 3.0, 'alpha': 0.3, 'beta': 0.7}}))
    m.train(data.ArrayDataset(x, y, 4, repeat=True), val_data=data.ArrayDataset(x[:4], y[:4], 4), save_path=str(tmp_path / 'c'),
            max_steps=2, save_freq=1)
    assert len(built) == 1
    assert built[0].region_calls == [dict(region_weight=1.0, crossentropy_weight=1.0, alpha=0.3, beta=0.7, smooth=1.0)]
