"""CPU: losses.BoundaryCrossentropy -- the registry and its checks, the numpy oracle of tests/boundary_oracle.py against the O(N^2)
definition and a hand-made case, its float64 gradient against central differences, the overlay, and the engine's calls of
DeviceModel.set_region_loss / set_boundary_loss."""

import os

import numpy as np
import pytest

import boundary_oracle as BO
import fake_train_metrics
from oracle import unet_oracle as O


def _planes():
    """small label planes: empty, full, one pixel, a lesion on two borders, a checkerboard, Bernoulli, one row, one column"""
    rng = np.random.default_rng(21)
    out = []
    for H, W in ((1, 1), (1, 9), (9, 1), (7, 11), (13, 19)):
        out.append(np.zeros((H, W), np.float32))
        out.append(np.ones((H, W), np.float32))
        one = np.zeros((H, W), np.float32)
        one[H - 1, 0] = 1.0
        out.append(one)
        lesion = np.zeros((H, W), np.float32)
        lesion[H - (H + 3) // 4:, :(W + 3) // 4] = 1.0
        out.append(lesion)
        yy, xx = np.mgrid[0:H, 0:W]
        out.append(((yy + xx) % 2).astype(np.float32))
        out.append((rng.random((H, W)) < 0.5).astype(np.float32))
        out.append((rng.random((H, W)) < 0.05).astype(np.float32))
    return out


def test_separable_oracle_equals_the_definition():
    for y in _planes():
        phi, d2 = BO.signed_distance_plane(y)
        phi_b, d2_b = BO.signed_distance_plane(y, edt=BO.edt2_brute)
        assert d2.dtype == np.int32 and phi.dtype == np.float32
        assert np.array_equal(d2, d2_b), y.shape
        assert np.array_equal(phi.view(np.uint32), phi_b.view(np.uint32)), y.shape
    # chunks smaller than a row pair: the same numbers
    y = _planes()[-2]
    assert np.array_equal(BO.edt2(y > 0.5, chunk_elems=7), BO.edt2_brute(y > 0.5))


def test_oracle_on_a_hand_made_plane():
    """3 x 5, G = the 2 x 2 block in the top left corner"""
    y = np.zeros((3, 5), np.float32)
    y[0:2, 0:2] = 1.0
    phi, d2 = BO.signed_distance_plane(y)
    assert d2.tolist() == [[4, 1, 1, 4, 9], [1, 1, 1, 4, 9], [1, 1, 2, 5, 10]]
    want = np.sqrt(np.asarray(d2, np.float64))
    want[0:2, 0:2] = 1.0 - want[0:2, 0:2]
    assert np.abs(phi - want).max() <= 1e-7 and phi[0, 0] == -1.0 and phi[1, 1] == 0.0 and phi[0, 2] == 1.0
    # the label rule: 0.5 is background, the next float foreground
    y[:] = 0.5
    assert not BO.signed_distance_plane(y)[0].any()
    y[2, 4] = np.nextafter(np.float32(0.5), np.float32(1.0))
    assert BO.signed_distance_plane(y)[1][0, 0] == 20 and BO.signed_distance_plane(y)[0][2, 4] == 0.0
    # empty and full: the term vanishes
    for v in (0.0, 1.0):
        phi, d2 = BO.signed_distance_plane(np.full((4, 6), v, np.float32))
        assert not phi.any() and not d2.any()


def _case():
    """2 x 6 x 5, random logits, image 0 without positives"""
    rng = np.random.default_rng(11)
    logits = rng.normal(0.0, 1.5, (2, 6, 5, 1))
    y = np.zeros((2, 6, 5), np.float32)
    y[1, 1:4, 2:5] = 1.0
    return y, logits


@pytest.mark.parametrize('cfg', [
    dict(),
    dict(boundary_weight=1.0, alpha=0.3, beta=0.7, smooth=0.1, weight_mul=3.0),
    dict(boundary_weight=0.5, crossentropy_weight=0.0, region_weight=2.0),
])
def test_analytic_gradient_matches_central_differences(cfg):
    """as tests/test_region_loss.py: h = 1e-6 in float64, 1e-7 of the largest gradient entry"""
    y, logits = _case()
    per, dper = BO.boundary_crossentropy(y, logits, **cfg)
    assert per.shape == (2,) and dper.shape == logits.shape
    h = 1e-6
    num = np.zeros_like(logits)
    for idx in np.ndindex(*logits.shape):
        lp, lm = logits.copy(), logits.copy()
        lp[idx] += h
        lm[idx] -= h
        num[idx] = (BO.boundary_crossentropy(y, lp, **cfg)[0].sum() - BO.boundary_crossentropy(y, lm, **cfg)[0].sum()) / (2 * h)
    assert np.abs(num - dper).max() <= 1e-7 * np.abs(dper).max()


def test_the_term_is_what_the_definition_says():
    import region_loss_ref as R
    y, logits = _case()
    per, dper = BO.boundary_crossentropy(y, logits, boundary_weight=0.25, weight_mul=3.0)
    per0, dper0 = R.tversky_crossentropy(y, logits, weight_mul=3.0)
    S = BO.boundary_sums(y, logits)
    assert S[0] == 0.0 and abs(S[1]) > 1.0                       # a healthy slice: the term vanishes
    assert np.abs(per - per0 - 0.25 * S / 30.0).max() <= 1e-15
    assert np.array_equal(dper[0], dper0[0]) and np.abs(dper[1] - dper0[1]).max() > 1e-4
    # under label smoothing the map still comes from the raw label
    cfg = dict(label_smoothing=True, label_smoothing_filter_size=3, label_smoothing_sigma=1.0)
    per_s, _ = BO.boundary_crossentropy(y, logits, boundary_weight=0.25, **cfg)
    per_s0, _ = R.tversky_crossentropy(y, logits, **cfg)
    assert np.abs(per_s - per_s0 - 0.25 * S / 30.0).max() <= 1e-15


def test_registry_and_validation():
    from dnncancerannotator_amd import losses
    for name in ('BoundaryCrossentropy', 'boundary_crossentropy'):
        b = losses.get(name)
        assert type(b) is losses.BoundaryCrossentropy and isinstance(b, losses.TverskyCrossentropy)
        assert b.boundary_cfg() == 0.01 and b.region_cfg() == losses.DiceCrossentropy().region_cfg()
    b = losses.get({'class_name': 'BoundaryCrossentropy', 'config': dict(boundary_weight=0.5, alpha=0.3, beta=0.7, weight_mul=3.0)})
    assert b.boundary_cfg() == 0.5 and b.region_cfg()['alpha'] == 0.3 and b.device_cfg() == losses.WeightedCrossentropy(weight_mul=3.0).device_cfg()
    assert losses.get(b) is b
    again = losses.get({'class_name': 'BoundaryCrossentropy', 'config': b.get_config()})
    assert again.get_config() == b.get_config() and again.get_config()['boundary_weight'] == 0.5
    assert not hasattr(losses.TverskyCrossentropy(), 'boundary_cfg')
    for bad in (0.0, -0.01, float('nan'), float('inf'), float('-inf'), '0.01', None, True):
        with pytest.raises(ValueError):
            losses.BoundaryCrossentropy(boundary_weight=bad)
    for bad in (dict(region_weight=0.0), dict(smooth=0.0), dict(alpha=0.0, beta=0.0)):      # the Tversky keys keep their checks
        with pytest.raises(ValueError):
            losses.BoundaryCrossentropy(**bad)


def test_overlay_selects_the_class():
    from dnncancerannotator_amd import load, losses
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    over = load._load_config_single(os.path.join(root, 'configs', 'additionals', 'boundary_loss.yaml'))
    cfg = load._apply_config({'deploy_options': {'loss': {'class_name': 'WeightedCrossentropy', 'config': {'weight_mul': 3.0}}}}, over)
    loss = losses.get(cfg['deploy_options']['loss'])
    assert type(loss) is losses.BoundaryCrossentropy and (loss.alpha, loss.beta, loss.boundary_weight, loss.weight_mul) == (0.5, 0.5, 0.01, 3.0)


OPTS = dict(n_filters_first=3, n_downsample=2, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')


def _config(loss):
    return {'model': 'UNetAnnotator', 'model_options': OPTS,
            'deploy_options': {'optimizer': 'adam', 'loss': loss, 'enable_multigpu': False, 'metrics': []}}


class _BoundaryFake(fake_train_metrics.FakeTrainMetricsDevice):
    def set_region_loss(self, cfg=None, **kw):
        self.loss_calls = getattr(self, 'loss_calls', []) + [('region', dict(cfg or {}, **kw))]

    def set_boundary_loss(self, boundary_weight):
        self.loss_calls = getattr(self, 'loss_calls', []) + [('boundary', boundary_weight)]


def test_engine_sets_the_boundary_loss_behind_the_region_loss(tmp_path, monkeypatch):
    from dnncancerannotator_amd import data, engine
    x, y = O.synthetic_batch(8, 16, 16, 1, seed_x=3, seed_y=4)
    monkeypatch.setenv('DNNCA_NO_FEEDER', '1')
    monkeypatch.setattr(fake_train_metrics, 'FakeTrainMetricsDevice', _BoundaryFake)
    region = dict(region_weight=1.0, crossentropy_weight=1.0, alpha=0.5, beta=0.5, smooth=1.0)
    # a Tversky loss: the region call alone
    built = fake_train_metrics.install(monkeypatch.setattr)
    engine.TFKerasModel(_config({'class_name': 'DiceCrossentropy', 'config': {'weight_mul': 3.0}})).train(
        data.ArrayDataset(x, y, 4, repeat=True), save_path=str(tmp_path / 'a'), max_steps=2, save_freq=100)
    assert len(built) == 1 and built[0].loss_calls == [('region', region)]
    # the new class: region, then boundary, once per device model
    built = fake_train_metrics.install(monkeypatch.setattr)
    m = engine.TFKerasModel(_config({'class_name': 'BoundaryCrossentropy', 'config': {'weight_mul': 3.0, 'boundary_weight': 0.02}}))
    m.train(data.ArrayDataset(x, y, 4, repeat=True), val_data=data.ArrayDataset(x[:4], y[:4], 4), save_path=str(tmp_path / 'b'),
            max_steps=2, save_freq=1)
    assert len(built) == 1 and built[0].loss_calls == [('region', region), ('boundary', 0.02)]
    # a model rebuilt for a bigger batch gets both again
    assert m._ensure_capacity(8)
    assert len(built) == 2 and built[1].loss_calls == [('region', region), ('boundary', 0.02)]
