"""CPU: the host side of MultiResUnet (models.MultiResUnet, configs/multiresunet.yaml) and its float64 reference statement
(tests/multires_ref.py): block widths, variable names and order, the refusals, and the reference against a known answer."""

import numpy as np
import pytest
import torch

import multires_ref as R
from dnncancerannotator_amd import engine, models

DEPLOY = {'optimizer': 'adam', 'enable_multigpu': False}


def test_block_widths_of_the_reference_and_of_the_small_model():
    # W = 1.67 U; int(W * 0.167), int(W * 0.333), int(W * 0.5) in double
    want32 = [(8, 17, 26), (17, 35, 53), (35, 71, 106), (71, 142, 213), (142, 284, 427)]
    assert models.multires_widths(32) == want32
    assert [sum(w) for w in want32] == [51, 105, 212, 426, 853]
    assert models.multires_widths(4) == [(1, 2, 3), (2, 4, 6), (4, 8, 13), (8, 17, 26), (17, 35, 53)]
    for level in range(5):
        assert R.widths(32 << level) == want32[level]


def test_variable_names_count_and_order():
    specs = R.param_specs(5, 32)
    names = [n for n, s, t in specs]
    assert len(names) == len(set(names))
    # the first block, in the order in which the reference's code calls its layers
    assert names[:24] == [
        'block1.shortcut.kernel', 'block1.shortcut.bn.beta', 'block1.shortcut.bn.moving_mean', 'block1.shortcut.bn.moving_variance',
        'block1.conv3.kernel', 'block1.conv3.bn.beta', 'block1.conv3.bn.moving_mean', 'block1.conv3.bn.moving_variance',
        'block1.conv5.kernel', 'block1.conv5.bn.beta', 'block1.conv5.bn.moving_mean', 'block1.conv5.bn.moving_variance',
        'block1.conv7.kernel', 'block1.conv7.bn.beta', 'block1.conv7.bn.moving_mean', 'block1.conv7.bn.moving_variance',
        'block1.cat_bn.gamma', 'block1.cat_bn.beta', 'block1.cat_bn.moving_mean', 'block1.cat_bn.moving_variance',
        'block1.out_bn.gamma', 'block1.out_bn.beta', 'block1.out_bn.moving_mean', 'block1.out_bn.moving_variance']
    assert names[24] == 'respath1.0.shortcut.kernel' and names[-4:] == ['head.kernel', 'head.bn.beta', 'head.bn.moving_mean',
                                                                       'head.bn.moving_variance']
    shapes = {n: s for n, s, t in specs}
    assert shapes['block1.shortcut.kernel'] == (1, 1, 5, 51) and shapes['block1.conv5.kernel'] == (3, 3, 8, 17)
    assert shapes['respath1.3.conv.kernel'] == (3, 3, 32, 32) and shapes['respath4.0.shortcut.kernel'] == (1, 1, 426, 256)
    assert shapes['up6.tconv.kernel'] == (2, 2, 256, 853) and shapes['up6.tconv.bias'] == (256,)
    assert shapes['block6.shortcut.kernel'] == (1, 1, 512, 426) and shapes['block9.conv3.kernel'] == (3, 3, 64, 8)
    assert shapes['head.kernel'] == (1, 1, 51, 1)
    # 9 blocks x 6 BatchNorms + 10 ResPath units x 3 + the head's; no conv has a bias, only the transposed convs do
    assert sum(n.endswith('.moving_mean') for n in names) == 9 * 6 + 10 * 3 + 1
    assert sum(n.endswith('.gamma') for n in names) == 9 * 2 + 10
    assert [n for n in names if n.endswith('.bias')] == ['up%d.tconv.bias' % u for u in (6, 7, 8, 9)]
    order = [n.split('.')[0] for n in names]
    assert list(dict.fromkeys(order)) == ['block1', 'respath1', 'block2', 'respath2', 'block3', 'respath3', 'block4', 'respath4', 'block5',
                                          'up6', 'block6', 'up7', 'block7', 'up8', 'block8', 'up9', 'block9', 'head']
    lay, (nt, ns) = R.layout(5, 32)
    assert nt + ns == sum(int(np.prod(s)) for s in shapes.values())


def test_constructor_and_config_round_trip():
    m = models.MultiResUnet(height=None, width=None, n_channels=5)
    assert m.arch == 'multires' and m.get_config() == dict(height=None, width=None, n_channels=5)
    again = models.MultiResUnet.from_config(m.get_config())
    assert again.get_config() == m.get_config() and again.n_filters_first == 32
    small = models.MultiResUnet(32, 32, 5, n_filters_first=4)
    assert models.MultiResUnet.from_config(small.get_config()).n_filters_first == 4


def test_refusals_before_the_device_is_touched(monkeypatch):
    with pytest.raises(NotImplementedError, match='n_channels'):
        models.MultiResUnet()
    with pytest.raises(NotImplementedError, match='n_channels'):
        models.MultiResUnet(height=32, width=32)
    with pytest.raises(ValueError, match='n_filters_first'):
        models.MultiResUnet(n_channels=5, n_filters_first=2)          # c1 = int(3.34 * 0.167) = 0
    with pytest.raises(ValueError, match='bf16'):
        models.MultiResUnet(n_channels=5, dtype='bf16')
    with pytest.raises(ValueError, match='kernel_regularizer'):
        models.MultiResUnet(n_channels=5, kernel_regularizer=None)
    with pytest.raises(ValueError, match='activation'):
        models.MultiResUnet(n_channels=5, activation='relu')

    def no_device(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(models.device, 'DeviceModel', no_device)
    with pytest.raises(ValueError, match='n_channels'):
        models.MultiResUnet(n_channels=5).build([2, 32, 32, 4])
    with pytest.raises(ValueError, match='height'):
        models.MultiResUnet(height=64, n_channels=5).build([2, 32, 32, 5])
    with pytest.raises(ValueError, match='width'):
        models.MultiResUnet(width=64, n_channels=5).build([2, 32, 32, 5])
    with pytest.raises(ValueError, match='multiples of 16'):
        models.MultiResUnet(n_channels=5).build([2, 24, 32, 5])
    with pytest.raises(ValueError, match='multiples of 16'):
        models.MultiResUnet(n_channels=5).build([2, 32, 40, 5])


def test_engine_resolves_the_model_and_refuses_sensitivity(tmp_path):
    cfg = dict(model='MultiResUnet', model_options=dict(height=None, width=None, n_channels=5), deploy_options=dict(DEPLOY))
    e = engine.TFKerasModel(cfg)
    assert isinstance(e.model, models.MultiResUnet)
    with pytest.raises(NotImplementedError, match='visualize_sensitivity'):
        e.eval(None, str(tmp_path), visualize_sensitivity=True)          # before the dataset or the device is looked at


def test_reference_statement_on_a_hand_computed_join():
    """one ResPath unit, 1 -> 1 channel, every kernel weight 1, on a 2 x 2 image, inference mode with moving mean 0 and moving
    variance 1 - eps (so the BatchNorms without gamma are the identity): s = x; o = relu(sum of the image) = relu(-2) = 0;
    r = relu(s + o) = relu(x); out = 2 r + 1"""
    one = lambda v: torch.tensor([v], dtype=torch.float64)
    P = {}
    for conv in ('u.0.shortcut', 'u.0.conv'):
        k = 1 if conv.endswith('shortcut') else 3
        P[conv + '.kernel'] = torch.ones(k, k, 1, 1, dtype=torch.float64)
        P[conv + '.bn.beta'], P[conv + '.bn.moving_mean'], P[conv + '.bn.moving_variance'] = one(0.0), one(0.0), one(1.0 - R.EPS)
    P['u.0.out_bn.gamma'], P['u.0.out_bn.beta'] = one(2.0), one(1.0)
    P['u.0.out_bn.moving_mean'], P['u.0.out_bn.moving_variance'] = one(0.0), one(1.0 - R.EPS)
    g = R._Graph(P, training=False)
    x = torch.tensor([[1.0, -2.0], [3.0, -4.0]], dtype=torch.float64)[None, None]
    out = g.respath('u', 1, 1, x, 1)[0, 0].numpy()
    np.testing.assert_allclose(out, [[3.0, 1.0], [7.0, 1.0]], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(g.tap['u.0.join'][0, 0].numpy(), [[1.0, 0.0], [3.0, 0.0]])
    # a positive image: o = 10 everywhere, out = 2 (x + 10) + 1
    g = R._Graph(P, training=False)
    out = g.respath('u', 1, 1, x.abs(), 1)[0, 0].numpy()
    np.testing.assert_allclose(out, [[23.0, 25.0], [27.0, 29.0]], rtol=0, atol=1e-12)
    # training mode: the output BatchNorm normalises relu(x) = [1, 0, 3, 0] with its batch statistics (mean 1, variance 1.5)
    g = R._Graph(P, training=True)
    g.bn('u.0.out_bn', torch.tensor([[1.0, 0.0], [3.0, 0.0]], dtype=torch.float64)[None, None], 1)
    np.testing.assert_allclose(g.state['u.0.out_bn.moving_mean'], [0.01], atol=1e-15)
    np.testing.assert_allclose(g.state['u.0.out_bn.moving_variance'], [(1.0 - R.EPS) * 0.99 + 0.01 * 1.5 * 4 / 3], atol=1e-15)


def test_reference_gradients_of_a_scale_less_batchnorm_do_not_see_a_gamma():
    lay, (nt, ns) = R.layout(5, 4)
    p, s = R.init(5, 4, seed=0, perturb=0.1)
    assert p.size == nt and s.size == ns
    x = np.random.default_rng(1).standard_normal((1, 16, 16, 5)).astype(np.float32)
    r = R.run(p, s, x, R.discs(1, 16, 16, 2), n_filters_first=4, training=True)
    assert r['logits'].shape == (1, 16, 16, 1) and np.isfinite(r['loss']) and r['grads'].shape == (nt,)
    assert not any(n.endswith('conv3.bn.gamma') for n in lay)
    # the bottom level of a 16 x 16 image is 1 x 1: its batch variance over one pixel is 0, the network still runs
    assert np.all(np.isfinite(r['grads'])) and np.all(np.isfinite(r['state']))
