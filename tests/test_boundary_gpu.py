"""-m gpu: the signed distance transform of the boundary loss alone (boundary_cols, boundary_rows), through
DeviceModel.signed_distance_of: d2 EQUAL and phi BIT-EQUAL to the numpy oracle of tests/boundary_oracle.py.

Shapes, chosen for where the two kernels can go wrong: 1 x 1; 1 x 70 (one row: no vertical neighbour); 70 x 1 (one column);
33 x 65 (one past the 32-row word of the column pass and the 64-lane wave); 97 x 130 (four row pieces, ragged block edges of the 16
columns a block of the column pass takes); 512 x 512 once (the far walk: one foreground pixel in a corner gives the far corner
d2 = 2 * 511^2, its complement has one background pixel); rows of 8192 and 8193 pixels (the last row that is staged in LDS and the
first that is read from global memory).  Patterns per small shape: empty, full, one pixel in each corner, a checkerboard, Bernoulli
at 0.5 and 0.01, a lesion on two borders, foreground in the top row only, labels of exactly 0.5 and nextafter(0.5, 1)."""

import numpy as np
import pytest

import boundary_oracle as BO

pytestmark = pytest.mark.gpu

MAXB = 4
SMALL = [(1, 1), (1, 70), (70, 1), (33, 65), (97, 130)]


@pytest.fixture(scope='module')
def model(gpu):
    """any model will do: signed_distance_of touches none of its tensors"""
    m = gpu.DeviceModel('unet', 1, 16, 16, MAXB, n_filters_first=3, n_downsample=1, rate=2, kernel_size=3, conv_stride=1, bn=False,
                        padding='same')
    yield m
    m.close()


def patterns(H, W, seed=5):
    """{name: label plane [H, W] float32}"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    out = {'empty': np.zeros((H, W), np.float32), 'full': np.ones((H, W), np.float32)}
    for name, (r, c) in dict(tl=(0, 0), tr=(0, W - 1), bl=(H - 1, 0), br=(H - 1, W - 1)).items():
        out['corner_' + name] = np.zeros((H, W), np.float32)
        out['corner_' + name][r, c] = 1.0
    yy, xx = np.mgrid[0:H, 0:W]
    out['checkerboard'] = ((yy + xx) % 2).astype(np.float32)
    out['bernoulli_0.5'] = (rng.random((H, W)) < 0.5).astype(np.float32)
    out['bernoulli_0.01'] = (rng.random((H, W)) < 0.01).astype(np.float32)
    out['two_borders'] = np.zeros((H, W), np.float32)
    out['two_borders'][H - (H + 3) // 4:, :(W + 3) // 4] = 1.0
    out['top_row'] = np.zeros((H, W), np.float32)
    out['top_row'][0, ::3] = 1.0                               # every column's "above" is the sentinel, two of three have none at all
    half = np.full((H, W), 0.5, np.float32)                    # 0.5 is background ...
    half[rng.random((H, W)) < 0.2] = np.nextafter(np.float32(0.5), np.float32(1.0))      # ... the next float is foreground
    out['half'] = half
    return out


def check(model, planes, what):
    """planes [n, H, W]: one call per MAXB planes; d2 equal, phi bit-equal to the oracle"""
    planes = np.asarray(planes, np.float32)
    want_phi, want_d2 = BO.signed_distance(planes)
    for b0 in range(0, len(planes), MAXB):
        phi, d2 = model.signed_distance_of(planes[b0:b0 + MAXB], want_d2=True)
        assert phi.dtype == np.float32 and d2.dtype == np.int32 and phi.shape == planes[b0:b0 + MAXB].shape
        bad = np.argwhere(d2 != want_d2[b0:b0 + MAXB])
        assert bad.size == 0, '%s: d2 differs at %d pixels, first (plane, y, x) %s: %d, oracle %d' % (
            what, len(bad), bad[0] + [b0, 0, 0], d2[tuple(bad[0])], want_d2[b0:b0 + MAXB][tuple(bad[0])])
        assert np.array_equal(phi.view(np.uint32), want_phi[b0:b0 + MAXB].view(np.uint32)), what
        only_phi = model.signed_distance_of(planes[b0:b0 + MAXB])          # d2_out == NULL: the same map
        assert np.array_equal(only_phi.view(np.uint32), phi.view(np.uint32)), what


@pytest.mark.parametrize('shape', SMALL, ids=lambda s: '%dx%d' % s)
def test_every_pattern_matches_the_oracle(model, shape):
    pats = patterns(*shape)
    check(model, list(pats.values()), '%dx%d %s' % (shape + (list(pats),)))
    phi = model.signed_distance_of(np.stack([pats['empty'], pats['full']]))
    assert not phi.any()                                        # the term vanishes on a healthy slice and on a full one


def test_far_walk_at_512(model):
    """one foreground pixel in the top left corner, and the complement (one background pixel): every walk is as long as it can be"""
    one = np.zeros((512, 512), np.float32)
    one[0, 0] = 1.0
    check(model, [one, 1.0 - one], '512x512')
    phi, d2 = model.signed_distance_of(np.stack([one, 1.0 - one]), want_d2=True)
    assert d2[0, 511, 511] == 2 * 511 ** 2 and d2[1, 511, 511] == 2 * 511 ** 2 and d2[0, 0, 0] == 1 and d2[1, 0, 0] == 1
    assert phi[0, 511, 511] == np.float32(np.sqrt(2.0 * 511 ** 2)) and phi[1, 511, 511] == np.float32(1.0) - phi[0, 511, 511]
    assert phi[0, 0, 0] == 0.0 and phi[1, 0, 0] == 1.0


@pytest.mark.parametrize('shape', [(1, 8192), (2, 8193)], ids=lambda s: '%dx%d' % s)
def test_rows_at_the_lds_limit(model, shape):
    """8192 pixels: the widest row that is staged in LDS; 8193: the first that the walk reads from global memory"""
    rng = np.random.default_rng(shape[1])
    y = (rng.random(shape) < 0.01).astype(np.float32)
    y[0, :700] = 0.0                                            # a long walk at the left edge
    check(model, [y], '%dx%d' % shape)


def test_a_batch_does_not_leak_between_images_and_repeats_bit_for_bit(model):
    H, W = 33, 65
    pats = patterns(H, W, seed=9)
    three = np.stack([pats['bernoulli_0.01'], pats['empty'], pats['two_borders']])
    phi, d2 = model.signed_distance_of(three, want_d2=True)
    for b in range(3):
        phi_b, d2_b = model.signed_distance_of(three[b:b + 1], want_d2=True)
        assert np.array_equal(d2[b], d2_b[0]) and np.array_equal(phi[b].view(np.uint32), phi_b[0].view(np.uint32))
    assert not phi[1].any() and not d2[1].any()
    model.signed_distance_of(np.ones((MAXB, 97, 130), np.float32))          # other sizes in between: the scratch is reused
    phi2, d22 = model.signed_distance_of(three, want_d2=True)
    assert np.array_equal(phi.view(np.uint32), phi2.view(np.uint32)) and np.array_equal(d2, d22)
    check(model, three, 'batch of 3')


def test_the_library_checks_the_planes(gpu, model):
    with pytest.raises(gpu._lib.DnncaError):
        model.signed_distance_of(np.zeros((MAXB + 1, 4, 4), np.float32))     # more planes than the model's batch
    with pytest.raises(gpu._lib.DnncaError):
        model.signed_distance_of(np.zeros((1, 1, 16385), np.float32))        # above kSurfaceMaxSide
    with pytest.raises(ValueError):
        model.signed_distance_of(np.zeros((4, 4), np.float32))
    check(model, [np.eye(5, 7, dtype=np.float32)], 'after the refusals')
