"""-m gpu: the step kernels' stores go through csrc/store_dev.h (raw-buffer stores, one descriptor per image or tensor, lanes that must
not store get an out-of-range offset).  Same values to the same addresses as before: a train step against the float64 oracle on
shapes that exercise every length of the last strip's row, the image base of the per-image descriptors and whole MFMA tiles;
run-to-run determinism of the forward pass (overlapping or spilled stores show up as differences); the launchers' size predicate."""

import numpy as np
import pytest

import helpers as Hp
from oracle import unet_oracle as O

UNET = dict(n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')
# last strip of 4, 12, 60 (two shapes: one and two strips) and 32 columns; one, two and three images; (3, 32, 128): whole 128 x 32
# tiles, the block-fused backward launches are planned
SHAPES = [(1, 8, 64), (3, 16, 72), (2, 24, 120), (2, 16, 152), (3, 32, 128)]


def _batch(B, H, W):
    rng = np.random.default_rng(23)
    x = rng.random((B, H, W, 1)).astype(np.float32)
    y = (rng.random((B, H, W)) < 0.05).astype(np.float32)
    return x, y


@pytest.mark.gpu
@pytest.mark.parametrize('B, H, W', SHAPES)
def test_train_step_through_the_store_helper_against_oracle(gpu, B, H, W):
    """configs/unet.yaml widths, one train step at lr 0 against the float64 oracle: loss 1e-4, every gradient tensor 2e-5 of its own
    scale (+ 10 x what plain float32 numpy costs that tensor), as test_vector_alu_kernels_of_the_3_channel_level_against_oracle."""
    spec = O.ModelSpec('unet', 1, **UNET)
    params = Hp.perturbed_params(spec, np.float64)
    x, y = _batch(B, H, W)
    cfg = dict(weight_mul=3.0)
    loss, grads, _, _ = O.loss_and_grads(spec, params, x.astype(np.float64), y, cfg, training=True)
    m = gpu.DeviceModel('unet', 1, H, W, B, **UNET)
    m.set_params(O.flatten(spec, params))
    out = m.train_step(x, y, 0.0, m.loss_cfg(**cfg))
    g = m.get_grads()
    plan = set(r[0] for r in m.plan())
    m.close()
    p32 = {n: v.astype(np.float32) for n, v in params.items()}
    _, g32, _, _ = O.loss_and_grads(spec, p32, x, y, cfg, training=True)
    gref, g32 = O.flatten(spec, grads), O.flatten(spec, g32).astype(np.float64)
    floor = [10 * np.abs(g32[sl] - gref[sl]).max() for _, sl in Hp.tensor_slices(spec)]
    errs = Hp.per_tensor_err(spec, g, gref)
    print('(%d, %d, %d): loss %.8f oracle %.8f; worst tensor %.2e; plan %s' % (B, H, W, out.loss, loss, max(errs.values()), sorted(plan)))
    assert abs(out.loss - loss) <= 1e-4 * max(1.0, abs(loss))
    Hp.assert_grads_per_tensor(spec, g, gref, 2e-5, floor=floor)
    assert {'first3_fwd', 'up3_fwd', 'tail3_3x1_3'} <= plan, plan
    if (B, H, W) == (3, 32, 128):
        assert {'fzb_up_6', 'fzb_up_12', 'fzb_down_6_12', 'fzb_down_3_6', 'pgbwd_tc_3x2_3'} <= plan, plan


@pytest.mark.gpu
@pytest.mark.parametrize('B, H, W', SHAPES)
def test_forward_is_bit_identical_from_run_to_run(gpu, B, H, W):
    """The forward pass has no atomics: three runs on one model give the same bits.  Two stores that overlap at a strip or tile seam
    with different values, or spill past a row's end, make runs differ."""
    x, _ = _batch(B, H, W)
    m = gpu.DeviceModel('unet', 1, H, W, B, **UNET)
    m.init_glorot(seed=2)
    outs = [np.array(m.forward(x, training=False), copy=True) for _ in range(3)]
    m.close()
    assert np.isfinite(outs[0]).all() and outs[0].shape[:3] == (B, H, W)
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


@pytest.mark.gpu
def test_launchers_decline_images_of_2_to_the_31_bytes():
    """The kernels address an image with a 32-bit byte offset through one buffer descriptor; the launchers' predicate (a host function
    of the C ABI: nothing is allocated) accepts an image while its bytes stay below 2^31."""
    from dnncancerannotator_amd import _lib
    fits = _lib.load().dnnca_store_image_fits
    assert fits(512, 512, 12) == 1
    assert fits(8192, 8192, 6) == 1                        # 1.5 GiB
    assert fits(1 << 13, 1 << 13, 8) == 0                  # exactly 2^31 bytes
    assert fits((1 << 13) - 1, 1 << 13, 8) == 1            # one row less
    assert fits(1 << 14, 1 << 14, 3) == 0                  # 3 GiB
    assert fits(1 << 31, 1 << 31, 12) == 0 and fits(1 << 40, 1, 1) == 0      # no overflow in the product
    assert fits(0, 512, 3) == 0 and fits(512, -1, 3) == 0
