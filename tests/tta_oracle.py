"""numpy oracle of the test-time-augmentation views (include/dnnca.h, dnnca_forward_tta).

A view is k = 4 t + 2 v + h in 0..7: flip the rows (v) and the columns (h), then (t) transpose.  apply_view takes a batch to its
view, invert_view takes a plane computed ON the view back to the original pixels, mean_of averages the mapped-back planes the way
the device does: float32 sum in ascending view order, float32 division."""

import numpy as np


def views_of(mask):
    """the views of a bit mask, ascending"""
    return [k for k in range(8) if mask >> k & 1]


def apply_view(x, k):
    """x [B, H, W, C] -> view k of it (H == W for k >= 4)"""
    x = np.asarray(x)
    if k & 2:
        x = x[:, ::-1]
    if k & 1:
        x = x[:, :, ::-1]
    if k & 4:
        x = np.swapaxes(x, 1, 2)
    return np.ascontiguousarray(x)


def invert_view(p, k):
    """p [B, H, W], a plane in the geometry of view k -> the original geometry: out[b,i,j] = p[b, t ? (j',i') : (i',j')]"""
    p = np.asarray(p)
    if k & 4:
        p = np.swapaxes(p, 1, 2)
    if k & 2:
        p = p[:, ::-1]
    if k & 1:
        p = p[:, :, ::-1]
    return np.ascontiguousarray(p)


def mean_of(planes, views):
    """planes [n, B, H, W]: the selected views' planes, each in its own view's geometry, in ascending view order; `views`: the mask"""
    ks = views_of(views)
    planes = np.asarray(planes, np.float32)
    assert len(planes) == len(ks)
    acc = invert_view(planes[0], ks[0]).astype(np.float32)
    for p, k in zip(planes[1:], ks[1:]):
        acc = (acc + invert_view(p, k)).astype(np.float32)
    return (acc / np.float32(len(ks))).astype(np.float32)
