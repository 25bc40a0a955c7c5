"""float64 statement of random_affine's resampling (dnnca_affine_f32, launch `aug_affine`), shared by test_affine_host.py and
test_affine_gpu.py.

Output pixel q = (row, column) of image b is sampled at s = L_b q + o_b with mats[b] = [[L00, L01, o0], [L10, L11, o1]].  The cell is
floor(s), the fractions are s - floor(s); the four taps are blended along the row, then along the column; a tap whose row or
column lies outside the plane is 0.  Everything here is float64: the device rounds each fraction to float32 once and every blend
three times (a subtraction, a product, a sum -- or two with a fused multiply-add) over two levels of blends, which is where the
tests' bound of 8 * 2^-24 * max|tap| comes from."""

import numpy as np

BOUND = 8.0 * 2.0 ** -24           # times max|tap|


def positions(mats, h, w):
    """s [B, h, w, 2] float64"""
    mats = np.asarray(mats, np.float64)
    qy, qx = np.mgrid[:h, :w].astype(np.float64)
    return (mats[:, None, None, :, 0] * qy[None, :, :, None] + mats[:, None, None, :, 1] * qx[None, :, :, None]) + mats[:, None, None, :, 2]


def _taps(plane, iy, ix):
    """plane [B, h, w, C] at integer positions iy, ix [B, h, w] (float64, any size): 0 outside"""
    B, h, w, _ = plane.shape
    inside = (iy >= 0) & (iy <= h - 1) & (ix >= 0) & (ix <= w - 1)
    cy = np.where(inside, iy, 0).astype(np.int64)
    cx = np.where(inside, ix, 0).astype(np.int64)
    b = np.arange(B)[:, None, None]
    return np.where(inside[..., None], plane[b, cy, cx], 0.0)


def affine(x, y, mats):
    """x [B, h, w, C], y [B, h, w] -> (x', y') float64 under mats [B, 2, 3]"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    planes = np.concatenate([x, y[..., None]], -1)
    s = positions(mats, *y.shape[1:])
    f = np.floor(s)
    a = s - f
    ay, ax = a[..., 0:1], a[..., 1:2]
    tl, tr = _taps(planes, f[..., 0], f[..., 1]), _taps(planes, f[..., 0], f[..., 1] + 1)
    bl, br = _taps(planes, f[..., 0] + 1, f[..., 1]), _taps(planes, f[..., 0] + 1, f[..., 1] + 1)
    top, bot = ax * (tr - tl) + tl, ax * (br - bl) + bl
    out = ay * (bot - top) + top
    return out[..., :-1], out[..., -1]


def matrix(h, w, theta_deg=0.0, z=1.0, t=(0.0, 0.0), g=None):
    """[2, 3] for a rotation by theta about the centre, zoom z, shift t and an integer 2 x 2 matrix g, composed as draw_affine does:
    L = g R(-theta) / z, o = c - L (c + t)"""
    c = np.array([(h - 1) / 2.0, (w - 1) / 2.0])
    th = np.deg2rad(theta_deg)
    r = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]]) if theta_deg else np.eye(2)
    lin = (np.eye(2) if g is None else np.asarray(g, np.float64)) @ r / z
    return np.concatenate([lin, (c - lin @ (c + np.asarray(t, np.float64)))[:, None]], 1)


def d4_numpy(a, k):
    """view k = 4 t + 2 v + h of tta.py of planes a [..., h, w, C?] with the plane axes at 1, 2: numpy flips, then the transpose"""
    if k & 2:
        a = np.flip(a, 1)
    if k & 1:
        a = np.flip(a, 2)
    if k & 4:
        a = np.swapaxes(a, 1, 2)
    return np.ascontiguousarray(a)
