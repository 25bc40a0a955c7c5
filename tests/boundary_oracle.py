"""numpy statement of the boundary (signed-distance) term of the loss, losses.BoundaryCrossentropy (not a test).

The map.  G = { y > 0.5 } of one H x W plane.  d2(q), an exact integer: for q outside G the smallest (qx - gx)^2 + (qy - gy)^2 over
g in G, for q inside G the smallest over the pixels of the plane outside G; 0 where that other set is empty.
    phi(q) = float32(sqrt(float64(d2)))          outside G
           = float32(1) - float32(sqrt(...))     inside G, in float32 (0 on the inner rim, negative deeper in)
           = 0                                   where the other set is empty (G empty, or G the whole plane)
edt2 computes d2 by the separable definition (a column pass, then the minimum over x' of (x - x')^2 + g(x')^2, in chunks of rows);
edt2_brute by the definition itself, for the small cases.

The loss, in float64 on top of tests/region_loss_ref.py:  S_b = sum_i p_i phi_i,
    L_b = (Tversky + cross-entropy)_b + l_bd S_b / (H W),   dL_b/dlogit_i = ... + l_bd phi_i p_i (1 - p_i) / (H W)
phi comes from the RAW label, also under label_smoothing, and is a constant."""

import numpy as np

import region_loss_ref as R
from oracle import unet_oracle as O

_FAR = 1 << 20                           # a column distance "none": above every real one, its square in int64


def _column_distance(mask):
    """[H, W] int64: rows between a pixel and the nearest True pixel of its column (_FAR: none)"""
    H, W = mask.shape
    rows = np.arange(H, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(mask, rows, -_FAR), axis=0)
    below = np.minimum.accumulate(np.where(mask, rows, 2 * _FAR)[::-1], axis=0)[::-1]
    return np.minimum(np.minimum(rows - above, below - rows), _FAR)


def edt2(mask, chunk_elems=1 << 23):
    """[H, W] int64: squared distance of every pixel to the nearest True pixel of mask; -1 everywhere when mask has none"""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    if not mask.any():
        return np.full((H, W), -1, np.int64)
    g2 = _column_distance(mask) ** 2
    xs = np.arange(W, dtype=np.int64)
    out = np.empty((H, W), np.int64)
    xstep = max(1, min(W, chunk_elems // W))              # a chunk is [rows, x, x'] of at most chunk_elems entries
    rstep = max(1, chunk_elems // (W * xstep))
    for x0 in range(0, W, xstep):
        dx2 = (xs[x0:x0 + xstep, None] - xs[None, :]) ** 2
        for r0 in range(0, H, rstep):
            out[r0:r0 + rstep, x0:x0 + xstep] = (dx2[None, :, :] + g2[r0:r0 + rstep, None, :]).min(axis=2)
    return out


def edt2_brute(mask):
    """the same by the definition: every pixel against every True pixel"""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return np.full((H, W), -1, np.int64)
    qy, qx = np.mgrid[0:H, 0:W]
    d = (qy[..., None] - ys.astype(np.int64)) ** 2 + (qx[..., None] - xs.astype(np.int64)) ** 2
    return d.min(axis=2)


def signed_distance_plane(y, edt=edt2):
    """(phi float32 [H, W], d2 int32 [H, W]) of one label plane"""
    G = np.asarray(y, np.float32) > np.float32(0.5)
    d2 = np.where(G, edt(~G), edt(G))
    none = d2 < 0
    d2 = np.where(none, 0, d2)
    d = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    phi = np.where(G, np.float32(1.0) - d, d).astype(np.float32)
    phi[none] = np.float32(0.0)
    return phi, d2.astype(np.int32)


def signed_distance(y, edt=edt2):
    """(phi float32, d2 int32) of label planes [B, H, W]"""
    y = np.asarray(y)
    planes = [signed_distance_plane(p, edt) for p in y]
    return np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])


def split_cfg(cfg):
    """(the keys of R.tversky_crossentropy, boundary_weight)"""
    cfg = dict(cfg or {})
    return cfg, float(cfg.pop('boundary_weight', 0.01))


def boundary_sums(label, logits):
    """[B] float64: S_b = sum_i p_i phi_i, phi from the raw labels [B, H, W]; logits [B, H, W, 1]"""
    p = 1.0 / (1.0 + np.exp(-np.asarray(logits, np.float64)[..., 0]))
    return (p * signed_distance(label)[0].astype(np.float64)).sum((1, 2))


def boundary_crossentropy(label, logits, **cfg):
    """(per-image loss [B], dloss_b/dlogits [B, H, W, 1]) in float64; cfg: the keys of R.tversky_crossentropy + boundary_weight"""
    rest, bw = split_cfg(cfg)
    logits = np.asarray(logits, np.float64)
    per, dper = R.tversky_crossentropy(label, logits, **rest)
    phi = signed_distance(label)[0].astype(np.float64)
    hw = float(phi.shape[1] * phi.shape[2])
    p = 1.0 / (1.0 + np.exp(-logits[..., 0]))
    per = per + bw * (p * phi).sum((1, 2)) / hw
    dper = dper + (bw * phi * p * (1.0 - p) / hw)[..., None]
    return per, dper


def loss_and_grads(spec, params, x, y, cfg, training=True):
    """R.loss_and_grads with the boundary term: (loss, grads, logits, new_state), one replica"""
    logits, new_state, backward, _ = O.forward(spec, params, x, training=training)
    per, dper = boundary_crossentropy(y, logits, **(cfg or {}))
    B = x.shape[0]
    loss = float(per.mean(dtype=np.float64)) + O.l2_penalty(spec, params)
    _, grads = backward(dper / logits.dtype.type(B))
    if spec.l2:
        for n in grads:
            if n.endswith('.kernel'):
                grads[n] = grads[n] + logits.dtype.type(2.0 * spec.l2) * params[n]
    return loss, grads, logits, new_state
