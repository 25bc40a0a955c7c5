"""float64 statement of losses.TverskyCrossentropy (not a test): the region term beside the oracle's weighted cross-entropy.

Per image b, p = sigmoid(logit), y the label (the blurred one under label_smoothing), sums over that image's pixels:
    I = sum p y, P = sum p, Y = sum y;  N = I + s,  D = (1 - a - b) I + a P + b Y + s,  T = N / D
    L_b = l_ce wBCE_b + l_r (1 - T_b)
    dL_b/dlogit_i = l_ce dwBCE_b/dlogit_i + l_r (C_b - A_b y_i) p_i (1 - p_i),  A_b = (D - (1 - a - b) N) / D^2,  C_b = a N / D^2
"""

import numpy as np

from oracle import unet_oracle as O

REGION_KEYS = ('region_weight', 'crossentropy_weight', 'alpha', 'beta', 'smooth')


def split_cfg(cfg):
    """(the keys of the weighted cross-entropy, the five region values with their defaults)"""
    cfg = dict(cfg or {})
    region = dict(region_weight=1.0, crossentropy_weight=1.0, alpha=0.5, beta=0.5, smooth=1.0)
    for k in REGION_KEYS:
        if k in cfg:
            region[k] = float(cfg.pop(k))
    return cfg, region


def loss_labels(label, cfg):
    """the labels the loss sees, in float64: blurred under label_smoothing and rounded to the labels' own dtype, as
    O.weighted_crossentropy does before it takes the positive rate"""
    ce, _ = split_cfg(cfg)
    label = np.asarray(label)
    if ce.get('label_smoothing'):
        label = O.gaussian_filter2d(label, ce.get('label_smoothing_filter_size', 6), ce.get('label_smoothing_sigma', 3)).astype(label.dtype)
    return label.astype(np.float64)


def region_sums(label, logits):
    """[B, 3]: I, P, Y per image; label [B, H, W] (already blurred if it is to be), logits [B, H, W, 1]"""
    p = 1.0 / (1.0 + np.exp(-np.asarray(logits, np.float64)[..., 0]))
    y = np.asarray(label, np.float64)
    return np.stack([(p * y).sum((1, 2)), p.sum((1, 2)), y.sum((1, 2))], axis=1)


def tversky_index(sums, alpha, beta, smooth):
    I, P, Y = sums[:, 0], sums[:, 1], sums[:, 2]
    return (I + smooth) / ((1.0 - alpha - beta) * I + alpha * P + beta * Y + smooth)


def tversky_crossentropy(label, logits, **cfg):
    """(per-image loss [B], dloss_b/dlogits [B, H, W, 1]) in float64; cfg: the keys of O.weighted_crossentropy + REGION_KEYS"""
    ce, r = split_cfg(cfg)
    logits = np.asarray(logits, np.float64)
    label = np.asarray(label)
    per_ce, dper_ce = O.weighted_crossentropy(label, logits, **ce)
    y = loss_labels(label, cfg)
    a, b, s = r['alpha'], r['beta'], r['smooth']
    p = 1.0 / (1.0 + np.exp(-logits[..., 0]))
    sums = region_sums(y, logits)
    I, P, Y = sums[:, 0], sums[:, 1], sums[:, 2]
    N = I + s
    D = (1.0 - a - b) * I + a * P + b * Y + s
    A = (D - (1.0 - a - b) * N) / D ** 2
    C = a * N / D ** 2
    per = r['crossentropy_weight'] * per_ce + r['region_weight'] * (1.0 - N / D)
    dreg = (C[:, None, None] - A[:, None, None] * y) * p * (1.0 - p)
    dper = r['crossentropy_weight'] * dper_ce + r['region_weight'] * dreg[..., None]
    return per, dper


def loss_and_grads(spec, params, x, y, cfg, training=True):
    """O.loss_and_grads with the compound loss: (loss, grads, logits, new_state), one replica"""
    logits, new_state, backward, _ = O.forward(spec, params, x, training=training)
    per, dper = tversky_crossentropy(y, logits, **(cfg or {}))
    B = x.shape[0]
    loss = float(per.mean(dtype=np.float64)) + O.l2_penalty(spec, params)
    _, grads = backward(dper / logits.dtype.type(B))
    if spec.l2:
        for n in grads:
            if n.endswith('.kernel'):
                grads[n] = grads[n] + logits.dtype.type(2.0 * spec.l2) * params[n]
    return loss, grads, logits, new_state


def train_steps(spec, params, batches, lr, cfg):
    """Adam steps (O.adam_step) over `batches` [(x, y)]: (losses, final params, gradients of the last step)"""
    m, v, losses, grads = {}, {}, [], None
    for t, (x, y) in enumerate(batches, 1):
        loss, grads, _, new_state = loss_and_grads(spec, params, x, y, cfg, training=True)
        params = O.adam_step(params, grads, m, v, t, lr)
        for n, val in new_state.items():
            params[n] = val
        losses.append(loss)
    return losses, params, grads
