"""numpy float32 restatement of the reference's region-based metrics (annotator/utils/metrics.py:80-510, utils/image.py:12-26): the
oracle of tests/test_region_metrics_host.py and tests/test_region_metrics_gpu.py.

Two parts of the reference cannot be run here (no TensorFlow / tensorflow-addons), so they are restated from their definitions:
  * tf.image.resize(method='bilinear', antialias=False) of TF 2.6 (resize_bilinear_op.cc): half-pixel centres, scale = in / out
    as float32, src = (i + 0.5) * scale - 0.5, lo = max(floor(src), 0), hi = min(ceil(src), in - 1), lerp = src - floor(src),
    top = tl + (tr - tl) * xl, bottom = bl + (br - bl) * xl, out = top + (bottom - top) * yl, every operation in float32.
    The target size is tf.cast(tf.cast(size, float16) * resize_factor, int32): a float16 product, truncated.
  * tfa.image.connected_components: 4-connectivity (up, down, left, right neighbours only).  The components here come from a
    union-find of our own (hook roots to the smaller root, compress by pointer jumping), cross-checked against scipy.ndimage.label.
Morphological opening: tf.nn.erosion2d then dilation2d with a zero k x k filter, SAME, out-of-bounds pixels ignored (they are
padding, not zeros); window [y - (k - 1) // 2, y + k // 2] for both.  Matching: IoU = float32(|L n P|) / float32(|L u P|) > theta."""

import numpy as np


def out_size(h, w, rf):
    """metrics.py:196-204: the resized (height, width)"""
    return int(np.float16(h) * np.float16(rf)), int(np.float16(w) * np.float16(rf))


def resize(img, oh, ow):
    """[..., h, w] float32 -> [..., oh, ow]: tf.image.resize bilinear (half-pixel centres); the identity at the same size"""
    img = np.asarray(img, np.float32)
    h, w = img.shape[-2:]
    if (oh, ow) == (h, w):
        return img

    def axis(n_in, n_out):
        scale = np.float32(np.float32(n_in) / np.float32(n_out))
        src = (np.arange(n_out, dtype=np.float32) + np.float32(0.5)) * scale - np.float32(0.5)
        fl = np.floor(src)
        lo = np.maximum(fl.astype(np.int64), 0)
        hi = np.minimum(np.ceil(src).astype(np.int64), n_in - 1)
        return lo, hi, (src - fl).astype(np.float32)

    y0, y1, ly = axis(h, oh)
    x0, x1, lx = axis(w, ow)
    tl, tr = img[..., y0, :][..., x0], img[..., y0, :][..., x1]
    bl, br = img[..., y1, :][..., x0], img[..., y1, :][..., x1]
    top = tl + (tr - tl) * lx
    bot = bl + (br - bl) * lx
    return (top + (bot - top) * ly[:, None]).astype(np.float32)


def _window(mask, k, op, pad):
    """op (AND / OR) over the k x k window of every pixel of [..., H, W]; out-of-bounds pixels take the identity `pad`"""
    lo = (k - 1) // 2
    H, W = mask.shape[-2:]
    p = np.full(mask.shape[:-2] + (H + k - 1, W + k - 1), pad, bool)
    p[..., lo:lo + H, lo:lo + W] = mask
    r = p[..., :, 0:W].copy()
    for d in range(1, k):
        r = op(r, p[..., :, d:d + W])
    out = r[..., 0:H, :].copy()
    for d in range(1, k):
        out = op(out, r[..., d:d + H, :])
    return out


def morph_open(mask, k):
    """utils/image.py:12-26 on boolean masks [..., H, W]"""
    return _window(_window(mask, k, np.logical_and, True), k, np.logical_or, False)


def ccl(mask):
    """4-connected components of every [H, W] plane of `mask` [..., H, W]: parent array of the same shape holding the flat index
    (over the whole array) of the component's root = its smallest pixel index; -1 for background"""
    mask = np.asarray(mask, bool)
    H, W = mask.shape[-2:]
    flat = mask.ravel()
    idx = np.arange(flat.size, dtype=np.int64).reshape(mask.shape)
    edges = []
    h = mask[..., :, 1:] & mask[..., :, :-1]
    edges.append((idx[..., :, 1:][h], idx[..., :, :-1][h]))
    v = mask[..., 1:, :] & mask[..., :-1, :]
    edges.append((idx[..., 1:, :][v], idx[..., :-1, :][v]))
    a = np.concatenate([e[0] for e in edges])
    b = np.concatenate([e[1] for e in edges])
    P = np.arange(flat.size, dtype=np.int64)
    while True:
        while True:                                   # compress: every pixel points at its root
            Q = P[P]
            if np.array_equal(Q, P):
                break
            P = Q
        ra, rb = P[a], P[b]
        diff = ra != rb
        if not diff.any():
            break
        lo_, hi_ = np.minimum(ra[diff], rb[diff]), np.maximum(ra[diff], rb[diff])
        np.minimum.at(P, hi_, lo_)                    # union: the larger root hooks to the smaller one
    out = np.where(flat, P, -1)
    return out.reshape(mask.shape)


def region_counts(prob, y, thresholds, iou=0.30, rf=1.0, k=5):
    """prob, y [B, H, W] -> int64 [T, 4]: (tp_label, fn, tp_pred, fp) per threshold, summed over the slices"""
    prob = np.asarray(prob, np.float32)
    y = np.asarray(y, np.float32)
    if prob.ndim == 4:
        prob = prob[..., 0]
    thr = np.atleast_1d(np.asarray(thresholds, np.float32)).ravel()
    if not 0.0 <= iou < 1.0:
        raise ValueError('IoU threshold outside [0, 1)')
    B, H, W = y.shape
    oh, ow = out_size(H, W, rf)
    lab = resize(y, oh, ow) > np.float32(0.5)                         # [B, oh, ow]
    pr = resize(prob, oh, ow)
    T = thr.size
    pm = pr[None] >= thr[:, None, None, None]                          # [T, B, oh, ow]
    if k > 1:
        pm = morph_open(pm, k)
    LL = ccl(lab).ravel()                                              # label roots: flat index over [B, oh, ow]
    LP = ccl(pm).ravel()                                               # prediction roots: flat index over [T, B, oh, ow]
    n = B * oh * ow
    SL = np.bincount(LL[LL >= 0], minlength=n)
    SP = np.bincount(LP[LP >= 0], minlength=T * n)
    LLt = np.tile(LL, T)
    both = (LP >= 0) & (LLt >= 0)
    keys = LLt[both] * (T * n) + LP[both]
    uk, inter = np.unique(keys, return_counts=True)
    rl, rp = uk // (T * n), uk % (T * n)
    union = SL[rl] + SP[rp] - inter
    hit = (inter.astype(np.float32) / union.astype(np.float32)) > np.float32(iou)
    t_of = rp // n
    label_roots = int((LL == np.arange(n)).sum())
    pred_roots = np.bincount(np.nonzero(LP == np.arange(T * n))[0] // n, minlength=T)
    out = np.zeros((T, 4), np.int64)
    for t in range(T):
        sel = hit & (t_of == t)
        tp_l = np.unique(rl[sel]).size
        tp_p = np.unique(rp[sel]).size
        out[t] = (tp_l, label_roots - tp_l, tp_p, pred_roots[t] - tp_p)
    return out
