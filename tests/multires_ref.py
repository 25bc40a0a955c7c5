"""Torch-CPU (autograd) statement of MultiResUnet (models/tf_models/multiresunet.py), in the manner of tests/torch_ref.py: the
float64 reference of the GPU tests, and -- run in float32 -- "what plain float32 costs".  Test infrastructure: the product never
imports it.

    conv2d_bn(x, f, k, act)  conv k x k, same, no bias -> BatchNorm without gamma (eps 1e-3, momentum 0.99) -> relu | nothing
    MultiResBlock(U, inp)    W = 1.67 U; shortcut = conv2d_bn 1x1 (c1 + c2 + c3, none); a, b, c = conv2d_bn 3x3 chained (relu);
                             out = BN(concat[a, b, c]); out = BN(relu(shortcut + out))
    ResPath(f, length, x)    length x { s = conv2d_bn 1x1 (none); o = conv2d_bn 3x3 (relu); x = BN(relu(s + o)) }

Variables in the order in which the reference's code calls its layers; trainable and non-trainable ones are two flat vectors, each
in that order (the layout of DeviceModel.get_params / get_state).  Layout: Conv2D HWIO, Conv2DTranspose [kh, kw, Cout, Cin]."""

from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import unet_oracle as O

EPS, MOMENTUM = 1e-3, 0.99


def widths(U):
    w = 1.67 * U
    return int(w * 0.167), int(w * 0.333), int(w * 0.5)


class _Graph:
    """Walks the network once.  With tensors (`P`: name -> tensor) it computes; without, it only lists the variables."""

    def __init__(self, P=None, training=False):
        self.P, self.training = P, training
        self.specs = []                  # (name, shape, trainable)
        self.state = OrderedDict()       # new moving statistics (training)
        self.decisions = []              # every ReLU mask and max-pool argmax, in call order
        self.pre = []                    # what they were taken on: ('relu', pre-activation) / ('pool', the pooled tensor), in call order
        self.tap = OrderedDict()         # named intermediate tensors

    def _var(self, name, shape, trainable=True):
        self.specs.append((name, tuple(shape), trainable))
        return None if self.P is None else self.P[name]

    def relu(self, t):
        if t is None:
            return None
        self.decisions.append((t > 0).detach().numpy().copy())
        self.pre.append(('relu', t.detach().numpy().copy()))
        return F.relu(t)

    def bn(self, prefix, t, c, gamma=True):
        g = self._var(prefix + '.gamma', [c]) if gamma else None
        b = self._var(prefix + '.beta', [c])
        mm = self._var(prefix + '.moving_mean', [c], False)
        mv = self._var(prefix + '.moving_variance', [c], False)
        if t is None:
            return None
        if self.training:
            n = t.shape[0] * t.shape[2] * t.shape[3]
            mean = t.mean((0, 2, 3))
            var = t.var((0, 2, 3), unbiased=False)
            self.state[prefix + '.moving_mean'] = (mm * MOMENTUM + mean * (1 - MOMENTUM)).detach().numpy()
            self.state[prefix + '.moving_variance'] = (mv * MOMENTUM + var * (n / max(n - 1, 1)) * (1 - MOMENTUM)).detach().numpy()
        else:
            mean, var = mm, mv
        t = (t - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + EPS)
        if gamma:
            t = t * g[None, :, None, None]
        return t + b[None, :, None, None]

    def conv_bn(self, prefix, t, cin, cout, k, act):
        w = self._var(prefix + '.kernel', [k, k, cin, cout])
        if t is not None:
            t = F.conv2d(t, w.permute(3, 2, 0, 1).contiguous(), None, padding=(k - 1) // 2)
        t = self.bn(prefix + '.bn', t, cout, gamma=False)
        return self.relu(t) if act else t

    def join_bn(self, prefix, s, o, c):
        r = None if s is None else self.relu(s + o)
        if r is not None:
            self.tap[prefix + '.join'] = r
        return self.bn(prefix + '.out_bn', r, c)

    def block(self, p, U, t, cin):
        c1, c2, c3 = widths(U)
        cs = c1 + c2 + c3
        s = self.conv_bn(p + '.shortcut', t, cin, cs, 1, False)
        a = self.conv_bn(p + '.conv3', t, cin, c1, 3, True)
        b = self.conv_bn(p + '.conv5', a, c1, c2, 3, True)
        c = self.conv_bn(p + '.conv7', b, c2, c3, 3, True)
        cat = None if t is None else torch.cat([a, b, c], 1)
        o = self.bn(p + '.cat_bn', cat, cs)
        return self.join_bn(p, s, o, cs), cs

    def respath(self, p, f, length, t, cin):
        for i in range(length):
            q = '%s.%d' % (p, i)
            s = self.conv_bn(q + '.shortcut', t, cin, f, 1, False)
            o = self.conv_bn(q + '.conv', t, cin, f, 3, True)
            t, cin = self.join_bn(q, s, o, f), f
        return t

    def network(self, x, n_channels, nff):
        t, c = x, n_channels
        skips = []
        for level in range(5):
            t, c = self.block('block%d' % (level + 1), nff << level, t, c)
            if level == 4:
                break
            out = t
            if t is not None:
                self.pre.append(('pool', t.detach().numpy().copy()))
                t, idx = F.max_pool2d(t, 2, 2, return_indices=True)
                self.decisions.append(idx.numpy().copy())
            skips.append((self.respath('respath%d' % (level + 1), nff << level, 4 - level, out, c), nff << level))
        for u in range(4):
            level = 3 - u
            U = nff << level
            p = 'up%d' % (6 + u)
            w = self._var(p + '.tconv.kernel', [2, 2, U, c])
            b = self._var(p + '.tconv.bias', [U])
            skip, cskip = skips[level]
            if t is not None:
                t = F.conv_transpose2d(t, w.permute(3, 2, 0, 1).contiguous(), b, stride=2)
                t = torch.cat([t, skip], 1)
            t, c = self.block('block%d' % (6 + u), U, t, U + cskip)
        return self.conv_bn('head', t, c, 1, 1, False)          # the logits: the sigmoid is the loss's


def param_specs(n_channels, n_filters_first=32):
    """[(name, shape, trainable)] in creation order"""
    g = _Graph()
    g.network(None, n_channels, n_filters_first)
    return g.specs


def layout(n_channels, n_filters_first=32):
    """{name: (offset, shape, trainable)}, (n_trainable, n_state)"""
    out, off = OrderedDict(), {True: 0, False: 0}
    for name, shape, tr in param_specs(n_channels, n_filters_first):
        out[name] = (off[tr], shape, tr)
        off[tr] += int(np.prod(shape))
    return out, (off[True], off[False])


def unflatten(lay, flat, trainable=True):
    return OrderedDict((n, np.asarray(flat[o:o + int(np.prod(s))]).reshape(s)) for n, (o, s, t) in lay.items() if t == trainable)


def flatten(lay, named, trainable=True, dtype=np.float64):
    n = sum(int(np.prod(s)) for (o, s, t) in lay.values() if t == trainable)
    flat = np.zeros(n, dtype)
    for name, (o, s, t) in lay.items():
        if t == trainable:
            flat[o:o + int(np.prod(s))] = np.asarray(named[name], dtype).ravel()
    return flat


def run(params, state, x, y=None, n_filters_first=32, training=False, dtype=torch.float64, loss_cfg=None, threads=1):
    """params / state: the flat trainable / non-trainable vectors; x [B, H, W, C]; y [B, H, W] or None (no loss, no gradients).
    Returns dict(logits [B, H, W, 1], loss, grads (flat), state (flat, the new moving statistics), decisions, pre, lay)."""
    if dtype != torch.float64 and threads and torch.get_num_threads() != threads:
        # one thread: the float32 run's summation order (and with it which seeds it finds free of flips) does not depend on
        # how many cores the machine has
        n = torch.get_num_threads()
        torch.set_num_threads(threads)
        try:
            return run(params, state, x, y, n_filters_first, training, dtype, loss_cfg, threads)
        finally:
            torch.set_num_threads(n)
    n_channels = x.shape[-1]
    lay, _ = layout(n_channels, n_filters_first)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    P = {}
    for n, v in unflatten(lay, params, True).items():
        P[n] = torch.tensor(np.asarray(v, npdt), dtype=dtype, requires_grad=y is not None)
    for n, v in unflatten(lay, state, False).items():
        P[n] = torch.tensor(np.asarray(v, npdt), dtype=dtype)
    g = _Graph(P, training)
    logits_t = g.network(torch.tensor(np.asarray(x, npdt), dtype=dtype).permute(0, 3, 1, 2), n_channels, n_filters_first)
    logits = logits_t.permute(0, 2, 3, 1).detach().numpy()
    out = dict(logits=logits, lay=lay, decisions=g.decisions, pre=g.pre, tap=g.tap)
    new_state = unflatten(lay, np.asarray(state, npdt), False)
    new_state.update(g.state)
    out['state'] = flatten(lay, new_state, False, npdt)
    if y is not None:
        per, dper = O.weighted_crossentropy(np.asarray(y, npdt), logits, **(loss_cfg or {}))
        B = x.shape[0]
        out['loss'] = float(per.mean(dtype=np.float64))
        logits_t.backward(torch.tensor(dper / npdt(B), dtype=dtype).permute(0, 3, 1, 2))
        grads = OrderedDict((n, P[n].grad.numpy()) for n, (o, s, t) in lay.items() if t)
        out['grads'] = flatten(lay, grads, True, npdt)
    return out


def same_decisions(a, b):
    """did two runs take every ReLU and max-pool decision the same way?"""
    return len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


def decision_safety(r64, r32):
    """How far is every ReLU / max-pool decision of the float64 run from what float32 rounding can turn?  A decision's margin is
    |pre-activation| (ReLU) or the lead of a window's maximum over its runner-up (max-pool; a lead of exactly 0 is a structural
    tie -- two ReLU zeros of one channel behind a BatchNorm -- and the same in any precision).  Returns (by tensor, by element):
    by tensor   the smallest margin of a tensor over the float32 run's LARGEST deviation on that tensor (twice that for a lead),
                minimum over the tensors: above 1 no float32 arithmetic with deviations of that size can flip anything;
    by element  margin over the float32 run's deviation at that very element, minimum over all decisions: above 1 is exactly
                "this float32 run flipped nothing", and the value says by how much its errors could grow before one does."""
    by_tensor = by_element = float('inf')
    for (kind, a), (_, b) in zip(r64['pre'], r32['pre']):
        dev = np.abs(b.astype(np.float64) - a)
        if kind == 'relu':
            margin = np.abs(a)
        else:
            B, C, H, W = a.shape
            win = lambda t: t.reshape(B, C, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)          # noqa: E731
            v = np.sort(win(a), -1)
            margin = v[..., 3] - v[..., 2]
            dev = 2 * win(dev).max(-1)
            margin, dev = margin[margin > 0], dev[margin > 0]
        if margin.size:
            by_tensor = min(by_tensor, float(margin.min()) / (float(dev.max()) + 1e-300))
            by_element = min(by_element, float((margin / (dev + 1e-300)).min()))
    return by_tensor, by_element


def init(n_channels, n_filters_first, seed, perturb=0.0):
    """glorot-uniform kernels, zero biases / betas, unit gammas, moving mean 0 / variance 1; perturb > 0: betas, gammas and the
    moving statistics moved off their symmetric start.  Returns (params, state) flat float32."""
    lay, _ = layout(n_channels, n_filters_first)
    rng = np.random.default_rng(seed)
    named = OrderedDict()
    for name, (o, s, t) in lay.items():
        if name.endswith('.kernel'):
            kh, kw, a, b = s
            lim = np.sqrt(6.0 / (kh * kw * (a + b)))
            named[name] = rng.uniform(-lim, lim, s)
        elif name.endswith('.gamma'):
            named[name] = 1.0 + perturb * rng.uniform(-1, 1, s)
        elif name.endswith('.moving_variance'):
            named[name] = 1.0 + perturb * rng.uniform(-0.5, 1, s)
        else:
            named[name] = perturb * rng.uniform(-1, 1, s)
    return flatten(lay, named, True, np.float32), flatten(lay, named, False, np.float32)


def discs(B, H, W, seed):
    """labels: one disc per image, some positives in every image"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    y = np.zeros((B, H, W), np.float32)
    for b in range(B):
        cy, cx = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W
        r = max(2.0, rng.uniform(0.15, 0.3) * min(H, W))
        y[b] = ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r)
    return y
