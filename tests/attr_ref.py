"""Torch-CPU autograd statement of the integrated-gradients attribution of `annotator evaluate --visualize_attribution`
(include/dnnca.h: dnnca_integrated_gradients; Sundararajan et al. 2017).  The reference of tests/test_attr_gpu.py in float64; the same
statement in float32 is the cost of the number format.  The network is that of tests/sens_ref.py, restated so that its logits can
be evaluated at many inputs.

For slice b of a network in INFERENCE mode, F_b(x) = sum over h, w of sigmoid(logits_b(x)):
    baseline  x0[b, :, :, c] a constant plane: 'black' 0, 'mean' the mean of x[b, :, :, c] in double rounded once to float32
    path      x(alpha) = x0 + alpha (x - x0); alpha_k = (k + 0.5) / m formed in double and rounded once to float32, k = 0 .. m - 1
    attr[b, h, w, c] = (x - x0)[b, h, w, c] * ((sum over k, ascending, of g_k[b, h, w, c]) / m),  g_k = d F_b / d x at x(alpha_k)
    signed[b, c] = sum over h, w of attr;  absolute[b, c] = sum over h, w of |attr|
    endpoints[b] = (F_b(x), F_b(x0))
x, x0 and alpha_k are float32 values; everything behind them runs in `dtype`."""

import numpy as np
import torch
import torch.nn.functional as F

BASELINES = ('black', 'mean')


def logits(spec, P, xt):
    """xt [B, C, H, W] -> logits [B, 1, H, W]; P {name: tensor}"""
    def act(t):
        return F.leaky_relu(t, spec.alpha) if spec.alpha else F.relu(t)

    def conv(prefix, t):
        w = P[prefix + '.kernel'].permute(3, 2, 0, 1)
        return act(F.conv2d(t, w, P[prefix + '.bias'], padding=(spec.k - 1) // 2))

    def bn(prefix, t):
        g, b, mm, mv = (P[prefix + s][None, :, None, None] for s in ('.gamma', '.beta', '.moving_mean', '.moving_variance'))
        return (t - mm) / torch.sqrt(mv + 1e-3) * g + b

    assert spec.padding == 'same'
    skips_all, bottoms = [], []
    for e in range(spec.n_encoders()):
        enc = 'encoder%d' % e if spec.arch == 'mulmo' else 'encoder'
        t = xt[:, e:e + 1] if spec.arch == 'mulmo' else xt
        skips = []
        for i in range(spec.n_down):
            p = '%s.down%d' % (enc, i)
            for j in range(spec.n_conv):
                t = conv('%s.conv%d' % (p, j), t)
                if spec.bn:
                    t = bn('%s.bn%d' % (p, j), t)
            skips.append(t)
            t = F.max_pool2d(t, spec.rate, spec.rate)
            if spec.bn:
                t = bn(p + '.pool_bn', t)
        skips_all.append(skips)
        bottoms.append(t)
    t = torch.cat(bottoms, 1) if spec.arch == 'mulmo' else bottoms[0]
    ref = skips_all[spec.reference_index if spec.arch == 'mulmo' else 0]
    for u in range(spec.n_down):
        p = 'decoder.up%d' % u
        t = F.conv_transpose2d(t, P[p + '.tconv.kernel'].permute(3, 2, 0, 1), P[p + '.tconv.bias'], stride=spec.rate)
        if spec.bn:
            t = bn(p + '.tconv_bn', t)
        t = torch.cat([t, ref[spec.n_down - 1 - u]], 1)
        for j in range(spec.n_conv):
            t = conv('%s.conv%d' % (p, j), t)
            if spec.bn:
                t = bn('%s.bn%d' % (p, j), t)
    return F.conv2d(t, P['head.kernel'].permute(3, 2, 0, 1), P['head.bias'])


def baseline_of(x, baseline):
    """float32 [B, 1, 1, C]"""
    x = np.asarray(x, np.float32)
    if baseline == 'black':
        return np.zeros((x.shape[0], 1, 1, x.shape[3]), np.float32)
    assert baseline == 'mean', baseline
    return x.astype(np.float64).mean(axis=(1, 2), keepdims=True).astype(np.float32)


def alphas(steps):
    return [np.float32((k + 0.5) / steps) for k in range(int(steps))]


def integrated_gradients(spec, params, x, steps, baseline='black', dtype=torch.float64):
    """(signed [B, C], absolute [B, C], endpoints [B, 2], attr [B, H, W, C]) as float64 arrays"""
    P = {n: torch.tensor(np.asarray(v), dtype=dtype) for n, v in params.items()}
    x = np.asarray(x, np.float32)
    xt = torch.tensor(x, dtype=dtype)
    x0 = torch.tensor(np.broadcast_to(baseline_of(x, baseline), x.shape).copy(), dtype=dtype)
    diff = xt - x0

    def f_of(inp):
        return torch.sigmoid(logits(spec, P, inp.permute(0, 3, 1, 2))).sum((1, 2, 3))

    acc = torch.zeros_like(xt)
    for a in alphas(steps):
        point = (x0 + torch.tensor(float(a), dtype=dtype) * diff).detach().requires_grad_(True)
        f_of(point).sum().backward()          # slices are independent: the gradient of the sum is each slice's own
        acc = acc + point.grad
    attr = diff * (acc / float(steps))
    with torch.no_grad():
        ends = torch.stack([f_of(xt), f_of(x0)], 1)
    return (attr.sum((1, 2)).double().numpy(), attr.abs().sum((1, 2)).double().numpy(), ends.double().numpy(), attr.double().numpy())


def gap(signed, endpoints):
    """completeness gap per slice: sum over c of signed[b, c] - (F_b(x) - F_b(x0))"""
    return np.asarray(signed).sum(1) - (np.asarray(endpoints)[:, 0] - np.asarray(endpoints)[:, 1])
