"""Torch-CPU autograd statement of the channel sensitivity of `annotator evaluate --visualize_sensitivity`
(annotator/utils/callbacks.py:290-313): the network in INFERENCE mode (BatchNorm on its moving statistics, sigmoid output),
g = d sum(prob) / d x, s[b, c] = sum over H, W of |g[b, h, w, c]|.  The reference of tests/test_sensitivity_gpu.py, in float64; the
same statement in float32 gives the cost of the number format.  The network follows tests/torch_ref.py (same variable names and
layout transposes)."""

import numpy as np
import torch
import torch.nn.functional as F


def sums(spec, params, x, dtype=torch.float64):
    """raw sums [B, C] (float64 array) for params {name: array} and x [B, H, W, C]"""
    P = {n: torch.tensor(np.asarray(v), dtype=dtype) for n, v in params.items()}
    xin = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    xt = xin.permute(0, 3, 1, 2)

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
    logits = F.conv2d(t, P['head.kernel'].permute(3, 2, 0, 1), P['head.bias'])
    torch.sigmoid(logits).sum().backward()
    return xin.grad.abs().sum((1, 2)).double().numpy()
