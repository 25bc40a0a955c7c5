"""Three operating points that real training reaches and uniform-noise inputs on perturbed weights never do (pure numpy: the case
table, the input builders, the parameter transforms and the float64 / float32 oracle runs; tests/test_operating_points.py proves
on the oracle alone that every case is decidable and has teeth, tests/test_operating_points_gpu.py holds the device to it).

  zero      exact zeros and exact ties: a disc of integers(1, 256) / 255 noise per image on a background of exactly 0.0 under
            Keras' zero-initialised biases.  The first conv's pre-activation is exactly 0.0 over the background in any precision
            and summation order, every 2 x 2 window of the background is a four-way tie, and two rules decide the gradient: the
            derivative of the activation at 0 (O._act_bwd: y > 0) and the element of a tied window that receives the max-pool
            gradient (O.maxpool_fwd: the first maximum in row-major order).  ReLU and LeakyReLU(0.3).
  saturate  logits of -30 .. 30: head.kernel *= s, head.bias = (bias - mid) * s with s = 30 / half-range of the float64 logits
            of the unchanged case; labels 'disagree' (the case's own) and 'agree' (y = [logit > 0]), plain loss and region loss.
  shift     every *.tconv.bias under BatchNorm moved by +-k sigma_c (sign alternating by channel; sigma_c the float64 batch
            standard deviation of that channel of the transposed conv's output): a channel with a large mean in front of a
            BatchNorm, which the float64 oracle does not see at all (shift_is_invariant below).

Every case is f32; the loss is the weighted cross-entropy with weight_mul = 3 (plus the default region term where asked)."""

import contextlib
from collections import OrderedDict

import numpy as np

import helpers as Hp
import region_loss_ref as R
from oracle import unet_oracle as O

COMMON = dict(rate=2, kernel_size=3, conv_stride=1, padding='same')
LEAKY = {'class_name': 'LeakyReLU', 'config': {'alpha': 0.3}}
LOSS = dict(weight_mul=3.0)

# name -> arch, input channels, B, max_batch, H, W, model options
SHAPES = OrderedDict([
    # the column-strip and block-fused 3/6/12-channel plan (tests/test_engine_gpu.py: test_block_fused_backward_against_oracle,
    # test_vector_alu_kernels_of_the_3_channel_level_against_oracle)
    ('u3_3x32x128', dict(arch='unet', C=1, B=3, max_batch=3, H=32, W=128, opts=dict(n_filters_first=3, n_downsample=3, bn=False))),
    ('u3_2x40x128', dict(arch='unet', C=1, B=2, max_batch=2, H=40, W=128, opts=dict(n_filters_first=3, n_downsample=3, bn=False))),
    # the three shapes of tests/test_region_loss_gpu.py, a ragged batch
    ('c3', dict(arch='unet', C=1, B=3, max_batch=4, H=40, W=24, opts=dict(n_filters_first=3, n_downsample=3, bn=False))),
    ('c16', dict(arch='mulmo', C=3, B=3, max_batch=4, H=12, W=20, opts=dict(n_filters_first=16, n_downsample=2, bn=True))),
    ('c64', dict(arch='unet', C=1, B=3, max_batch=4, H=10, W=14, opts=dict(n_filters_first=64, n_downsample=1, bn=False))),
    ('b16_2x32x32', dict(arch='unet', C=1, B=2, max_batch=2, H=32, W=32, opts=dict(n_filters_first=16, n_downsample=2, bn=True))),
    ('b16_2x64x64', dict(arch='unet', C=1, B=2, max_batch=2, H=64, W=64, opts=dict(n_filters_first=16, n_downsample=2, bn=True))),
    ('b64_2x16x32', dict(arch='unet', C=1, B=2, max_batch=2, H=16, W=32, opts=dict(n_filters_first=64, n_downsample=1, bn=True))),
    ('b64_2x32x32', dict(arch='unet', C=1, B=2, max_batch=2, H=32, W=32, opts=dict(n_filters_first=64, n_downsample=1, bn=True))),
])

# input seed per (shape, activation) of the exact-zero cases.  A seed is replaced here, on the CPU, when the float32 oracle flips a
# decision on it (test_operating_points.py::test_every_case_is_decidable_by_the_reference_alone: over 1e-4 of a tensor's scale);
# never by a wider bound.
ZERO_SEED = {}
ZERO_SEED_DEFAULT = 41
SATURATE_SHAPES = ('c3', 'c16', 'c64')
SHIFT_SHAPES = ('c16', 'b16_2x64x64', 'b64_2x32x32')
SHIFT_SIGMAS = 16.0
NOISE_SEED = 8                            # tests/test_region_loss_gpu.py's batch


def zero_cases():
    return [('zero', shape, act) for shape in SHAPES for act in ('relu', 'leaky')]


def saturate_cases():
    return [('saturate', shape, labels, region) for shape in SATURATE_SHAPES for labels in ('disagree', 'agree')
            for region in (False, True)]


def shift_cases():
    return [('shift', shape, SHIFT_SIGMAS) for shape in SHIFT_SHAPES]


def all_cases():
    return zero_cases() + saturate_cases() + shift_cases()


def case_id(case):
    return '-'.join('region' if v is True else 'plain' if v is False else ('%g' % v if isinstance(v, float) else str(v)) for v in case)


def spec_of(shape, act='relu'):
    s = SHAPES[shape]
    full = dict(COMMON)
    full.update(s['opts'])
    if act == 'leaky':
        full['activation'] = LEAKY
    return O.ModelSpec(s['arch'], s['C'], **full)


def device_kwargs(shape, act='relu', **extra):
    s = SHAPES[shape]
    return Hp.device_kwargs(spec_of(shape, act), s['H'], s['W'], s['max_batch'], **extra)


# ---- inputs ------------------------------------------------------------------------------------------------------------------

def _disc(H, W, cy, cx, r):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def zero_disc_batch(B, H, W, C, seed):
    """(x [B, H, W, C] float32, y [B, H, W] float32): per image one disc of integers(1, 256) / 255 noise (no zero inside it) on a
    background of exactly 0.0, the label a disc of half the radius at the same centre.  Image 1 (image 0 of a single one) has
    its centre above the first row plus half a radius, so its disc -- and its label -- is cut by the top border."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, H, W, C), np.float32)
    y = np.zeros((B, H, W), np.float32)
    r = max(2.0, min(H, W) / 3.5)
    for b in range(B):
        cy = H / 2.0 + rng.integers(-1, 2)
        cx = W / 2.0 + rng.integers(-(W // 6), W // 6 + 1)
        if b == min(1, B - 1):
            cy = r / 2.0
        disc = _disc(H, W, cy, cx, r)
        noise = (rng.integers(1, 256, (H, W, C)) / 255.0).astype(np.float32)
        x[b] = np.where(disc[..., None], noise, np.float32(0.0))
        y[b] = _disc(H, W, cy, cx, r / 2.0)
    assert (x == 0).any() and y.any()
    return x, y


def noise_batch(shape, seed=NOISE_SEED):
    """the batch of tests/test_region_loss_gpu.py: uniform noise, image 0 without positives, image 2 (the last one) with a lesion
    that touches two borders"""
    s = SHAPES[shape]
    B, H, W = s['B'], s['H'], s['W']
    rng = np.random.default_rng(seed)
    x = rng.random((B, H, W, s['C'])).astype(np.float32)
    y = np.zeros((B, H, W), np.float32)
    y[1, H // 4:H // 2, W // 4:W // 2 + 2] = 1.0
    y[B - 1, H - H // 4:H, 0:W // 4] = 1.0
    return x, y


# ---- parameters --------------------------------------------------------------------------------------------------------------

def zero_bias_params(spec):
    """helpers.perturbed_params with every *.bias at 0.0: Keras' initial state"""
    p = Hp.perturbed_params(spec, np.float64)
    for n in p:
        if n.endswith('.bias'):
            p[n] = np.zeros_like(p[n])
    return p


def _round32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def saturate_head(spec, params, x, training=True):
    """params with the head scaled so that the float64 logits (of a training-mode pass, or of an inference pass) span -30 .. 30"""
    logits = O.forward(spec, params, x.astype(np.float64), training=training)[0]
    lo, hi = float(logits.min()), float(logits.max())
    s = 30.0 / (0.5 * (hi - lo))
    out = dict(params)
    out['head.kernel'] = _round32(params['head.kernel'] * s)
    out['head.bias'] = _round32((params['head.bias'] - 0.5 * (hi + lo)) * s)
    return out


@contextlib.contextmanager
def patched(name, fn):
    """the oracle with O.<name> replaced"""
    old = getattr(O, name)
    setattr(O, name, fn)
    try:
        yield old
    finally:
        setattr(O, name, old)


def tconv_sigmas(spec, params, x):
    """{decoder.upU: float64 batch standard deviation per channel of the transposed conv's output (before its BatchNorm)}"""
    seen = []
    orig = O.tconv_fwd

    def spy(t, w, b):
        out = orig(t, w, b)
        seen.append(out[0].std((0, 1, 2)))
        return out
    with patched('tconv_fwd', spy):
        O.forward(spec, params, x.astype(np.float64), training=True)
    assert len(seen) == spec.n_down
    return {'decoder.up%d' % u: s for u, s in enumerate(seen)}


def shift_tconv_bias(spec, params, x, sigmas):
    """params with every *.tconv.bias moved by +- sigmas * sigma_c, the sign alternating by channel"""
    assert spec.bn
    out = dict(params)
    for p, sd in tconv_sigmas(spec, params, x).items():
        sign = np.where(np.arange(len(sd)) % 2 == 0, 1.0, -1.0)
        out[p + '.tconv.bias'] = _round32(params[p + '.tconv.bias'] + sign * sigmas * sd)
    return out


# ---- the oracle, float64 and float32 -----------------------------------------------------------------------------------------

def oracle_run(spec, params, x, y, region, dtype):
    """(loss, flat gradients float64, logits, new_state) of one train step in `dtype`; region: with the default region term
    (tests/region_loss_ref.py; the loss itself is then formed in float64 from the `dtype` logits)"""
    p = {n: np.asarray(v).astype(dtype) for n, v in params.items()}
    if not region:
        loss, grads, logits, state = O.loss_and_grads(spec, p, x.astype(dtype), y, LOSS, training=True)
    else:
        logits, state, backward, _ = O.forward(spec, p, x.astype(dtype), training=True)
        per, dper = R.tversky_crossentropy(y, logits, **LOSS)
        loss = float(per.mean(dtype=np.float64))
        _, grads = backward((dper / x.shape[0]).astype(dtype))
    return loss, O.flatten(spec, grads).astype(np.float64), logits, state


def allowance(spec, gref, g32):
    """{tensor: allowed max-abs error}: 2e-5 max|g_ref| + 10 x the float32 oracle's error on that tensor (the rule of
    test_block_fused_backward_against_oracle); a degenerate tensor (helpers.degenerate_tensors: analytically zero, float32 noise
    in any implementation) gets 2e-5 of its sibling's scale on top, as helpers.assert_grads_per_tensor_nofixture judges it"""
    sl = dict(Hp.tensor_slices(spec))
    deg = Hp.degenerate_tensors(spec)
    out = OrderedDict()
    for n, s in sl.items():
        a = 2e-5 * np.abs(gref[s]).max() + 10.0 * np.abs(g32[s] - gref[s]).max()
        if n in deg:
            a += 2e-5 * np.abs(gref[sl[Hp.sibling_of(n)]]).max()
        out[n] = float(a)
    return out


def errors_over_allowance(spec, g, gref, allowed):
    """{tensor: max|g - gref| / allowed}"""
    g = np.asarray(g, np.float64)
    assert g.shape == gref.shape and np.isfinite(g).all()
    return OrderedDict((n, float(np.abs(g[s] - gref[s]).max() / allowed[n])) for n, s in Hp.tensor_slices(spec))


def float32_cost(spec, gref, g32):
    """{non-degenerate tensor: the float32 oracle's max-abs error / the tensor's scale}"""
    deg = Hp.degenerate_tensors(spec)
    return OrderedDict((n, float(np.abs(g32[s] - gref[s]).max() / np.abs(gref[s]).max()))
                       for n, s in Hp.tensor_slices(spec) if n not in deg)


_built, _ref = {}, {}


def build(case):
    """(spec, params {name: float64 array, float32-representable}, x float32, y float32, region) of a case -- built once"""
    if case not in _built:
        kind, shape = case[0], case[1]
        s = SHAPES[shape]
        if kind == 'zero':
            act = case[2]
            spec = spec_of(shape, act)
            x, y = zero_disc_batch(s['B'], s['H'], s['W'], s['C'], ZERO_SEED.get((shape, act), ZERO_SEED_DEFAULT))
            params, region = zero_bias_params(spec), False
        elif kind == 'saturate':
            labels, region = case[2], case[3]
            spec = spec_of(shape)
            x, y = noise_batch(shape)
            params = saturate_head(spec, Hp.perturbed_params(spec, np.float64), x)
            if labels == 'agree':
                logits = O.forward(spec, params, x.astype(np.float64), training=True)[0]
                y = (logits[..., 0] > 0).astype(np.float32)
        elif kind == 'shift':
            spec = spec_of(shape)
            x, y = noise_batch(shape)
            params, region = shift_tconv_bias(spec, Hp.perturbed_params(spec, np.float64), x, case[2]), False
        else:
            raise ValueError(case)
        x.setflags(write=False)
        y.setflags(write=False)
        _built[case] = (spec, params, x, y, region)
    return _built[case]


def reference(case, with_float32=True):
    """dict(loss, grads, logits, state, and with_float32: loss32, grads32, allowed) of the oracle on a case -- computed once"""
    if (case, True) in _ref:
        return _ref[(case, True)]
    key = (case, with_float32)
    if key not in _ref:
        spec, params, x, y, region = build(case)
        loss, g, logits, state = oracle_run(spec, params, x, y, region, np.float64)
        ref = dict(loss=loss, grads=g, logits=logits, state=state)
        if with_float32:
            ref['loss32'], ref['grads32'], _, _ = oracle_run(spec, params, x, y, region, np.float32)
            ref['allowed'] = allowance(spec, g, ref['grads32'])
        _ref[key] = ref
    return _ref[key]


# ---- what an exact-zero case contains, and the two wrong rules ---------------------------------------------------------------

def first_level_counts(spec, params, x):
    """(tied windows, windows, exact zeros, values) at the first encoder level of the float64 oracle: windows of the first max-pool
    whose maximum occurs more than once, and exactly-zero values in front of that pool -- the pooled tensor itself without
    BatchNorm; under BatchNorm (the background is a non-zero constant behind it) the first conv's activation, where the zeros
    that the activation rule decides are"""
    convs, pools = [], []
    conv, pool = O.conv2d_fwd, O.maxpool_fwd

    def spy_conv(*a, **k):
        out = conv(*a, **k)
        if len(convs) < 1:
            convs.append(out[0])
        return out

    def spy_pool(t, r):
        if not pools:
            pools.append((t, r))
        return pool(t, r)
    with patched('conv2d_fwd', spy_conv), patched('maxpool_fwd', spy_pool):
        O.forward(spec, params, x.astype(np.float64), training=True)
    t, r = pools[0]
    B, H, W, C = t.shape
    win = t[:, :H // r * r, :W // r * r].reshape(B, H // r, r, W // r, r, C).transpose(0, 1, 3, 5, 2, 4).reshape(-1, r * r)
    tied = int(((win == win.max(-1, keepdims=True)).sum(-1) > 1).sum())
    zeros_in = convs[0] if spec.bn else t
    return tied, len(win), int((zeros_in == 0).sum()), int(zeros_in.size)


def act_bwd_one_at_zero(y, dy, alpha):
    """the wrong activation rule: act'(0) = 1"""
    return dy * np.where(y >= 0, 1.0, alpha).astype(dy.dtype)


def maxpool_fwd_last(x, r):
    """the wrong pool rule: the LAST maximum in row-major window order"""
    B, H, W, C = x.shape
    Ho, Wo = H // r, W // r
    xw = x[:, :Ho * r, :Wo * r, :].reshape(B, Ho, r, Wo, r, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, Ho, Wo, C, r * r)
    idx = r * r - 1 - xw[..., ::-1].argmax(-1)
    y = np.take_along_axis(xw, idx[..., None], -1)[..., 0]
    return y, (idx, x.shape, r)


# ---- the attribution case ----------------------------------------------------------------------------------------------------

ATTR_STEPS = 4
_attr = {}


@contextlib.contextmanager
def position_independent_convs(max_pool2d=None):
    """tests/attr_ref.py with its two convolutions written as sums of shifted planes times scalar weights, in one fixed order.
    A library convolution may add the terms of a pixel in an order that depends on where the pixel lies in its tile or vector
    (measured: torch's float64 conv2d on one CPU gives the interior of a constant region one value, on another values an ulp
    apart), and then noise decides the ties of a constant region in the REFERENCE.  Elementwise products and sums are the same
    IEEE operations at every pixel: the statement is the same, and a constant region stays constant on any machine."""
    import attr_ref
    F = attr_ref.F
    import torch

    def conv2d(t, w, b=None, padding=0):
        co, ci, kh, kw = w.shape
        H, W = t.shape[2] + 2 * padding - kh + 1, t.shape[3] + 2 * padding - kw + 1
        tp = F.pad(t, (padding, padding, padding, padding)) if padding else t
        out = None
        for ky in range(kh):
            for kx in range(kw):
                for c in range(ci):
                    term = tp[:, c:c + 1, ky:ky + H, kx:kx + W] * w[:, c, ky, kx].view(1, co, 1, 1)
                    out = term if out is None else out + term
        return out if b is None else out + b.view(1, co, 1, 1)

    def conv_transpose2d(t, w, b=None, stride=1):
        ci, co, r, r2 = w.shape
        assert r == r2 == stride
        B, _, H, W = t.shape
        rows = []
        for a in range(r):
            cols = []
            for c in range(r):
                out = None
                for i in range(ci):
                    term = t[:, i:i + 1] * w[i, :, a, c].view(1, co, 1, 1)
                    out = term if out is None else out + term
                cols.append(out if b is None else out + b.view(1, co, 1, 1))
            rows.append(torch.stack(cols, -1))                    # [B, co, H, W, r]
        return torch.stack(rows, 3).reshape(B, co, H * r, W * r)  # [B, co, H, r, W, r]

    class Stable:
        """attr_ref's view of torch.nn.functional: everything but the three replaced functions is torch's"""
        def __getattr__(self, name):
            return getattr(F, name)
    stable = Stable()
    stable.conv2d, stable.conv_transpose2d = conv2d, conv_transpose2d
    if max_pool2d is not None:
        stable.max_pool2d = max_pool2d
    attr_ref.F = stable
    try:
        yield F
    finally:
        attr_ref.F = F


def attribution_case():
    """case (a) of tests/attr_cases.py (unet, 3 channels, 3 filters, 2 levels, BatchNorm, 32 x 48, B = 3 of max_batch 4) with
    LeakyReLU(0.3), zero biases and the zero-background input: dict(spec, params, x, kw (device kwargs), ref {baseline: float64
    torch autograd (signed, absolute, endpoints, map)}, cost {baseline: {quantity: float32 cost of the same statement}}).
    (torch is imported here only: the rest of this module is numpy)"""
    if not _attr:
        import torch
        import attr_cases as AC
        import attr_ref
        c = AC.CASES['a']
        spec = O.ModelSpec(c['arch'], c['C'], **dict(COMMON, activation=LEAKY, **c['opts']))
        params = zero_bias_params(spec)
        x, _ = zero_disc_batch(c['B'], c['H'], c['W'], c['C'], ZERO_SEED_DEFAULT)
        ref, cost = {}, {}
        for bl in attr_ref.BASELINES:
            with position_independent_convs():
                ref[bl], f32 = (attr_ref.integrated_gradients(spec, params, x, ATTR_STEPS, bl, dt) for dt in (torch.float64, torch.float32))
            cost[bl] = AC.errors(f32, ref[bl])
        _attr.update(spec=spec, params=params, x=x, ref=ref, cost=cost, kw=Hp.device_kwargs(spec, c['H'], c['W'], c['max_batch']))
    return _attr


def attribution_with_last_maximum(baseline):
    """the float64 statement of the attribution case with the wrong pool rule (the last maximum of a window: max_pool2d of the
    flipped tensor, flipped back -- 32 x 48 is made of whole windows at both levels)"""
    import torch
    import attr_ref
    a = attribution_case()
    pool = attr_ref.F.max_pool2d

    def last(t, k, s):
        return pool(t.flip(2, 3), k, s).flip(2, 3)
    with position_independent_convs(max_pool2d=last):
        return attr_ref.integrated_gradients(a['spec'], a['params'], a['x'], ATTR_STEPS, baseline, torch.float64)


WRONG_RULES = OrderedDict([('act', ('_act_bwd', act_bwd_one_at_zero)), ('pool', ('maxpool_fwd', maxpool_fwd_last))])


def wrong_rule_grads(case, rule):
    """flat float64 gradients of the oracle with one wrong rule patched in"""
    spec, params, x, y, region = build(case)
    with patched(*WRONG_RULES[rule]):
        return oracle_run(spec, params, x, y, region, np.float64)[1]
