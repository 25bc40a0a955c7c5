"""The float64 reference of a dense plan ONE LAUNCH AT A TIME (test infrastructure; pure numpy on the oracle's primitives).

Every tensor of a plan keeps a data and a gradient buffer of its own for the life of the model, so after a pass the stored inputs
and the stored output of every launch can be read back (csrc/debug_tools.hip: dnnca_debug_ops / _tensor / _bn_coef).  The checker
feeds the STORED inputs of a launch to a float64 statement of that one operation, with the kernel's rounding points, and compares
with the STORED output.  Device and reference then differ by one fp32 accumulation, not by a cascade of bf16 rounding flips, and
the project's fp32 rule applies to the bf16 kernels at any size:

    per tensor   |dev - ref| <= 2e-5 max|ref| + 10 max|ref32 - ref|            (ref32: the same statement in float32 numpy)
    bf16-stored  to_bf16(ref - a) <= dev <= to_bf16(ref + a) element by element, a = that tensor's allowance (rounding is
                 monotone: exactly "dev is the rounding of some value within the allowance"; no share of elements left out)
    statistics   mean within 1e-5 of the channel's standard deviation, inv within 1e-5 relative, each + 10 x the float32 cost;
                 moving statistics within 1e-5

Rounding points (csrc/kernels_igemm.hip, kernels_misc.hip):
  * the bf16 kernels (3x3 convs whose sources and output are multiples of 32 channels, transposed convs of multiples of 64 under
    dtype bf16) round activations, gradients and weights to bf16 while staging and accumulate in fp32; bias and activation are
    applied to the fp32 accumulator, a bf16-stored output is rounded on store; the bias gradient is summed from the staged
    (rounded) output gradient;
  * BatchNorm apply is fmaf(x, scale, shift) in float32 from the coefficient table: mirrored EXACTLY here (the product of two
    float32 is exact in float64) so that it cannot become a source of rounding flips; the max-pool fused behind it takes the maxima
    (and records their positions) of those float32 values before they are rounded for a bf16-stored output;
  * batch statistics are those of the stored (rounded) values;
  * a gradient buffer with several writers is overwritten by the first (in backward order) and added to by the later ones; a
    bf16-stored one is rounded by every writer, so the interval rule is carried through the writers (each stage monotone).

`ratio` of a result is the smallest multiple of the allowance at which the tensor passes (0: the reference reproduces it exactly)."""

import numpy as np

from bf16_emul_case import to_bf16
from oracle import unet_oracle as O

REL, COST = 2e-5, 10.0
STAT_REL, STATE_TOL = 1e-5, 1e-5
DECIDABLE = 1e-4            # a case whose float32 cost reaches this share of a tensor's scale cannot decide (tests/test_layerwise.py)
SLOTS = ('inA', 'inB', 'out')


class View:
    def __init__(self, text):
        self.H, self.W, self.C, self.ps, self.hd, self.hg, self.id = [int(v) for v in text.split(',')]


def parse_ops(text):
    """the lines of dnnca_debug_ops -> [dict]"""
    ops = []
    for line in text.strip().splitlines():
        kv = dict(tok.split('=', 1) for tok in line.split())
        o = dict(type=kv['type'], name=kv['name'], k=int(kv['k']), alpha=float(kv['alpha']), mask_alpha=float(kv['mask_alpha']),
                 src_bn=[int(v) for v in kv['src_bn'].split(',')])
        for n in ('op', 'w_off', 'b_off', 'mm_off', 'mv_off', 'need_din', 'accA', 'accB', 'maskA', 'maskB', 'premasked', 'elided'):
            o[n] = int(kv[n])
        for s in SLOTS:
            o[s] = View(kv[s])
        assert o['op'] == len(ops)
        ops.append(o)
    return ops


def tensor_table(ops):
    """{id: dict(view, prod (op index or None), readers [(op index, slot index)], any (op, slot))}"""
    T = {}
    for i, o in enumerate(ops):
        for s, slot in enumerate(SLOTS):
            v = o[slot]
            if not v.id:
                continue
            t = T.setdefault(v.id, dict(view=v, prod=None, readers=[], any=(i, s)))
            if slot == 'out':
                t['prod'] = i
            else:
                t['readers'].append((i, s))
    return T


# ---- the launches, in float64 (ft = np.float64) or float32 -------------------------------------------------------------------------

def _rb(a, bf16):
    return to_bf16(a) if bf16 else np.asarray(a, np.float64)


def _alpha(op):
    return None if op['alpha'] < 0 else op['alpha']


def conv_out(x, w, b, alpha, bf16, ft):
    return O.conv2d_fwd(_rb(x, bf16).astype(ft), _rb(w, bf16).astype(ft), np.asarray(b, ft), 'same', alpha)[0]


def conv_back(x, w, dz, bf16, ft):
    """(dx, dw, dbias) of a conv from its stored input and its stored PRE-activation output gradient"""
    k = w.shape[0]
    p = (k - 1) // 2
    xp = np.pad(_rb(x, bf16).astype(ft), ((0, 0), (p, k - 1 - p), (p, k - 1 - p), (0, 0)))
    return O.conv2d_bwd((xp, _rb(w, bf16).astype(ft), None, None, 'same', x.shape), _rb(dz, bf16).astype(ft))


def tconv_out(x, w, b, bf16, ft):
    return O.tconv_fwd(_rb(x, bf16).astype(ft), _rb(w, bf16).astype(ft), np.asarray(b, ft))[0]


def tconv_back(x, w, dy, bf16, ft):
    return O.tconv_bwd((_rb(x, bf16).astype(ft), _rb(w, bf16).astype(ft)), _rb(dy, bf16).astype(ft))


def bn_affine(x, sc, sh):
    """fmaf(x, scale, shift) of float32 operands, exactly: x * scale is exact in float64, one rounding to float32"""
    return (np.asarray(x, np.float64) * np.asarray(sc, np.float64) + np.asarray(sh, np.float64)).astype(np.float32).astype(np.float64)


def bn_stats(x):
    """float64 (mean, biased variance) per channel of the stored values"""
    x = np.asarray(x, np.float64)
    m = x.mean((0, 1, 2))
    return m, ((x - m) ** 2).mean((0, 1, 2))


def bn_stats32(x):
    """what the float32 oracle makes of them (O.bn_fwd: float32 values, means accumulated wide, rounded to float32): (mean, inv)"""
    x = np.asarray(x, np.float32)
    m = x.mean((0, 1, 2), dtype=np.float64).astype(np.float32)
    xc = x - m
    v = (xc * xc).mean((0, 1, 2), dtype=np.float64).astype(np.float32)
    return m.astype(np.float64), (np.float32(1.0) / np.sqrt(v + np.float32(O.BN_EPS))).astype(np.float64)


def bn_back(x, dy, mean, inv, gamma, ft):
    x, dy, mean, inv, gamma = (np.asarray(v, ft) for v in (x, dy, mean, inv, gamma))
    return O.bn_bwd(((x - mean) * inv, inv, gamma, True), dy)


def head_chain(feat, w, b, y, cfg, ft):
    """head, loss and the head's backward on the stored features: (logits, dfeat, dw, db)"""
    feat = np.asarray(feat, ft)
    w4 = np.asarray(w, ft).reshape(1, 1, -1, 1)
    logits, cache = O.conv2d_fwd(feat, w4, np.asarray(b, ft), 'same', None)
    _, dper = O.weighted_crossentropy(y, logits, **cfg)
    d, dw, db = O.conv2d_bwd(cache, dper / ft(feat.shape[0]))
    return logits, d, dw, db


# ---- intervals ---------------------------------------------------------------------------------------------------------------------

def stage_interval(stages, t, rnd):
    """[lo, hi] of a buffer written by `stages` = [(contribution, allowance, mask or None)], every allowance scaled by t"""
    lo = hi = 0.0
    for c, a, mask in stages:
        lo, hi = lo + c - t * a, hi + c + t * a
        if mask is not None:          # act' in {1, alpha >= 0}
            lo, hi = lo * mask, hi * mask
        if rnd:
            lo, hi = to_bf16(lo), to_bf16(hi)
    return lo, hi


def smallest_multiple(dev, stages, rnd):
    """the smallest t at which lo(t) <= dev <= hi(t) everywhere (0: exact; to 0.1 %)"""
    def ok(t):
        lo, hi = stage_interval(stages, t, rnd)
        return bool(np.all((lo <= dev) & (dev <= hi)))
    if ok(0.0):
        return 0.0
    t = 2.0 ** -20
    while not ok(t):
        t *= 2.0
        if t > 1e15:
            return float('inf')
    a, b = t / 2.0, t
    for _ in range(10):
        mid = 0.5 * (a + b)
        a, b = (a, mid) if ok(mid) else (mid, b)
    return b


# ---- the checker -------------------------------------------------------------------------------------------------------------------

class Checker:
    """ops: parse_ops(...) of the pass under test; get(op, slot, grad) -> stored view [B, H, W, C]; coef(op) -> [4, C];
    params / state0: the flat vectors the pass ran with; dtype 'bf16' or 'f32'"""

    def __init__(self, ops, get, coef, params, state0, dtype):
        self.ops, self.dtype = ops, dtype
        self._get, self._coef = get, coef
        self.p = np.asarray(params, np.float64)
        self.s0 = np.asarray(state0, np.float64)
        self.T = tensor_table(ops)
        self.results = []
        self.pool_cache = {}
        self._mem = {}

    def get(self, op, slot, grad=0):
        key = (self.ops[op][SLOTS[slot]].id, grad)
        if key not in self._mem:
            self._mem[key] = np.asarray(self._get(op, slot, grad), np.float64)
        return self._mem[key]

    def coef(self, op):
        key = ('coef', op)
        if key not in self._mem:
            self._mem[key] = np.asarray(self._coef(op), np.float32).reshape(4, -1)
        return self._mem[key]

    # which launches contract in bf16 (use_bf16 / use_bf16_tc of csrc/kernels_igemm.hip)
    def bf16_conv(self, o):
        return self.dtype == 'bf16' and o['k'] == 3 and o['inA'].C % 32 == 0 and o['inB'].C % 32 == 0 and o['out'].C % 32 == 0

    def bf16_tconv(self, o):
        return self.dtype == 'bf16' and o['inA'].C % 64 == 0 and o['out'].C % 64 == 0

    def kernel(self, o):
        if o['type'] == 'CONV':
            shape = (o['k'], o['k'], o['inA'].C + o['inB'].C, o['out'].C)
        elif o['type'] == 'TCONV':
            shape = (o['k'], o['k'], o['out'].C, o['inA'].C)
        else:
            shape = (o['inA'].C,)
        n = int(np.prod(shape))
        w = self.p[o['w_off']:o['w_off'] + n].reshape(shape)
        nb = 1 if o['type'] == 'HEAD' else shape[-1] if o['type'] == 'CONV' else shape[2] if o['type'] == 'TCONV' else shape[0]
        return w, self.p[o['b_off']:o['b_off'] + nb]

    def conv_input(self, i):
        """the conv's sources as its staging code sees them: stored, or a BatchNorm's input normalised on load (Op::elided)"""
        o, parts = self.ops[i], []
        for k in range(2 if o['inB'].C else 1):
            b = o['src_bn'][k]
            if b >= 0 and self.ops[b]['elided']:
                c = self.coef(b)
                parts.append(bn_affine(self.get(b, 0), c[0], c[1]))
            else:
                parts.append(self.get(i, k))
        return np.concatenate(parts, -1)

    def add(self, kind, name, ratio, cost, scale=1.0, **extra):
        r = dict(kind=kind, name=name, ratio=float(ratio), cost=float(cost / scale) if scale > 0 else 0.0)
        r.update(extra)
        self.results.append(r)

    def compare(self, kind, name, dev, ref, ref32, rnd=False, scale=None):
        if scale is None:
            scale = float(np.abs(ref).max())
        a = max(REL * scale + COST * float(np.abs(np.asarray(ref32, np.float64) - ref).max()), 1e-300)
        if rnd:
            ratio = smallest_multiple(dev, [(ref, a, None)], True)
        else:
            ratio = float(np.abs(dev - ref).max()) / a
        self.add(kind + ('/bf16-stored' if rnd else ''), name, ratio, float(np.abs(np.asarray(ref32, np.float64) - ref).max()), scale)

    def compare_out(self, i, kind, ref, ref32):
        o = self.ops[i]
        self.compare(kind, o['name'], self.get(i, 2), ref, ref32, rnd=bool(o['out'].hd))

    # ---- forward ---------------------------------------------------------------------------------------------------------------
    def forward(self, training, logits=None, state1=None):
        """every stored output of the pass; training: the batch statistics and (state1) the moving statistics behind the step"""
        for i, o in enumerate(self.ops):
            t = o['type']
            if t == 'CONV':
                x, (w, b), bf = self.conv_input(i), self.kernel(o), self.bf16_conv(o)
                kind = 'conv_fwd' + ('[bf16]' if bf else '[f32]')
                self.compare_out(i, kind, conv_out(x, w, b, _alpha(o), bf, np.float64), conv_out(x, w, b, _alpha(o), bf, np.float32))
            elif t == 'TCONV':
                x, (w, b), bf = self.get(i, 0), self.kernel(o), self.bf16_tconv(o)
                kind = 'tconv_fwd' + ('[bf16]' if bf else '[f32]')
                self.compare_out(i, kind, tconv_out(x, w, b, bf, np.float64), tconv_out(x, w, b, bf, np.float32))
            elif t == 'BN':
                self.bn_forward(i, training, state1)
            elif t == 'POOL':
                p = self.T[o['inA'].id]['prod']
                if p is not None and self.ops[p]['type'] == 'BN':      # fused behind the apply: maxima of the float32 values
                    c = self.coef(p)
                    xin = bn_affine(self.get(p, 0), c[0], c[1])
                else:
                    xin = self.get(i, 0)
                ref, self.pool_cache[i] = O.maxpool_fwd(xin, o['k'])
                self.compare_out(i, 'pool', ref, ref)
            elif t == 'HEAD' and logits is not None:
                w, b = self.kernel(o)
                ref = head_logits(self.get(i, 0), w, b, np.float64)
                self.compare('head_fwd', o['name'], np.asarray(logits, np.float64).reshape(ref.shape), ref, head_logits(self.get(i, 0), w, b, np.float32))
        return self.results

    def bn_forward(self, i, training, state1):
        o = self.ops[i]
        C = o['inA'].C
        x = self.get(i, 0)
        sc, sh, mean, inv = (v.astype(np.float64) for v in self.coef(i))
        gamma, beta = self.p[o['w_off']:o['w_off'] + C], self.p[o['b_off']:o['b_off'] + C]
        mm0, mv0 = self.s0[o['mm_off']:o['mm_off'] + C], self.s0[o['mv_off']:o['mv_off'] + C]
        if training:
            m, v = bn_stats(x)
            inv_ref = 1.0 / np.sqrt(v + O.BN_EPS)
            m32, inv32 = bn_stats32(x)
            am = STAT_REL * np.sqrt(v) + COST * np.abs(m32 - m) + 1e-300
            ai = STAT_REL * inv_ref + COST * np.abs(inv32 - inv_ref)
            self.add('bn_mean', o['name'], float((np.abs(mean - m) / am).max()), float((np.abs(m32 - m) / (np.sqrt(v) + 1e-300)).max()))
            self.add('bn_inv', o['name'], float((np.abs(inv - inv_ref) / ai).max()), float((np.abs(inv32 - inv_ref) / inv_ref).max()))
            if state1 is not None:
                n = x.shape[0] * x.shape[1] * x.shape[2]
                new_m = mm0 * O.BN_MOMENTUM + m * (1 - O.BN_MOMENTUM)
                new_v = mv0 * O.BN_MOMENTUM + v * (n / max(n - 1, 1)) * (1 - O.BN_MOMENTUM)
                s1 = np.asarray(state1, np.float64)
                for what, ref, off in (('mean', new_m, o['mm_off']), ('variance', new_v, o['mv_off'])):
                    tol = STATE_TOL * max(1.0, float(np.abs(ref).max()))
                    self.add('bn_moving_' + what, o['name'], float(np.abs(s1[off:off + C] - ref).max()) / tol, 0.0)
        else:
            mean_ref, inv_ref = mm0, 1.0 / np.sqrt(mv0 + O.BN_EPS)
            i32 = (np.float32(1.0) / np.sqrt(mv0.astype(np.float32) + np.float32(O.BN_EPS))).astype(np.float64)
            self.compare('bn_infer_mean', o['name'], mean, mean_ref, mean_ref)
            self.compare('bn_infer_inv', o['name'], inv, inv_ref, i32)
        # the table is consistent in itself: scale = gamma inv, shift = beta - mean scale (float32 arithmetic of the fold)
        g32, b32, i32, m32 = (v.astype(np.float32) for v in (gamma, beta, inv, mean))
        self.compare('bn_coef', o['name'] + '.scale', sc, gamma * inv, g32 * i32)
        self.compare('bn_coef', o['name'] + '.shift', sh, beta - mean * sc, b32 - m32 * sc.astype(np.float32))
        if not o['elided']:
            ref = bn_affine(x, sc, sh)
            self.compare_out(i, 'bn_apply', ref, ref)

    # ---- backward --------------------------------------------------------------------------------------------------------------
    def pool_rides(self, b, pool_into_bn):
        """the max-pool behind BatchNorm b whose backward rides in the BatchNorm's passes (fast_pool_into_bn: f32 tensors), or None"""
        if not pool_into_bn:
            return None
        o = self.ops[b]
        if o['inA'].hd or o['out'].hg or o['inA'].hg or o['out'].H % 2 or o['out'].W % 2:
            return None
        for r, s in self.T[o['out'].id]['readers']:
            q = self.ops[r]
            if q['type'] == 'POOL' and q['k'] == 2 and not q['out'].hg and not q['maskA']:
                return r
        return None

    def backward(self, y, cfg, grads, pool_into_bn=False):
        """every gradient buffer and every variable's gradient of the step whose forward pass self.forward(True) has just checked"""
        ops = self.ops
        g = np.asarray(grads, np.float64)
        contrib, riding = {}, {}
        for b, o in enumerate(ops):
            if o['type'] == 'BN':
                r = self.pool_rides(b, pool_into_bn)
                if r is not None:
                    riding[r] = b

        def var(kind, o, what, off, ref, ref32, scale=None):
            ref = np.asarray(ref, np.float64).ravel()
            self.compare(kind, '%s.%s' % (o['name'], what), g[off:off + ref.size], ref, np.asarray(ref32).ravel(), scale=scale)

        for i in range(len(ops) - 1, -1, -1):
            o, t = ops[i], ops[i]['type']
            if t == 'HEAD':
                w, b = self.kernel(o)
                r64, r32 = (head_chain(self.get(i, 0), w, b, y, cfg, ft) for ft in (np.float64, np.float32))
                contrib[(i, 0)] = (r64[1], r32[1])
                var('head_wgrad', o, 'kernel', o['w_off'], r64[2], r32[2])
                var('head_wgrad', o, 'bias', o['b_off'], r64[3], r32[3])
            elif t == 'CONV':
                x, (w, _), bf = self.conv_input(i), self.kernel(o), self.bf16_conv(o)
                dz = self.get(i, 2, 1)
                r64, r32 = (conv_back(x, w, dz, bf, ft) for ft in (np.float64, np.float32))
                ca = o['inA'].C
                if o['need_din']:
                    contrib[(i, 0)] = (r64[0][..., :ca], r32[0][..., :ca])
                    if o['inB'].C:
                        contrib[(i, 1)] = (r64[0][..., ca:], r32[0][..., ca:])
                kind = 'conv_wgrad' + ('[bf16]' if bf else '[f32]')
                var(kind, o, 'kernel', o['w_off'], r64[1], r32[1])
                var(kind, o, 'bias', o['b_off'], r64[2], r32[2])
            elif t == 'TCONV':
                x, (w, _), bf = self.get(i, 0), self.kernel(o), self.bf16_tconv(o)
                dy = self.get(i, 2, 1)
                r64, r32 = (tconv_back(x, w, dy, bf, ft) for ft in (np.float64, np.float32))
                contrib[(i, 0)] = (r64[0], r32[0])
                kind = 'tconv_wgrad' + ('[bf16]' if bf else '[f32]')
                var(kind, o, 'kernel', o['w_off'], r64[1], r32[1])
                # A bias in front of a BatchNorm: the BatchNorm's backward takes the channel mean out of dy, so the sum IS zero and
                # max|ref| is rounding noise, no scale.  The scale of a sum that cancels is the sum of the magnitudes (its condition).
                rd = self.T[o['out'].id]['readers']
                cancels = len(rd) == 1 and ops[rd[0][0]]['type'] == 'BN'
                var(kind + ('/cancelling' if cancels else ''), o, 'bias', o['b_off'], r64[2], r32[2],
                    scale=float(np.abs(_rb(dy, bf)).sum((0, 1, 2)).max()) if cancels else None)
            elif t == 'POOL':
                if i not in riding:
                    d = O.maxpool_bwd(self.pool_cache[i], self.get(i, 2, 1))
                    contrib[(i, 0)] = (d, d)
            elif t == 'BN':
                C = o['inA'].C
                pool = next((r for r, b in riding.items() if b == i), None)
                if pool is None:
                    dy = self.get(i, 2, 1)
                else:          # the routed gradient is added on the fly; dy holds what the other readers wrote, if any
                    others = [r for r, s in self.T[o['out'].id]['readers'] if r != pool and ops[r]['need_din']]
                    dy = O.maxpool_bwd(self.pool_cache[pool], self.get(pool, 2, 1)) + (self.get(i, 2, 1) if others else 0.0)
                _, _, mean, inv = self.coef(i)
                gamma = self.p[o['w_off']:o['w_off'] + C]
                r64, r32 = (bn_back(self.get(i, 0), dy, mean, inv, gamma, ft) for ft in (np.float64, np.float32))
                contrib[(i, 0)] = (r64[0], r32[0])
                var('bn_wgrad', o, 'gamma', o['w_off'], r64[1], r32[1])
                var('bn_wgrad', o, 'beta', o['b_off'], r64[2], r32[2])

        for tid, tt in sorted(self.T.items()):
            writers = sorted(((r, s) for r, s in tt['readers'] if (r, s) in contrib), reverse=True)
            if not writers:
                continue
            stages, run, kinds = [], 0.0, []
            for n, (r, s) in enumerate(writers):
                q = ops[r]
                acc = q['accA'] if s == 0 else q['accB']
                if bool(acc) != (n > 0) and not (q['type'] == 'BN' and q['inA'].hg):
                    self.add('acc_flag', q['name'], float('inf'), 0.0)
                c64, c32 = contrib[(r, s)]
                run = run + c64
                mask = None
                if q['maskA'] if s == 0 else q['maskB']:
                    mask = np.where(self.get(r, s) > 0, 1.0, q['mask_alpha'])
                    run = run * mask
                a = REL * float(np.abs(run).max()) + COST * float(np.abs(np.asarray(c32, np.float64) - c64).max())
                stages.append((c64, max(a, 1e-300), mask))
                kinds.append(q['type'].lower())
            prod = tt['prod']
            if prod is not None and ops[prod]['type'] == 'CONV' and ops[prod]['alpha'] >= 0 and not ops[prod]['premasked']:
                stages.append((0.0, 0.0, np.where(self.get(prod, 2) > 0, 1.0, ops[prod]['alpha'])))      # g_act_bwd, in place
                kinds.append('act')
            r0, s0 = writers[0]
            dev = self.get(r0, s0, 1)
            rnd = bool(tt['view'].hg)
            ratio = smallest_multiple(dev, stages, rnd)
            cost = max(float(np.abs(np.asarray(contrib[w][1], np.float64) - contrib[w][0]).max()) for w in writers)
            lo, hi = stage_interval(stages, 0.0, rnd)
            self.add('dgrad[%s]%s' % ('+'.join(kinds), '/bf16-stored' if rnd else ''), 'd(%s)' % self.tensor_name(tid), ratio, cost,
                     float(np.abs(lo).max()))
        return self.results

    def tensor_name(self, tid):
        tt = self.T[tid]
        return self.ops[tt['prod']]['name'] + '.out' if tt['prod'] is not None else 'input'


def head_logits(feat, w, b, ft):
    return (np.asarray(feat, ft) @ np.asarray(w, ft).reshape(-1, 1)) + np.asarray(b, ft)


def summarise(results):
    """{launch kind: (worst ratio, name of the worst, worst float32 cost as a share of the tensor's scale)}"""
    out = {}
    for r in results:
        k = out.get(r['kind'])
        if k is None or r['ratio'] > k[0]:
            out[r['kind']] = (r['ratio'], r['name'], max(r['cost'], k[2] if k else 0.0))
        else:
            out[r['kind']] = (k[0], k[1], max(k[2], r['cost']))
    return out


def failures(results, bound=1.0):
    return [r for r in results if not r['ratio'] <= bound]
