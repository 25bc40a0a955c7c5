"""Test double for tests/test_layerwise.py: a dense unet plan whose op table and stored tensors come from the bf16-emulating oracle
itself.  It builds the op table the way Model::build does (csrc/model.hip: ops, accumulation flags, activation-mask fusion, the
bf16-stored tensors of ig_plan_half), prints it in the text format of dnnca_debug_ops, and runs a pass launch by launch with the
statements of tests/layerwise.py on the values it has STORED (f32 tensors unrounded in float64, bf16 tensors rounded).  The
checker must reproduce it exactly.  `mutant` plants one of the defects the checker has to catch.  Test infrastructure only."""

import numpy as np

import layerwise as L
from bf16_emul_case import to_bf16
from oracle import unet_oracle as O

MUTANTS = ('halo_column', 'dropped_k_chunk', 'ragged_next_image', 'skip_overwritten', 'stale_coefficients', 'stats_unrounded',
           'tconv_mean_without_bias')


class FakeDense:
    def __init__(self, spec, H, W, max_batch, dtype='bf16', mutant=None):
        assert spec.arch == 'unet' and spec.padding == 'same' and spec.n_conv == 2
        assert mutant is None or mutant in MUTANTS
        self.spec, self.dtype, self.mutant, self.max_batch = spec, dtype, mutant, max_batch
        self.ops, self.nT, self.nS = [], 0, 0
        self._ntensors = 0
        self._build(H, W)
        self._masks()
        self._half()
        self.params = np.zeros(self.nT)
        self.state = np.zeros(self.nS)
        self.grads = np.zeros(self.nT)
        self.data, self.grad, self.coefs = {}, {}, {}
        self.prev_coefs = {}
        self.B = 0

    # ---- the plan ----------------------------------------------------------------------------------------------------------
    def _tensor(self, H, W, C):
        self._ntensors += 1
        return dict(H=H, W=W, C=C, hd=0, hg=0, id=self._ntensors)

    def _param(self, n, trainable=True):
        if trainable:
            off, self.nT = self.nT, self.nT + n
        else:
            off, self.nS = self.nS, self.nS + n
        return off

    def _op(self, type, name, inA, out, inB=None, **kw):
        o = dict(type=type, name=name, inA=inA, inB=inB, out=out, k=0, alpha=-1.0, w_off=-1, b_off=-1, mm_off=-1, mv_off=-1,
                 need_din=1, accA=0, accB=0, maskA=0, maskB=0, premasked=0, mask_alpha=0.0, elided=0, src_bn=[-1, -1])
        o.update(kw)
        self.ops.append(o)
        return o

    def _build(self, H, W):
        sp = self.spec
        K, r = sp.k, sp.rate

        def conv(name, a, b, out, need_din):
            cin = a['C'] + (b['C'] if b else 0)
            w = self._param(K * K * cin * out['C'])
            self._op('CONV', name, a, out, b, k=K, alpha=sp.alpha, need_din=int(need_din), w_off=w, b_off=self._param(out['C']))

        def bn(name, a, out):
            C = a['C']
            w, b = self._param(C), self._param(C)
            self._op('BN', name, a, out, w_off=w, b_off=b, mm_off=self._param(C, False), mv_off=self._param(C, False))

        cur = self.xin = self._tensor(H, W, sp.in_channels)
        skips, first = [], True
        for i, f in enumerate(sp.encoder_filters()):
            p = 'encoder.down%d' % i
            for j in range(2):
                a = self._tensor(H, W, f)
                conv('%s.conv%d' % (p, j), cur, None, a, not first)
                first, cur = False, a
                if sp.bn:
                    n = self._tensor(H, W, f)
                    bn('%s.bn%d' % (p, j), cur, n)
                    cur = n
            skips.append(cur)
            H, W = H // r, W // r
            pooled = self._tensor(H, W, f)
            self._op('POOL', p + '.pool', cur, pooled, k=r)
            cur = pooled
            if sp.bn:
                n = self._tensor(H, W, f)
                bn(p + '.pool_bn', cur, n)
                cur = n
        for u, f in enumerate(reversed(sp.encoder_filters())):
            p = 'decoder.up%d' % u
            H, W = H * r, W * r
            t = self._tensor(H, W, f)
            w = self._param(r * r * f * cur['C'])
            self._op('TCONV', p + '.tconv', cur, t, k=r, w_off=w, b_off=self._param(f))
            cur = t
            if sp.bn:
                n = self._tensor(H, W, f)
                bn(p + '.tconv_bn', cur, n)
                cur = n
            for j in range(2):
                a = self._tensor(H, W, f)
                conv('%s.conv%d' % (p, j), cur, skips[sp.n_down - 1 - u] if j == 0 else None, a, True)
                cur = a
                if sp.bn:
                    n = self._tensor(H, W, f)
                    bn('%s.bn%d' % (p, j), cur, n)
                    cur = n
        w = self._param(cur['C'])
        self._op('HEAD', 'head', cur, None, w_off=w, b_off=self._param(1))
        written = set()
        for o in reversed(self.ops):
            if not o['need_din']:
                continue
            o['accA'] = int(o['inA']['id'] in written)
            written.add(o['inA']['id'])
            if o['inB']:
                o['accB'] = int(o['inB']['id'] in written)
                written.add(o['inB']['id'])
        for b, o in enumerate(self.ops):
            if o['type'] == 'BN':
                for q in self.ops:
                    if q['type'] == 'CONV':
                        for k, s in enumerate(('inA', 'inB')):
                            if q[s] and q[s]['id'] == o['out']['id']:
                                q['src_bn'][k] = b

    def _readers(self, t):
        return [(q, s) for q in self.ops for s in ('inA', 'inB') if q[s] and q[s]['id'] == t['id']]

    def _masks(self):          # fast_plan_masks
        for o in self.ops:
            if o['type'] != 'CONV' or o['alpha'] < 0:
                continue
            rd = self._readers(o['out'])
            if not rd or (rd[0][0]['type'] == 'CONV' and not rd[0][0]['need_din']):
                continue
            q, s = rd[0]
            q['maskA' if s == 'inA' else 'maskB'] = 1
            q['mask_alpha'] = o['alpha']
            o['premasked'] = 1

    def _half(self):           # ig_plan_half
        if self.dtype != 'bf16':
            return

        def takes(q):
            if q['type'] == 'CONV':
                return q['k'] == 3 and all(t['C'] % 64 == 0 for t in (q['inA'], q['inB'] or q['out'], q['out']))
            return q['type'] == 'TCONV' and q['inA']['C'] % 64 == 0 and q['out']['C'] % 64 == 0

        hd, hg = {}, {}
        for bn in self.ops:
            if bn['type'] != 'BN':
                continue
            users = self._readers(bn['out'])
            ok = bool(users) and all(takes(q) if q['type'] != 'POOL' else not q['maskA'] for q, _ in users)
            if ok:
                hd[bn['out']['id']] = True
                if all(q['need_din'] for q, _ in users):
                    hg[bn['out']['id']] = True
            prod = next(q for q in self.ops if q['out'] and q['out']['id'] == bn['inA']['id'])
            pre = prod['type'] != 'CONV' or prod['alpha'] < 0 or prod['premasked']
            if len(self._readers(bn['inA'])) == 1 and pre and takes(prod):
                hd[bn['inA']['id']] = True
            if not bn['accA'] and takes(prod) and pre and (prod['type'] == 'TCONV' or prod['need_din']):
                hg[bn['inA']['id']] = True
        changed = True
        while changed:
            changed = False
            for q in self.ops:
                if q['type'] == 'CONV' and q['inB'] and hd.get(q['inA']['id'], False) != hd.get(q['inB']['id'], False):
                    hd[q['inA']['id']] = hd[q['inB']['id']] = False
                    changed = True
        for q in self.ops:
            for s in L.SLOTS:
                if q[s]:
                    q[s]['hd'], q[s]['hg'] = int(hd.get(q[s]['id'], False)), int(hg.get(q[s]['id'], False))

    def ops_text(self):
        lines = []
        for i, o in enumerate(self.ops):
            s = ('op=%d type=%s name=%s k=%d alpha=%.9g w_off=%d b_off=%d mm_off=%d mv_off=%d need_din=%d accA=%d accB=%d maskA=%d maskB=%d '
                 'premasked=%d mask_alpha=%.9g elided=%d src_bn=%d,%d') % (
                i, o['type'], o['name'], o['k'], o['alpha'], o['w_off'], o['b_off'], o['mm_off'], o['mv_off'], o['need_din'], o['accA'],
                o['accB'], o['maskA'], o['maskB'], o['premasked'], o['mask_alpha'], o['elided'], o['src_bn'][0], o['src_bn'][1])
            for slot in L.SLOTS:
                t = o[slot]
                s += ' %s=%s' % (slot, '%d,%d,%d,%d,%d,%d,%d' % (t['H'], t['W'], t['C'], t['C'], t['hd'], t['hg'], t['id']) if t else '0,0,0,0,0,0,0')
            lines.append(s)
        return '\n'.join(lines) + '\n'

    # ---- the device's face -------------------------------------------------------------------------------------------------
    def set_params(self, flat):
        self.params = np.asarray(flat, np.float64).copy()

    def set_state(self, flat):
        self.state = np.asarray(flat, np.float64).copy()

    def get_state(self):
        return self.state.copy()

    def get_grads(self):
        return self.grads.copy()

    def tensor(self, op, slot, grad):
        t = self.ops[op][L.SLOTS[slot]]
        store = self.grad if grad else self.data
        if not t or t['id'] not in store:
            raise ValueError('no buffer')
        return store[t['id']][:self.B]

    def bn_coef(self, op):
        return self.coefs[op]

    # ---- the passes --------------------------------------------------------------------------------------------------------
    def _ck(self):
        return L.Checker(L.parse_ops(self.ops_text()), None, None, self.params, self.state, self.dtype)

    def _store(self, t, v, grad=False):
        (self.grad if grad else self.data)[t['id']] = to_bf16(v) if t['hg' if grad else 'hd'] else np.asarray(v, np.float64)

    def _kernel(self, ck, i):
        return ck.kernel(ck.ops[i])

    def forward(self, x, training=False):
        ck, mut = self._ck(), self.mutant
        self.B = len(x)
        self.data = {self.xin['id']: np.asarray(x, np.float64)}
        self.prev_coefs, self.coefs = self.coefs, {}
        self.pool_cache = {}
        logits = None
        for i, o in enumerate(self.ops):
            po, t = ck.ops[i], o['type']
            if t == 'CONV':
                xs = np.concatenate([self.data[o[s]['id']] for s in ('inA', 'inB') if o[s]], -1)
                (w, b), bf = ck.kernel(po), ck.bf16_conv(po)
                al = L._alpha(po)
                z = L.conv_out(xs, w, b, None, bf, np.float64)
                if o['name'] == 'decoder.up1.conv0' and mut in ('halo_column', 'dropped_k_chunk', 'ragged_next_image'):
                    xr, wr = L._rb(xs, bf), L._rb(w, bf)
                    if mut == 'halo_column':          # tile x 0..15, rows 0..15 of image 0: the halo column 16 is read one pixel to the right
                        z[0, :16, 15] += conv_rows(xr[0, :, 17] - xr[0, :, 16], wr[:, 2])[:16]
                    elif mut == 'dropped_k_chunk':    # the centre tap's channels 32..63 never reach one 16 x 16 tile of image 0
                        z[0, :16, :16] -= xr[0, :16, :16, 32:64] @ wr[1, 1, 32:64]
                    else:                             # the last row of image 1 comes from the next image
                        bad = xr.copy()
                        bad[1, -1] = xr[2, -1]
                        z[1] = L.conv_out(bad, w, b, None, bf, np.float64)[1]
                y = z if al is None else O._act_fwd(z, al)
                self._store(o['out'], y)
            elif t == 'TCONV':
                (w, b), bf = ck.kernel(po), ck.bf16_tconv(po)
                self._store(o['out'], L.tconv_out(self.data[o['inA']['id']], w, b, bf, np.float64))
                if mut in ('stats_unrounded', 'tconv_mean_without_bias') and o['name'] == 'decoder.up0.tconv':
                    self._raw = L.tconv_out(self.data[o['inA']['id']], w, b, bf, np.float64) - (b if mut == 'tconv_mean_without_bias' else 0.0)
            elif t == 'BN':
                C = o['inA']['C']
                xin = self.data[o['inA']['id']]
                gamma, beta = self.params[o['w_off']:o['w_off'] + C], self.params[o['b_off']:o['b_off'] + C]
                mm, mv = self.state[o['mm_off']:o['mm_off'] + C], self.state[o['mv_off']:o['mv_off'] + C]
                if training:
                    m, v = L.bn_stats(xin)
                    if mut == 'stats_unrounded' and o['name'] == 'decoder.up0.tconv_bn':
                        m, v = L.bn_stats(self._raw)
                    if mut == 'tconv_mean_without_bias' and o['name'] == 'decoder.up0.tconv_bn':
                        m = L.bn_stats(self._raw)[0]
                    n = xin.shape[0] * xin.shape[1] * xin.shape[2]
                    self.state[o['mm_off']:o['mm_off'] + C] = mm * O.BN_MOMENTUM + m * (1 - O.BN_MOMENTUM)
                    self.state[o['mv_off']:o['mv_off'] + C] = mv * O.BN_MOMENTUM + v * (n / max(n - 1, 1)) * (1 - O.BN_MOMENTUM)
                else:
                    m, v = mm, mv
                mean = m.astype(np.float32)
                inv = np.float32(1.0) / np.sqrt(v.astype(np.float32) + np.float32(O.BN_EPS))
                sc = gamma.astype(np.float32) * inv
                self.coefs[i] = np.stack([sc, beta.astype(np.float32) - mean * sc, mean, inv])
                use = self.coefs[i]
                if mut == 'stale_coefficients' and training and o['name'] == 'encoder.down1.bn0' and i in self.prev_coefs:
                    use = self.prev_coefs[i]
                self._affine = L.bn_affine(xin, use[0], use[1])
                self._store(o['out'], self._affine)
                self._affine_of = o['out']['id']
            elif t == 'POOL':
                src = self._affine if self.spec.bn and self._affine_of == o['inA']['id'] else self.data[o['inA']['id']]
                y, self.pool_cache[i] = O.maxpool_fwd(src, o['k'])
                self._store(o['out'], y)
            else:
                w, b = ck.kernel(po)
                logits = L.head_logits(self.data[o['inA']['id']], w, b, np.float64)
        return logits

    def train_step(self, x, y, cfg):
        """forward(training=True) + backward at lr = 0"""
        self.forward(x, training=True)
        ck, mut = self._ck(), self.mutant
        self.grad = {}
        g = self.grads = np.zeros(self.nT)

        def put(off, v):
            g[off:off + v.size] = np.asarray(v, np.float64).ravel()

        def write(o, slot, c):
            t = o[slot]
            acc = o['accA' if slot == 'inA' else 'accB']
            if mut == 'skip_overwritten' and o['name'] == 'encoder.down0.pool':
                acc = 0
            v = (self.grad[t['id']] if acc else 0.0) + c
            if o['maskA' if slot == 'inA' else 'maskB']:
                v = v * np.where(self.data[t['id']] > 0, 1.0, o['mask_alpha'])
            self._store(t, v, grad=True)

        for i in range(len(self.ops) - 1, -1, -1):
            o, po, t = self.ops[i], ck.ops[i], self.ops[i]['type']
            if t == 'HEAD':
                w, b = ck.kernel(po)
                _, d, dw, db = L.head_chain(self.data[o['inA']['id']], w, b, y, cfg, np.float64)
                put(o['w_off'], dw)
                put(o['b_off'], db)
                write(o, 'inA', d)
            elif t == 'CONV':
                if o['alpha'] >= 0 and not o['premasked']:
                    self.grad[o['out']['id']] = self.grad[o['out']['id']] * np.where(self.data[o['out']['id']] > 0, 1.0, o['alpha'])
                xs = np.concatenate([self.data[o[s]['id']] for s in ('inA', 'inB') if o[s]], -1)
                dx, dw, db = L.conv_back(xs, ck.kernel(po)[0], self.grad[o['out']['id']], ck.bf16_conv(po), np.float64)
                put(o['w_off'], dw)
                put(o['b_off'], db)
                if o['need_din']:
                    ca = o['inA']['C']
                    if o['inB']:
                        write(o, 'inB', dx[..., ca:])
                    write(o, 'inA', dx[..., :ca])
            elif t == 'TCONV':
                dx, dw, db = L.tconv_back(self.data[o['inA']['id']], ck.kernel(po)[0], self.grad[o['out']['id']], ck.bf16_tconv(po), np.float64)
                put(o['w_off'], dw)
                put(o['b_off'], db)
                write(o, 'inA', dx)
            elif t == 'POOL':
                write(o, 'inA', O.maxpool_bwd(self.pool_cache[i], self.grad[o['out']['id']]))
            else:
                C = o['inA']['C']
                co = self.coefs[i]
                dx, dg, db = L.bn_back(self.data[o['inA']['id']], self.grad[o['out']['id']], co[2], co[3], self.params[o['w_off']:o['w_off'] + C], np.float64)
                put(o['w_off'], dg)
                put(o['b_off'], db)
                write(o, 'inA', dx)


def conv_rows(col, wk):
    """col [H, C]: one input column; wk [3, C, CO]: the taps ky = 0..2 of one kx -> their contribution to the output column [H, CO]"""
    H = col.shape[0]
    p = np.pad(col, ((1, 1), (0, 0)))
    return sum(p[ky:ky + H] @ wk[ky] for ky in range(3))
