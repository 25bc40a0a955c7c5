"""The per-launch comparison of tests/test_layerwise_gpu.py as a stand-alone program, so that it can run in a child process with
DNNCA_IGB_NW = 4 / 8 (the library reads the switch once per process; see tests/bf16_emul_case.py).  Prints one JSON line.

    python tests/layerwise_case.py <case name>

A case builds the model, sets helpers.perturbed_params weights and state, runs forward(training=False) and one train_step(lr = 0),
reads every stored tensor back (csrc/debug_tools.hip) and holds every launch to tests/layerwise.py.  The case table is shared with
tests/test_layerwise.py, which proves on the CPU that every case can decide (float32 cost below 1e-4 of every tensor's scale)."""

import ctypes as C
import json
import os
import sys
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import helpers as Hp                      # noqa: E402
import layerwise as L                     # noqa: E402
from oracle import unet_oracle as O       # noqa: E402

LOSS = dict(weight_mul=3.0)
SHIFT_SIGMAS = 16.0                       # tests/operating_points.py: SHIFT_SIGMAS

# all unet: the smallest shapes that leave partial 16 x 16 and 32 x 16 tiles in both directions and still build every launch of the mix
CASES = OrderedDict([
    ('bn64_2x16x16', dict(f0=64, n_down=2, bn=True, cin=32, B=2, max_batch=2, H=16, W=16, dtype='bf16')),      # the whole-step test's 0.8 case
    ('bn64_3of4x24x40', dict(f0=64, n_down=2, bn=True, cin=32, B=3, max_batch=4, H=24, W=40, dtype='bf16')),   # ragged, non-square
    ('bn32_2x24x24', dict(f0=32, n_down=2, bn=True, cin=32, B=2, max_batch=2, H=24, W=24, dtype='bf16')),      # mixed f32 / bf16 storage
    ('nobn64_2x24x40', dict(f0=64, n_down=2, bn=False, cin=32, B=2, max_batch=2, H=24, W=40, dtype='bf16')),   # no stored bf16 z
    ('bn64_c1_2x40x24', dict(f0=64, n_down=2, bn=True, cin=1, B=2, max_batch=2, H=40, W=24, dtype='bf16')),    # unet_big's first layer
    ('bn64_1x48x48', dict(f0=64, n_down=2, bn=True, cin=32, B=1, max_batch=1, H=48, W=48, dtype='bf16')),      # beyond the whole-step test
    ('f32_bn64_2x24x40', dict(f0=64, n_down=2, bn=True, cin=32, B=2, max_batch=2, H=24, W=40, dtype='f32')),   # control: the checker's floor
    # the first case's network with every *.tconv.bias moved by +-16 sigma of its channel (tests/operating_points.py)
    ('bn64_2x16x16_shift', dict(f0=64, n_down=2, bn=True, cin=32, B=2, max_batch=2, H=16, W=16, dtype='bf16', shift=SHIFT_SIGMAS)),
])


def spec_of(case):
    return O.ModelSpec('unet', case['cin'], rate=2, kernel_size=3, conv_stride=1, padding='same', n_filters_first=case['f0'],
                       n_downsample=case['n_down'], bn=case['bn'])


def inputs(case):
    """(spec, params, x, y): uniform noise, a rectangle of positives in every image"""
    spec = spec_of(case)
    B, H, W = case['B'], case['H'], case['W']
    x = np.random.default_rng(3).random((B, H, W, case['cin'])).astype(np.float32)
    y = np.zeros((B, H, W), np.float32)
    for b in range(B):
        y[b, H // 4:H // 2, W // 4 + b:W // 2 + b] = 1.0
    params = Hp.perturbed_params(spec, np.float64)
    if case.get('shift'):
        import operating_points as OP
        params = OP.shift_tconv_bias(spec, params, x, case['shift'])
    return spec, params, x, y


def check_model(case, ops_text, forward, train_step, tensor, bn_coef, get_grads, get_state, params, state0, x, y, pool_into_bn):
    """the two passes of a case on anything with the device's face; returns (results of the inference pass, of the train step)"""
    logits = forward(x)
    ck = L.Checker(L.parse_ops(ops_text()), tensor, bn_coef, params, state0, case['dtype'])
    r_eval = list(ck.forward(False, logits=logits))
    train_step(x, y)
    ck = L.Checker(L.parse_ops(ops_text()), tensor, bn_coef, params, state0, case['dtype'])
    ck.forward(True, state1=get_state() if case['bn'] else None)
    r_train = list(ck.backward(y, LOSS, get_grads(), pool_into_bn=pool_into_bn()))
    return r_eval, r_train


def report(results):
    return {k: [v[0], v[1], v[2]] for k, v in L.summarise(results).items()}


# ---- the device ----------------------------------------------------------------------------------------------------------------
_FP = C.POINTER(C.c_float)


class Readback:
    """ctypes bindings of the read-back aids of csrc/debug_tools.hip"""

    def __init__(self, dm, batch):
        self.dm, self.batch = dm, batch
        lib = dm.lib
        lib.dnnca_debug_ops.restype = lib.dnnca_debug_tensor.restype = lib.dnnca_debug_bn_coef.restype = C.c_int
        lib.dnnca_debug_ops.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        lib.dnnca_debug_tensor.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _FP, C.c_size_t]
        lib.dnnca_debug_bn_coef.argtypes = [C.c_void_p, C.c_int, _FP]
        self.ops = None

    def _ok(self, rc):
        if rc != 0:
            raise RuntimeError(self.dm.lib.dnnca_last_error().decode())

    def ops_text(self):
        buf = C.create_string_buffer(1 << 20)
        self._ok(self.dm.lib.dnnca_debug_ops(self.dm.handle, buf, len(buf)))
        self.ops = L.parse_ops(buf.value.decode())
        return buf.value.decode()

    def tensor(self, op, slot, grad, batch=None):
        v = self.ops[op][L.SLOTS[slot]]
        out = np.empty((self.batch if batch is None else batch, v.H, v.W, v.C), np.float32)
        self._ok(self.dm.lib.dnnca_debug_tensor(self.dm.handle, op, slot, grad, out.shape[0], out.ctypes.data_as(_FP), out.size))
        return out

    def tensor_n(self, op, slot, grad, batch, n):
        """[return code, message] of a call that is expected to be refused"""
        out = np.empty(max(n, 1), np.float32)
        rc = self.dm.lib.dnnca_debug_tensor(self.dm.handle, op, slot, grad, batch, out.ctypes.data_as(_FP), n)
        return [rc, self.dm.lib.dnnca_last_error().decode() if rc else '']

    def bn_coef(self, op):
        out = np.empty((4, self.ops[op]['inA'].C), np.float32)
        self._ok(self.dm.lib.dnnca_debug_bn_coef(self.dm.handle, op, out.ctypes.data_as(_FP)))
        return out


def run(device, name):
    case = CASES[name]
    spec, params, x, y = inputs(case)
    m = device.DeviceModel(**Hp.device_kwargs(spec, case['H'], case['W'], case['max_batch'], dtype=case['dtype']))
    try:
        flat, state0 = O.flatten(spec, params), O.flatten(spec, params, trainable=False)
        m.set_params(flat)
        if m.n_state:
            m.set_state(state0)
        rb = Readback(m, case['B'])
        plans = {}

        def forward(xv):
            out = m.forward(xv, training=False, return_logits=True)[1]
            plans['eval'] = Hp.inference_plan_names(m, case['B'])
            return out

        def train_step(xv, yv):
            plans['loss'] = float(m.train_step(xv, yv, 0.0, m.loss_cfg(**LOSS)).loss)
            rows = m.plan(variants=True, batch=case['B'])
            plans['train'] = sorted(set(r[0] for r in rows) | set(r[0].split('#')[0] for r in rows))

        def pool_into_bn():
            return any(n.startswith('bn_bwd_apply#p') and not n.endswith('#p0') for n in plans['train'])

        r_eval, r_train = check_model(case, rb.ops_text, forward, train_step, rb.tensor, rb.bn_coef, m.get_grads, m.get_state,
                                      flat.astype(np.float32), state0.astype(np.float32), x, y, pool_into_bn)
        # the aids refuse what they cannot serve
        last = len(rb.ops) - 1
        n_out = int(np.prod([case['B'], rb.ops[0]['out'].H, rb.ops[0]['out'].W, rb.ops[0]['out'].C]))
        refusals = [rb.tensor_n(0, 2, 0, case['max_batch'] + 1, n_out), rb.tensor_n(0, 2, 0, case['B'], n_out + 1), rb.tensor_n(last, 2, 0, case['B'], 1)]
        bf16_stored = sorted(set('%s.%s%s' % (o['name'], s, '.g' if g else '') for o in rb.ops for s in L.SLOTS for g in (0, 1)
                                 if (o[s].hg if g else o[s].hd)))
    finally:
        m.close()
    return dict(case=name, eval=report(r_eval), train=report(r_train), fail_eval=L.failures(r_eval), fail_train=L.failures(r_train),
                plan=plans['train'], plan_eval=plans['eval'], loss=plans['loss'], refusals=refusals, bf16_stored=bf16_stored)


if __name__ == '__main__':
    from dnncancerannotator_amd import device as dev
    dev.init_device(0)
    print(json.dumps(run(dev, sys.argv[1])))
