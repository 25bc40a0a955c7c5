"""The cases of the integrated-gradients tests (tests/test_attr_gpu.py, tests/test_attr_host.py) and their references, computed once
per session: tests/attr_ref.py in float64 (the reference) and in float32 (the cost of the number format).

  (a) unet, 3 input channels, 3 first filters, 2 levels, BatchNorm, 32 x 48, max_batch 4 run at B = 3 (ragged, non-square)
  (b) mulmo, 3 input channels, 16 first filters, 2 levels, BatchNorm, 40 x 48, B = 2 (dense data-gradient path, one first conv per
      encoder)
  (d) unet, 5 input channels, 3 first filters, 2 levels, no BatchNorm, 24 x 40, B = 2: two channel groups (4 + 1) in attr_first and
      half-filled 16 x 16 tiles on both axes
  (e) as (d) with LeakyReLU alpha = 0.999: a mask flipped by a rounding error moves the result by 1e-3 of what it moves under ReLU,
      so this case holds the strict line (a kernel that ignores or misapplies the mask is still off by about 1e-3 of the map)
  (c) configs/unet.yaml's hyper-parameters, 3 input channels, 512 x 512, B = 1, steps = 2 only: the grid structure at full width

Parameters: helpers.perturbed_params.  Inputs: uniform random, a PANEL of 8 seeds per case -- a ReLU whose pre-activation is a
rounding error away from 0 flips its mask (and a max-pool whose two largest inputs are a rounding error apart its argmax), an
m-step path has m times the chance of one, and the device's flips need not be the float32 statement's: no seed is picked because
it happens to pass; the cost of a case and quantity is the LARGEST float32-vs-float64 cost over the panel, both baselines and all
step counts."""

import numpy as np
import torch

import attr_ref
import helpers as Hp
from oracle import unet_oracle as O

PANEL = tuple(range(101, 109))           # input seeds
STEPS = (1, 4, 16)
LEAKY = {'class_name': 'LeakyReLU', 'config': {'alpha': 0.999}}
CASES = {
    'a': dict(arch='unet', C=3, H=32, W=48, max_batch=4, B=3, opts=dict(n_filters_first=3, n_downsample=2, bn=True)),
    'b': dict(arch='mulmo', C=3, H=40, W=48, max_batch=2, B=2, opts=dict(n_filters_first=16, n_downsample=2, bn=True)),
    'c': dict(arch='unet', C=3, H=512, W=512, max_batch=1, B=1, opts=dict(n_filters_first=3, n_downsample=3, bn=False)),
    'd': dict(arch='unet', C=5, H=24, W=40, max_batch=2, B=2, opts=dict(n_filters_first=3, n_downsample=2, bn=False)),
    'e': dict(arch='unet', C=5, H=24, W=40, max_batch=2, B=2, opts=dict(n_filters_first=3, n_downsample=2, bn=False, activation=LEAKY)),
}
QUANTITIES = ('signed', 'absolute', 'endpoints', 'map_l2', 'map_max')
_SPEC, _REF = {}, {}


def spec_of(name):
    """(spec, device kwargs, params {name: float64 array})"""
    if name not in _SPEC:
        c = CASES[name]
        full = dict(rate=2, kernel_size=3, conv_stride=1, padding='same')
        full.update(c['opts'])
        spec = O.ModelSpec(c['arch'], c['C'], **full)
        _SPEC[name] = (spec, Hp.device_kwargs(spec, c['H'], c['W'], c['max_batch']), Hp.perturbed_params(spec, np.float64))
    return _SPEC[name]


def input_of(name, seed):
    c = CASES[name]
    return np.random.default_rng(seed).random((c['B'], c['H'], c['W'], c['C'])).astype(np.float32)


def errors(got, ref):
    """{quantity: error} of (signed, absolute, endpoints, map) against the reference: max-abs for the sums and endpoints, the
    relative L2 error and the max-abs error for the map"""
    e = {q: float(np.abs(np.asarray(g, np.float64) - r).max()) for q, g, r in zip(QUANTITIES[:3], got, ref)}
    m, rm = np.asarray(got[3], np.float64), ref[3]
    e['map_l2'] = float(np.linalg.norm((m - rm).ravel()) / np.linalg.norm(rm.ravel()))
    e['map_max'] = float(np.abs(m - rm).max())
    return e


def reference(name, seed, steps, baseline):
    """(float64 reference (signed, absolute, endpoints, map), {quantity: float32-vs-float64 cost}) -- computed once.  The slices
    are independent (inference mode), so the small cases evaluate the whole panel as one batch: eight times fewer torch calls"""
    if (name, seed, steps, baseline) not in _REF:
        spec, kw, params = spec_of(name)
        c = CASES[name]
        group = list(PANEL) if seed in PANEL and c['H'] * c['W'] <= 4096 else [seed]
        x = np.concatenate([input_of(name, s) for s in group])
        both = [attr_ref.integrated_gradients(spec, params, x, steps, baseline, dt) for dt in (torch.float64, torch.float32)]
        for i, s in enumerate(group):
            ref, f32 = (tuple(v[i * c['B']:(i + 1) * c['B']] for v in r) for r in both)
            _REF[(name, s, steps, baseline)] = (ref, errors(f32, ref))
    return _REF[(name, seed, steps, baseline)]


def pooled_cost(name, steps=STEPS, panel=PANEL):
    """{quantity: the largest float32-vs-float64 cost over the panel, both baselines and the step counts}"""
    costs = [reference(name, s, m, bl)[1] for s in panel for m in steps for bl in attr_ref.BASELINES]
    return {q: max(c[q] for c in costs) for q in QUANTITIES}
