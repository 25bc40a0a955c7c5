"""float64 restatement of the configurable optimizers (dnnca_model_set_optimizer): Keras 2.6 OptimizerV2 semantics [TF-2.6], written
from its documentation -- gradient transforms in Keras' order (clipvalue, then clipnorm per variable or global_clipnorm), then Adam,
AdamW (decoupled decay, the Keras >= 2.11 / PyTorch form with the learning-rate factor) or SGD with momentum / Nesterov.

One step is computed from the float32 state the device held BEFORE the step (weights, slots) and the float32 gradient it produced
(get_grads()), so the run-to-run noise of the gradients never enters: only the optimizer's own arithmetic is compared.

What the oracle shares with the device, because it is part of the definition and not of the arithmetic under test:
  * the float32 values of lr, beta_1, beta_2, epsilon, momentum, the clips (they cross the C ABI as floats);
  * lr_t = (float)(lr sqrt(1 - beta_2^t) / (1 - beta_1^t)) and lrwd = (float)(lr weight_decay), formed in double on the host;
  * gh = (float)(g * gscale), then the clamp of clipvalue, which is exact: the vector whose norm is measured.  gscale is 1 except
    under data parallel;
  * the scale c / max(norm, c), formed in double from the double norm and rounded to float once.

Bounds (the tol_* of step()), per element, with u32 = 2^-24 (half an ulp, relative):
  weights   test_adam_kernel_with_history holds g_adam's weight change to 1e-5 lr + 1.5e-7 (the second term: the float32 rounding of
            weights below 2 and of the difference).  That is the starting point for Adam / AdamW.  New terms:
              - norm clipping: the device's scale and the oracle's are both within u32 of the exact quotient, whose norms differ by
                n 2^-52 at most -- they differ by 2 u32 -- and the device rounds the product g * scale once more: the gradient the
                update sees is off by delta = 3 u32, relative.  With m' = b1 m + (1 - b1) g, v' = b2 v + (1 - b2) g^2 and
                u = m' / (sqrt v' + eps):  |du| <= ((1 - b1) / sqrt(1 - b2) + |u|) delta, because v' >= (1 - b2) g^2.  Times lr_t.
              - decay: p - lrwd p is one fused multiply-add on the device, one rounding: u32 |p| (counted as u32 (1 + lrwd) |p|,
                which also covers an unfused product).
            SGD has no normalisation, so its bound is counted from its own roundings: a' = mom a - lr g rounds two products and a
            difference, 3 u32 (|mom a| + |lr g|) =: ea (+ lr |g| delta under norm clipping); p' = p + a' adds u32 |p'|.  Nesterov:
            mom ea + 3 u32 (|mom a'| + |lr g|) + lr |g| delta + u32 |p'|.  momentum 0: u32 lr |g| + lr |g| delta + u32 |p'|.
            The rounding of the final sum, u32 max(|p|, |p'|), is floored at the 1.5e-7 of the starting point.
  slots     the starting point is 1e-6 of the slot's largest magnitude; norm clipping adds (1 - b1) |g| delta to m and
            2 (1 - b2) g^2 delta to v.  SGD's accumulator: ea as above.  SGD leaves v untouched: compared for equality.
  norms     both sides accumulate exact squares of floats in double: n 2^-52 relative for a sum of n terms (any order)."""

import collections

import numpy as np

U32 = 2.0 ** -24
DELTA = 3 * U32

Spec = collections.namedtuple('Spec', 'kind beta1 beta2 epsilon momentum nesterov weight_decay clipvalue clipnorm global_clipnorm')


def spec(kind, beta1=0.9, beta2=0.999, epsilon=1e-7, momentum=0.0, nesterov=False, weight_decay=0.0, clipvalue=0.0, clipnorm=0.0,
         global_clipnorm=0.0):
    assert kind in ('adam', 'adamw', 'sgd')
    return Spec(kind, beta1, beta2, epsilon, momentum, bool(nesterov), weight_decay, clipvalue, clipnorm, global_clipnorm)


def device_kwargs(s):
    """the keywords of DeviceModel.set_optimizer for a Spec"""
    return s._asdict()


def variable_slices(param_infos):
    """[(name, slice into the flat trainable vector)] of the trainable variables, in param_infos() order"""
    return [(name, slice(off, off + int(np.prod(shape)))) for name, shape, trainable, off in param_infos if trainable]


def f32(x):
    return float(np.float32(x))


def lr_t_of(s, lr, t, q=f32):
    """[TF-2.6] Adam._prepare_local: lr * sqrt(1 - beta_2^t) / (1 - beta_1^t), in double from the float parameters, rounded to float"""
    return q(q(lr) * np.sqrt(1.0 - q(s.beta2) ** t) / (1.0 - q(s.beta1) ** t))


def transforms(s, slices, g, gscale=1.0, q=f32):
    """[TF-2.6] OptimizerV2._transform_unaggregated_gradients order: clipvalue, clipnorm, global_clipnorm.
    -> (gh float64: g * gscale after clipvalue; global norm; per-variable norms; float32 scale per variable, as float64)"""
    if q is f32:
        gh = np.asarray(g, np.float32) * np.float32(gscale)
    else:
        gh = np.asarray(g, np.float64) * gscale
    if s.clipvalue:
        gh = np.clip(gh, -gh.dtype.type(s.clipvalue), gh.dtype.type(s.clipvalue))
    gh = gh.astype(np.float64)
    per = np.array([np.sqrt(np.sum(gh[sl] ** 2)) for _, sl in slices])
    total = float(np.sqrt(np.sum(gh ** 2)))
    scales = np.ones(len(slices))
    if s.clipnorm:
        c = q(s.clipnorm)
        scales = np.array([q(c / max(n, c)) for n in per])
    elif s.global_clipnorm:
        c = q(s.global_clipnorm)
        scales[:] = q(c / max(total, c))
    return gh, total, per, scales


def step(s, slices, decay, p, m, v, g, t, lr, gscale=1.0, round32=True):
    """one optimizer step, iteration t (1 for the first), from float32 p, m, v, g.  decay: one flag per variable (AdamW).
    -> dict p, m, v (float64), norm, norms, scales, and the per-element tolerances tol_p, tol_m, tol_v derived above.
    round32=False: nothing is rounded to float -- state, parameters, lr_t, lrwd and the scale stay doubles: the recurrences alone, as
    tests/test_optimizer_host.py holds them against torch.optim"""
    q = f32 if round32 else float
    p, m, v = (np.asarray(a, np.float32 if round32 else np.float64).astype(np.float64) for a in (p, m, v))
    gh, total, per, scales = transforms(s, slices, g, gscale, q)
    sc = np.ones_like(gh)
    for (_, sl), k in zip(slices, scales):
        sc[sl] = k
    gi = gh * sc
    delta = DELTA if (s.clipnorm or s.global_clipnorm) else 0.0
    lr32 = q(lr)
    floor = 1.5e-7
    if s.kind == 'sgd':
        mom = q(s.momentum)
        if mom == 0.0:
            p1, m1 = p - lr32 * gi, m
            tol_m = np.zeros_like(p)
            tol_p = (U32 + delta) * lr32 * np.abs(gi)
        else:
            m1 = mom * m - lr32 * gi                                    # [TF-2.6] SGD: accum = momentum * accum - lr * g
            ea = 3 * U32 * (np.abs(mom * m) + np.abs(lr32 * gi)) + delta * lr32 * np.abs(gi)
            tol_m = ea
            if s.nesterov:
                p1 = p + mom * m1 - lr32 * gi                           # var += momentum * accum - lr * g
                tol_p = mom * ea + 3 * U32 * (np.abs(mom * m1) + np.abs(lr32 * gi)) + delta * lr32 * np.abs(gi)
            else:
                p1 = p + m1                                             # var += accum
                tol_p = ea
        tol_p = tol_p + np.maximum(U32 * np.maximum(np.abs(p), np.abs(p1)), floor)
        return dict(p=p1, m=m1, v=v, norm=total, norms=per, scales=scales, tol_p=tol_p, tol_m=tol_m, tol_v=np.zeros_like(p))
    b1, b2, eps = q(s.beta1), q(s.beta2), q(s.epsilon)
    lr_t = lr_t_of(s, lr, t, q)
    m1 = m * b1 + gi * (1.0 - b1)                                       # [TF-2.6] Adam: m_t = beta_1 m + (1 - beta_1) g
    v1 = v * b2 + gi * gi * (1.0 - b2)                                  #               v_t = beta_2 v + (1 - beta_2) g^2
    u = m1 / (np.sqrt(v1) + eps)
    p0, tol_decay = p, 0.0
    if s.kind == 'adamw':
        lrwd = q(lr32 * q(s.weight_decay))                          # decoupled decay first: p <- p - lr * weight_decay * p
        flags = np.zeros_like(p)
        for (_, sl), d in zip(slices, decay):
            flags[sl] = 1.0 if d else 0.0
        p0 = p - lrwd * p * flags
        tol_decay = flags * U32 * (1.0 + lrwd) * np.abs(p)
    p1 = p0 - lr_t * u                                                  # p <- p - lr_t m_t / (sqrt(v_t) + eps)
    tol_p = 1e-5 * lr32 + floor + tol_decay + lr_t * ((1.0 - b1) / np.sqrt(1.0 - b2) + np.abs(u)) * delta
    tol_m = 1e-6 * np.abs(m1).max() + (1.0 - b1) * np.abs(gi) * delta
    tol_v = 1e-6 * np.abs(v1).max() + 2.0 * (1.0 - b2) * gi * gi * delta
    return dict(p=p1, m=m1, v=v1, norm=total, norms=per, scales=scales, tol_p=tol_p, tol_m=tol_m, tol_v=tol_v)


def norm_tol(norm, n):
    """n 2^-52 relative: two double accumulations of n exact squares, in whatever order (floored for a zero norm)"""
    return np.maximum(np.abs(norm) * n * 2.0 ** -52, 1e-300)


def check(got_p, got_m, got_v, want):
    """the worst error / bound of the three vectors against a step()'s result (<= 1 passes)"""
    worst = {}
    for key, got in (('p', got_p), ('m', got_m), ('v', got_v)):
        err = np.abs(np.asarray(got, np.float64) - want[key])
        tol = want['tol_' + key]
        if not np.any(tol):
            worst[key] = 0.0 if not np.any(err) else np.inf
        else:
            worst[key] = float((err / np.maximum(tol, 1e-300)).max())
    return worst
