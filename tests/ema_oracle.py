"""float64 restatement of the weight average's recurrence (dnnca_model_set_ema; tf.train.ExponentialMovingAverage with num_updates).

The oracle is fed the float32 weight vectors theta_1 .. theta_T that the device itself produced (get_params() after every step), so
the run-to-run noise of the gradients never enters the comparison: only the average's own arithmetic is compared."""

import numpy as np


def om_of(n, decay, warmup):
    """the kernel argument of update n (n = 1 for the first): (float)(1 - d_n), d_n formed in double"""
    d = min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)
    return np.float32(1.0 - d)


def run(thetas, e0, decay, warmup, first_update=1):
    """e_T in float64 from e_0 and the float32 vectors theta_first .. theta_(first + T - 1): e <- e - om * (e - theta), om float-rounded"""
    e = np.asarray(e0, np.float64).copy()
    for k, theta in enumerate(thetas):
        om = float(om_of(first_update + k, decay, warmup))
        e -= om * (e - np.asarray(theta, np.float64))
    return e


def bound(thetas, e0, floor=2.0 ** -10):
    """T * 2^-21 * M_i per element.  One update rounds at most three times (difference, product, difference) on magnitudes of at
    most 2 M_i -- 3 * 2^-24 * 2 M_i < 2^-21 M_i -- plus the rounding of om, which the oracle shares; an earlier error is multiplied by
    d <= 1.  M_i = max over the steps of max(|theta_t,i|, |e_0,i|), floored at 2^-10"""
    big = np.abs(np.asarray(e0, np.float64))
    for theta in thetas:
        big = np.maximum(big, np.abs(np.asarray(theta, np.float64)))
    return len(thetas) * 2.0 ** -21 * np.maximum(big, floor)
