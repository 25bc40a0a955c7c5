"""Slices of the reference's region-metric tests (annotator/tests/test_region_metrics.py), restated in numpy: circles of radius
10..30 on 200 x 200 slices, a batch of 10, the lesions kept or dropped by a shuffled indicator, so the expected counts are known by
construction.  Shared by tests/test_region_metrics_host.py (oracle) and tests/test_region_metrics_gpu.py (device)."""

import numpy as np

SIZE, BATCH = 200, 10
THRESHOLDS_1 = np.array([0.5], np.float32)
THRESHOLDS_10 = np.array([0.001] + [i / 9 for i in range(1, 10)], np.float32)     # [0.001, 1/9, ..., 1]


def draw_circle(img, radius, cx, cy, value=1.0):
    """test_region_metrics.py draw_circle: pixels (row, col) with sqrt((col - cx)^2 + (row - cy)^2) < radius get += value"""
    h, w = img.shape
    rows, cols = np.mgrid[0:h, 0:w]
    dist = np.sqrt(((cols - cx) ** 2 + (rows - cy) ** 2).astype(np.float32))
    return img + (dist < np.float32(radius)).astype(img.dtype) * img.dtype.type(value)


class Scenario:
    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.rng = rng
        self.radius = rng.integers(10, 30, BATCH)
        self.cx, self.cy = rng.integers(30, 70, BATCH), rng.integers(80, 120, BATCH)
        self.cx_off, self.cy_off = rng.integers(130, 170, BATCH), rng.integers(80, 120, BATCH)

    def circles(self, off=False):
        cx, cy = (self.cx_off, self.cy_off) if off else (self.cx, self.cy)
        return np.stack([draw_circle(np.zeros((SIZE, SIZE), np.float32), r, x, y) for r, x, y in zip(self.radius, cx, cy)])

    def indicator(self, rate):
        n = int(BATCH * rate)
        return self.rng.permutation(np.r_[np.ones(n, np.float32), np.zeros(BATCH - n, np.float32)]), n

    def tp_fn(self, rate):
        """every slice has a lesion; the prediction finds a `rate` share of them -> (y, prob, tp, fn)"""
        y = self.circles()
        ind, n = self.indicator(rate)
        return y, y * ind[:, None, None], n, BATCH - n

    def tp_fp(self, rate):
        """every slice has a predicted region; a `rate` share of them is a lesion -> (y, prob, tp, fp)"""
        p = self.circles()
        ind, n = self.indicator(rate)
        return p * ind[:, None, None], p, n, BATCH - n

    def off(self, rate):
        """predicted regions far from every lesion on a `rate` share of the slices -> (prob addend, count)"""
        ind, n = self.indicator(rate)
        return self.circles(off=True) * ind[:, None, None], n


def scenarios(seed):
    """[(name, y, prob, expected (tp_label, fn, tp_pred, fp) for every threshold)]"""
    s = Scenario(seed)
    out = []
    for rate in (0.0, 0.4, 0.5, 1.0):
        y, p, tp, fn = s.tp_fn(rate)
        out.append(('tp_fn_%.1f' % rate, y, p, (tp, fn, tp, 0)))
        y, p, tp, fp = s.tp_fp(rate)
        out.append(('tp_fp_%.1f' % rate, y, p, (tp, 0, tp, fp)))
    y, p, tp, fn = s.tp_fn(0.4)
    offs, n_off = s.off(0.7)
    out.append(('mixed', y, p + offs, (tp, fn, tp, n_off)))
    z = np.zeros((BATCH, SIZE, SIZE), np.float32)
    out.append(('null', z, z.copy(), (0, 0, 0, 0)))
    return out


def random_slices(seed, n=20, size=SIZE, lo=0.2, hi=1.0):
    """test_region_metrics.py generate_random_samples: 5 circles of radius U(5, size / 20) anywhere, labels as counts of circles,
    predictions of 5 other circles with graded probabilities U(lo, hi) (summed where they overlap)"""
    rng = np.random.default_rng(seed)

    def one(graded, near=None):
        img = np.zeros((size, size), np.float32)
        centres = []
        for i in range(5):
            r, cx, cy = rng.uniform(5.0, max(size / 20, 8.0)), rng.uniform(0, size), rng.uniform(0, size)
            if near is not None and i < 3:          # three of the predicted circles near a lesion: matches and misses both occur
                r, cx, cy = near[i][0] * rng.uniform(0.6, 1.4), near[i][1] + rng.uniform(-6, 6), near[i][2] + rng.uniform(-6, 6)
            centres.append((r, cx, cy))
            img = draw_circle(img, r, cx, cy, rng.uniform(lo, hi) if graded else 1.0)
        return img, centres

    ys, ps = [], []
    for _ in range(n):
        y, c = one(False)
        ys.append(y)
        ps.append(one(True, c)[0])
    return np.stack(ys), np.stack(ps)
