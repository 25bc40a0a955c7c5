"""The bootstrap over exams of dnnca_bootstrap_sums / dnnca_bootstrap_detection (include/dnnca.h) in numpy and Python integers:
the draws from intensity_oracle.philox4x32_10, the multiplicities, the weighted statistics as the header defines them, AP as a
fractions.Fraction converted once.  Test infrastructure only."""

from fractions import Fraction

import numpy as np

from intensity_oracle import philox4x32_10

FP_EIGHTHS = (1, 2, 4, 8, 16, 32, 64)      # int(x * 8) of casewise.DETECTION_FP_RATES
EXAM_DTYPE = np.dtype([('tumours', '<i4'), ('score_rank', '<i4')])
CANDIDATE_DTYPE = np.dtype([('exam', '<i4'), ('hit', '<i4'), ('level', '<i4')])
ROW_DTYPE = np.dtype([('positive_exams', '<i8'), ('tumours', '<i8'), ('candidates', '<i8'), ('tp', '<i8'), ('fp', '<i8'),
                      ('auroc_pairs', '<i8'), ('auroc_twice', '<i8'), ('tp_at', '<i8', (7,)), ('ap', '<f8')])


def plain(E):
    return np.arange(E, dtype=np.int32), np.array([E], np.int32)


def draws(E, pool, strata, R, seed):
    """[R, E]: the exam every draw of every replicate picks"""
    pool, strata = np.asarray(pool, np.int64), np.asarray(strata, np.int64)
    assert strata.sum() == E and sorted(pool.tolist()) == list(range(E))
    quads = (E + 3) // 4
    counter = np.zeros((R, quads, 4), np.uint32)
    counter[..., 0] = np.arange(quads, dtype=np.uint32)[None, :]
    counter[..., 1] = np.arange(R, dtype=np.uint32)[:, None]
    x = philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32)).reshape(R, quads * 4)[:, :E].astype(np.uint64)
    ends = np.cumsum(strata)
    s = np.searchsorted(ends, np.arange(E), side='right')
    n, o = strata[s].astype(np.uint64), (ends - strata)[s]
    return pool[o[None, :] + ((x * n[None, :]) >> np.uint64(32)).astype(np.int64)]


def multiplicities(E, pool, strata, R, seed):
    """[R, E] int64: how often every exam is drawn"""
    return np.stack([np.bincount(d, minlength=E) for d in draws(E, pool, strata, R, seed)]).astype(np.int64)


def sums(cols, mult):
    """[R, K] int64 (the products stay below 2^46 and their sums below 2^63 for every E the library takes)"""
    return np.asarray(mult, np.int64) @ np.asarray(cols, np.int64)


def detection_row(exams, cands, m):
    """the statistics of one replicate with multiplicities m [E]: dict of Python integers, 'ap_exact' (Fraction; None without a
    drawn tumour) and 'ap' (float, 0.0 for None)"""
    E = len(exams)
    m = [int(v) for v in m]
    tum, rank = [int(t) for t in exams['tumours']], [int(r) for r in exams['score_rank']]
    T = sum(a * t for a, t in zip(m, tum))
    P = sum(a for a, t in zip(m, tum) if t > 0)
    twice = sum(m[p] * m[n] * (2 * (rank[p] > rank[n]) + (rank[p] == rank[n])) for p in range(E) if tum[p] > 0 and m[p]
                for n in range(E) if tum[n] == 0 and m[n])
    tp = fp = before = 0
    tp_at, ap = [0] * 7, Fraction(0)
    for i, c in enumerate(cands):
        w = m[int(c['exam'])]
        tp, fp = tp + w * int(c['hit']), fp + w * (1 - int(c['hit']))
        if i + 1 == len(cands) or int(cands[i + 1]['level']) != int(c['level']):         # the level ends here
            if T > 0 and tp + fp > 0:
                ap += Fraction((tp - before) * tp, T * (tp + fp))
            for k, x8 in enumerate(FP_EIGHTHS):
                if fp * 8 <= x8 * E:
                    tp_at[k] = tp
            before = tp
    return dict(positive_exams=P, tumours=T, candidates=tp + fp, tp=tp, fp=fp, auroc_pairs=P * (E - P), auroc_twice=twice, tp_at=tp_at,
                ap_exact=ap if T > 0 else None, ap=float(ap) if T > 0 else 0.0)


def detection(exams, cands, mult):
    """(rows structured [R] of ROW_DTYPE, the exact APs [R]) over the multiplicities mult [R, E]"""
    rows, exact = np.zeros(len(mult), ROW_DTYPE), []
    for r, m in enumerate(mult):
        d = detection_row(exams, cands, m)
        exact.append(d.pop('ap_exact'))
        for k, v in d.items():
            rows[r][k] = v
    return rows, exact


def levels_of(cands):
    return int(cands['level'][-1]) + 1 if len(cands) else 0
