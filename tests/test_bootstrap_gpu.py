"""-m gpu: the bootstrap over exams through the C ABI (kernels_bootstrap.hip: boot_sums, boot_detect; dnnca_bootstrap_sums,
dnnca_bootstrap_detection) against tests/bootstrap_oracle.py.

Multiplicities, sums and every integer of a detection row must EQUAL the oracle's; ap is held to the oracle's exact fraction
within (L + 8) 2^-53 relative (at most four roundings per non-negative term plus L - 1 additions) and is 0.0 exactly where the
fraction is 0; two calls are bit-identical.  Host outputs carry guard regions pre-filled with a sentinel."""

import ctypes as C

import numpy as np
import pytest

import bootstrap_cases as BC
import bootstrap_oracle as BO
from test_lesion_gpu import SENTINEL, UNET

pytestmark = pytest.mark.gpu

EINVAL = -1
SEEDS = (0, 1, (1 << 63) + 5)
I32 = C.POINTER(C.c_int32)


@pytest.fixture(scope='module')
def dm(gpu):
    m = gpu.DeviceModel('unet', 1, 64, 64, 3, **UNET)
    yield m
    m.close()


def raw(n_items, dtype, extra=4):
    return np.full((n_items + extra) * np.dtype(dtype).itemsize, SENTINEL, np.uint8).view(dtype)


def untouched(*bufs):
    return all((b.view(np.uint8) == SENTINEL).all() for b in bufs)


def i32(a):
    return None if a is None else a.ctypes.data_as(I32)


def sums_call(dm, cols, pool, strata, R, seed, S=None, E=None, K=None):
    """dnnca_bootstrap_sums on guarded outputs -> (return code, out [R, K], multiplicities [R, E], the guarded buffers)"""
    E = cols.shape[0] if E is None else E
    K = cols.shape[1] if K is None else K
    out, mult = raw(max(R, 1) * max(K, 1), np.int64), raw(max(R, 1) * max(E, 1), np.uint16)
    S = (0 if strata is None else len(strata)) if S is None else S
    rc = dm.lib.dnnca_bootstrap_sums(dm.handle, i32(cols), E, K, i32(pool), i32(strata), S, R, seed,
                                     out.ctypes.data_as(C.POINTER(C.c_int64)), mult.ctypes.data_as(C.POINTER(C.c_uint16)))
    if rc:
        return rc, None, None, (out, mult)
    assert untouched(out[R * K:], mult[R * E:]), 'written past an output'
    return rc, out[:R * K].reshape(R, K).copy(), mult[:R * E].reshape(R, E).copy(), (out, mult)


def detection_call(dm, exams, cands, pool, strata, R, seed, E=None, N=None, S=None):
    """dnnca_bootstrap_detection on guarded outputs -> (return code, rows [R], multiplicities [R, E], the guarded buffers)"""
    from dnncancerannotator_amd import _lib
    E = len(exams) if E is None else E
    N = len(cands) if N is None else N
    out, mult = raw(max(R, 1), BO.ROW_DTYPE), raw(max(R, 1) * max(E, 1), np.uint16)
    rc = dm.lib.dnnca_bootstrap_detection(dm.handle, None if exams is None else exams.ctypes.data_as(C.POINTER(_lib.BootstrapExam)), E,
                                          None if cands is None else cands.ctypes.data_as(C.POINTER(_lib.BootstrapCandidate)), N,
                                          i32(pool), i32(strata), len(strata) if S is None else S, R, seed,
                                          out.ctypes.data_as(C.POINTER(_lib.BootstrapDetectionRow)), mult.ctypes.data_as(C.POINTER(C.c_uint16)))
    if rc:
        return rc, None, None, (out, mult)
    assert untouched(out[R:], mult[R * E:]), 'written past an output'
    return rc, out[:R].copy(), mult[:R * E].reshape(R, E).copy(), (out, mult)


def uneven(E):
    """two uneven strata, 1 + (E - 1), over a pool that is not the identity"""
    return np.arange(E, dtype=np.int32)[::-1].copy(), np.array([1, E - 1], np.int32)


# ---- 1. the multiplicities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [1, 2, 5, 63, 64, 65, 257, 1025])
def test_multiplicities_equal_the_oracle(dm, E):
    cols = np.ones((E, 1), np.int32)
    exams, cands = np.zeros(E, BO.EXAM_DTYPE), np.zeros(0, BO.CANDIDATE_DTYPE)
    for pool, strata in [BO.plain(E)] + ([uneven(E)] if E > 1 else []):
        for seed in SEEDS:
            for R in (1, 3, 130):
                want = BO.multiplicities(E, pool, strata, R, seed)
                if R == 3:           # the same table from either call
                    rc, _, got, _ = detection_call(dm, exams, cands, pool, strata, R, seed)
                else:
                    rc, total, got, _ = sums_call(dm, cols, pool, strata, R, seed)
                    assert rc == 0 and (total == E).all()
                what = 'E %d strata %s seed %d R %d' % (E, strata.tolist(), seed, R)
                assert rc == 0 and got.tolist() == want.tolist(), what
                assert (got.sum(1) == E).all(), what
                at = 0
                for n in strata:     # within a stratum the draws stay in it
                    assert (got[:, pool[at:at + n]].sum(1) == n).all(), what
                    at += n


# ---- 2. bootstrap_sums -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E,K', [(5, 1), (65, 7), (257, 64), (1025, 7), (1025, 64)])
def test_sums_equal_the_oracle(dm, E, K):
    rng = np.random.default_rng(E * 100 + K)
    cols = rng.integers(-1000, 1000, (E, K)).astype(np.int32)
    if E == 1025:                    # the sums pass 2^32 in either direction
        cols[:, 0], cols[:, 1] = 2 ** 31 - 1, -(2 ** 31 - 1)
        cols[::2, 2] = 2 ** 31 - 1
        cols[1::2, 2] = -(2 ** 31 - 1)
    for pool, strata in (BO.plain(E), uneven(E)):
        rc, got, mult, _ = sums_call(dm, cols, pool, strata, 9, 3)
        want = BO.sums(cols, BO.multiplicities(E, pool, strata, 9, 3))
        assert rc == 0 and got.tolist() == want.tolist()
        if E == 1025:
            assert abs(int(got[0, 0])) > 2 ** 32 and abs(int(got[0, 1])) > 2 ** 32
        rc, again, mult2, _ = sums_call(dm, cols, pool, strata, 9, 3)
        assert again.tobytes() == got.tobytes() and mult2.tobytes() == mult.tobytes()


# ---- 3. bootstrap_detection --------------------------------------------------------------------------------------------------
def tile():
    from dnncancerannotator_amd import _lib
    return _lib.BOOTSTRAP_TILE


def exams_of(E, seed, tumours=True):
    rng = np.random.default_rng(seed)
    exams = np.zeros(E, BO.EXAM_DTYPE)
    if tumours:
        exams['tumours'] = rng.integers(0, 3, E) * (rng.random(E) < 0.6)
    scores = rng.integers(0, max(2, E // 2), E)                      # tied scores
    exams['score_rank'] = np.unique(scores, return_inverse=True)[1]
    return exams


def cands_of(E, N, seed, levels='mixed', exams=None, skip=()):
    """N candidates over the exams not in `skip`; levels: 'one', 'distinct', 'mixed' (runs of 1..5), or an array"""
    rng = np.random.default_rng(seed + 17)
    cands = np.zeros(N, BO.CANDIDATE_DTYPE)
    allowed = np.array([e for e in range(E) if e not in skip], np.int32)
    cands['exam'] = allowed[rng.integers(0, len(allowed), N)]
    positive = exams['tumours'][cands['exam']] > 0 if exams is not None else np.ones(N, bool)
    cands['hit'] = (rng.random(N) < 0.5) & positive
    if isinstance(levels, str):
        step = {'one': np.zeros(N, np.int32), 'distinct': np.ones(N, np.int32), 'mixed': (rng.random(N) < 0.4).astype(np.int32)}[levels]
        if N:
            step[0] = 0
        levels = np.cumsum(step)
    cands['level'] = levels
    return cands


def detection_cases():
    T = tile()
    out = []
    for N in (0, 1, 255, 256, 257, 2 * T + 3):
        ex = exams_of(40, N)
        out.append(('N %d' % N, ex, cands_of(40, N, N, exams=ex)))
    ex = exams_of(33, 1)
    out.append(('one level', ex, cands_of(33, T + 9, 2, 'one', exams=ex)))
    out.append(('all levels distinct', ex, cands_of(33, T + 9, 3, 'distinct', exams=ex)))
    # a level of 40 candidates that straddles the first tile edge, single levels around it
    lv = np.concatenate([np.arange(T - 20), np.full(40, T - 20), T - 19 + np.arange(50)])
    out.append(('a level across a tile edge', ex, cands_of(33, len(lv), 4, lv, exams=ex)))
    # a level longer than a tile that ends inside the third one
    lv = np.concatenate([np.arange(10), np.full(2 * T + 5, 10), 11 + np.arange(30) // 2])
    out.append(('a level longer than a tile', ex, cands_of(33, len(lv), 5, lv, exams=ex)))
    # the top level belongs to one exam of three: a third of the replicates give it no weight
    ex3 = exams_of(3, 6)
    ex3['tumours'] = [1, 0, 2]
    c = cands_of(3, 30, 7, 'mixed', exams=ex3, skip=(0,))
    c['level'] += 1
    top = np.zeros(2, BO.CANDIDATE_DTYPE)
    top['hit'] = [1, 0]
    out.append(('a zero-weight top level', ex3, np.concatenate([top, c])))
    ex = exams_of(20, 8)
    out.append(('exams without candidates', ex, cands_of(20, 300, 9, exams=ex, skip=tuple(range(0, 20, 2)))))
    ex = exams_of(20, 10, tumours=False)
    out.append(('no tumours at all', ex, cands_of(20, 300, 11, exams=ex)))
    ex2 = np.zeros(2, BO.EXAM_DTYPE)
    ex2['tumours'], ex2['score_rank'] = [1, 0], [1, 0]
    out.append(('one positive and one negative exam', ex2, cands_of(2, 5, 12, exams=ex2)))
    return out


def hold_ap(got, exact, L, what):
    for r, (g, x) in enumerate(zip(got, exact)):
        if not x:                    # None (no tumour drawn) or an exact 0
            assert g == 0.0, '%s: replicate %d ap %r where the exact value is 0' % (what, r, g)
            continue
        err = abs(BO.Fraction(float(g)) - x) / x
        assert err <= BO.Fraction(L + 8, 2 ** 53), '%s: replicate %d ap %r off by %.3g (bound %.3g)' % (
            what, r, g, float(err), (L + 8) * 2.0 ** -53)


def test_detection_equals_the_oracle(dm):
    R, seed = 24, 5
    for what, exams, cands in detection_cases():
        E = len(exams)
        for pool, strata in [BO.plain(E)] + ([uneven(E)] if E > 2 else []):
            rc, got, mult, _ = detection_call(dm, exams, cands, pool, strata, R, seed)
            assert rc == 0, what
            want_mult = BO.multiplicities(E, pool, strata, R, seed)
            assert mult.tolist() == want_mult.tolist(), what
            want, exact = BO.detection(exams, cands, want_mult)
            for name in BO.ROW_DTYPE.names[:-1]:
                assert got[name].tolist() == want[name].tolist(), '%s: %s' % (what, name)
            hold_ap(got['ap'], exact, BO.levels_of(cands), what)
            rc, again, _, _ = detection_call(dm, exams, cands, pool, strata, R, seed)
            assert again.tobytes() == got.tobytes(), what + ': differs from run to run'
            if what == 'no tumours at all':
                assert (got['tumours'] == 0).all() and (got['ap'] == 0.0).all()
            if what == 'a zero-weight top level':
                assert ((mult[:, 0] == 0) & (got['candidates'] > 0)).any()
            if what == 'one positive and one negative exam' and len(strata) == 1:
                assert 4 <= int((got['auroc_pairs'] == 0).sum()) <= R - 4


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(dm):
    E, K, R = 6, 3, 4
    cols = np.ones((E, K), np.int32)
    pool, strata = BO.plain(E)
    exams, cands = exams_of(E, 1), cands_of(E, 10, 1)
    bad_pool = pool.copy()
    bad_pool[2] = 1

    def cand(**kw):
        c = cands.copy()
        for k, (i, v) in kw.items():
            c[k][i] = v
        return c

    def exam(**kw):
        x = exams.copy()
        for k, v in kw.items():
            x[k][0] = v
        return x
    sums = [dict(E=0), dict(E=16385), dict(K=0), dict(K=65), dict(R=0), dict(R=(1 << 20) + 1), dict(S=0), dict(S=9),
            dict(strata=np.array([E, 0], np.int32)), dict(strata=np.array([E + 1, -1], np.int32)), dict(strata=np.array([E - 1], np.int32)),
            dict(pool=bad_pool), dict(pool=None), dict(strata=None, S=1), dict(cols=None)]
    for kw in sums:
        a = dict(cols=cols, pool=pool, strata=strata, R=R, seed=0, S=None, E=E, K=K)
        a.update(kw)
        rc, _, _, bufs = sums_call(dm, a['cols'], a['pool'], a['strata'], a['R'], a['seed'], S=a['S'], E=a['E'], K=a['K'])
        assert rc == EINVAL and untouched(*bufs), kw
        assert dm.lib.dnnca_last_error()
    assert dm.lib.dnnca_bootstrap_sums(dm.handle, i32(cols), E, K, i32(pool), i32(strata), 1, R, 0, None, None) == EINVAL      # no out
    detections = [dict(E=0), dict(E=16385), dict(N=-1), dict(N=(1 << 22) + 1), dict(R=0), dict(R=(1 << 20) + 1), dict(S=0), dict(S=9),
                  dict(strata=np.array([E - 1], np.int32)), dict(strata=np.array([3, 0, 3], np.int32)), dict(pool=bad_pool),
                  dict(cands=cand(exam=(3, E))), dict(cands=cand(exam=(3, -1))), dict(cands=cand(hit=(4, 2))), dict(cands=cand(hit=(4, -1))),
                  dict(cands=cand(level=(0, 1))), dict(cands=cand(level=(9, int(cands['level'][8]) + 2))),
                  dict(cands=cand(level=(9, int(cands['level'][8]) - 1))), dict(exams=exam(tumours=-1)), dict(exams=exam(score_rank=-1)),
                  dict(exams=None), dict(cands=None), dict(pool=None)]
    for kw in detections:
        a = dict(exams=exams, cands=cands, pool=pool, strata=strata, R=R, seed=0, E=E, N=len(cands), S=None)
        a.update(kw)
        rc, _, _, bufs = detection_call(dm, a['exams'], a['cands'], a['pool'], a['strata'], a['R'], a['seed'], E=a['E'], N=a['N'], S=a['S'])
        assert rc == EINVAL and untouched(*bufs), kw
    # the calls still work afterwards
    rc, got, _, _ = sums_call(dm, cols, pool, strata, R, 0)
    assert rc == 0 and (got == E).all()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------
def test_device_model_calls_equal_the_existing_functions_on_the_resample_written_out(dm):
    from dnncancerannotator_amd import casewise
    exams, cands = casewise.detection_bootstrap_inputs(BC.CASES)
    E, L = len(BC.CASES), BO.levels_of(cands)
    for stratified in (False, True):
        strata = casewise.bootstrap_pool(exams['tumours'] > 0, stratified)
        out = dm.bootstrap_detection(exams, cands, BC.REPLICATES, seed=BC.SEED, strata=strata, multiplicities=True)
        assert out['multiplicities'].tolist() == BO.multiplicities(E, strata[0], strata[1], BC.REPLICATES, BC.SEED).tolist()
        plain = dm.bootstrap_detection(exams, cands, BC.REPLICATES, seed=BC.SEED, strata=strata)
        assert all(plain[k].tobytes() == np.ascontiguousarray(out[k]).tobytes() for k in plain.dtype.names)
        left_out = 0
        for row in out:
            curves, auroc = BC.reference_values(BC.CASES, row['multiplicities'])
            BC.hold_to_reference(casewise.detection_replicate_values(row, E), row, curves, auroc, L)
            left_out += int(row['multiplicities'][0] == 0)
        assert 0 < left_out < BC.REPLICATES          # the top-ranked candidate's exam is left out by some replicates
    # bootstrap_sums: the same draws as bootstrap_detection for the same (seed, E, strata)
    counts = np.array([[c['tumours'], len(c['hits']), sum(c['hits'])] for c in BC.CASES], np.int32)
    got = dm.bootstrap_sums(counts, BC.REPLICATES, seed=BC.SEED, strata=strata, multiplicities=True)
    assert got['multiplicities'].tobytes() == np.ascontiguousarray(out['multiplicities']).tobytes()
    assert got['sums'][:, 0].tolist() == out['tumours'].tolist() and got['sums'][:, 2].tolist() == out['tp'].tolist()
    assert got['sums'][:, 1].tolist() == out['candidates'].tolist()
