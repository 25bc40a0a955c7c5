"""-m gpu: what a model owns, it owns alone.  Several models of different kernel plans live in one process, are stepped in turn,
closed in the middle and replaced by models of another description; a train step that stops on an error, a dry plan dump and a
`force_generic` neighbour leave nothing behind that a later step could find.  Every case ends with the tensors of the same model
stepped alone.

The reference of a model is its own lone run: an eval step, then three train steps at lr 1e-3 on fixed inputs, every step's loss,
gradients, weights, BatchNorm statistics and Adam slots recorded.  Two lone runs are made per model.  Where they agree bit for bit
(BITWISE; established on the library as it stood before the kernel plans moved into Model, and asserted by the first test) every
case compares bit for bit.  The 3-channel pixel-group plan sums its conv weight gradients with float atomics: there the first
step's loss and the head's gradients are held bit for bit and everything else to four times the difference of the two lone runs
(the rule of tests/test_train_metrics_gpu.py).

No case uses threads."""

import ctypes as C

import numpy as np
import pytest

from test_lesion_gpu import UNET
from test_train_metrics_gpu import _bits

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
LR, STEPS = 1e-3, 3
DENSE = dict(UNET, n_downsample=1, bn=True)
# key -> (arch, in_channels, H, W, batch = max_batch, dtype, options)
MODELS = {
    'A': ('unet', 1, 16, 16, 3, 'f32', UNET),                                   # pixel-group plan
    'B': ('unet', 1, 10, 14, 3, 'f32', dict(DENSE, n_filters_first=16)),        # split-bf16 plan + the igemm plan
    'C': ('unet', 1, 16, 16, 2, 'bf16', dict(DENSE, n_filters_first=64)),       # igb prep, half-stored tensors
    'D': ('unet', 1, 10, 14, 3, 'f32', dict(UNET, n_filters_first=64, n_downsample=1)),      # takes a closed model's place
}
BITWISE = {'A': False, 'B': True, 'C': True, 'D': True}
SMOOTH_REFUSED = 17          # fast_label_smooth takes filter sizes 1 .. 15
# the train plan of a force_generic model of A's description (launch order, from the library before the move): g_ launches only
ENC, DEC = 'conv_fwd conv_fwd pool_fwd ', 'tconv_fwd conv_fwd conv_fwd '
CONV_BWD, TCONV_BWD = 'act_bwd conv_wgrad conv_dgrad ', 'tconv_wgrad tconv_dgrad '
GENERIC_PLAN = ['g_' + n for n in (ENC * 3 + DEC * 3 + 'head_fwd step_init label_stats loss head_bwd ' + (CONV_BWD * 2 + TCONV_BWD) * 3 +
                                   ('pool_bwd ' + CONV_BWD * 2) * 2 + 'pool_bwd ' + CONV_BWD + 'act_bwd conv_wgrad finalize_scalars adam').split()]


def make(gpu, key, **kw):
    arch, c, h, w, b, dtype, opts = MODELS[key]
    m = gpu.DeviceModel(arch, c, h, w, b, dtype=dtype, **dict(opts, **kw))
    m.init_glorot(seed=7 + ord(key))
    return m


def batch(key):
    _, c, h, w, b, _, _ = MODELS[key]
    rng = np.random.default_rng(100 + ord(key))
    return rng.random((b, h, w, c)).astype(np.float32), (rng.random((b, h, w)) < 0.25).astype(np.float32)


def cfg_of(m, **kw):
    return m.loss_cfg(weight_mul=3.0, **kw)


def train(m, key):
    """one train step; what it left"""
    x, y = batch(key)
    out = m.train_step(x, y, LR, cfg_of(m))
    mm, vv, it = m.get_opt_state()
    return dict(loss=np.float32(out.loss), grads=m.get_grads(), params=m.get_params(), state=m.get_state(), m=mm, v=vv, it=it)


def evaluate(m, key):
    x, y = batch(key)
    return np.float32(m.eval_step(x, y, cfg_of(m)).loss)


def head_slices(m):
    return [slice(off, off + int(np.prod(shape))) for name, shape, tr, off in m.param_infos() if tr and name.startswith('head.')]


_LONE = {}


def lone(gpu, key):
    """two runs of the model alone, each on a fresh model: (eval loss, [step records]) twice, and the head's slices"""
    if key not in _LONE:
        runs = []
        for _ in range(2):
            m = make(gpu, key)
            runs.append((evaluate(m, key), [train(m, key) for _ in range(STEPS)]))
            head = head_slices(m)
            m.close()
        _LONE[key] = (runs, head)
    return _LONE[key]


def differing_words(a, b):
    return int((_bits(a) != _bits(b)).sum())


def assert_as_alone(gpu, key, steps, what, state=True):
    """steps: the records of the model's first len(steps) train steps in some company; they equal the lone run's"""
    (ref, ref2), head = lone(gpu, key)
    for k, got in enumerate(steps):
        b, c = ref[1][k], ref2[1][k]
        assert got['it'] == b['it'], (what, key, k)
        names = ('loss', 'grads', 'params', 'm', 'v') + (('state',) if state else ())
        if BITWISE[key]:
            for n in names:
                assert differing_words(got[n], b[n]) == 0, (what, key, k, n)
            continue
        if k == 0:
            assert differing_words(got['loss'], b['loss']) == 0, (what, key, 'loss')
            for s in head:
                assert differing_words(got['grads'][s], b['grads'][s]) == 0, (what, key, 'head gradient')
        for n in names:
            x, y, z = (np.asarray(t[n], np.float64).ravel() for t in (got, b, c))
            if y.size:
                assert np.abs(x - y).max() <= 4 * np.abs(y - z).max() + 1e-6 * np.abs(y).max(), (what, key, k, n)


def test_lone_runs_repeat_where_the_cases_compare_bit_for_bit(gpu):
    seen = {}
    for key in MODELS:
        ((e1, r1), (e2, r2)), head = lone(gpu, key)
        words = {n: sum(differing_words(a[n], b[n]) for a, b in zip(r1, r2)) for n in ('loss', 'grads', 'params', 'state', 'm', 'v')}
        first_head = sum(differing_words(r1[0]['grads'][s], r2[0]['grads'][s]) for s in head)
        print('%s: eval loss %s, differing words over %d steps %s, head gradient of step 1: %d' % (key, e1 == e2, STEPS, words, first_head))
        seen[key] = (words, first_head)
    for key in MODELS:
        ((e1, r1), (e2, r2)), head = lone(gpu, key)
        words, first_head = seen[key]
        assert differing_words(e1, e2) == 0 and differing_words(r1[0]['loss'], r2[0]['loss']) == 0 and first_head == 0, key
        assert len({r['loss'].tobytes() for r in r1}) == STEPS, 'the steps of %s do not move its loss' % key
        if BITWISE[key]:
            assert not any(words.values()), (key, words)


def test_interleaved_models_step_as_alone(gpu):
    ms = {k: make(gpu, k) for k in 'ABC'}
    got = {k: [] for k in ms}
    for _ in range(STEPS):
        for k in 'ABC':
            got[k].append(train(ms[k], k))
    for k in 'ABC':
        assert_as_alone(gpu, k, got[k], 'interleaved')
        ms[k].close()


def test_a_model_closed_in_the_middle_takes_nothing_along(gpu):
    ms = {k: make(gpu, k) for k in 'ABC'}
    got = {k: [] for k in ms}
    for s in range(STEPS):
        for k in 'ABC' if s == 0 else 'BC':
            got[k].append(train(ms[k], k))
        if s == 0:
            ms['A'].close()
    for k in 'ABC':
        assert_as_alone(gpu, k, got[k], 'closed in the middle')
    ms['B'].close()
    ms['C'].close()


def test_a_model_created_after_a_closed_one_starts_clean(gpu):
    lone(gpu, 'D')          # (the first test made it: D's reference comes from a model that took nobody's place)
    b = make(gpu, 'B')
    steps = [train(b, 'B')]
    b.close()
    d = make(gpu, 'D')       # may get B's address
    got = [train(d, 'D')]
    d.close()
    assert_as_alone(gpu, 'B', steps, 'before its close')
    assert_as_alone(gpu, 'D', got, 'created after a close')


@pytest.mark.parametrize('key', ['A', 'B'])
def test_a_step_that_stops_on_an_error_leaves_nothing_behind(gpu, key):
    from dnncancerannotator_amd._lib import DnncaError
    m = make(gpu, key)
    x, y = batch(key)
    with pytest.raises(DnncaError) as err:          # refused by loss_and_backward, behind the forward pass of the step
        m.train_step(x, y, LR, cfg_of(m, label_smoothing=True, label_smoothing_filter_size=SMOOTH_REFUSED))
    assert err.value.code == EINVAL and 'label_smoothing' in str(err.value)
    e = evaluate(m, key)
    got = [train(m, key)]
    m.close()
    # the refused step's forward pass was a training one: it moved the BatchNorm statistics, which the eval loss reads
    if not MODELS[key][6]['bn']:
        assert differing_words(e, lone(gpu, key)[0][0][0]) == 0
    assert_as_alone(gpu, key, got, 'after a refused step', state=False)


@pytest.mark.parametrize('key', ['A', 'B'])
def test_a_dry_plan_leaves_nothing_behind(gpu, key):
    m = make(gpu, key)
    plan = m.plan(variants=True, mode='train')
    got = [train(m, key) for _ in range(STEPS)]
    assert m.plan(variants=True, mode='train') == plan
    m.close()
    assert_as_alone(gpu, key, got, 'after a dry plan')


def test_a_generic_model_beside_a_tuned_one(gpu):
    tuned = make(gpu, 'A')
    generic = make(gpu, 'A', force_generic=True)
    got = [train(tuned, 'A')]
    names = [r[0] for r in generic.plan(mode='train')]
    print('generic plan:', names)
    assert all(n.startswith('g_') for n in names), names
    assert names == GENERIC_PLAN
    first = train(generic, 'A')
    assert [r[0] for r in generic.plan(mode='train')] == names
    # no stamps: the generic model has no pixel-group plan (and asking does not make one)
    f = generic.lib.dnnca_debug_read_stamps
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]
    buf = (C.c_ulonglong * 8)()
    assert f(generic.handle, buf, 8) == ESTATE and f(tuned.handle, buf, 8) == ESTATE
    got.append(train(tuned, 'A'))
    assert np.isfinite(first['loss'])
    tuned.close()
    generic.close()
    assert_as_alone(gpu, 'A', got, 'beside a generic model')
