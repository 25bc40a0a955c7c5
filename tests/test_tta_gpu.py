"""-m gpu: test-time augmentation through the C ABI (kernels_tta.hip: tta_view_in, tta_accumulate; dnnca_forward_tta).

The two kernels move values and add them in a fixed order, so everything here must EQUAL the numpy oracle (tests/tta_oracle.py) bit
for bit: the views, the float32 mean, and a whole dnnca_forward_tta against the host composition of plain forwards (forward of every
view, mapped back, averaged) -- after checking that two plain forwards of one input agree bit for bit themselves.  Host buffers carry
guard regions behind them, pre-filled with a sentinel: nothing may be written past what the call was given.

Shapes: sides 31 / 32 / 33 / 48 straddle the 32-pixel LDS tile of the transposed arms (partial tiles at the right and bottom edges,
more than one tile, more than one block), 1 and 7 are smaller than a tile; (1, 3, 33, 1), (1, 33, 3, 5) and (2, 16, 64, 3) give the
mirrored-run arms rows that are shorter and longer than a wave and a block."""

import os

import numpy as np
import pytest

import tta_oracle as TO
from test_lesion_gpu import UNET

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 16, 0xAB          # guard floats behind every host output
LOGIT_TOL, PROB_ROUNDING = 2e-4, 2.0 ** -22      # tests/test_inference_gpu.py (only if plain forwards do not repeat bit for bit)
SIDES = [1, 7, 31, 32, 33, 48]


def guarded(n):
    return np.full((n + GUARD) * 4, SENTINEL, np.uint8).view(np.float32)


def unguard(buf, n, shape):
    assert (buf[n:].view(np.uint8) == SENTINEL).all(), 'written past the end of the output'
    return buf[:n].reshape(shape).copy()


def same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert got.tobytes() == want.tobytes(), 'max |d| %.3e' % float(np.abs(got.astype(np.float64) - want).max())


@pytest.fixture(scope='module')
def dm(gpu):
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    yield m
    m.close()


def view_of(dm, x, k):
    from dnncancerannotator_amd._lib import check, fptr
    x = np.ascontiguousarray(x, np.float32)
    B, h, w, c = x.shape
    dst = guarded(x.size)
    check(dm.lib.dnnca_tta_view_of(dm.handle, fptr(x), B, h, w, c, k, fptr(dst)))
    return unguard(dst, x.size, TO.apply_view(x, k).shape)


def mean_of(dm, planes, views, is_logits=0):
    from dnncancerannotator_amd._lib import check, fptr
    planes = np.ascontiguousarray(planes, np.float32)
    _, B, h, w = planes.shape
    out = guarded(B * h * w)
    check(dm.lib.dnnca_tta_mean_of(dm.handle, fptr(planes), B, h, w, views, is_logits, fptr(out)))
    return unguard(out, B * h * w, (B, h, w))


def drawn(shape, seed):
    return np.random.default_rng(seed).random(shape).astype(np.float32)


# ---- 1. the views ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (2, 5, 7, 2), (1, 3, 33, 1), (1, 33, 3, 5), (2, 16, 64, 3)], ids=str)
def test_flip_views_equal_the_oracle(dm, shape):
    x = drawn(shape, 1)
    for k in range(4):
        same(view_of(dm, x, k), TO.apply_view(x, k))


@pytest.mark.parametrize('c', [1, 3, 5])
@pytest.mark.parametrize('side', SIDES)
def test_all_eight_views_of_squares_equal_the_oracle(dm, side, c):
    x = drawn((2 if side == 33 else 1, side, side, c), 2)
    for k in range(8):
        same(view_of(dm, x, k), TO.apply_view(x, k))


def test_more_channels_than_one_lds_pass(dm):
    """the transposed gather stages 8 channels per pass: 9 and 17 channels take a second and a third, partial one"""
    for c in (8, 9, 17):
        x = drawn((1, 33, 33, c), 3)
        for k in (4, 7):
            same(view_of(dm, x, k), TO.apply_view(x, k))


# ---- 2. the mean -----------------------------------------------------------------------------------------------------------------
MASKS = [1 << k for k in range(8)] + [0x0F, 0xFF, 0x07, 0xB4]


@pytest.mark.parametrize('side', SIDES)
def test_mean_of_squares_equals_the_oracle(dm, side):
    B = 2 if side == 33 else 1
    for views in MASKS:
        planes = drawn((len(TO.views_of(views)), B, side, side), 4 + views)
        same(mean_of(dm, planes, views), TO.mean_of(planes, views))


@pytest.mark.parametrize('shape', [(2, 5, 7), (1, 16, 64)], ids=str)
def test_mean_of_flips_on_rectangles_equals_the_oracle(dm, shape):
    for views in [m for m in MASKS if m < 16]:
        planes = drawn((len(TO.views_of(views)),) + shape, 5 + views)
        same(mean_of(dm, planes, views), TO.mean_of(planes, views))


# ---- 3. the shared sigmoid -------------------------------------------------------------------------------------------------------
def random_weights(m, seed):
    """random values in every variable; the moving variances positive"""
    rng = np.random.default_rng(seed)
    m.set_params(rng.normal(0.0, 0.4, m.n_trainable).astype(np.float32))
    if m.n_state:
        state = rng.normal(0.0, 0.3, m.n_state).astype(np.float32)
        for name, shape, trainable, off in m.param_infos():
            if not trainable and name.endswith('moving_variance'):
                n = int(np.prod(shape))
                state[off:off + n] = rng.uniform(0.5, 1.5, n)
        m.set_state(state)


def test_mean_of_logits_is_the_forwards_sigmoid(dm):
    random_weights(dm, 6)
    x = drawn((3, 16, 16, 1), 7)
    prob, logits = dm.forward(x, training=False, return_logits=True)
    assert (logits < 0).any() and (logits > 0).any()
    same(mean_of(dm, logits[None, ..., 0], 1, is_logits=1), prob[..., 0])


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------
def composed(m, x, views):
    """the host composition: forward of every view, mapped back, averaged"""
    planes = [m.forward(TO.apply_view(x, k), training=False)[..., 0] for k in TO.views_of(views)]
    return TO.mean_of(planes, views)


def assert_tta(m, x, views, what):
    """forward_tta against the host composition, in prob_out and in get_prob: bit for bit when plain forwards repeat bit for bit"""
    first, logits = m.forward(x, training=False, return_logits=True)
    exact = first.tobytes() == m.forward(x, training=False).tobytes()
    want = composed(m, x, views)
    got = m.forward_tta(x, views)[..., 0]
    kept = m.last_prob(len(x))
    d = float(np.abs(got.astype(np.float64) - want).max())
    print('%s: plain forwards repeat bit for bit: %s; forward_tta vs host composition max |d| %.3e' % (what, exact, d))
    same(kept, got)
    if exact:
        same(got, want)
    else:       # the tolerance of tests/test_inference_gpu.py for probabilities
        assert d <= LOGIT_TOL * max(1.0, float(np.abs(logits).max())) + PROB_ROUNDING, (what, d)
    assert m.forward_tta(x, views, return_prob=False) is None
    same(m.last_prob(len(x)), got)                  # and from run to run


CASES = {
    'unet_16x32_flips': (dict(arch='unet', in_channels=3, height=16, width=32, max_batch=3, **UNET), 0x0F, (3, 2)),
    'unet_48x48_d4': (dict(arch='unet', in_channels=1, height=48, width=48, max_batch=2, **UNET), 0xFF, (2,)),
    'mulmo_bn_16x16_d4': (dict(arch='mulmo', in_channels=3, height=16, width=16, max_batch=2, **dict(UNET, bn=True)), 0xFF, (2,)),
    'multires_16x16_flips': (dict(arch='multires', in_channels=5, height=16, width=16, max_batch=2, n_filters_first=4, n_downsample=4,
                                  padding='same'), 0x0F, (2,)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_forward_tta_equals_the_host_composition(gpu, name):
    kw, views, batches = CASES[name]
    m = gpu.DeviceModel(**kw)
    try:
        random_weights(m, 8)
        for B in batches:
            x = drawn((B, kw['height'], kw['width'], kw['in_channels']), 9 + B)
            assert_tta(m, x, views, '%s B=%d' % (name, B))
    finally:
        m.close()


# ---- 5. consumers and state ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def wide(gpu):
    m = gpu.DeviceModel('unet', 3, 16, 32, 3, **UNET)
    random_weights(m, 10)
    yield m
    m.close()


def test_consumers_read_the_mean_and_nothing_else_changes(wide):
    m = wide
    x = drawn((3, 16, 32, 3), 11)
    y = (x[..., 0] > 0.5).astype(np.float32)
    p0, s0 = m.get_params(), m.get_state()
    plain = m.forward(x, training=False)
    panels_plain = m.render_composite(y, 3, ratio=1.0)[:, :, :3 * 32]
    want = composed(m, x, 0x0F)
    thr = float(np.median(want))
    kw = dict(threshold=thr, filter_size=1, max_lesions=64)
    host = m.lesion_table(prob=want, **kw)
    m.forward_tta(x, 0x0F, return_prob=False)
    dev = m.lesion_table(batch=3, **kw)
    assert dev[1].tolist() == host[1].tolist() and dev[1].sum() > 0
    assert dev[0].tobytes() == host[0].tobytes() and np.array_equal(dev[2], host[2])
    # the composite's feature panels show the batch as it was given, not the last view (both flips) of it
    panels = m.render_composite(y, 3, ratio=1.0)[:, :, :3 * 32]
    assert np.array_equal(panels, panels_plain)
    m.forward(TO.apply_view(x, 3), training=False, return_prob=False)
    assert not np.array_equal(m.render_composite(y, 3, ratio=1.0)[:, :, :3 * 32], panels_plain)
    assert m.get_params().tobytes() == p0.tobytes() and m.get_state().tobytes() == s0.tobytes()
    assert m.forward(x, training=False).tobytes() == plain.tobytes()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(dm, wide):
    from dnncancerannotator_amd._lib import fptr
    sq, rect = drawn((4, 16, 16, 1), 12), drawn((4, 16, 32, 3), 13)
    planes = drawn((8, 4, 16, 32), 14)
    for m in (dm, wide):
        m.sync()
        m.profile_reset()
        m.profile_enable(1)
    try:
        out = guarded(0)                          # too small for anything: a refused call must not touch it
        lib = dm.lib
        cases = [('views 0', lambda: lib.dnnca_forward_tta(dm.handle, fptr(sq), 2, 0, fptr(out))),
                 ('views 256', lambda: lib.dnnca_forward_tta(dm.handle, fptr(sq), 2, 256, fptr(out))),
                 ('view 4 at 16 x 32', lambda: lib.dnnca_forward_tta(wide.handle, fptr(rect), 2, 1 << 4, fptr(out))),
                 ('d4 at 16 x 32', lambda: lib.dnnca_forward_tta(wide.handle, fptr(rect), 2, 0xFF, fptr(out))),
                 ('batch 0', lambda: lib.dnnca_forward_tta(dm.handle, fptr(sq), 0, 0x0F, fptr(out))),
                 ('batch max_batch + 1', lambda: lib.dnnca_forward_tta(dm.handle, fptr(sq), 4, 0x0F, fptr(out))),
                 ('mean_of views 0', lambda: lib.dnnca_tta_mean_of(dm.handle, fptr(planes), 2, 16, 32, 0, 0, fptr(out))),
                 ('mean_of views 256', lambda: lib.dnnca_tta_mean_of(dm.handle, fptr(planes), 2, 16, 32, 256, 0, fptr(out))),
                 ('mean_of view 5 at 16 x 32', lambda: lib.dnnca_tta_mean_of(dm.handle, fptr(planes), 2, 16, 32, 1 << 5, 0, fptr(out))),
                 ('mean_of batch 0', lambda: lib.dnnca_tta_mean_of(dm.handle, fptr(planes), 0, 16, 32, 1, 0, fptr(out))),
                 ('mean_of batch max_batch + 1', lambda: lib.dnnca_tta_mean_of(dm.handle, fptr(planes), 4, 16, 32, 1, 0, fptr(out))),
                 ('view_of view 8', lambda: lib.dnnca_tta_view_of(dm.handle, fptr(rect), 2, 16, 32, 3, 8, fptr(out))),
                 ('view_of view 4 at 16 x 32', lambda: lib.dnnca_tta_view_of(dm.handle, fptr(rect), 2, 16, 32, 3, 4, fptr(out)))]
        for what, call in cases:
            assert call() == -1, what             # DNNCA_EINVAL
            assert lib.dnnca_last_error()
            assert (out.view(np.uint8) == SENTINEL).all(), what
        assert dm.profile() == [] and wide.profile() == []
    finally:
        for m in (dm, wide):
            m.profile_enable(0)
            m.profile_reset()


# ---- 7. launches -----------------------------------------------------------------------------------------------------------------
def test_launches_and_untouched_plans(wide):
    m = wide
    before = {mode: m.plan(variants=True, mode=mode) for mode in ('train', 'eval', 'forward')}
    x = drawn((3, 16, 32, 3), 15)
    m.sync()
    m.profile_reset()
    m.profile_enable(1)
    try:
        m.forward_tta(x, 0x0F)
        rows = {name: (n, by) for name, n, _, by, _ in m.profile()}
    finally:
        m.profile_enable(0)
        m.profile_reset()
    assert rows['tta_accumulate'][0] == 4 and rows['tta_view_in'][0] == 3 and 'g_sigmoid' not in rows
    assert rows['tta_view_in'][1] == 8.0 * x.size                          # read once, written once
    assert rows['tta_accumulate'][1] == (8.0 + 3 * 12.0) / 4 * x[..., 0].size     # the first view writes, three add in place
    forward = [r[0] for r in m.plan(mode='forward') if r[0] != 'g_sigmoid']
    assert all(rows[k][0] == 4 * forward.count(k) for k in set(forward))   # one forward per view
    for mode, plan in before.items():
        assert m.plan(variants=True, mode=mode) == plan
        assert not [r[0] for r in plan if r[0].startswith('tta')]


# ---- 8. the command line ---------------------------------------------------------------------------------------------------------
def test_cli_predict_tta(gpu, tmp_path):
    import yaml
    from dnncancerannotator_amd import __main__ as cli, casewise as CW, engine
    from dnncancerannotator_amd.runs.train import make_dataset
    cfg = {'model': 'UNetAnnotator', 'model_options': UNET, 'deploy_options': {'optimizer': 'adam', 'enable_multigpu': False},
           'data_options': {'eval': {'batch_size': 2}}}
    run = str(tmp_path / 'run')
    data = 'synthetic:16x16x2'
    e = engine.TFKerasModel(cfg)
    ds = make_dataset([data], cfg['data_options']['eval'], training=False, include_meta=True, labels=False)
    e._build(ds)
    m = e.device_model
    random_weights(m, 16)
    e.current_step = 1
    e.save(os.path.join(run, 'checkpoints', 'ckpt-1'))
    with open(os.path.join(run, 'options.yaml'), 'w') as f:
        yaml.safe_dump({'config': cfg}, f)
    batches = list(ds)
    thr = float(np.median(composed(m, batches[0][0], 0x0F)))
    texts = {}
    for name, flags in (('bare', []), ('none', ['--tta', 'none']), ('flips', ['--tta', 'flips'])):
        out = str(tmp_path / name)
        assert cli.main(['predict', '--save_path', run, '--data_path', data, '--output', out, '--export_images', '--threshold', repr(thr),
                         '--filter_size', '1'] + flags) == 0
        texts[name] = {}
        for d, _, fs in os.walk(out):
            for fn in fs:
                with open(os.path.join(d, fn), 'rb') as f:
                    texts[name][os.path.relpath(os.path.join(d, fn), out)] = f.read()
    assert texts['bare'] == texts['none'] and 'lesions.csv' in texts['bare'] and len(texts['bare']) == 2 + sum(len(b[0]) for b in batches)
    lines = []
    for x, paths, ids in batches:
        rows, _, _ = m.lesion_table(prob=composed(m, x, 0x0F), threshold=thr, filter_size=1)
        lines += [CW.lesion_values(paths[r['slice']], ids[r['slice']], r) for r in rows]
    assert lines and texts['flips']['lesions.csv'].decode() == CW.plain_csv(CW.LESION_COLUMNS, lines)
    assert texts['flips']['lesions.csv'] != texts['bare']['lesions.csv']        # a random network is not flip-invariant
    m.close()
