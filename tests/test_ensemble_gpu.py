"""-m gpu: ensembles through the C ABI (kernels_ensemble.hip: ens_join; dnnca_model_set_members, dnnca_member_store,
dnnca_member_get, dnnca_forward_ensemble, dnnca_get_ensemble_spread, dnnca_ensemble_of) against tests/ensemble_oracle.py.

The mean must EQUAL the oracle's float32 sum and division bit for bit; between, within and total must lie within 2^-18 of their
float64 values plus 2^-23 on every pixel (tests/spread_oracle.py: tolerance), between exactly 0 for one member and for equal
members.  A whole dnnca_forward_ensemble must equal the host composition -- every member loaded into a second model, forwarded
there, the planes joined by dnnca_ensemble_of -- and leave the model's own weights as they were, bit for bit.  Host outputs carry
guard regions pre-filled with a sentinel.

Shapes of the kernel alone: 1 pixel; 255 and 257, one short of and one past a block of 256 threads; (3, 5, 7) with an odd number of
pixels, so that the planes of the one allocation are not 16-byte aligned; (2, 33, 35) and (1, 64, 64) with several blocks."""

import os

import numpy as np
import pytest

import ensemble_oracle as EO
from test_ema_gpu import UNET3
from test_lesion_gpu import UNET
from test_tta_gpu import LOGIT_TOL, PROB_ROUNDING, drawn, guarded, random_weights, same, unguard

pytestmark = pytest.mark.gpu

ESTATE = -4
PLANES = [(1, 1, 1), (1, 1, 255), (1, 1, 257), (3, 5, 7), (2, 33, 35), (1, 64, 64)]
COUNTS = [1, 2, 3, 16]


@pytest.fixture(scope='module')
def dm(gpu):
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    yield m
    m.close()


def ensemble_of(dm, means, withins=None):
    """dnnca_ensemble_of with guarded outputs -> (mean, between, within, total) [B, h, w]"""
    from dnncancerannotator_amd._lib import check, fptr
    means = np.ascontiguousarray(means, np.float32)
    n, B, h, w = means.shape
    if withins is not None:
        withins = np.ascontiguousarray(withins, np.float32)
    outs = [guarded(B * h * w) for _ in range(4)]
    check(dm.lib.dnnca_ensemble_of(dm.handle, fptr(means), fptr(withins) if withins is not None else None, n, B, h, w,
                                   *[fptr(o) for o in outs]))
    return tuple(unguard(o, B * h * w, (B, h, w)) for o in outs)


def within_tolerance(got, want, what, extra=0.0):
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want)
    tol = EO.tolerance(want) + extra
    worst = int(np.argmax(err - tol))
    print('%s: max |d| %.3e, worst pixel %.3e of %.3e allowed (want %.6e)' % (what, err.max(), err.flat[worst], tol.flat[worst],
                                                                             want.flat[worst]))
    assert (err <= tol).all(), what


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', EO.FAMILIES)
@pytest.mark.parametrize('plane', PLANES, ids=str)
def test_ensemble_of_against_the_oracle(dm, plane, family):
    for n in COUNTS:
        means = EO.family(family, (n,) + plane, 100 + n)
        for withins in (None, EO.drawn_withins(means.shape, 200 + n)):
            what = '%s %s n=%d %s' % (family, plane, n, 'plain' if withins is None else 'with withins')
            mean, between, inside, total = ensemble_of(dm, means, withins)
            same(mean, EO.mean_of(means))
            within_tolerance(between, EO.between_of(means), what + ' between')
            within_tolerance(inside, EO.within_of(means, withins), what + ' within')
            within_tolerance(total, EO.total_of(means, withins), what + ' total')
            if n == 1:
                assert not between.any()
            if withins is None:
                assert not inside.any() and total.tobytes() == between.tobytes()


def test_equal_members_give_exactly_zero(dm):
    one = EO.family('uniform', (1, 2, 33, 35), 7)
    for n in (2, 3, 16):
        mean, between, inside, total = ensemble_of(dm, np.repeat(one, n, axis=0))
        assert not between.any() and not inside.any() and not total.any()
    mean, between, inside, total = ensemble_of(dm, np.repeat(one, 2, axis=0))
    same(mean, one[0])           # (a + a) / 2 is exact


def test_mean_alone_and_refusals(dm):
    from dnncancerannotator_amd._lib import fptr
    means = EO.family('uniform', (3, 3, 5, 7), 8)
    same(dm.ensemble_of(means, spread=False), EO.mean_of(means))
    mean, between, inside, total = dm.ensemble_of(means, EO.drawn_withins(means.shape, 9))
    same(mean, EO.mean_of(means))
    out = guarded(0)
    lib, h = dm.lib, dm.handle
    cases = [('n 0', lambda: lib.dnnca_ensemble_of(h, fptr(means), None, 0, 3, 5, 7, fptr(out), None, None, None)),
             ('n 17', lambda: lib.dnnca_ensemble_of(h, fptr(means), None, 17, 3, 5, 7, fptr(out), None, None, None)),
             ('batch 0', lambda: lib.dnnca_ensemble_of(h, fptr(means), None, 3, 0, 5, 7, fptr(out), None, None, None)),
             ('batch max_batch + 1', lambda: lib.dnnca_ensemble_of(h, fptr(means), None, 3, 4, 5, 7, fptr(out), None, None, None)),
             ('null means', lambda: lib.dnnca_ensemble_of(h, None, None, 3, 3, 5, 7, fptr(out), None, None, None)),
             ('null mean_out', lambda: lib.dnnca_ensemble_of(h, fptr(means), None, 3, 3, 5, 7, None, None, None, None)),
             ('between without total', lambda: lib.dnnca_ensemble_of(h, fptr(means), None, 3, 3, 5, 7, fptr(out), fptr(out), fptr(out), None)),
             ('set_members 17', lambda: lib.dnnca_model_set_members(h, 17)),
             ('set_members -1', lambda: lib.dnnca_model_set_members(h, -1))]
    for what, call in cases:
        assert call() == -1, what             # DNNCA_EINVAL
    unguard(out, 0, (0,))


# ---- 2. members ------------------------------------------------------------------------------------------------------------------
def drawn_members(m, n, seed):
    """n (params, state) pairs drawn with different seeds, read back from the model (which keeps the last)"""
    out = []
    for i in range(n):
        random_weights(m, seed + i)
        out.append((m.get_params(), m.get_state()))
    return out


def _batch(m, B, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((B,) + m.in_shape).astype(np.float32)
    y = (rng.random((B,) + m.in_shape[:2]) < 0.1).astype(np.float32)
    return x, y


def test_members_come_back_and_the_models_weights_stay(gpu):
    kw = dict(n_filters_first=16, n_downsample=2, rate=2, kernel_size=3, conv_stride=1, bn=True, padding='same')
    m, twin = (gpu.DeviceModel('mulmo', 3, 12, 20, 2, **kw) for _ in range(2))
    try:
        members = drawn_members(m, 3, 30)
        random_weights(m, 40)
        p0, s0 = m.get_params(), m.get_state()
        assert s0.size and p0.tobytes() != members[0][0].tobytes()
        twin.set_params(p0), twin.set_state(s0)
        m.set_members(members)
        for i, (p, s) in enumerate(members):
            got_p, got_s = m.member(i)
            assert got_p.tobytes() == p.tobytes() and got_s.tobytes() == s.tobytes()
        x, y = _batch(m, 2, 41)
        for views, spread in ((1, False), (0x0F, True)):
            m.forward_ensemble(x, views, spread=spread)
            assert m.get_params().tobytes() == p0.tobytes() and m.get_state().tobytes() == s0.tobytes()
        for i, (p, s) in enumerate(members):          # nor has a call touched a member
            got_p, got_s = m.member(i)
            assert got_p.tobytes() == p.tobytes() and got_s.tobytes() == s.tobytes()
        cfg = m.loss_cfg(weight_mul=3.0)
        a, b = m.train_step(x, y, 1e-2, cfg), twin.train_step(x, y, 1e-2, cfg)
        assert a.loss == b.loss
        assert m.get_params().tobytes() == twin.get_params().tobytes() and m.get_state().tobytes() == twin.get_state().tobytes()
        assert m.get_params().tobytes() != p0.tobytes()
        m.set_members([])
        with pytest.raises(gpu._lib.DnncaError) as e:
            m.forward_ensemble(x)
        assert e.value.code == ESTATE and 'no members' in str(e.value)
    finally:
        m.close(), twin.close()


def test_an_unset_slot_and_exchanged_weights_are_refused(gpu):
    from dnncancerannotator_amd._lib import check, fptr
    m = gpu.DeviceModel('unet', 1, 16, 16, 2, **UNET)
    try:
        random_weights(m, 50)
        p, s = m.get_params(), m.get_state()
        x = drawn((2, 16, 16, 1), 51)
        plain = m.forward(x)
        check(m.lib.dnnca_model_set_members(m.handle, 2))
        check(m.lib.dnnca_member_store(m.handle, 1, fptr(p), p.size, fptr(s) if s.size else None, s.size))
        with pytest.raises(gpu._lib.DnncaError) as e:
            m.forward_ensemble(x)
        assert e.value.code == ESTATE and 'member 0' in str(e.value) and 'never stored' in str(e.value)
        with pytest.raises(gpu._lib.DnncaError) as e:
            m.member(0)
        assert e.value.code == ESTATE
        assert m.lib.dnnca_member_store(m.handle, 2, fptr(p), p.size, None, 0) == -1            # outside 0..1
        assert m.lib.dnnca_member_store(m.handle, 0, fptr(p), p.size - 1, None, 0) == -1        # a vector of another model
        check(m.lib.dnnca_member_store(m.handle, 0, fptr(p), p.size, fptr(s) if s.size else None, s.size))
        same(m.forward_ensemble(x), plain)              # two copies of the model's own weights: (a + a) / 2
        m.set_ema(0.5)
        m.exchange_ema()
        try:
            with pytest.raises(gpu._lib.DnncaError) as e:
                m.forward_ensemble(x)
            assert e.value.code == ESTATE and 'averaged weights are in use' in str(e.value)
        finally:
            m.exchange_ema()
        same(m.forward_ensemble(x), plain)
        with pytest.raises(gpu._lib.DnncaError) as e:      # a mean without spread leaves no components
            m.last_ensemble_spread(2)
        assert e.value.code == ESTATE
        m.forward_ensemble(x, spread=True, return_prob=False)
        between, inside = m.last_ensemble_spread(2)
        assert not between.any() and not inside.any() and not m.last_spread(2).any()
        m.forward_tta_spread(x, 0x0F)                      # the plane is now the views' spread, not an ensemble's
        with pytest.raises(gpu._lib.DnncaError) as e:
            m.last_ensemble_spread(2)
        assert e.value.code == ESTATE
    finally:
        m.close()


# ---- 3. forward_ensemble against the host composition ------------------------------------------------------------------------------
def _multires(gpu):
    from dnncancerannotator_amd import models
    return models.MultiResUnet(n_channels=5, n_filters_first=4).build([1, 16, 16, 5], seed=0)


# name -> (builder, batch fed, view masks)
MODELS = {
    'unet3_1x16x16': (lambda g: g.DeviceModel('unet', 1, 16, 16, 1, **UNET3), 1, (1, 0x0F, 0xFF)),
    'unet3_ragged_3_of_4x40x24': (lambda g: g.DeviceModel('unet', 1, 40, 24, 4, **UNET3), 3, (1, 0x0F)),
    'mulmo16_bn_12x20x3': (lambda g: g.DeviceModel('mulmo', 3, 12, 20, 2, n_filters_first=16, n_downsample=2, rate=2, kernel_size=3,
                                                    conv_stride=1, bn=True, padding='same'), 2, (1, 0x0F)),
    'unet64_bf16_10x14': (lambda g: g.DeviceModel('unet', 1, 10, 14, 2, n_filters_first=64, n_downsample=1, rate=2, kernel_size=3,
                                                   conv_stride=1, bn=True, padding='same', dtype='bf16'), 2, (1, 0x0F)),
    'multires4_1x16x16': (_multires, 1, (1, 0x0F, 0xFF)),
}


def composed(ref, members, x, views):
    """every member loaded into `ref` and forwarded there -> (means [n, B, H, W], withins or None)"""
    means, withins = [], []
    for p, s in members:
        ref.set_params(p)
        if ref.n_state:
            ref.set_state(s)
        if views == 1:
            means.append(ref.forward(x, training=False)[..., 0])
        else:
            prob, spread = ref.forward_tta_spread(x, views)
            means.append(prob[..., 0]), withins.append(spread)
    return np.stack(means), (np.stack(withins) if withins else None)


@pytest.mark.parametrize('name', list(MODELS))
def test_forward_ensemble_equals_the_host_composition(gpu, name):
    builder, B, masks = MODELS[name]
    m, ref = builder(gpu), builder(gpu)
    try:
        members = drawn_members(ref, 3, 60)
        if ref.n_state:
            assert members[0][1].tobytes() != members[1][1].tobytes()      # the moving statistics differ between the members
        random_weights(m, 70)
        p0, s0 = m.get_params(), m.get_state()
        m.set_members(members)
        x = drawn((B,) + m.in_shape, 71)
        first, logits = ref.forward(x, training=False, return_logits=True)
        exact = first.tobytes() == ref.forward(x, training=False).tobytes()
        extra = 0.0 if exact else LOGIT_TOL * max(1.0, float(np.abs(logits).max())) + PROB_ROUNDING
        for views in masks:
            what = '%s views 0x%02X (plain forwards repeat: %s)' % (name, views, exact)
            means, withins = composed(ref, members, x, views)
            want = ensemble_of(ref, means, withins)
            got_mean = m.forward_ensemble(x, views, spread=True)[..., 0]
            got = (got_mean,) + m.last_ensemble_spread(B) + (m.last_spread(B),)
            same(m.last_prob(B), got_mean)
            for g, w, part in zip(got, want, ('mean', 'between', 'within', 'total')):
                if exact:
                    same(g, w)
                else:
                    within_tolerance(g, w.astype(np.float64), '%s %s' % (what, part), extra)
            within_tolerance(got[1], EO.between_of(means), what + ' between', extra)
            within_tolerance(got[2], EO.within_of(means, withins), what + ' within', extra)
            within_tolerance(got[3], EO.total_of(means, withins), what + ' total', extra)
            assert got[1].any()                              # members drawn with different seeds disagree
            if views == 1:
                assert not got[2].any() and got[3].tobytes() == got[1].tobytes()
            else:
                assert got[2].any()                          # a random network is not flip-invariant
            # without the spread: the same mean, and the spread plane is no longer valid
            same(m.forward_ensemble(x, views)[..., 0], got_mean)
            with pytest.raises(gpu._lib.DnncaError):
                m.last_spread(B)
            # 4. determinism: a second call is identical bit for bit
            assert m.forward_ensemble(x, views, spread=True, return_prob=False) is None
            again = (m.last_prob(B),) + m.last_ensemble_spread(B) + (m.last_spread(B),)
            for g, a in zip(got, again):
                same(a, g)
        assert m.get_params().tobytes() == p0.tobytes() and m.get_state().tobytes() == s0.tobytes()
        # three copies of one member: it is that member's forward, and nothing lies between them
        m.set_members([members[1]] * 3)
        views = masks[-1]
        means, withins = composed(ref, [members[1]], x, views)
        m.forward_ensemble(x, views, spread=True, return_prob=False)
        between, inside = m.last_ensemble_spread(B)
        assert not between.any()
        if exact and withins is not None:
            within_tolerance(inside, withins[0].astype(np.float64), name + ' three copies: within')
    finally:
        m.close(), ref.close()


def test_launches_and_untouched_plans(gpu):
    """ens_join runs once per member, beside the launches of the members' own forwards; a model without members plans what it did"""
    m = gpu.DeviceModel('unet', 3, 16, 32, 3, **UNET)
    try:
        plans = {mode: m.plan(variants=True, mode=mode) for mode in ('train', 'eval', 'forward')}
        members = drawn_members(m, 4, 80)
        m.set_members(members)
        x = drawn((3, 16, 32, 3), 81)
        m.forward_ensemble(x, 0x0F, spread=True, return_prob=False)
        m.sync()
        m.profile_reset()
        m.profile_enable(1)
        try:
            m.forward_ensemble(x, 0x0F, spread=True, return_prob=False)
            m.sync()
            rows = {name: (k, by) for name, k, _, by, _ in m.profile()}
        finally:
            m.profile_enable(0)
            m.profile_reset()
        assert rows['ens_join'][0] == 4 and rows['tta_moments'][0] == 16 and rows['tta_view_in'][0] == 12, rows
        # floats moved per pixel by members 0 .. 3 (see ens_launch_join): 5 + 9 + 11 + 11
        assert rows['ens_join'][1] == 4.0 * (5 + 9 + 11 + 11) / 4 * x[..., 0].size
        for mode, plan in plans.items():
            assert m.plan(variants=True, mode=mode) == plan
            assert not [r[0] for r in plan if r[0].startswith('ens')]
    finally:
        m.close()


# ---- 5. the command line ---------------------------------------------------------------------------------------------------------
def _files(root):
    out = {}
    for d, _, fs in os.walk(root):
        for fn in fs:
            with open(os.path.join(d, fn), 'rb') as f:
                out[os.path.relpath(os.path.join(d, fn), root)] = f.read()
    return out


def _run_with_two_checkpoints(tmp_path, labels):
    """a run directory with the checkpoints 1 and 2 of two differently drawn models -> (model, batches, run, data, the two members)"""
    import yaml
    from dnncancerannotator_amd import engine
    from dnncancerannotator_amd.runs.train import make_dataset
    cfg = {'model': 'UNetAnnotator', 'model_options': UNET, 'deploy_options': {'optimizer': 'adam', 'enable_multigpu': False},
           'data_options': {'eval': {'batch_size': 2}}}
    run, data = str(tmp_path / 'run'), 'synthetic:16x16x2'
    e = engine.TFKerasModel(cfg)
    ds = make_dataset([data], cfg['data_options']['eval'], training=False, include_meta=True, labels=labels)
    e._build(ds)
    members = {}
    for step in (1, 2):
        random_weights(e.device_model, 16 + step)
        members[step] = (e.device_model.get_params(), e.device_model.get_state())
        e.current_step = step
        e.save(os.path.join(run, 'checkpoints', 'ckpt-%d' % step))
    with open(os.path.join(run, 'options.yaml'), 'w') as f:
        yaml.safe_dump({'config': cfg}, f)
    return e.device_model, list(ds), run, data, members


def _member_planes(m, members, x):
    """the plain forward of every member on x, by loading it into m -> (means [n, B, H, W], the device's join of them)"""
    means = []
    for p, s in members:
        m.set_params(p)
        if m.n_state:
            m.set_state(s)
        means.append(m.forward(x, training=False)[..., 0])
    means = np.stack(means)
    joined = m.ensemble_of(means)
    same(joined[0], EO.mean_of(means))
    return means, joined


def test_cli_predict_ensemble(gpu, tmp_path):
    from dnncancerannotator_amd import __main__ as cli, casewise as CW
    m, batches, run, data, members = _run_with_two_checkpoints(tmp_path, labels=False)
    order = [members[2], members[1]]                # --step 2 is member 0, run:1 the other
    thr = float(np.median(_member_planes(m, order, batches[0][0])[1][0]))
    base = ['predict', '--save_path', run, '--data_path', data, '--step', '2', '--threshold', repr(thr), '--filter_size', '1', '--output']
    texts = {}
    for name, flags in (('before', []), ('mean', ['--ensemble', run + ':1']), ('spread', ['--ensemble', run + ':1', '--uncertainty']),
                        ('after', [])):
        assert cli.main(base + [str(tmp_path / name)] + flags) == 0
        texts[name] = _files(str(tmp_path / name))
    assert texts['after'] == texts['before'] and sorted(texts['before']) == ['lesions.csv', 'slices.csv']
    assert sorted(texts['mean']) == ['lesions.csv', 'slices.csv'] and texts['mean'] != texts['before']
    assert sorted(set(texts['spread']) - set(texts['mean'])) == ['lesion_uncertainty.csv', 'slice_ensemble_uncertainty.csv',
                                                                 'slice_uncertainty.csv']
    assert all(texts['spread'][k] == v for k, v in texts['mean'].items())
    lesion_lines, slice_lines, spread_lines, component_lines = [], [], [], []
    for x, paths, ids in batches:
        _, (mean, between, inside, total) = _member_planes(m, order, x)
        assert between.any() and not inside.any() and total.tobytes() == between.tobytes()
        rows, totals, _, srows, stotals = m.lesion_table_spread(prob=mean, spread=total, threshold=thr, filter_size=1)
        plain = m.lesion_table(prob=mean, threshold=thr, filter_size=1)
        assert plain[0].tobytes() == rows.tobytes() and np.array_equal(plain[1], totals)
        for b in range(len(x)):
            mine = rows['slice'] == b
            lesion_lines += [CW.lesion_values(paths[b], ids[b], r) for r in rows[mine]]
            slice_lines.append(CW.slice_values(paths[b], ids[b], rows[mine], totals[b]))
            spread_lines.append(CW.slice_uncertainty_values(paths[b], ids[b], rows[mine], srows[mine], totals[b], stotals[b]))
            component_lines.append(CW.slice_ensemble_uncertainty_values(paths[b], ids[b], between[b], inside[b]))
    assert lesion_lines and texts['mean']['lesions.csv'].decode() == CW.plain_csv(CW.LESION_COLUMNS, lesion_lines)
    assert texts['mean']['slices.csv'].decode() == CW.plain_csv(CW.SLICE_COLUMNS, slice_lines)
    assert texts['spread']['slice_uncertainty.csv'].decode() == CW.plain_csv(CW.SLICE_UNCERTAINTY_COLUMNS, spread_lines)
    assert texts['spread']['slice_ensemble_uncertainty.csv'].decode() == CW.plain_csv(CW.SLICE_ENSEMBLE_UNCERTAINTY_COLUMNS, component_lines)
    m.close()


def test_cli_evaluate_ensemble(gpu, tmp_path):
    from dnncancerannotator_amd import __main__ as cli, casewise as CW
    import spread_oracle as SO
    m, batches, run, data, members = _run_with_two_checkpoints(tmp_path, labels=True)
    order = [members[2], members[1]]
    thr = float(np.median(_member_planes(m, order, batches[0][0])[1][0]))
    base = ['evaluate', '--save_path', run, '--data_path', data, '--export_csv', '--skip_visualization', '--step_range', '2', '2',
            '--exam_lesions', '--exam_threshold', repr(thr), '--exam_filter_size', '1', '--tag', 'plain', '--export_path']
    flags = ['--ensemble', run + ':1', '--uncertainty', '--uncertainty_threshold', repr(thr)]
    texts = {}
    for name, more in (('before', []), ('ens', flags), ('after', [])):
        assert cli.main(base + [str(tmp_path / name)] + more) == 0
        texts[name] = _files(str(tmp_path / name))
    assert texts['after'] == texts['before'] and 'plain/exam_lesion_cases.csv' in texts['before']
    a, b = texts['before'], texts['ens']
    assert sorted(set(b) - set(a)) == ['plain/ensemble_uncertainty_results.csv', 'plain/uncertainty_results.csv',
                                       'plain/uncertainty_slices.csv']
    # the loss column is member 0's own: the plain evaluation's
    loss = lambda text: text.decode().splitlines()[1].split(',')[1]      # noqa: E731
    assert loss(b['plain/results.csv']) == loss(a['plain/results.csv'])
    # the exam-lesion tables: lesion_table_matched on the oracle's mean plane, slice by slice as the pass walks them
    found, outs, last = [], [[], [], []], None
    for x, y, paths, ids in batches:
        _, (mean, between, inside, total) = _member_planes(m, order, x)
        yy = np.asarray(y, np.float32).reshape(mean.shape)
        continues = []
        for p, k in zip(paths, ids):
            continues.append(last is not None and p == last[0] and int(k) == last[1] + 1)
            last = (p, int(k))
        found += CW.slice_records(m.lesion_table_matched(yy, prob=mean, continues=continues, threshold=thr, filter_size=1), list(zip(paths, ids)))
        for o, plane in zip(outs, (between, inside, total)):
            o += list(SO.outcome(mean, plane, yy, [thr])[0])
    lead, cases = [2, repr(thr)], []
    for exam, recs in CW.by_exam(found).items():
        cases.append(CW.match_records(CW.match_exam_lesions, exam, recs, 1, iou=CW.EXAM_IOU)[0])
    assert b['plain/exam_lesion_cases.csv'].decode() == CW.plain_csv(['step', 'threshold'] + CW.EXAM_CASE_COLUMNS, [lead + c for c in cases])
    assert b['plain/exam_lesion_results.csv'].decode() == CW.plain_csv(['step', 'threshold'] + CW.EXAM_RESULT_COLUMNS,
                                                                       [lead + CW.exam_match_summary(cases)])
    assert b['plain/ensemble_uncertainty_results.csv'].decode() == CW.plain_csv(
        ['step', 'threshold'] + CW.ENSEMBLE_UNCERTAINTY_RESULT_COLUMNS, [lead + CW.ensemble_outcome_summary(*outs)])
    assert b['plain/uncertainty_results.csv'].decode() == CW.plain_csv(['step', 'threshold'] + CW.UNCERTAINTY_RESULT_COLUMNS,
                                                                       [lead + CW.outcome_summary(outs[2])])
    m.close()
