"""-m gpu: mask refinement (dnnca_model_set_lesion_refine; kernels_refine.hip: region_hyst_seed / _keep, region_close,
region_complement, region_hole_border / _fill around the region_ccl_* launches) through DeviceModel.  Everything is an integer or an
extremum, so rows, totals and masks must EQUAL the numpy oracle (tests/refine_oracle.py) bit for bit.  The planes are a few slices
of at most 96 x 96 pixels and no multiple of the 32-pixel tile: most are 70 x 45 (tile seams at rows 32 and 64 and column 32) with
batch 3.  Probabilities are drawn from three levels: BG below `low`, LOW between `low` and the threshold, HIGH above it."""

import ctypes as C

import numpy as np
import pytest

import lesion_oracle as LO
import match_oracle as MO
import refine_oracle as RO

pytestmark = pytest.mark.gpu

UNET = dict(n_filters_first=3, n_downsample=3, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same')
H, W = 70, 45
BG, LOW, HIGH = np.float32(0.1), np.float32(0.4), np.float32(0.8)
THR, LO_THR = 0.5, 0.3
NEW = ('region_hyst_seed', 'region_hyst_keep', 'region_close', 'region_complement', 'region_hole_border', 'region_hole_fill')
FILL, ALL3 = dict(fill_holes=True), dict(hysteresis=LO_THR, closing=3, fill_holes=True)
PLAN_MODES = ('lesion', 'lesion_linked', 'lesion_matched', 'lesion_features', 'surface')


@pytest.fixture(scope='module')
def model(gpu):
    m = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    yield m
    m.close()


@pytest.fixture
def dm(model):
    yield model
    model.set_lesion_refine()


def plane(b=3, h=H, w=W, value=BG):
    return np.full((b, h, w), value, np.float32)


def same(got, want):
    assert got[1].tolist() == want[1].tolist(), (got[1], want[1])
    assert got[0].tolist() == want[0].tolist()
    assert got[0].tobytes() == want[0].tobytes()
    assert np.array_equal(got[2], want[2])


def refine_kw(refine):
    cfg = RO.config(refine)
    return dict(hysteresis=cfg['hysteresis'], closing=cfg['closing'], fill_holes=cfg['fill_holes'])


def run(dm, prob, refine, threshold=THR, rf=1.0, k=1, min_area=0, max_lesions=256):
    """set the refinement, lesion_table on the host planes, compare with the oracle -> (rows, totals, masks)"""
    dm.set_lesion_refine(**refine_kw(refine))
    got = dm.lesion_table(prob=prob, threshold=threshold, resize_factor=rf, filter_size=k, min_area=min_area, max_lesions=max_lesions)
    same(got, RO.lesion_table(prob, threshold, rf, k, min_area, max_lesions, refine=refine))
    return got


def ring(p, y0, y1, x0, x1, hy0, hy1, hx0, hx1, b=0, value=HIGH):
    """a filled rectangle [y0, y1] x [x0, x1] (inclusive) with the hole [hy0, hy1] x [hx0, hx1]"""
    p[b, y0:y1 + 1, x0:x1 + 1] = value
    p[b, hy0:hy1 + 1, hx0:hx1 + 1] = BG


# ---- holes ---------------------------------------------------------------------------------------------------------------------
def test_holes_across_a_seam_and_a_corner_are_filled(dm):
    p = plane()
    ring(p, 26, 38, 5, 15, 30, 34, 8, 11, b=0)           # the hole crosses the seam at row 32
    ring(p, 26, 38, 26, 38, 30, 34, 30, 34, b=0)         # the hole covers the tile corner (32, 32)
    ring(p, 58, 69, 27, 40, 62, 66, 30, 35, b=1)         # corner (64, 32), the ring on the plane's last row
    rows, totals, masks = run(dm, p, FILL)
    assert totals.tolist() == [2, 1, 0]
    assert rows['area'].tolist() == [13 * 11, 13 * 13, 12 * 14]
    assert run(dm, p, None)[0]['area'].tolist() == [13 * 11 - 20, 13 * 13 - 25, 12 * 14 - 30]


def test_holes_open_to_the_border_stay(dm):
    p = plane()
    ring(p, 0, 10, 5, 15, 0, 5, 8, 10, b=0)              # the hole reaches row 0
    ring(p, 40, 50, 20, 44, 44, 46, 24, 30, b=1)         # a hole ...
    p[1, 45, 31:45] = BG                                 # ... joined to the last column by a one-pixel channel across the seam at 32
    ring(p, 40, 50, 20, 44, 44, 46, 24, 30, b=2)         # the same without the channel: filled
    rows, totals, masks = run(dm, p, FILL)
    assert rows['area'].tolist() == [11 * 11 - 18, 11 * 25 - 21 - 14, 11 * 25]
    assert not masks[0, 0:6, 8:11].any() and not masks[1, 45, 24:45].any() and masks[2, 44:47, 24:31].all()


def test_diagonal_ring_island_and_full_planes(dm):
    p = plane()
    for y, x in [(30, 31), (30, 32), (30, 33), (34, 31), (34, 32), (34, 33), (31, 30), (32, 30), (33, 30), (31, 34), (32, 34), (33, 34)]:
        p[0, y, x] = HIGH                                # four arms that touch only diagonally, round the tile corner (32, 32)
    ring(p, 10, 18, 10, 18, 12, 16, 12, 16, b=1)
    p[1, 14, 14] = HIGH                                  # an island inside the hole inside the ring
    assert run(dm, p, None)[1].tolist() == [4, 2, 0]
    rows, totals, masks = run(dm, p, FILL)
    assert totals.tolist() == [1, 1, 0] and rows['area'].tolist() == [12 + 9, 81]
    full = np.stack([plane(1)[0], plane(1, value=HIGH)[0]])
    rows, totals, masks = run(dm, full, FILL)
    assert totals.tolist() == [0, 1] and not masks[0].any() and masks[1].all()


def test_nothing_leaks_between_slices(dm):
    p = plane()
    p[0, H - 1, :W - 1] = HIGH                           # slice 0: its last pixel is background ...
    p[1, 0, 0:10] = LOW                                  # ... beside slice 1's first pixel: a low region without a high pixel
    p[1, H - 1, W - 1] = HIGH                            # and a high pixel before slice 2's low first pixel
    p[2, 0, 0:7] = LOW
    p[2, 5:12, 5:12] = HIGH
    p[2, 7:9, 7:9] = BG
    rows, totals, masks = run(dm, p, dict(hysteresis=LO_THR, fill_holes=True))
    assert totals.tolist() == [1, 1, 1] and rows['area'].tolist() == [W - 1, 1, 49]
    run(dm, p, ALL3)


# ---- closing -------------------------------------------------------------------------------------------------------------------
def gap_plane(size, gap):
    """six pairs of bars `gap` apart: horizontal and vertical gaps in the middle of a tile, across a seam, and a bar `gap` pixels
    from the plane's border.  Slice 0: gaps along x, slice 1: along y, slice 2: the border cases"""
    p = plane(h=96, w=96)
    t = 3                                                # bar thickness along the gap's axis; 8 pixels across it
    for b, put in ((0, lambda s, a0, a1, c0: s.__setitem__((slice(c0, c0 + 8), slice(a0, a1)), HIGH)),
                   (1, lambda s, a0, a1, c0: s.__setitem__((slice(a0, a1), slice(c0, c0 + 8)), HIGH))):
        mid = 33 + (31 - gap) // 2                       # both bars and the gap inside the tile [32, 64) when they fit
        put(p[b], mid - t, mid, 8)                       # (8 pixels from the border: beyond the reach of the largest window)
        put(p[b], mid + gap, mid + gap + t, 8)
        seam = 64 - gap // 2                             # the gap lies across the seam at 64
        put(p[b], seam - t, seam, 40)
        put(p[b], seam + gap, seam + gap + t, 40)
    p[2, 4:12, gap:gap + t] = HIGH                       # `gap` background columns before the first column ...
    p[2, 96 - gap - t:96 - gap, 40:48] = HIGH            # ... and rows behind the last row
    return p


@pytest.mark.parametrize('size', [3, 15])
def test_closing_bridges_gaps_below_its_size(dm, size):
    closes = run(dm, gap_plane(size, size - 1), dict(closing=size))
    stays = run(dm, gap_plane(size, size), dict(closing=size))
    assert closes[1].tolist()[:2] == [2, 2] and stays[1].tolist()[:2] == [4, 4]
    assert (closes[0]['area'][:4] == 8 * (6 + size - 1)).all() and (stays[0]['area'][:8] == 24).all()
    # the closed mask contains the input, and closing twice is closing once (the second pass on the mask as probabilities)
    plain = run(dm, gap_plane(size, size - 1), None)
    assert not (plain[2] & ~closes[2]).any()
    again = run(dm, (closes[2] > 0).astype(np.float32), dict(closing=size))
    assert np.array_equal(again[2], closes[2])


def test_closing_on_a_plane_smaller_than_its_window(dm):
    p = (np.random.RandomState(3).rand(3, 8, 8) < 0.3).astype(np.float32)
    rows, totals, masks = run(dm, p, dict(closing=15))
    assert 0 < (masks > 0).sum() and not ((p > 0.5) & ~(masks > 0)).any()
    run(dm, p, dict(closing=3))


# ---- hysteresis ----------------------------------------------------------------------------------------------------------------
def test_hysteresis_keeps_regions_with_a_seed(dm):
    p = plane()
    p[0, 5, 2:41] = LOW
    p[0, 5, 40] = HIGH                                   # the only high pixel lies in the second tile, the body in the first
    p[0, 20:24, 2:30] = LOW                              # no high pixel: dropped
    p[1, 10:60, 20] = LOW                                # a column through three tiles, seeded at its far end
    p[1, 59, 20] = HIGH
    p[2, 40, 3:9] = LOW
    p[2, 40, 6] = np.nan                                 # NaN is background: the high pixel's side survives alone
    p[2, 40, 8] = HIGH
    rows, totals, masks = run(dm, p, dict(hysteresis=LO_THR))
    assert totals.tolist() == [1, 1, 1] and rows['area'].tolist() == [39, 50, 2]
    assert run(dm, p, None)[0]['area'].tolist() == [1, 1, 1]


def test_hysteresis_comparisons_are_greater_or_equal(dm):
    low, thr = np.float32(LO_THR), np.float32(THR)
    p = plane()
    p[0, 10, 5:12] = low                                 # exactly `low` ...
    p[0, 10, 12] = thr                                   # ... beside exactly the threshold: kept
    p[0, 10, 4] = np.nextafter(low, np.float32(0))       # just below `low`: outside
    p[1, 10, 5:12] = low
    p[1, 10, 12] = np.nextafter(thr, np.float32(0))      # just below the threshold: no seed
    rows, totals, _ = run(dm, p, dict(hysteresis=float(low)), threshold=float(thr))
    assert totals.tolist() == [1, 0, 0] and rows['area'].tolist() == [8]
    # the largest valid low
    just = np.nextafter(thr, np.float32(0))
    q = plane()
    q[0, 3, 3:6] = just
    q[0, 3, 6] = thr
    q[0, 3, 2] = np.nextafter(just, np.float32(0))
    rows, totals, _ = run(dm, q, dict(hysteresis=float(just)), threshold=float(thr))
    assert rows['area'].tolist() == [4]


# ---- composition ---------------------------------------------------------------------------------------------------------------
def blobs(seed, b=3, h=H, w=W):
    """smooth random planes on the levels 1/8, 3/8, 5/8, 7/8: a coarse random grid, enlarged and shifted per slice"""
    rs = np.random.RandomState(seed)
    coarse = rs.rand(b, (h + 6) // 7 + 2, (w + 6) // 7 + 2)
    big = np.kron(coarse, np.ones((7, 7)))
    out = np.empty((b, h, w), np.float32)
    for i in range(b):
        dy, dx = rs.randint(0, 7, 2)
        noise = rs.rand(h, w) * 0.18
        out[i] = np.floor(np.clip(big[i, dy:dy + h, dx:dx + w] + noise, 0, 0.999) * 4) / 4 + 0.125
    return out


def test_all_three_on_random_blobs(dm):
    p = blobs(11)
    refine = dict(hysteresis=LO_THR, closing=5, fill_holes=True)
    rows, totals, masks = run(dm, p, refine, k=5, min_area=6)
    plain = run(dm, p, None, k=5, min_area=6)
    assert totals.sum() > 0 and (masks > 0).sum() > (plain[2] > 0).sum()
    run(dm, p, refine, k=5, min_area=6, max_lesions=2)
    run(dm, p, dict(hysteresis=LO_THR), k=3)
    run(dm, p, dict(closing=7), k=3, min_area=3)


def test_order_hysteresis_before_the_opening(dm):
    p = plane()
    p[0, 10:18, 5:13] = LOW                              # a block without a high pixel ...
    p[0, 13, 13:20] = LOW                                # ... a one-pixel bridge that the opening removes ...
    p[0, 10:18, 20:28] = LOW                             # ... and a block with one
    p[0, 14, 24] = HIGH
    rows, totals, _ = run(dm, p, dict(hysteresis=LO_THR), k=3)
    assert totals.tolist() == [2, 0, 0] and rows['area'].tolist() == [64, 64]       # both blocks: the seed counted before the split


def test_resized_planes(dm):
    """resize_factor 0.5 of 90 x 70 -> 45 x 35.  The planes hold multiples of 1/8 and every weight of this resize is 1/2: the
    float32 and the float64 statement of the bilinear formula give the same two masks (asserted)"""
    p = blobs(5, 3, 90, 70)
    oh, ow = LO.O.out_size(90, 70, 0.5)
    a, b = LO.O.resize(p, oh, ow), LO.resize64(p, oh, ow)
    for t in (np.float32(THR), np.float32(LO_THR)):
        assert np.array_equal(a >= t, b >= t)
    refine = dict(hysteresis=LO_THR, closing=3, fill_holes=True)
    rows, totals, masks = run(dm, p, refine, rf=0.5, k=3, min_area=2)
    assert masks.shape == (3, 45, 35) and totals.sum() > 0
    same((rows, totals, masks), RO.lesion_table(p, THR, 0.5, 3, 2, refine=refine, resize=LO.resize64))


# ---- every entry point ---------------------------------------------------------------------------------------------------------
def test_every_entry_point_shares_the_refined_mask(dm):
    p = blobs(23)
    rs = np.random.RandomState(4)
    y = (blobs(29) > 0.6).astype(np.float32)
    kw = dict(threshold=THR, resize_factor=1.0, filter_size=3, min_area=4, max_lesions=64)
    cont = [False, True, True]
    dm.set_lesion_refine()
    plain = dm.lesion_table_matched(y, prob=p, continues=cont, mask=True, **kw)
    dm.set_lesion_refine(**refine_kw(ALL3))
    want = RO.lesion_table(p, THR, 1.0, 3, 4, 64, refine=ALL3)
    assert (want[2] > 0).sum() > (plain[2] > 0).sum()
    same(dm.lesion_table(prob=p, **kw), want)
    same(dm.lesion_table_spread(prob=p, spread=rs.rand(*p.shape).astype(np.float32), **kw)[:3], want)
    same(dm.lesion_table_features(prob=p, x=rs.rand(*p.shape, 2).astype(np.float32), **kw)[:3], want)
    linked = dm.lesion_table_linked(prob=p, continues=cont, **kw)
    same(linked[:3], want)
    matched = dm.lesion_table_matched(y, prob=p, continues=cont, mask=True, **kw)
    same(matched[:3], want)
    assert matched[3].tobytes() == linked[3].tobytes() and len(linked[3]) > 0
    maps = RO.row_maps(p, THR, 1.0, 3, 4, 64, refine=ALL3)
    import link_oracle as KO
    assert linked[3].tolist() == KO.links_of_maps(maps, cont).tolist()
    assert matched[7].tolist() == MO.pairs_of_maps(MO.true_maps(y, 1.0, 64), maps).tolist()
    for i in (4, 5, 6):                                  # the label side is the unrefined call's
        assert matched[i].tobytes() == plain[i].tobytes()
    counts, samples, edges = dm.surface_distances(y, prob=p, threshold=THR, filter_size=3, min_area=4, edges=True)
    wc, ws, we = RO.surface(p, y, THR, 1.0, 3, 4, refine=ALL3)
    assert counts.tolist() == wc.tolist() and samples.tolist() == ws.tolist() and np.array_equal(edges, we)


def test_filled_ring_has_the_discs_hausdorff_distance(dm):
    yy, xx = np.mgrid[0:H, 0:W]
    r2 = (yy - 33) ** 2 + (xx - 22) ** 2
    disc = (r2 <= 15 ** 2).astype(np.float32)[None]
    hollow = disc * (r2 > 7 ** 2)
    kw = dict(threshold=THR, filter_size=1)
    dm.set_lesion_refine()
    ring_d2 = dm.surface_distances(disc, prob=hollow, **kw)[1]
    disc_d2 = dm.surface_distances(disc, prob=disc, **kw)[1]
    assert ring_d2['d2'].max() >= 25 and disc_d2['d2'].max() == 0
    dm.set_lesion_refine(fill_holes=True)
    counts, filled_d2, _ = dm.surface_distances(disc, prob=hollow, **kw)
    assert filled_d2.tobytes() == disc_d2.tobytes() and counts[0, 0] == counts[0, 1] == counts[0, 2]


def test_last_forward_and_host_planes_give_the_same_table(gpu):
    from oracle import unet_oracle as OU
    m = gpu.DeviceModel('unet', 2, 32, 48, 3, **UNET)
    try:
        spec = OU.ModelSpec('unet', 2, **UNET)
        m.set_params(OU.flatten(spec, OU.init_params(spec, seed=5)))
        x, _ = OU.synthetic_batch(3, 32, 48, 2, seed_x=7, seed_y=8)
        prob = m.forward(x, training=False)[..., 0]
        thr, low = float(np.quantile(prob, 0.6)), float(np.quantile(prob, 0.4))
        assert 0 < low < thr
        refine = dict(hysteresis=low, closing=3, fill_holes=True)
        m.set_lesion_refine(**refine)
        kw = dict(threshold=thr, filter_size=3, min_area=2, max_lesions=64)
        dev = m.lesion_table(batch=3, **kw)
        same(dev, m.lesion_table(prob=prob, **kw))
        same(dev, RO.lesion_table(prob, thr, 1.0, 3, 2, 64, refine=refine))
        assert dev[1].sum() > 0 and m.last_prob(3).tobytes() == prob.tobytes()
    finally:
        m.close()


# ---- off is off, plans, chains, refusals ---------------------------------------------------------------------------------------
def plans(m):
    return {mode: [r[0] for r in m.plan(mode=mode, batch=3)] for mode in PLAN_MODES}


def visit(m, p, y):
    """every entry point once with the same arguments (a plan replays those of the pass's last call) -> lesion_table's result"""
    kw = dict(threshold=THR, filter_size=3)
    m.lesion_table_linked(prob=p, continues=[False] * 3, **kw)
    m.lesion_table_matched(y, prob=p, continues=[False] * 3, **kw)
    m.lesion_table_features(prob=p, x=p[..., None], **kw)
    m.surface_distances(y, prob=p, **kw)
    return m.lesion_table(prob=p, **kw)


def test_off_is_off_and_on_is_listed(gpu, dm):
    p = blobs(31)
    y = (blobs(33) > 0.6).astype(np.float32)
    fresh = gpu.DeviceModel('unet', 1, 16, 16, 3, **UNET)
    try:
        want, want_plans = visit(fresh, p, y), plans(fresh)
    finally:
        fresh.close()
    assert dm.lesion_refine() == (None, 0, False)
    dm.set_lesion_refine(**refine_kw(ALL3))
    assert dm.lesion_refine() == (pytest.approx(LO_THR), 3, True)
    same(visit(dm, p, y), RO.lesion_table(p, THR, 1.0, 3, refine=ALL3))
    on = plans(dm)
    for mode in PLAN_MODES:
        assert set(NEW) <= set(on[mode]), mode
        assert on[mode].count('region_ccl_tile') == want_plans[mode].count('region_ccl_tile') + 2
    dm.set_lesion_refine(closing=5)
    assert [n for n in plans(dm)['lesion'] if n in NEW] == ['region_close']
    dm.set_lesion_refine()
    got = visit(dm, p, y)
    assert plans(dm) == want_plans and not set(NEW) & {n for names in want_plans.values() for n in names}
    same(got, want)
    same(want, LO.lesion_table(p, THR, 1.0, 3))


def test_changing_the_refinement_ends_a_chain(dm):
    from dnncancerannotator_amd._lib import DnncaError
    p = blobs(37)
    y = (blobs(41) > 0.6).astype(np.float32)
    kw = dict(threshold=THR, filter_size=3)
    dm.set_lesion_refine(fill_holes=True)
    first = dm.lesion_table_linked(prob=p, continues=[False, True, True], **kw)
    dm.lesion_table_matched(y, prob=p, continues=[False, True, True], **kw)
    dm.set_lesion_refine(fill_holes=True)                # the same configuration: the chains go on
    again = dm.lesion_table_linked(prob=p, continues=[True, True, True], **kw)
    assert again[0].tobytes() == first[0].tobytes() and len(again[3]) > len(first[3])
    dm.lesion_table_matched(y, prob=p, continues=[True, True, True], **kw)
    dm.set_lesion_refine(fill_holes=True, closing=3)     # another one: continues[0] is refused as before any chain
    for call in (lambda: dm.lesion_table_linked(prob=p, continues=[True, True, True], **kw),
                 lambda: dm.lesion_table_matched(y, prob=p, continues=[True, True, True], **kw)):
        with pytest.raises(DnncaError) as e:
            call()
        assert e.value.code == -1 and 'continues[0]' in str(e.value)
    dm.lesion_table_linked(prob=p, continues=[False, True, True], **kw)
    dm.lesion_table_linked(prob=p, continues=[True, True, True], **kw)


def test_refusals_change_and_launch_nothing(dm):
    from dnncancerannotator_amd import _lib
    from dnncancerannotator_amd._lib import DnncaError
    dm.set_lesion_refine(hysteresis=0.25, closing=5, fill_holes=True)
    bad = [(float('nan'), 0, 0), (-0.1, 0, 0), (1.0, 0, 0), (1.5, 0, 0), (0.0, -1, 0), (0.0, 2, 0), (0.0, 14, 0), (0.0, 16, 0),
           (0.0, 17, 0), (0.0, 0, 2), (0.0, 0, -1)]
    for low, closing, fill in bad:
        c = _lib.LesionRefine(low, closing, fill)
        assert dm.lib.dnnca_model_set_lesion_refine(dm.handle, C.byref(c)) == -1, (low, closing, fill)
        assert dm.lesion_refine() == (0.25, 5, True)
    with pytest.raises(DnncaError):
        dm.set_lesion_refine(closing=4)
    assert dm.lib.dnnca_model_get_lesion_refine(dm.handle, None) == -1
    p = blobs(43)
    y = np.zeros_like(p)
    dm.sync()
    dm.profile_reset()
    dm.profile_enable(1)
    try:
        for thr in (0.25, 0.2):                          # not above hysteresis_low
            for call in (lambda: dm.lesion_table(prob=p, threshold=thr), lambda: dm.lesion_table_spread(prob=p, spread=p, threshold=thr),
                         lambda: dm.lesion_table_features(prob=p, x=p[..., None], threshold=thr),
                         lambda: dm.lesion_table_linked(prob=p, continues=[False] * 3, threshold=thr),
                         lambda: dm.lesion_table_matched(y, prob=p, continues=[False] * 3, threshold=thr),
                         lambda: dm.surface_distances(y, prob=p, threshold=thr)):
                with pytest.raises(DnncaError) as e:
                    call()
                assert e.value.code == -1 and 'hysteresis_low' in str(e.value)
        assert dm.profile() == []
    finally:
        dm.profile_enable(0)
        dm.profile_reset()
    assert dm.lesion_refine() == (0.25, 5, True)
    assert dm.lib.dnnca_model_set_lesion_refine(dm.handle, None) == 0 and dm.lesion_refine() == (None, 0, False)


def test_run_to_run(dm):
    p = blobs(47)
    dm.set_lesion_refine(hysteresis=LO_THR, closing=5, fill_holes=True)
    a = dm.lesion_table(prob=p, filter_size=3, min_area=3)
    b = dm.lesion_table(prob=p, filter_size=3, min_area=3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[1].sum() > 0
