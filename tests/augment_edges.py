"""The augmentation kernels (csrc/kernels_aug.hip) at the shapes where they can go wrong: inputs, references and checks shared by
tests/test_augment_edges_gpu.py (the HIP kernels) and tests/test_augment_edges.py (a CPU rehearsal of the same checks).

Every check takes a "device" object:
    augment(raw, params, out_size, label_index, channels) -> x, y          dnnca_augment_u8; sets .launches {kernel: count}
    augment_burst(calls) -> [(x, y)]            the calls back to back, nothing read or synchronised in between, then ONE sync
    warp(x, y, ctrl, wv) -> xw, yw                                           dnnca_warp_f32
    warp_groups(x, y, group_of, ctrl, wv) -> xw, yw                          dnnca_warp_groups_f32
    warp_groups_burst(calls) -> [(xw, yw)]      like augment_burst
Outputs are pre-filled with SENTINEL by the device object, so a pixel no thread wrote shows.

GpuDevice drives a DeviceModel.  NumpyDevice restates the kernels' arithmetic in float32 numpy -- integer window sums, float32
mean, the float64 flow of the oracle cast to float32 and the float32 bilinear taps at the kernel's flat offsets, the pinned rings
as rows that an upload reads when the stream gets to it -- and takes a `mutation`: the defects the checks are meant to catch,
which could not be run on a GPU (most of them index out of bounds there).  With no mutation it shows how much of every bound the
float32 arithmetic itself uses; the reference is oracle/augment_oracle.py throughout.

References are computed once per case (lru_cache) and never written to.  Test infrastructure only."""

import ctypes as C
import functools

import numpy as np

from oracle import augment_oracle as A

SENTINEL = np.float32(-7.0)
F32 = np.float32

# (B, hs, ws, cs, label, ho, wo); what each is for: AUG_WHY.  The two-channel shapes carry three images: with one feature channel
# a batch needs a third image to hold an adjusted random channel, a factor-1.0 image AND an adjusted constant channel.
AUG_SHAPES = {
    'two_blocks_label_first': (3, 80, 72, 3, 0, 72, 64),
    'odd_eight_channels': (2, 41, 53, 8, 3, 30, 47),
    'no_margin': (3, 64, 48, 2, 1, 64, 48),
    'block_cap': (3, 528, 520, 2, 1, 520, 512),
}
AUG_WHY = {
    'two_blocks_label_first': 'n = 4608 output pixels: bx = 2, the grid-stride loop and the cross-block atomicAdd; label_index 0',
    'odd_eight_channels': 'odd (hs - ho), odd margins, odd wo under flip, cs = 8 = AUG_MAXC, label in the middle',
    'no_margin': 'ho = hs, wo = ws: the only legal draws are (0, 0, ., .)',
    'block_cap': 'n = 266 240: 65 blocks of 4096 pixels asked for, capped at 64 -- the loop takes a second trip in block 0',
}
AUG_VARIANTS = ('default', 'subset', 'none')
X_BOUND = 2e-6          # contrast: float32 mean against float64 mean (tests/test_augment.py)
POSITION_BOUND, SMOOTH_BOUND = 1e-2, 1e-3           # tests/test_augment.py, tests/test_intrawarp_gpu.py
FLOAT32_ROOM = 1e-4     # the float32 restatement must stay a hundred times inside POSITION_BOUND


# ---------------------------------------------------------------------------------------------------------- crop / flip / contrast
@functools.lru_cache(maxsize=None)
def aug_case(name):
    """raw [B, hs, ws, cs] uint8, draws, and per variant the channels passed to the device and the oracle's (x, y)"""
    B, hs, ws, cs, label, ho, wo = AUG_SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    raw = rng.integers(0, 256, (B, hs, ws, cs), dtype=np.uint8)
    feat = [c for c in range(cs) if c != label]
    my, mx = hs - ho, ws - wo
    params = []
    for b in range(B):
        dy = int(rng.integers(-(my // 2), my - my // 2 + 1))
        dx = int(rng.integers(-(mx // 2), mx - mx // 2 + 1))
        params.append((dy, dx, int(rng.integers(0, 2)), float(F32(rng.uniform(0.8, 1.2)))))
    params[0] = (-(my // 2), mx - mx // 2, 1, float(F32(1.2)))        # top = 0, left + wo = ws, flipped
    params[1] = params[1][:3] + (1.0,)                                 # the identity factor
    if len(feat) >= 2:                 # constant channels under factor 1.2: the integer sum is exact, (v - mean) must vanish
        raw[0, :, :, feat[0]], raw[0, :, :, feat[-1]] = 255, 0
    else:
        raw[2, :, :, feat[0]], raw[2, :, :, label] = 255, 0
        assert params[2][3] != 1.0
    # 'subset': a proper subset of the feature channels; with a single feature channel the subset names it and the label (whose bit
    # the library must clear: the label is never adjusted)
    subset = tuple(feat[::2]) if len(feat) >= 2 else (feat[0], label)
    no_contrast = [p[:3] + (1.0,) for p in params]
    ref = {'default': A.augment_batch(raw, params, (ho, wo), label),
           'subset': A.augment_batch(raw, params, (ho, wo), label, [c for c in subset if c != label]),
           'none': A.augment_batch(raw, no_contrast, (ho, wo), label)}
    channels = {'default': None, 'subset': subset, 'none': ()}
    for a in (raw,) + tuple(v for r in ref.values() for v in r):
        a.setflags(write=False)
    return dict(raw=raw, params=params, out_size=(ho, wo), label=label, feat=feat, channels=channels, ref=ref)


def check_augment(dev, name, variant):
    """y bit-exact; x bit-exact where the factor is 1.0 or the channel is outside the mask, |dx| <= 2e-6 elsewhere; with no channel
    to adjust the sums kernel is not launched.  Returns the worst |dx| of the adjusted channels."""
    case = aug_case(name)
    channels = case['channels'][variant]
    x, y = dev.augment(case['raw'], case['params'], case['out_size'], case['label'], channels)
    xr, yr = case['ref'][variant]
    assert x.shape == xr.shape and y.shape == yr.shape
    assert np.array_equal(y, yr), 'label: crop / flip / 255 are exact and the label is never adjusted'
    masked = set(case['feat'] if channels is None else channels)
    worst = 0.0
    for b, p in enumerate(case['params']):
        for k, c in enumerate(case['feat']):
            if p[3] == 1.0 or c not in masked:
                assert np.array_equal(x[b, ..., k], xr[b, ..., k]), 'image %d channel %d must be bit-exact' % (b, c)
            else:
                d = float(np.abs(x[b, ..., k] - xr[b, ..., k]).max())
                worst = max(worst, d)
                assert d <= X_BOUND, 'image %d channel %d: |dx| %.3g' % (b, c, d)
    print('augment %s / %s: worst |dx| of the adjusted channels %.3g' % (name, variant, worst))
    if dev.launches is not None:
        assert dev.launches.get('aug_apply') == 1, dev.launches
        assert dev.launches.get('aug_sums', 0) == (0 if variant == 'none' else 1), dev.launches
    return worst


RING_MAX_BATCH = 2


@functools.lru_cache(maxsize=None)
def augment_burst_case():
    """six calls of batch 2 (the model's max_batch) with draws of their own, then one of batch 5: its draws outgrow the ring's rows"""
    rng = np.random.default_rng(77)
    hs, ws, cs, label, ho, wo = 24, 20, 3, 2, 16, 12
    calls = []
    for i in range(7):
        B = RING_MAX_BATCH if i < 6 else 5
        raw = rng.integers(0, 256, (B, hs, ws, cs), dtype=np.uint8)
        # every call's draws differ from every other call's in every field
        params = [(i - 3 + b % 2, 3 - i - b % 2, (i + b) % 2, float(F32(0.8 + 0.05 * i + 0.01 * b))) for b in range(B)]
        calls.append((raw, params, (ho, wo), label, None))
    refs = [A.augment_batch(raw, params, out, lab) for raw, params, out, lab, _ in calls]
    return calls, refs


def check_augment_burst(dev):
    """a row of the pinned ring overwritten before its upload has run shows as one call's output carrying another call's draws"""
    calls, refs = augment_burst_case()
    outs = dev.augment_burst(calls)
    worst = 0.0
    for i, ((x, y), (xr, yr)) in enumerate(zip(outs, refs)):
        assert np.array_equal(y, yr), 'call %d: label' % i
        d = float(np.abs(x - xr).max())
        worst = max(worst, d)
        assert d <= X_BOUND, 'call %d: |dx| %.3g' % (i, d)
    print('augment burst: worst |dx| %.3g over %d calls' % (worst, len(calls)))
    return worst


# ------------------------------------------------------------------------------------------------------------------- warp: images
def exact_images(B, H, W, C, seed=5):
    """multiples of 1/256 in [0, 1): every lerp at alpha 0 or 1 is exact in float32"""
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 256, (B, H, W, C)) / 256.0).astype(F32)
    y = (rng.integers(0, 256, (B, H, W)) / 256.0).astype(F32)
    return x, y


KINDS = ('row', 'col', 'smooth')


def ramp_images(B, H, W, kinds):
    """x [B, H, W, C], y [B, H, W]: `kinds` names the image of every feature channel, then the label's: the row ramp yy / H, the
    column ramp xx / W (a warped ramp IS the sampling position q - flow(q), clamps included) or a smooth image"""
    yy, xx = np.mgrid[:H, :W].astype(F32)
    img = {'row': yy / H, 'col': xx / W, 'smooth': 0.5 + 0.25 * np.sin(yy / 7.0) * np.cos(xx / 5.0)}
    chans = [img[k].astype(F32) for k in kinds]
    x = np.stack([np.stack(chans[:-1], -1)] * B).astype(F32)
    y = np.stack([chans[-1]] * B).astype(F32)
    return x, y


def shift_coeffs(shifts, n=4, H=40, W=72):
    """pure affine flow: w = 0, v = the constant (sy, sx); shifts [..., 2] -> ctrl [..., n, 2], wv [..., n + 3, 2]"""
    shifts = np.asarray(shifts, np.float64)
    rng = np.random.default_rng(6)
    ctrl = rng.uniform(0, 1, shifts.shape[:-1] + (n, 2)) * [H, W]
    wv = np.zeros(shifts.shape[:-1] + (n + 3, 2))
    wv[..., n + 2, :] = shifts
    return ctrl, wv


def shifted(img, sy, sx):
    """img [H, W, ...] sampled at (clip(qy - sy), clip(qx - sx)): what a constant integer flow makes of it -- no spline in here"""
    H, W = img.shape[:2]
    return img[np.clip(np.arange(H) - sy, 0, H - 1)][:, np.clip(np.arange(W) - sx, 0, W - 1)]


EXACT = dict(B=2, H=40, W=72, C=3)         # 2880 pixels = 11 x 256 + 64: a partial last block
EXACT_GROUP_OF = [0, 1, 2, 1]              # channel 0 | channels 1 + label | channel 2
# per image (warp) and per image and group (groups): sy != sx everywhere; image 1 holds a row shift larger than H (every row clamps)
EXACT_SHIFTS = [(3, -5), (47, 2)]
EXACT_GROUP_SHIFTS = [[(3, -5), (-2, 7), (1, 4)], [(47, 2), (-6, -1), (5, -80)]]


def check_warp_identity(dev, entry):
    """zero coefficients: output bit-identical to the input, last row and column (alpha 1 on the clamped floor) included"""
    B, H, W, Cc = (EXACT[k] for k in 'BHWC')
    x0, y0 = exact_images(B, H, W, Cc)
    if entry == 'warp':
        ctrl, wv = shift_coeffs(np.zeros((B, 2)))
        xw, yw = dev.warp(x0, y0, ctrl, wv)
    else:
        ctrl, wv = shift_coeffs(np.zeros((B, 3, 2)))
        xw, yw = dev.warp_groups(x0, y0, EXACT_GROUP_OF, ctrl, wv)
    assert np.array_equal(xw, x0) and np.array_equal(yw, y0)


def check_warp_shift(dev, entry):
    """constant integer flows: out = img[clip(qy - sy), clip(qx - sx)] bit for bit -- pins H against W without a spline"""
    B, H, W, Cc = (EXACT[k] for k in 'BHWC')
    x0, y0 = exact_images(B, H, W, Cc)
    if entry == 'warp':
        xw, yw = dev.warp(x0, y0, *shift_coeffs(EXACT_SHIFTS))
        for b, (sy, sx) in enumerate(EXACT_SHIFTS):
            assert np.array_equal(xw[b], shifted(x0[b], sy, sx)), 'image %d' % b
            assert np.array_equal(yw[b], shifted(y0[b], sy, sx)), 'label %d' % b
    else:
        xw, yw = dev.warp_groups(x0, y0, EXACT_GROUP_OF, *shift_coeffs(EXACT_GROUP_SHIFTS))
        for b in range(B):
            for c in range(Cc):
                assert np.array_equal(xw[b, ..., c], shifted(x0[b, ..., c], *EXACT_GROUP_SHIFTS[b][EXACT_GROUP_OF[c]])), (b, c)
            assert np.array_equal(yw[b], shifted(y0[b], *EXACT_GROUP_SHIFTS[b][EXACT_GROUP_OF[Cc]])), b


# ---------------------------------------------------------------------------------------------------------- warp: against the oracle
def _draw(rng, shape, H, W, max_diff, stddev):
    """random_warp's draws (augment.draw_warp) for an H x W rectangle: source uniform in [0, H) x [0, W), float32"""
    src = (rng.uniform(0.0, 1.0, shape + (2,)) * [H, W]).astype(F32)
    diff = np.clip(rng.normal(0.0, stddev, shape + (2,)), -max_diff, max_diff).astype(F32)
    return src, src + diff


def _jittered_grid(rng, n, H, W):
    """n points, one in each cell of a grid over the H x W rectangle, jittered inside its cell"""
    rows = max(1, int(round(np.sqrt(n * H / W))))
    cols = -(-n // rows)
    cell = np.stack(np.divmod(np.arange(n), cols), -1).astype(np.float64)
    return (cell + rng.uniform(0.2, 0.8, (n, 2))) * [H / rows, W / cols]


GROUPS4 = (('row', 'row', 'col', 'smooth', 'col'), [0, 1, 2, 3, 0])       # tests/test_intrawarp_gpu.py: [[0, label], [1], [2], [3]]
GROUPS8 = (('row', 'col', 'smooth', 'row', 'col', 'smooth', 'row', 'col', 'col'), [0, 1, 1, 2, 2, 3, 3, 4, 0])
WARP3 = ('row', 'col', 'smooth', 'smooth')
WARP8 = ('row', 'col', 'smooth', 'col', 'row', 'smooth', 'row', 'col', 'smooth')
# name: (entry, B, H, W, kinds (features..., label), group_of or None, n, how the coefficients are made)
WARP_CASES = {
    'warp_40x72': ('warp', 2, 40, 72, WARP3, None, 100, ('solve', 5, 2.0)),
    'warp_72x40_c8': ('warp', 2, 72, 40, WARP8, None, 100, ('solve', 5, 2.0)),
    'warp_clamps_64x48': ('warp', 2, 64, 48, WARP3, None, 100, ('solve', 100, 20.0)),
    'warp_n150': ('warp', 1, 40, 72, WARP3, None, 150, ('solve', 5, 2.0)),
    'warp_n1_c1': ('warp', 2, 40, 72, ('row', 'col'), None, 1, ('one',)),
    'warp_n2046_c1': ('warp', 1, 16, 24, ('row', 'col'), None, 2046, ('many',)),
    'groups_40x72': ('groups', 2, 40, 72) + GROUPS4 + (100, ('solve', 5, 2.0)),
    'groups_72x40_c8': ('groups', 2, 72, 40) + GROUPS8 + (100, ('solve', 5, 2.0)),
    'groups_n150': ('groups', 1, 40, 72) + GROUPS4 + (150, ('solve', 5, 2.0)),
    'groups_n1_c1': ('groups', 2, 40, 72, ('row', 'col'), [0, 1], 1, ('one',)),
    'groups_n2046_c1': ('groups', 1, 16, 24, ('row', 'col'), [1, 0], 2046, ('many',)),
}


@functools.lru_cache(maxsize=None)
def warp_case(name):
    """images, coefficients [B, G, n, 2] / [B, G, n + 3, 2] (G = 1 for dnnca_warp_f32) and the oracle's image of every channel"""
    from dnncancerannotator_amd import augment
    entry, B, H, W, kinds, group_of, n, how = WARP_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x0, y0 = ramp_images(B, H, W, kinds)
    Cc = x0.shape[-1]
    table = [0] * (Cc + 1) if group_of is None else list(group_of)
    G = max(table) + 1
    src = dst = None
    if how[0] == 'solve':          # the project's host solve feeds the device, the oracle solves for itself from the same points
        src, dst = _draw(rng, (B, G, n), H, W, how[1], how[2])
        ctrl, wv = augment.solve_intrawarp(src, dst)
    elif how[0] == 'one':          # one control point: its weight alone bends the flow, the linear rows shear and shift it
        ctrl = rng.uniform(0.3, 0.7, (B, G, 1, 2)) * [H, W]
        wv = np.zeros((B, G, 4, 2))
        wv[:, :, 0] = rng.choice([-1.0, 1.0], (B, G, 2)) * rng.uniform(1e-4, 2e-4, (B, G, 2))
        wv[:, :, 1:3] = rng.uniform(-0.02, 0.02, (B, G, 2, 2))
        wv[:, :, 3] = rng.uniform(1.5, 3.0, (B, G, 2)) * rng.choice([-1.0, 1.0], (B, G, 2))
    else:                          # 2046 points on a jittered grid, weights small enough that the flow stays within a few pixels
        ctrl = np.stack([np.stack([_jittered_grid(rng, n, H, W) for _ in range(G)]) for _ in range(B)])
        wv = np.zeros((B, G, n + 3, 2))
        wv[:, :, :n] = rng.normal(0.0, 4e-5, (B, G, n, 2))
        wv[:, :, n + 2] = rng.uniform(1.5, 2.5, (B, G, 2))
    full = np.concatenate([x0, y0[..., None]], -1)
    ref = np.empty(full.shape, np.float64)
    flow_max = 0.0
    for b in range(B):
        for g in range(G):
            chans = [c for c in range(Cc + 1) if table[c] == g]
            if src is not None:
                ref[b][..., chans] = A.warp_image(full[b][..., chans], src[b, g], dst[b, g])
            else:
                ref[b][..., chans] = A.warp_image_coeffs(full[b][..., chans], ctrl[b, g], wv[b, g])
            flow_max = max(flow_max, float(np.abs(A.warp_flow(H, W, ctrl[b, g], wv[b, g])).max()))
    for a in (x0, y0, ctrl, wv, ref):
        a.setflags(write=False)
    return dict(entry=entry, x0=x0, y0=y0, kinds=kinds, table=table, ctrl=ctrl, wv=wv, ref=ref, flow_max=flow_max, H=H, W=W)


def check_warp_case(dev, name, position_bound=POSITION_BOUND, smooth_bound=SMOOTH_BOUND):
    """ramp channels (sampling positions) to 1e-2 pixel, smooth channels to 1e-3, and every ramp moved by more than a pixel.
    Returns (worst position error in pixels, worst smooth error, the device's (xw, yw))."""
    case = warp_case(name)
    x0, y0, H, W = case['x0'], case['y0'], case['H'], case['W']
    if case['entry'] == 'warp':
        xw, yw = dev.warp(x0, y0, case['ctrl'][:, 0], case['wv'][:, 0])
    else:
        xw, yw = dev.warp_groups(x0, y0, case['table'], case['ctrl'], case['wv'])
    out = np.concatenate([xw, yw[..., None]], -1)
    src = np.concatenate([x0, y0[..., None]], -1)
    position = smooth = 0.0
    moved = []
    for c, kind in enumerate(case['kinds']):
        err = float(np.abs(out[..., c] - case['ref'][..., c]).max())
        if kind == 'smooth':
            smooth = max(smooth, err)
        else:
            scale = H if kind == 'row' else W
            position = max(position, err * scale)
            moved.append(min(float(np.abs(out[b, ..., c] - src[b, ..., c]).max()) * scale for b in range(len(out))))
    print('warp %s: position error %.3g px, smooth error %.3g, least motion of a ramp %.2f px, largest flow %.1f px'
          % (name, position, smooth, min(moved), case['flow_max']))
    assert position <= position_bound, 'position error %.3g px' % position
    assert smooth <= smooth_bound, 'smooth error %.3g' % smooth
    assert min(moved) > 1.0, 'a channel group did not move: %s' % moved
    return position, smooth, (xw, yw)


@functools.lru_cache(maxsize=None)
def warp_groups_burst_case():
    """six calls of two groups with coefficients of their own, then one of four groups: its row outgrows the ring's"""
    rng = np.random.default_rng(78)
    B, H, W, n = 1, 12, 20, 8
    kinds = ('row', 'col', 'smooth', 'col')
    x0, y0 = ramp_images(B, H, W, kinds)
    full = np.concatenate([x0, y0[..., None]], -1)
    calls, refs = [], []
    for i in range(7):
        table = [0, 1, 1, 0] if i < 6 else [0, 1, 2, 3]
        G = max(table) + 1
        ctrl = rng.uniform(0, 1, (B, G, n, 2)) * [H, W]
        wv = np.zeros((B, G, n + 3, 2))
        wv[:, :, :n] = rng.normal(0.0, 2e-4, (B, G, n, 2))
        wv[:, :, n + 2] = [[(1.5 + 0.5 * i) * (-1) ** g, (4.0 - 0.5 * i) * (-1) ** (g + i)] for g in range(G)]
        ref = np.empty(full.shape, np.float64)
        for g in range(G):
            chans = [c for c in range(4) if table[c] == g]
            ref[0][..., chans] = A.warp_image_coeffs(full[0][..., chans], ctrl[0, g], wv[0, g])
        calls.append((x0, y0, table, ctrl, wv))
        refs.append(ref)
    return calls, refs, kinds, (H, W)


def check_warp_groups_burst(dev):
    calls, refs, kinds, (H, W) = warp_groups_burst_case()
    outs = dev.warp_groups_burst(calls)
    worst = 0.0
    for i, ((xw, yw), ref) in enumerate(zip(outs, refs)):
        out = np.concatenate([xw, yw[..., None]], -1)
        for c, kind in enumerate(kinds):
            err = float(np.abs(out[..., c] - ref[..., c]).max())
            if kind == 'smooth':
                assert err <= SMOOTH_BOUND, 'call %d channel %d: smooth error %.3g' % (i, c, err)
            else:
                err *= H if kind == 'row' else W
                worst = max(worst, err)
                assert err <= POSITION_BOUND, 'call %d channel %d: position error %.3g px' % (i, c, err)
    print('warp_groups burst: worst position error %.3g px over %d calls' % (worst, len(calls)))
    return worst


# ------------------------------------------------------------------------------------------------------------- the numpy stand-in
class _Ring:
    """kAugRing pinned rows and the stream behind them: submit() copies the caller's bytes into the next row at once (waiting first
    for the upload that last read that row) and queues work that reads the row only when the stream gets to it"""
    ROWS = 4

    def __init__(self, read_row_zero=False):
        self.row_bytes, self.rows, self.k, self.queue, self.read_row_zero = 0, None, 0, [], read_row_zero

    def _run(self, upto):
        for row, n, work in self.queue[:upto]:
            work(self.rows[0 if self.read_row_zero else row][:n].tobytes())
        del self.queue[:upto]

    def sync(self):
        self._run(len(self.queue))

    def submit(self, data, work, min_row_bytes=0):
        if len(data) > self.row_bytes:              # regrow: the stream is drained, the rows are replaced
            self.sync()
            self.row_bytes = max(len(data), min_row_bytes)
            self.rows = np.zeros((self.ROWS, self.row_bytes), np.uint8)
        k, self.k = self.k, (self.k + 1) % self.ROWS
        last = [i for i, item in enumerate(self.queue) if item[0] == k]
        if last:
            self._run(last[-1] + 1)                 # the event recorded behind the upload that read row k
        self.rows[k, :len(data)] = np.frombuffer(data, np.uint8)
        self.queue.append((k, len(data), work))


PARAM_DTYPE = np.dtype([('dy', np.int32), ('dx', np.int32), ('flip', np.int32), ('contrast', np.float32)])
MUTATIONS = ('swap_hw', 'tail_unwritten', 'coeffs_256', 'sums_4096', 'label_bit', 'ring_row_0')


class NumpyDevice:
    """float32 restatement of csrc/kernels_aug.hip (see the module docstring); `mutation`: one of MUTATIONS or None"""

    def __init__(self, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.mutation = mutation
        self.launches = None
        self.aug_ring = _Ring(mutation == 'ring_row_0')
        self.warpg_ring = _Ring(mutation == 'ring_row_0')

    # ---- k_aug_sums / k_aug_apply
    def _augment(self, raw, prm, out_size, label, mask):
        B, hs, ws, cs = raw.shape
        ho, wo = out_size
        n = ho * wo
        if self.mutation != 'label_bit':
            mask &= ~(1 << label)
        self.launches = {'aug_apply': 1}
        if mask:
            self.launches['aug_sums'] = 1
        x = np.full((B, ho, wo, cs - 1), SENTINEL, F32)
        y = np.full((B, ho, wo), SENTINEL, F32)
        inv_n = F32(1.0) / F32(n)
        for b in range(B):
            top, left = (hs - ho) // 2 + int(prm['dy'][b]), (ws - wo) // 2 + int(prm['dx'][b])
            win = raw[b, top:top + ho, left:left + wo, :]
            summed = win.reshape(n, cs)[:4096] if self.mutation == 'sums_4096' else win.reshape(n, cs)
            sums = summed.astype(np.uint32).sum(0, dtype=np.uint32)
            if prm['flip'][b]:
                win = win[:, ::-1]
            f = F32(prm['contrast'][b])
            k = 0
            for c in range(cs):
                v = win[..., c].astype(F32) / F32(255.0)
                if (mask >> c) & 1 and f != F32(1.0):
                    mean = (F32(sums[c]) * inv_n) / F32(255.0)
                    v = (v - mean) * f + mean
                if c == label:
                    y[b] = v
                else:
                    x[b, ..., k] = v
                    k += 1
        return x, y

    @staticmethod
    def _mask(cs, label, channels):
        mask = 0
        for c in ([c for c in range(cs) if c != label] if channels is None else channels):
            mask |= 1 << int(c)
        return mask

    def augment(self, raw, params, out_size, label, channels):
        return self.augment_burst([(raw, params, out_size, label, channels)])[0]

    def augment_burst(self, calls):
        outs = [None] * len(calls)
        for i, (raw, params, out_size, label, channels) in enumerate(calls):
            def work(row, i=i, raw=raw, out_size=out_size, label=label, mask=self._mask(raw.shape[-1], label, channels)):
                outs[i] = self._augment(raw, np.frombuffer(row, PARAM_DTYPE), out_size, label, mask)
            self.aug_ring.submit(np.array([tuple(p) for p in params], PARAM_DTYPE).tobytes(), work,
                                 RING_MAX_BATCH * PARAM_DTYPE.itemsize)
        self.aug_ring.sync()
        return outs

    # ---- k_warp / k_warp_groups
    def _taps(self, H, W, ctrl, wv):
        n = len(ctrl)
        ctrl, wv = np.array(ctrl, np.float64), np.array(wv, np.float64)
        if self.mutation == 'coeffs_256':           # the copy into LDS stops after one pass of 256 threads
            ctrl.reshape(-1)[256:] = 0.0
            wv[:n].reshape(-1)[256:] = 0.0
        flow = A.warp_flow(H, W, ctrl, wv).astype(F32)
        idx = np.arange(H * W)
        qy, qx = idx // W, idx % W
        sy, sx = qy.astype(F32) - flow[:, 0], qx.astype(F32) - flow[:, 1]
        ch, cw = (W, H) if self.mutation == 'swap_hw' else (H, W)
        fy = np.minimum(np.maximum(np.floor(sy), F32(0)), F32(ch - 2))
        fx = np.minimum(np.maximum(np.floor(sx), F32(0)), F32(cw - 2))
        ay = np.minimum(np.maximum(sy - fy, F32(0)), F32(1))
        ax = np.minimum(np.maximum(sx - fx, F32(0)), F32(1))
        o00 = fy.astype(np.int64) * W + fx.astype(np.int64)
        written = idx < (H * W // 256) * 256 if self.mutation == 'tail_unwritten' else np.ones(H * W, bool)
        return o00, ay, ax, written

    @staticmethod
    def _sample(plane, out, taps, W):
        """plane, out [H * W] float32: the four taps at the kernel's flat offsets (o10 = o00 + W), lerps in float32"""
        o00, ay, ax, written = taps
        tl, tr, bl, br = (np.take(plane, o00 + d, mode='clip') for d in (0, 1, W, W + 1))
        top, bot = ax * (tr - tl) + tl, ax * (br - bl) + bl
        out[written] = (ay * (bot - top) + top)[written]

    def _warp_groups(self, x, y, table, ctrl, wv):
        B, H, W, Cc = x.shape
        xo, yo = np.full(x.shape, SENTINEL, F32), np.full(y.shape, SENTINEL, F32)
        for b in range(B):
            for g in range(ctrl.shape[1]):
                taps = self._taps(H, W, ctrl[b, g], wv[b, g])
                for c in range(Cc):
                    if table[c] == g:
                        plane, out = np.ascontiguousarray(x[b, ..., c]).reshape(-1), np.empty(H * W, F32)
                        out[:] = SENTINEL
                        self._sample(plane, out, taps, W)
                        xo[b, ..., c] = out.reshape(H, W)
                if table[Cc] == g:
                    self._sample(y[b].reshape(-1), yo[b].reshape(-1), taps, W)
        return xo, yo

    def warp(self, x, y, ctrl, wv):
        return self._warp_groups(x, y, [0] * (x.shape[-1] + 1), np.asarray(ctrl)[:, None], np.asarray(wv)[:, None])

    def warp_groups(self, x, y, group_of, ctrl, wv):
        return self.warp_groups_burst([(x, y, group_of, ctrl, wv)])[0]

    def warp_groups_burst(self, calls):
        outs = [None] * len(calls)
        for i, (x, y, table, ctrl, wv) in enumerate(calls):
            ctrl, wv, table = np.ascontiguousarray(ctrl, np.float64), np.ascontiguousarray(wv, np.float64), np.asarray(table, np.int32)

            def work(row, i=i, x=x, y=y, cs=ctrl.shape, ws=wv.shape, nt=len(table)):
                nc, nw = int(np.prod(cs)) * 8, int(np.prod(ws)) * 8
                outs[i] = self._warp_groups(x, y, list(np.frombuffer(row[nc + nw:nc + nw + nt * 4], np.int32)),
                                            np.frombuffer(row[:nc], np.float64).reshape(cs),
                                            np.frombuffer(row[nc:nc + nw], np.float64).reshape(ws))
            self.warpg_ring.submit(ctrl.tobytes() + wv.tobytes() + table.tobytes(), work)
        self.warpg_ring.sync()
        return outs

    def close(self):
        pass


# ------------------------------------------------------------------------------------------------------------------ the HIP kernels
class GpuDevice:
    """the same calls on a DeviceModel('unet', c, h, w, max_batch, n_filters_first=3, n_downsample=1); profile: count launches.
    The network needs even sizes; the augmentation entry points take their sizes per call, so an odd h or w is rounded up for the
    model alone."""

    def __init__(self, gpu, c, h, w, max_batch, profile=False):
        self.gpu = gpu
        self.m = gpu.DeviceModel('unet', c, h + h % 2, w + w % 2, max_batch, n_filters_first=3, n_downsample=1, rate=2, kernel_size=3,
                                 conv_stride=1, padding='same')
        self.launches = None
        self.profile = profile
        if profile:
            self.m.profile_enable(1)

    def close(self):
        self.m.close()

    def _count(self):
        return {row[0]: row[1] for row in self.m.profile()}

    def augment(self, raw, params, out_size, label, channels):
        m, (ho, wo) = self.m, out_size
        B, cs = raw.shape[0], raw.shape[-1]
        if not hasattr(m, '_aug'):
            m._aug = (self.gpu.RawDeviceBuffer(), self.gpu.RawDeviceBuffer(), self.gpu.RawDeviceBuffer())
        m._aug[1].upload(np.full(B * ho * wo * (cs - 1), SENTINEL, F32))
        m._aug[2].upload(np.full(B * ho * wo, SENTINEL, F32))
        if self.profile:
            m.profile_reset()
        xb, yb = m.augment_u8(raw, params, out_size, label, contrast_channels=channels)
        out = xb.to_host(), yb.to_host()
        self.launches = self._count() if self.profile else None
        return out

    def augment_burst(self, calls):
        from dnncancerannotator_amd import _lib
        m = self.m
        staged = []
        for raw, params, (ho, wo), label, channels in calls:          # everything a call needs is on the device before the first call
            B, hs, ws, cs = raw.shape
            src = self.gpu.RawDeviceBuffer()
            src.upload(raw)
            xo = self.gpu.DeviceBuffer(np.full((B, ho, wo, cs - 1), SENTINEL, F32))
            yo = self.gpu.DeviceBuffer(np.full((B, ho, wo), SENTINEL, F32))
            prm = (_lib.AugParam * B)(*[_lib.AugParam(int(p[0]), int(p[1]), int(p[2]), float(p[3])) for p in params])
            staged.append((src, xo, yo, prm, (B, hs, ws, cs, label, NumpyDevice._mask(cs, label, channels), ho, wo)))
        m.sync()
        for src, xo, yo, prm, (B, hs, ws, cs, label, mask, ho, wo) in staged:        # back to back: no read, no sync
            rc = m.lib.dnnca_augment_u8(m.handle, src.ptr, B, hs, ws, cs, label, mask, prm, ho, wo, xo.ptr, yo.ptr)
            assert rc == _lib.OK, m.lib.dnnca_last_error().decode()
            C.memset(prm, 0xff, C.sizeof(prm))      # the caller's buffer is free when the call returns
        m.sync()
        return [(xo.to_host(), yo.to_host()) for _, xo, yo, _, _ in staged]

    def warp(self, x, y, ctrl, wv):
        m = self.m
        if not hasattr(m, '_warp'):
            m._warp = (self.gpu.RawDeviceBuffer(), self.gpu.RawDeviceBuffer())
        m._warp[0].upload(np.full(x.shape, SENTINEL, F32))
        m._warp[1].upload(np.full(y.shape, SENTINEL, F32))
        xw, yw = m.warp(self.gpu.DeviceBuffer(x), self.gpu.DeviceBuffer(y), ctrl, wv)
        return xw.to_host(), yw.to_host()

    def warp_groups(self, x, y, group_of, ctrl, wv):
        m = self.m
        if not hasattr(m, '_warp_groups'):
            m._warp_groups = (self.gpu.RawDeviceBuffer(), self.gpu.RawDeviceBuffer())
        m._warp_groups[0].upload(np.full(x.shape, SENTINEL, F32))
        m._warp_groups[1].upload(np.full(y.shape, SENTINEL, F32))
        xd, yd = self.gpu.DeviceBuffer(x), self.gpu.DeviceBuffer(y)
        xw, yw = m.warp_groups(xd, yd, group_of, ctrl, wv)
        m.sync()
        return xw.to_host(), yw.to_host()

    def warp_groups_burst(self, calls):
        from dnncancerannotator_amd import _lib
        m = self.m
        dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731
        staged = []
        for x, y, table, ctrl, wv in calls:
            ctrl, wv = np.array(ctrl, np.float64), np.array(wv, np.float64)
            staged.append((self.gpu.DeviceBuffer(x), self.gpu.DeviceBuffer(y), self.gpu.DeviceBuffer(np.full(x.shape, SENTINEL, F32)),
                           self.gpu.DeviceBuffer(np.full(y.shape, SENTINEL, F32)), np.array(table, np.int32), ctrl, wv))
        m.sync()
        for xd, yd, xo, yo, table, ctrl, wv in staged:
            B, H, W, Cc = xd.shape
            rc = m.lib.dnnca_warp_groups_f32(m.handle, xd.ptr, yd.ptr, B, H, W, Cc, ctrl.shape[1], table.ctypes.data_as(C.POINTER(C.c_int)),
                                             ctrl.shape[2], dptr(ctrl), dptr(wv), xo.ptr, yo.ptr)
            assert rc == _lib.OK, m.lib.dnnca_last_error().decode()
            ctrl.fill(np.nan), wv.fill(np.nan), table.fill(0)           # the caller's buffers are free when the call returns
        m.sync()
        return [(xo.to_host(), yo.to_host()) for _, _, xo, yo, _, _, _ in staged]
