"""Host side of the train-time augmentation (annotator/data.py:62-111 `train_ds`, :538-575 option parsing): the random draws.

The reference applies, per image and in the order of `data_options.train.augment_options` (configs/additionals/data_options.yaml:9-13):
    random_crop      crop to `output_size` at the centre offset + clip(int(N(0, stddev)), min_, max_)     (data.py:677-689)
    random_flip      tf.image.random_flip_left_right: flip when U[0,1) < 0.5                              (data.py:620-625)
    random_contrast  tf.image.random_contrast(lower, upper) on the feature channels                       (data.py:586-609)
    random_warp      tfa.image.sparse_image_warp                                                          (data.py:725-763)
and, from the overlays configs/additionals/intra_channelwarp_std{3,5,10,20}.yaml,
    random_intrachannelwarp   a random_warp of its own for every channel group of the slice, label included (data.py:656-715)
and, this project's own (configs/additionals/affine_augment.yaml, d4_augment.yaml; the reference has no rotation, zoom or D4 view),
    random_affine    rotation, zoom, shift and a flip / transpose of the plane about its centre, bilinear, zero outside
    random_intensity gamma, smooth bias field, Gaussian blur and Gaussian / Rician noise, drawn per image AND feature channel
                     (configs/additionals/intensity_augment.yaml)
All seven run on the device (`dnnca_augment_u8`, `dnnca_affine_f32`, `dnnca_warp_f32`, `dnnca_warp_groups_f32`,
`dnnca_intensity_f32`) in the fixed order crop, flip, contrast, affine, warp, intra-channel warp, intensity (noise added before a
resampling would be smoothed away by it); this module draws their per-image
parameters with a numpy generator (TensorFlow's own random streams cannot be reproduced without TensorFlow, so the draws are not
bit-compatible with a TF run -- their distributions are the reference's) and solves the small spline systems of the warps.
"""

import logging
from collections import namedtuple

import numpy as np

AugmentPlan = namedtuple('AugmentPlan', ['crop', 'flip', 'contrast', 'warp', 'output_size', 'intrawarp', 'intensity', 'affine'],
                         defaults=(None, None, None))
# warp: (ctrl, wv) or None; intrawarp: (ctrl [B, G, n, 2], wv [B, G, n + 3, 2], group_of [Cs]: group of every raw-slice channel) or None
# contrast_channels: the raw-slice channels random_contrast adjusts (target_channels), None: every feature channel
# affine: float64 [B, 2, 3] from draw_affine (output pixel -> source position, rows (row, column)) or None
# intensity: uint32 [B, C, 32] from draw_intensity (one record per image and feature channel) or None
# (`affine` stays the last field of both tuples; build them with intensity= and affine= by keyword)
RawBatch = namedtuple('RawBatch', ['raw', 'params', 'output_size', 'label_index', 'warp', 'intrawarp', 'contrast_channels', 'intensity',
                                   'affine'], defaults=(None, None, None, None))


def contrast_channels(plan, n_channels, label_index):
    """random_contrast's `target_channels` (data.py:586-609 gathers exactly the named channels of the raw slice, adjusts them and
    puts them back) as the tuple dnnca_augment_u8 takes, checked against the slice: an index outside the `n_channels` raw channels,
    or the label's, is a ValueError (the reference would fail in tf.gather, or adjust the label).  None -- no random_contrast, or no
    `target_channels` -- keeps this project's default: EVERY feature channel, wherever the label stands.  The reference's own
    default is range(len(slice_types) - 1) (data.py:91), which is the same set only when the label is the last slice type; with
    the label elsewhere it would adjust the label and skip the last feature channel.  The project keeps "every feature channel"."""
    if plan is None or plan.contrast is None or plan.contrast.get('target_channels') is None:
        return None
    out = tuple(int(c) for c in plan.contrast['target_channels'])
    for c in out:
        if not 0 <= c < n_channels:
            raise ValueError('random_contrast: target channel %d is outside the %d channels of the raw slice' % (c, n_channels))
        if c == label_index:
            raise ValueError('random_contrast: target channel %d is the label channel' % c)
    return out



def plain_params(n):
    """the draws of a batch that is only converted (evaluation: centre crop, no flip, no contrast)"""
    return [(0, 0, 0, 1.0)] * n


def raw_to_float(batch):
    """Host statement of what the device does with an un-augmented RawBatch (params None): centre crop to output_size, / 255,
    label channel -> y, the other channels -> x (annotator/data.py:195-206,766-788).  For consumers without the device path."""
    if batch.params is not None:
        raise ValueError('raw_to_float converts evaluation batches only (no random draws)')
    raw = np.asarray(batch.raw)
    oh, ow = batch.output_size
    gy, gx = (raw.shape[1] - oh) // 2, (raw.shape[2] - ow) // 2
    c = raw[:, gy:gy + oh, gx:gx + ow, :]
    feat = [i for i in range(raw.shape[-1]) if i != batch.label_index]
    x = np.empty(c.shape[:-1] + (len(feat),), np.float32)
    for j, i in enumerate(feat):
        x[..., j] = c[..., i]
    np.divide(x, np.float32(255.0), out=x)
    y = c[..., batch.label_index].astype(np.float32)
    np.divide(y, np.float32(255.0), out=y)
    return x, y


_KNOWN = ('random_crop', 'random_flip', 'random_contrast', 'random_warp', 'random_intrachannelwarp', 'random_affine', 'random_intensity')
AFFINE_SYMMETRIES = ('none', 'flips', 'd4')      # the names of the TTA modes (tta.MODES): what `--tta` averages over, train-time
INTRAWARP_POINTS = 100          # data.py:706 passes n_points=100 to every group's random_warp, whatever the option says
_warned = set()


def parse_augment_options(options, output_size):
    """data.py:538-551 + the defaults of train_ds (data.py:87-93).  options None -> {'random_crop': {}} like train_ds."""
    if options is None:
        options = {'random_crop': {}}
    crop, flip, contrast, warp, intrawarp, affine, intensity = None, False, None, None, None, None, None
    for name, conf in options.items():
        conf = dict(conf or {})
        if name not in _KNOWN:
            raise KeyError('unknown augment option %r (the reference looks up augment_%s, data.py:543)' % (name, name))
        if name == 'random_crop':
            crop = dict(stddev=4, max_=6, min_=-6)
            crop.update({k: v for k, v in conf.items() if k != 'output_size'})
            if 'output_size' in conf:
                output_size = tuple(conf['output_size'])
        elif name == 'random_flip':
            flip = True
        elif name == 'random_contrast':
            contrast = dict(lower=0.8, upper=1.2)
            contrast.update({k: v for k, v in conf.items() if k != 'target_channels'})
            contrast['target_channels'] = conf.get('target_channels')          # None: every feature channel (data.py:91)
        elif name == 'random_warp':
            warp = dict(n_points=100, max_diff=5, stddev=2.0)                  # data.py:725 random_warp defaults
            warp.update({k: v for k, v in conf.items() if k != 'process_in_batch'})
        elif name == 'random_intrachannelwarp':
            # data.py:656 `paired=((0, -1),)`, data.py:692 random_intrachannelwarp defaults; the option's n_points never reaches
            # random_warp (data.py:706), so the shipped `n_points: 50` has no effect in the reference
            intrawarp = dict(n_points=INTRAWARP_POINTS, max_diff=5, stddev=2.0, paired=((0, -1),))
            intrawarp.update({k: v for k, v in conf.items() if k in ('max_diff', 'stddev')})
            if 'paired' in conf:
                intrawarp['paired'] = tuple(tuple(int(i) for i in pair) for pair in conf['paired'])
            unknown = set(conf) - {'n_points', 'max_diff', 'stddev', 'paired'}
            if unknown:
                raise TypeError('random_intrachannelwarp got unexpected options %s (data.py:692)' % sorted(unknown))
            if conf.get('n_points', INTRAWARP_POINTS) != INTRAWARP_POINTS and 'intrawarp_n_points' not in _warned:
                _warned.add('intrawarp_n_points')
                logging.warning('random_intrachannelwarp: n_points %r is ignored, every group is warped with %d control points '
                                '(annotator/data.py:706)', conf['n_points'], INTRAWARP_POINTS)
        elif name == 'random_affine':
            affine = _parse_affine(conf)
        elif name == 'random_intensity':
            intensity = _parse_intensity(conf)
    return AugmentPlan(crop, flip, contrast, warp, tuple(output_size), intrawarp, intensity=intensity, affine=affine)


def _parse_affine(conf):
    """random_affine's keys with their defaults (all of them the identity), checked: a bad value is a ValueError here"""
    unknown = set(conf) - {'rotate_deg', 'scale', 'shift', 'symmetry'}
    if unknown:
        raise TypeError('random_affine got unexpected options %s' % sorted(unknown))

    def number(key, value):
        if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not np.isfinite(value):
            raise ValueError('random_affine: %s = %r is not a finite number' % (key, value))
        return float(value)
    rotate = number('rotate_deg', conf.get('rotate_deg', 0))
    if not 0.0 <= rotate <= 180.0:
        raise ValueError('random_affine: rotate_deg = %r is outside [0, 180]' % (conf['rotate_deg'],))
    scale = conf.get('scale', (1, 1))
    if isinstance(scale, (str, bytes)) or not hasattr(scale, '__len__') or len(scale) != 2:
        raise ValueError('random_affine: scale = %r is not a pair [lo, hi]' % (scale,))
    lo, hi = number('scale[0]', scale[0]), number('scale[1]', scale[1])
    if not 0.0 < lo <= hi:
        raise ValueError('random_affine: scale = %r does not satisfy 0 < lo <= hi' % (scale,))
    shift = number('shift', conf.get('shift', 0))
    if shift < 0.0:
        raise ValueError('random_affine: shift = %r is negative' % (conf['shift'],))
    symmetry = conf.get('symmetry', 'none')
    if symmetry not in AFFINE_SYMMETRIES:
        raise ValueError('random_affine: symmetry = %r is none of %s' % (symmetry, ', '.join(AFFINE_SYMMETRIES)))
    return dict(rotate_deg=rotate, scale=(lo, hi), shift=shift, symmetry=symmetry)


INTENSITY_WORDS = 32            # uint32 words of one record of draw_intensity (include/dnnca.h: dnnca_intensity_f32)
INTENSITY_GAMMA, INTENSITY_BIAS, INTENSITY_BLUR, INTENSITY_NOISE, INTENSITY_RICIAN = 1, 2, 4, 8, 16      # word 0
INTENSITY_MAX_RADIUS = 8        # the halo the kernel stages: blur sigma <= 8 / 3
INTENSITY_DISTRIBUTIONS = ('rician', 'gaussian')
# the nine (i, j) of the bias polynomial sum a_ij P_i(u) P_j(v), 1 <= i + j <= 3, in the order of the record's words 2..10
INTENSITY_BIAS_TERMS = ((1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3))


def _parse_intensity(conf):
    """random_intensity's terms, checked: {'gamma': {range, prob}, 'bias_field': {strength, prob}, 'blur': {sigma, prob}, 'noise':
    {sigma, prob, distribution}, 'target_channels'}.  A term that is absent, has prob 0 or can only draw the identity (gamma range
    [1, 1], strength 0, no blur sigma, noise sigma [0, 0]) is None: it is off and takes no draw.  `prob` defaults to 1, a range may
    be given as one number, `distribution` defaults to rician (magnitude MRI).  A bad value is a ValueError here."""
    unknown = set(conf) - {'gamma', 'bias_field', 'blur', 'noise', 'target_channels'}
    if unknown:
        raise TypeError('random_intensity got unexpected options %s' % sorted(unknown))

    def number(key, value):
        if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not np.isfinite(value):
            raise ValueError('random_intensity: %s = %r is not a finite number' % (key, value))
        return float(value)

    def pair(key, value):
        if isinstance(value, (list, tuple)) and len(value) == 2:
            lo, hi = number(key + '[0]', value[0]), number(key + '[1]', value[1])
        elif isinstance(value, (list, tuple, str, bytes, dict)) or value is None:
            raise ValueError('random_intensity: %s = %r is neither a number nor a pair [lo, hi]' % (key, value))
        else:
            lo = hi = number(key, value)
        if lo > hi:
            raise ValueError('random_intensity: %s = %r has lo > hi' % (key, value))
        return lo, hi

    def term(name, keys):
        sub = conf.get(name)
        if sub is None:
            return None, 0.0
        if not isinstance(sub, dict):
            raise ValueError('random_intensity: %s = %r is not a mapping' % (name, sub))
        unknown = set(sub) - set(keys) - {'prob'}
        if unknown:
            raise TypeError('random_intensity.%s got unexpected options %s' % (name, sorted(unknown)))
        prob = number(name + '.prob', sub.get('prob', 1.0))
        if not 0.0 <= prob <= 1.0:
            raise ValueError('random_intensity: %s.prob = %r is outside [0, 1]' % (name, sub['prob']))
        return sub, prob

    out = dict(gamma=None, bias_field=None, blur=None, noise=None, target_channels=None)
    sub, prob = term('gamma', ('range',))
    if sub is not None:
        lo, hi = pair('gamma.range', sub.get('range', (1.0, 1.0)))
        if lo <= 0.0:
            raise ValueError('random_intensity: gamma.range = %r does not satisfy 0 < lo' % (sub['range'],))
        if prob > 0.0 and (lo, hi) != (1.0, 1.0):
            out['gamma'] = dict(range=(lo, hi), prob=prob)
    sub, prob = term('bias_field', ('strength',))
    if sub is not None:
        strength = number('bias_field.strength', sub.get('strength', 0.0))
        if strength < 0.0:
            raise ValueError('random_intensity: bias_field.strength = %r is negative' % (sub['strength'],))
        if prob > 0.0 and strength > 0.0:
            out['bias_field'] = dict(strength=strength, prob=prob)
    sub, prob = term('blur', ('sigma',))
    if sub is not None and 'sigma' in sub:
        lo, hi = pair('blur.sigma', sub['sigma'])
        if lo <= 0.0 or hi > INTENSITY_MAX_RADIUS / 3.0:
            raise ValueError('random_intensity: blur.sigma = %r is outside (0, 8/3] (the radius ceil(3 sigma) is at most %d)'
                             % (sub['sigma'], INTENSITY_MAX_RADIUS))
        if prob > 0.0:
            out['blur'] = dict(sigma=(lo, hi), prob=prob)
    sub, prob = term('noise', ('sigma', 'distribution'))
    if sub is not None:
        lo, hi = pair('noise.sigma', sub.get('sigma', (0.0, 0.0)))
        if lo < 0.0:
            raise ValueError('random_intensity: noise.sigma = %r is negative' % (sub['sigma'],))
        distribution = sub.get('distribution', INTENSITY_DISTRIBUTIONS[0])
        if not isinstance(distribution, str) or distribution not in INTENSITY_DISTRIBUTIONS:
            raise ValueError('random_intensity: noise.distribution = %r is none of %s' % (distribution, ', '.join(INTENSITY_DISTRIBUTIONS)))
        if prob > 0.0 and hi > 0.0:
            out['noise'] = dict(sigma=(lo, hi), prob=prob, distribution=distribution)
    if conf.get('target_channels') is not None:
        out['target_channels'] = tuple(conf['target_channels'])
    return out


def intensity_is_on(plan):
    """whether random_intensity can change anything: the key is there and at least one of its terms is on"""
    return plan is not None and plan.intensity is not None and any(plan.intensity[k] is not None for k in ('gamma', 'bias_field', 'blur', 'noise'))


def intensity_channels(plan, n_channels, label_index):
    """random_intensity's `target_channels`, raw-slice channels checked as contrast_channels() checks random_contrast's (an index
    outside the `n_channels` raw channels, or the label's, is a ValueError), returned as the FEATURE channels draw_intensity takes
    (the raw index less one behind the label).  None -- no random_intensity, or no `target_channels` -- is every feature channel."""
    if plan is None or plan.intensity is None or plan.intensity.get('target_channels') is None:
        return None
    out = []
    for c in plan.intensity['target_channels']:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
            raise ValueError('random_intensity: target channel %r is not an integer' % (c,))
        c = int(c)
        if not 0 <= c < n_channels:
            raise ValueError('random_intensity: target channel %d is outside the %d channels of the raw slice' % (c, n_channels))
        if c == label_index:
            raise ValueError('random_intensity: target channel %d is the label channel' % c)
        out.append(c - (1 if label_index is not None and c > label_index else 0))
    return tuple(out)


def blur_taps(sigma):
    """(R, float32 [9]): the radius ceil(3 sigma) and the taps w_k ~ exp(-k^2 / 2 sigma^2), k = 0..R, normalised in float64 so that
    w_0 + 2 sum w_k = 1 and then rounded to float32; 0 beyond R"""
    radius = min(int(np.ceil(3.0 * sigma)), INTENSITY_MAX_RADIUS)
    e = np.exp(-np.arange(radius + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    taps = np.zeros(INTENSITY_MAX_RADIUS + 1, np.float32)
    taps[:radius + 1] = e / (e[0] + 2.0 * e[1:].sum())
    return radius, taps


def draw_intensity(rng, n, options, n_feature_channels, targets=None):
    """random_intensity's draws for `n` images of `n_feature_channels` channels: uint32 [n, C, 32], one 128-byte record per image
    and feature channel in the layout of include/dnnca.h (floats as their float32 bit patterns):
        0 flags (1 gamma, 2 bias, 4 blur, 8 noise, 16 Rician) | 1 gamma | 2..10 bias a[9] | 11 blur radius R | 12..20 taps w[0..8]
        | 21 noise sigma | 22, 23 Philox key | 24..31 zero
    targets: the feature channels the option acts on (intensity_channels), None: all; any other channel gets an all-zero record and
    takes no draw.  The order of the draws is part of the contract: images, then channels; within a channel gamma, bias, blur,
    noise; within a term one uniform < prob decides whether it is active (only when 0 < prob < 1) and an active term then draws its
    values (only where the range is not a point):
        gamma  g = exp(U[ln lo, ln hi])
        bias   a ~ U[-1, 1]^9, then t ~ U[0, strength]; a <- a t / sum|a|, so |f| <= sum|a| <= strength on the plane
        blur   sigma ~ U[lo, hi] -> blur_taps
        noise  sigma ~ U[lo, hi], then the key: two 32-bit words
    A term that is off in `options` takes no draw at all, and a record with nothing active is all zero."""
    rec = np.zeros((n, n_feature_channels, INTENSITY_WORDS), np.uint32)
    fl = rec.view(np.float32)
    gamma, bias, blur, noise = (options[k] for k in ('gamma', 'bias_field', 'blur', 'noise'))
    channels = range(n_feature_channels) if targets is None else sorted(set(int(c) for c in targets))

    def active(term):
        return term is not None and (term['prob'] >= 1.0 or bool(rng.random() < term['prob']))

    def ranged(lo, hi, log=False):
        if not lo < hi:
            return float(lo)
        return float(np.exp(rng.uniform(np.log(lo), np.log(hi)))) if log else float(rng.uniform(lo, hi))

    for b in range(n):
        for c in channels:
            flags = 0
            if active(gamma):
                flags |= INTENSITY_GAMMA
                fl[b, c, 1] = ranged(*gamma['range'], log=True)
            if active(bias):
                flags |= INTENSITY_BIAS
                a = rng.uniform(-1.0, 1.0, 9)
                t = float(rng.uniform(0.0, bias['strength']))
                norm = np.abs(a).sum()
                a32 = (a * (t / norm) if norm > 0 else np.zeros(9)).astype(np.float32)
                while np.abs(a32.astype(np.float64)).sum() > bias['strength']:      # float32 rounding must not lift the bound
                    a32 = np.nextafter(a32, np.float32(0))
                fl[b, c, 2:11] = a32
            if active(blur):
                flags |= INTENSITY_BLUR
                radius, taps = blur_taps(ranged(*blur['sigma']))
                rec[b, c, 11] = radius
                fl[b, c, 12:21] = taps
            if active(noise):
                flags |= INTENSITY_NOISE | (INTENSITY_RICIAN if noise['distribution'] == 'rician' else 0)
                fl[b, c, 21] = ranged(*noise['sigma'])
                rec[b, c, 22:24] = rng.integers(0, 1 << 32, 2, dtype=np.uint64)
            rec[b, c, 0] = flags
    return rec


def check_affine_size(plan, output_size):
    """symmetry d4 transposes the plane: it needs a square one (as tta.mask_of asks of `--tta d4`)"""
    if plan is not None and plan.affine is not None and plan.affine['symmetry'] == 'd4' and int(output_size[0]) != int(output_size[1]):
        raise ValueError('random_affine: symmetry d4 transposes the slices and needs a square output_size, not %d x %d; '
                         'the symmetry that works there is flips' % (output_size[0], output_size[1]))


def d4_matrix(k):
    """View k = 4 t + 2 v + h of tta.py as the exact integer 2 x 2 matrix G of its index map: out[q] = in[G (q - c) + c] in
    (row, column).  v mirrors the rows, h the columns, t transposes the mirrored plane (square planes only)."""
    h, v, t = k & 1, (k >> 1) & 1, (k >> 2) & 1
    g = np.array([[-1.0 if v else 1.0, 0.0], [0.0, -1.0 if h else 1.0]])
    return g[:, ::-1].copy() if t else g


def draw_params(rng, n, plan):
    """Per-image draws [(dy, dx, flip, contrast)] for `n` images."""
    out = []
    for _ in range(n):
        dy = dx = 0
        if plan.crop is not None:
            d = rng.normal(0.0, plan.crop['stddev'], 2)
            d = np.clip(np.trunc(d).astype(np.int64), plan.crop['min_'], plan.crop['max_'])      # tf.cast(float -> int32) truncates
            dy, dx = int(d[0]), int(d[1])
        flip = int(plan.flip and rng.random() < 0.5)
        contrast = float(rng.uniform(plan.contrast['lower'], plan.contrast['upper'])) if plan.contrast is not None else 1.0
        out.append((dy, dx, flip, contrast))
    return out


def draw_affine(rng, n, options, output_size):
    """random_affine's draws for `n` images of `output_size`: float64 [n, 2, 3], row r = (L[r, 0], L[r, 1], o[r]) of the map from
    an output pixel q to its source position s = L q + o in (row, column).  Per image, each only when its range is not a point:
    theta ~ U[-R, R] degrees, z = exp(U[ln lo, ln hi]), t ~ U[-S, S]^2 (row, then column), then the symmetry element G (`flips`: view
    0..3 of tta.py, `d4`: view 0..7, uniform).  With c the centre ((H - 1) / 2, (W - 1) / 2): L = G R(-theta) / z, o = c - L (c + t).
    G is an exact integer matrix, so with theta = 0, z = 1, t = 0 every entry is an exact integer or half-integer."""
    rot, (lo, hi), shift, symmetry = options['rotate_deg'], options['scale'], options['shift'], options['symmetry']
    c = np.array([(int(output_size[0]) - 1) / 2.0, (int(output_size[1]) - 1) / 2.0])
    out = np.empty((n, 2, 3), np.float64)
    for b in range(n):
        theta = float(rng.uniform(-rot, rot)) if rot > 0 else 0.0
        z = float(np.exp(rng.uniform(np.log(lo), np.log(hi)))) if lo < hi else float(lo)
        t = rng.uniform(-shift, shift, 2) if shift > 0 else np.zeros(2)
        k = int(rng.integers(4 if symmetry == 'flips' else 8)) if symmetry != 'none' else 0
        if theta == 0.0:
            r = np.eye(2)
        else:
            cs, sn = np.cos(np.deg2rad(theta)), np.sin(np.deg2rad(theta))
            r = np.array([[cs, sn], [-sn, cs]])                # R(-theta)
        lin = d4_matrix(k) @ r
        if z != 1.0:
            lin = lin / z
        out[b, :, :2] = lin
        out[b, :, 2] = c - lin @ (c + t)
    return out


def draw_warp(rng, n, size, n_points=100, max_diff=5, stddev=2.0):
    """Control points of random_warp (data.py:748-752) for `n` square images of edge `size`: source uniform in [0, size)^2,
    destination = source + clip(N(0, stddev), -max_diff, max_diff).  Returns (source, dest) float32 [n, n_points, 2]."""
    raw = rng.uniform(0.0, float(size), (n, n_points, 2)).astype(np.float32)
    diff = np.clip(rng.normal(0.0, stddev, (n, n_points, 2)), -max_diff, max_diff).astype(np.float32)
    return raw, raw + diff


def channel_groups(n_channels, paired=((0, -1),)):
    """The channel groups of random_intrachannelwarp (data.py:693-704) for a raw slice of `n_channels` channels (`slice_types`
    order, label included, before the feature/label split): the `paired` lists in their order with negative indices counted from
    the end, then every channel in no pair on its own, ascending.  An index out of range or named twice is a ValueError (the
    reference would fail in tf.gather, or stack a channel short)."""
    groups, seen = [], set()
    for pair in paired:
        group = []
        for ch in pair:
            i = int(ch) + n_channels if int(ch) < 0 else int(ch)
            if not 0 <= i < n_channels:
                raise ValueError('random_intrachannelwarp: channel %d of paired=%r is out of range for %d channels' % (ch, paired, n_channels))
            if i in seen:
                raise ValueError('random_intrachannelwarp: channel %d is named twice in paired=%r' % (i, paired))
            seen.add(i)
            group.append(i)
        groups.append(group)
    return groups + [[i] for i in range(n_channels) if i not in seen]


def group_table(groups, n_channels):
    """int32 [n_channels]: the group every channel belongs to"""
    table = np.full(n_channels, -1, np.int32)
    for g, group in enumerate(groups):
        table[group] = g
    assert (table >= 0).all()
    return table


def draw_intrawarp(rng, n, size, n_groups, max_diff=5, stddev=2.0):
    """Control points of random_intrachannelwarp for `n` square images of edge `size`: an independent random_warp draw
    (data.py:748-752, always INTRAWARP_POINTS points: data.py:706) for each of the `n_groups` channel groups of every image.
    Returns (source, dest) float32 [n, n_groups, 100, 2]."""
    src, dst = draw_warp(rng, n * n_groups, size, INTRAWARP_POINTS, max_diff, stddev)
    shape = (n, n_groups, INTRAWARP_POINTS, 2)
    return src.reshape(shape), dst.reshape(shape)


def solve_intrawarp(source, dest):
    """solve_warp over the n * G systems of [n, G, k, 2] control points: (ctrl [n, G, k, 2], wv [n, G, k + 3, 2]) float64"""
    n, g, k, _ = np.shape(dest)
    ctrl, wv = solve_warp(np.reshape(source, (n * g, k, 2)), np.reshape(dest, (n * g, k, 2)))
    return ctrl.reshape(n, g, k, 2), wv.reshape(n, g, k + 3, 2)


def _phi2(r):
    """tfa interpolate_spline._phi for order 2 on squared distances: 0.5 r log(max(r, 1e-10))"""
    return 0.5 * r * np.log(np.maximum(r, 1e-10))


def solve_warp(source, dest):
    """The polyharmonic-spline system of tfa.image.sparse_image_warp (order 2, no regularisation, no boundary points):
    train points = dest, train values = dest - source; [[phi(|ci-cj|^2), B], [B^T, 0]] [w; v] = [f; 0] with B = [c, 1].
    Returns (ctrl = dest, wv [n, n_points + 3, 2]) float64 for dnnca_warp_f32."""
    source, dest = np.asarray(source, np.float64), np.asarray(dest, np.float64)
    n, k, _ = dest.shape
    out = np.empty((n, k + 3, 2), np.float64)
    for b in range(n):
        c, f = dest[b], dest[b] - source[b]
        d2 = ((c[:, None, :] - c[None, :, :]) ** 2).sum(-1)
        lhs = np.zeros((k + 3, k + 3))
        lhs[:k, :k] = _phi2(d2)
        lhs[:k, k:k + 2] = c
        lhs[:k, k + 2] = 1.0
        lhs[k:, :k] = lhs[:k, k:].T
        rhs = np.zeros((k + 3, 2))
        rhs[:k] = f
        out[b] = np.linalg.solve(lhs, rhs)
    return dest, out
