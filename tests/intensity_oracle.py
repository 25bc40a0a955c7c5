"""random_intensity stated in numpy, for tests/test_intensity_host.py and tests/test_intensity_gpu.py: what dnnca_intensity_f32
(include/dnnca.h) does to a float32 batch x [B, H, W, C] under records rec uint32 [B, C, 32], per plane and in this order
    1. gamma   v <= 0 ? 0 : v ** g
    2. bias    v * exp(f),  f = sum a_ij P_i(u) P_j(t), P Legendre, u = 2 row / (H - 1) - 1, t = 2 col / (W - 1) - 1 (0 on a size of 1)
    3. blur    along the rows, then along the columns, taps w[0..R], edge pixels replicated
    4. noise   Philox4x32-10 on the counter (row * W + col, 0, 0, 0) -> Box-Muller -> Gaussian or Rician
    5. clamp   to [0, 1]
and a plane whose flags are 0 comes out as it went in.  `intensity(x, rec)` is the float64 statement on the float32 inputs and the
records' float32 values.  `intensity(x, rec, np.float32)` is the float32 RESTATEMENT: the same steps with every operation rounded to
float32 (the elementary functions evaluated in float64 and rounded once, i.e. a correctly rounded float32 libm), in the order the
kernel documents.  Its distance from the float64 statement is the yardstick of the device's tolerance: the device may be 4 x as far,
rounded up to a power of two (BOUND), because its powf, expf, logf, sinpif / cospif and its fused blur sums may each differ from
numpy's by a few ulp.  Errors are counted in units of 2^-24 (max(1, max|x| of the plane) + 6 sigma_noise)."""

import numpy as np

GAMMA, BIAS, BLUR, NOISE, RICIAN = 1, 2, 4, 8, 16
WORDS, RMAX = 32, 8
BIAS_TERMS = ((1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3))

# worst distance of the float32 restatement from the float64 statement over cases() and the 8 x 512 x 512 x 3 overlay case, in units:
# 2.89 on the small cases (3 x 33 x 47 x 3, all four terms with Rician noise), 3.11 on the overlay case
# (test_intensity_host.test_restatement_sets_the_device_bound measures both again on every run)
CPU_WORST = 3.12
BOUND = 16.0               # 4 x CPU_WORST = 12.5, rounded up to a power of two


# ------------------------------------------------------------------------------------------------------------------ Philox
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3, SC'11).  counter uint32 [..., 4],
    key two 32-bit words -> uint32 [..., 4]"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def normals(h, w, key, T=np.float64):
    """(z0, z1) [h, w] of the plane's pixels: u1 = ((r0 >> 9) + 1) 2^-23 in (0, 1], u2 = (r1 >> 8) 2^-24, Box-Muller"""
    counter = np.zeros((h * w, 4), np.uint32)
    counter[:, 0] = np.arange(h * w, dtype=np.uint64).astype(np.uint32)
    r = philox4x32_10(counter, key)
    u1 = ((r[:, 0] >> 9).astype(np.float64) + 1.0) * 2.0 ** -23
    a2 = (r[:, 1] >> 8).astype(np.float64) * 2.0 ** -23              # 2 u2, exact in float32 too
    rad = np.sqrt((T(-2.0) * np.log(u1).astype(T)).astype(np.float64)).astype(T)
    z0 = rad * np.cos(np.pi * a2).astype(T)
    z1 = rad * np.sin(np.pi * a2).astype(T)
    return z0.reshape(h, w), z1.reshape(h, w)


# ----------------------------------------------------------------------------------------------------------------- records
def taps(sigma):
    """(R, float32 [9]): R = ceil(3 sigma), w_k ~ exp(-k^2 / 2 sigma^2) normalised in float64 to w_0 + 2 sum w_k = 1"""
    radius = int(np.ceil(3.0 * sigma))
    assert 1 <= radius <= RMAX
    e = np.exp(-np.arange(radius + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    out = np.zeros(RMAX + 1, np.float32)
    out[:radius + 1] = e / (e[0] + 2.0 * e[1:].sum())
    return radius, out


def record(gamma=None, bias=None, blur=None, noise=None, rician=False, key=(0, 0)):
    """one record: gamma g, bias a[9], blur sigma, noise sigma (each None: the term is off)"""
    r = np.zeros(WORDS, np.uint32)
    f = r.view(np.float32)
    if gamma is not None:
        r[0] |= GAMMA
        f[1] = gamma
    if bias is not None:
        r[0] |= BIAS
        f[2:11] = bias
    if blur is not None:
        r[0] |= BLUR
        r[11], f[12:21] = taps(blur)
    if noise is not None:
        r[0] |= NOISE | (RICIAN if rician else 0)
        f[21] = noise
        r[22], r[23] = key
    return r


def random_records(rng, B, C, which, strength=0.3):
    """[B, C, 32]: a different record per image and channel with the terms named in `which` (of 'gamma', 'bias', 'blur', 'noise',
    'rician') active, values from the shipped overlay's ranges"""
    out = np.zeros((B, C, WORDS), np.uint32)
    for b in range(B):
        for c in range(C):
            kw = {}
            if 'gamma' in which:
                kw['gamma'] = np.exp(rng.uniform(np.log(0.7), np.log(1.5)))
            if 'bias' in which:
                a = rng.uniform(-1, 1, 9)
                kw['bias'] = a * (strength * 0.999 / np.abs(a).sum())
            if 'blur' in which:
                kw['blur'] = rng.uniform(0.5, 1.5)
            if 'noise' in which or 'rician' in which:
                kw.update(noise=rng.uniform(0.01, 0.05), rician='rician' in which, key=tuple(int(k) for k in rng.integers(0, 1 << 32, 2)))
            out[b, c] = record(**kw)
    return out


# --------------------------------------------------------------------------------------------------------------- the steps
def _coord(n, T):
    if n == 1:
        return np.zeros(1, T)
    i = np.arange(n)
    if T is np.float64:
        return 2.0 * i / (n - 1) - 1.0
    d = np.float32(n - 1)
    return (i.astype(np.float32) * np.float32(2) - d) / d


def _legendre(u, T):
    return [np.ones_like(u), u, T(1.5) * u * u - T(0.5), (T(2.5) * u * u - T(1.5)) * u]


def _blur_axis(p, w, radius, axis, T):
    pad = [(0, 0), (0, 0)]
    pad[axis] = (radius, radius)
    q = np.pad(p, pad, mode='edge')
    n = p.shape[axis]
    take = lambda o: np.take(q, range(radius + o, radius + o + n), axis)      # noqa: E731
    acc = T(w[0]) * take(0)
    for k in range(1, radius + 1):
        acc = acc + T(w[k]) * (take(-k) + take(k))
    return acc


def plane(v, r, T=np.float64):
    """one plane v float32 [H, W] under the record r, computed in T"""
    flags = int(r[0])
    if flags == 0:
        return v.astype(T)
    f = r.view(np.float32)
    h, w = v.shape
    v = v.astype(T)
    if flags & GAMMA:
        pos = v > 0
        v = np.where(pos, np.power(np.where(pos, v, 1).astype(np.float64), np.float64(f[1])).astype(T), T(0))
    if flags & BIAS:
        pu, pt = _legendre(_coord(h, T), T), _legendre(_coord(w, T), T)
        field = None
        for a, (i, j) in zip(f[2:11], BIAS_TERMS):
            term = T(a) * (pu[i][:, None] * pt[j][None, :])
            field = term if field is None else field + term
        v = v * np.exp(field.astype(np.float64)).astype(T)
    if flags & BLUR:
        v = _blur_axis(_blur_axis(v, f[12:21], int(r[11]), 1, T), f[12:21], int(r[11]), 0, T)
    if flags & NOISE:
        z0, z1 = normals(h, w, (r[22], r[23]), T)
        s = T(f[21])
        v = v + s * z0
        if flags & RICIAN:
            q = s * z1
            v = np.sqrt((v * v + q * q).astype(np.float64)).astype(T)
    return np.minimum(np.maximum(v, T(0)), T(1))


def intensity(x, rec, T=np.float64):
    """x float32 [B, H, W, C], rec uint32 [B, C, 32] -> [B, H, W, C] in T (float64: the statement, float32: the restatement)"""
    x, rec = np.asarray(x, np.float32), np.asarray(rec, np.uint32)
    out = np.empty(x.shape, T)
    for b in range(x.shape[0]):
        for c in range(x.shape[3]):
            out[b, :, :, c] = plane(x[b, :, :, c], rec[b, c], T)
    return out


def units(x, rec):
    """[B, 1, 1, C]: the error unit of every plane, 2^-24 (max(1, max|x|) + 6 sigma)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    sigma = np.where(rec[..., 0] & NOISE, rec[..., 21].view(np.float32).astype(np.float64), 0.0)
    return (2.0 ** -24 * (np.maximum(1.0, np.abs(x).max(axis=(1, 2))) + 6.0 * sigma))[:, None, None, :]


def worst_units(got, want, x, rec):
    """the largest |got - want| of the batch in the units of its plane"""
    return float((np.abs(np.asarray(got, np.float64) - want) / units(x, rec)).max())


# -------------------------------------------------------------------------------------------------------- noise statistics
NOISE_HW, NOISE_SIGMA = 256, 0.05
NOISE_KEYS = ((0x243F6A88, 0x85A308D3), (0x13198A2E, 0x03707344))      # one per channel of the 256 x 256 x 2 plane
RICIAN_KEY = (0xA4093822, 0x299F31D0)


def noise_case():
    """(x, rec): one 256 x 256 x 2 plane of 0.5 under Gaussian noise of sigma 0.05 with NOISE_KEYS (0.5 +- 0.05 * 5.7 is never clamped)"""
    x = np.full((1, NOISE_HW, NOISE_HW, 2), 0.5, np.float32)
    return x, np.stack([record(noise=NOISE_SIGMA, key=k) for k in NOISE_KEYS])[None]


def rician_case():
    """(x, rec): one 256 x 256 x 1 plane of zeros under Rician noise: the output is Rayleigh with scale sigma"""
    return np.zeros((1, NOISE_HW, NOISE_HW, 1), np.float32), record(noise=NOISE_SIGMA, rician=True, key=RICIAN_KEY)[None, None]


def check_noise_statistics(x, out):
    """5-sigma bounds on z = (out - in) / sigma, N = 65536 per channel: mean, variance, lag-1 autocorrelation along rows and
    along columns, correlation between the two channels"""
    z = (np.asarray(out, np.float64) - x.astype(np.float64))[0] / np.float64(np.float32(NOISE_SIGMA))
    n = NOISE_HW * NOISE_HW
    stats = {}
    for c in range(2):
        zc = z[..., c]
        stats['mean %d' % c] = (abs(zc.mean()), 5 / np.sqrt(n))
        stats['var %d' % c] = (abs(zc.var() - 1), 5 * np.sqrt(2 / n))
        d = zc - zc.mean()
        stats['lag-1 rows %d' % c] = (abs((d[:, 1:] * d[:, :-1]).mean() / zc.var()), 5 / np.sqrt(n))
        stats['lag-1 columns %d' % c] = (abs((d[1:] * d[:-1]).mean() / zc.var()), 5 / np.sqrt(n))
    stats['channels'] = (abs(np.corrcoef(z[..., 0].ravel(), z[..., 1].ravel())[0, 1]), 5 / np.sqrt(n))
    for name, (value, bound) in stats.items():
        print('%-18s %.5f  (bound %.5f)' % (name, value, bound))
        assert value < bound, (name, value, bound)
    return stats


def check_rician_mean(out):
    """the mean of Rayleigh(sigma) noise is sigma sqrt(pi / 2), its variance (2 - pi / 2) sigma^2"""
    s = np.float64(np.float32(NOISE_SIGMA))
    m, se = np.asarray(out, np.float64).mean(), s * np.sqrt((2 - np.pi / 2) / (NOISE_HW * NOISE_HW))
    print('rician mean %.6f, expected %.6f +- 5 x %.6f' % (m, s * np.sqrt(np.pi / 2), se))
    assert abs(m - s * np.sqrt(np.pi / 2)) < 5 * se


# ------------------------------------------------------------------------------------------------------------------- cases
TERMS =(('gamma',), ('bias',), ('blur',), ('noise',), ('rician',), ('gamma', 'bias', 'blur', 'noise'), ('gamma', 'bias', 'blur', 'rician'))
# (B, H, W, C): 3 x 33 x 47 at C = 1, 3, 5 (partial 32 x 8 tiles on both edges, several blocks); one more than the tile each way;
# a row, a column, a point; 5 x 5, smaller than the halo of R = 8
SHAPES = ((3, 33, 47, 1), (3, 33, 47, 3), (3, 33, 47, 5), (2, 9, 33, 3), (2, 1, 9, 3), (2, 9, 1, 3), (2, 1, 1, 3), (2, 5, 5, 3))


def case(shape, which, seed=0):
    """(x, rec) of one case: x in [0, 1) with channel 0 in [-0.3, 1.4] as random_contrast can leave it; the 5 x 5 plane blurs at R = 8"""
    B, h, w, C = shape
    rng = np.random.default_rng([seed, B, h, w, C, len(which), sum(map(len, which))])
    x = rng.random(shape).astype(np.float32)
    x[..., 0] = x[..., 0] * np.float32(1.7) - np.float32(0.3)
    rec = random_records(rng, B, C, which)
    if (h, w) == (5, 5) and 'blur' in which:
        for b in range(B):
            for c in range(C):
                rec[b, c, 11], rec[b, c, 12:21] = RMAX, taps(2.6 - 0.05 * c)[1].view(np.uint32)
    return x, rec


def overlay_options():
    """configs/additionals/intensity_augment.yaml as parse_augment_options gives it"""
    import os
    from dnncancerannotator_amd import augment, load
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    over = load._apply_config({'data_options': {'train': {'augment_options': {'random_crop': None}}}},
                              load._load_config_single(os.path.join(root, 'configs', 'additionals', 'intensity_augment.yaml')))
    return augment.parse_augment_options(over['data_options']['train']['augment_options'], (512, 512)).intensity


def overlay_case(B=8, h=512, w=512, C=3, seed=8):
    """the workload shape with records drawn from the shipped overlay"""
    from dnncancerannotator_amd import augment
    rec = augment.draw_intensity(np.random.default_rng(seed), B, overlay_options(), C)
    x = np.random.default_rng(seed + 1).random((B, h, w, C)).astype(np.float32)
    x[..., 0] = x[..., 0] * np.float32(1.7) - np.float32(0.3)
    return x, rec


def cases():
    for shape in SHAPES:
        for which in TERMS:
            yield shape, which
