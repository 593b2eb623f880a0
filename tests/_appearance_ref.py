"""The rule of n3d_patch_appearance (include/n3d.h, n3d_appear_desc) in numpy, operation by operation: the same Philox4x32-10 in pure
integers, the same tap order in the blur, the same summation order (FOLD) in the statistics.  Patches are (Cv, P, P, P) float32
arrays; every stage takes the mask that was taken on entry and returns a new float32 array.  fp64 throughout, one rounding to
float32 where the rule stores.  Used by the fixture generator, the CPU tests and the GPU tests."""
import numpy as np

MAX_RADIUS = 6
CHUNK = 1024
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """one block in Python integers: counter (c0, c1, c2, c3), key (k0, k1) -> (w0, w1, w2, w3)"""
    c0, c1, c2, c3 = (int(c) & MASK32 for c in counter)
    k0, k1 = (int(k) & MASK32 for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def philox_voxels(n, key):
    """the four words of the counters (v, 0, 0, 0), v = 0 .. n-1, as four uint64 arrays holding 32-bit values (integer arithmetic
    only: a 32 x 32 -> 64 product fits uint64)"""
    c0 = np.arange(n, dtype=np.uint64)
    c1, c2, c3 = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    k0, k1 = np.uint64(int(key[0]) & MASK32), np.uint64(int(key[1]) & MASK32)
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return c0, c1, c2, c3


def normals(n, key):
    """(4, n) float64: the Box-Muller normals z0..z3 of the voxels 0 .. n-1"""
    w = [a.astype(np.float64) for a in philox_voxels(n, key)]
    z = []
    for wa, wb in ((w[0], w[1]), (w[2], w[3])):
        u1, u2 = (wa + 1.0) * 2.0 ** -32, wb * 2.0 ** -32
        rho, th = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
        z += [rho * np.cos(th), rho * np.sin(th)]
    return np.stack(z)


def entry_mask(x):
    """x != 0 on entry (-0.0 is zero)"""
    return np.asarray(x, np.float32) != 0


def noise(x, mask, sigma, key):
    Cv, n = x.shape[0], x[0].size
    z = normals(n, key)[:Cv].reshape(x.shape)
    y = (x.astype(np.float64) + np.float64(sigma) * z).astype(np.float32)
    return np.where(mask, y, x)


def blur_weights(sigma):
    """(r, w[0 .. r]) as the host passes them: scipy's _gaussian_kernel1d, truncate 4"""
    sigma = np.float64(sigma)
    r = int(4.0 * sigma + 0.5)
    if r == 0:
        return 0, np.ones(1)
    k = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    w = w / w.sum()
    return r, w[r:].copy()


def _pass(a, axis, r, w):
    P = a.shape[axis]
    idx = np.arange(-r, P + r)
    idx = np.where(idx < 0, -idx - 1, np.where(idx >= P, 2 * P - 1 - idx, idx))
    pad = np.take(a, idx, axis=axis)
    acc = None
    for k in range(-r, r + 1):
        term = w[abs(k)] * np.take(pad, np.arange(k + r, k + r + P), axis=axis)
        acc = term if acc is None else acc + term
    return acc


def blur(x, mask, radii, weights):
    y = x.copy()
    for c in range(x.shape[0]):
        r, w = int(radii[c]), np.asarray(weights[c], np.float64)
        assert 0 <= r <= MAX_RADIUS and r <= x.shape[1]
        a = x[c].astype(np.float64)
        for axis in range(3):
            a = _pass(a, axis, r, w)
        y[c] = np.where(mask[c], a.astype(np.float32), x[c])
    return y


def fold(a):
    """FOLD of a 1-D float64 array padded with +0.0 to a multiple of 256"""
    a = np.asarray(a, np.float64)
    rows = -(-max(a.size, 1) // 256)
    a = np.concatenate((a, np.zeros(rows * 256 - a.size))).reshape(rows, 256)
    lane = np.zeros(256)
    for i in range(rows):
        lane = lane + a[i]
    s = 128
    while s >= 1:
        lane = lane[:s] + lane[s:2 * s]
        s //= 2
    return lane[0]


def fixed_sum(terms, mask):
    """the rule's sum of the terms of one channel (terms outside the mask count +0.0)"""
    a = np.where(mask, terms, 0.0).reshape(-1)
    n = -(-a.size // CHUNK)
    a = np.concatenate((a, np.zeros(n * CHUNK - a.size)))
    return fold([fold(a[i * CHUNK:(i + 1) * CHUNK]) for i in range(n)])


def _stats(xc, mc):
    n = int(mc.sum())
    lo, hi = np.float64(xc[mc].min()), np.float64(xc[mc].max())
    return n, lo, hi, fixed_sum(xc, mc) / np.float64(n)


def contrast(x, mask, factors):
    y = x.copy()
    for c in range(x.shape[0]):
        if not mask[c].any():
            continue
        xc = x[c].astype(np.float64)
        n, lo, hi, m = _stats(xc, mask[c])
        v = np.minimum(np.maximum((xc - m) * np.float64(factors[c]) + m, lo), hi)
        y[c] = np.where(mask[c], v.astype(np.float32), x[c])
    return y


def gamma(x, mask, gammas):
    y = x.copy()
    with np.errstate(all="ignore"):
        for c in range(x.shape[0]):
            mc = mask[c]
            if not mc.any():
                continue
            xc = x[c].astype(np.float64)
            n, lo, hi, m = _stats(xc, mc)
            d = xc - m
            sd = np.sqrt(fixed_sum(d * d, mc) / np.float64(n))
            rng = hi - lo
            base = np.where(mc, (xc - lo) / (rng + 1e-7), 0.0)
            x1 = (np.power(base, np.float64(gammas[c])) * rng + lo).astype(np.float32).astype(np.float64)
            m1 = fixed_sum(x1, mc) / np.float64(n)
            d1 = x1 - m1
            sd1 = np.sqrt(fixed_sum(d1 * d1, mc) / np.float64(n))
            v = (x1 - m1) / (sd1 + 1e-8) * sd + m
            y[c] = np.where(mc, v.astype(np.float32), x[c])
    return y


def apply_draw(x, draw):
    """all four stages of one patch: draw = None, or a dict with any of "noise": (sigma, (k0, k1)), "blur": sigmas, "contrast":
    factors, "gamma": gammas (what Appearance.draw returns)"""
    x = np.asarray(x, np.float32)
    if not draw:
        return x.copy()
    mask = entry_mask(x)
    if draw.get("noise") is not None:
        x = noise(x, mask, draw["noise"][0], draw["noise"][1])
    if draw.get("blur") is not None:
        rw = [blur_weights(s) for s in draw["blur"]]
        x = blur(x, mask, [r for r, _ in rw], [w for _, w in rw])
    if draw.get("contrast") is not None:
        x = contrast(x, mask, draw["contrast"])
    if draw.get("gamma") is not None:
        x = gamma(x, mask, draw["gamma"])
    return x


def apply_batch(x, draws):
    return np.stack([apply_draw(xb, d) for xb, d in zip(x, draws)])


def make_data(seed, shape):
    """integer values 10 .. 110, non-integers and about 30 % background, float32"""
    rs = np.random.RandomState(seed)
    ints = rs.randint(10, 111, shape).astype(np.float32)
    frac = (rs.uniform(10, 110, shape)).astype(np.float32)
    x = np.where(rs.uniform(size=shape) < 0.5, ints, frac)
    x[rs.uniform(size=shape) < 0.3] = 0
    return np.ascontiguousarray(x, np.float32)


def steps(a, b, scale):
    """|a - b| in float32 steps of the magnitude `scale` (the spacing of float32 at scale)"""
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.float64(np.spacing(np.float32(scale)))
