"""The rule of n3d_patch_artefact (include/n3d.h) in numpy, operation by operation: the integer nearest-exact index, the eight
taps of the composed low-resolution stage in their stated order, the bias field's Philox coefficients, coordinates, powers and term
order, and the dropout.  Patches are (Cv, P, P, P) float32 arrays; every stage takes the mask that was taken on entry and returns a
new float32 array.  fp64 throughout, one rounding to float32 where the rule stores.  Used by the CPU tests and the GPU tests."""
from fractions import Fraction

import numpy as np

from _appearance_ref import entry_mask, philox4x32_10, steps  # noqa: F401  (re-exported for the tests)

MAX_ORDER = 3


def extent(P, scale):
    """batchgeneratorsv2's target extent: Python's round of P * scale, at least 1"""
    return max(1, round(P * float(scale)))


def nearest_index(P, n):
    """N(i), i = 0 .. n-1: the voxel of a P-wide axis that nearest-exact down-sampling to n reads, in integers"""
    i = np.arange(n, dtype=np.int64)
    return np.minimum(((2 * i + 1) * P) // (2 * n), P - 1)


def axis_taps(P, n):
    """(a0, a1, l1) per output index o = 0 .. P-1 of one axis"""
    # the rule's one fused multiply-add, exactly: the rounded quotient times (o + 0.5) minus 0.5 in rationals, rounded once
    scale = Fraction(float(np.float64(n) / np.float64(P)))
    src = np.array([max(float(scale * Fraction(2 * o + 1, 2) - Fraction(1, 2)), 0.0) for o in range(P)], np.float64)
    i0 = np.minimum(src.astype(np.int64), n - 1)
    i1 = i0 + (i0 < n - 1)
    N = nearest_index(P, n)
    return N[i0], N[i1], src - i0.astype(np.float64)


def lowres_channel(xc, n):
    """the eight-tap sum of one channel as float64 (before the rounding to float32)"""
    P = xc.shape[0]
    a0, a1, l1 = axis_taps(P, n)
    a, l = (a0, a1), (1.0 - l1, l1)
    x64 = np.asarray(xc, np.float64)
    acc = np.zeros((P, P, P))
    for ti in (0, 1):
        for tj in (0, 1):
            for tk in (0, 1):
                w = (l[ti][:, None, None] * l[tj][None, :, None]) * l[tk][None, None, :]
                acc = acc + w * x64[np.ix_(a[ti], a[tj], a[tk])]
    return acc


def lowres(x, mask, n):
    y = x.copy()
    P = x.shape[1]
    for c in range(x.shape[0]):
        assert 1 <= n[c] <= P
        if n[c] == P:
            continue
        y[c] = np.where(mask[c], lowres_channel(x[c], int(n[c])).astype(np.float32), x[c])
    return y


def bias_terms(order):
    return [(a, b, c) for a in range(order + 1) for b in range(order + 1 - a) for c in range(order + 1 - a - b)]


def bias_coefs(key, channel, order, rng):
    out = []
    for t in range(len(bias_terms(order))):
        w0 = philox4x32_10((t, 3, channel, 0), key)[0]
        out.append((np.float64(w0) * 2.0 ** -32 * 2.0 - 1.0) * np.float64(rng))
    return np.array(out, np.float64)


def bias_coords(P):
    return (2 * np.arange(P) - P + 1).astype(np.float64) / np.float64(P - 1)


def bias_poly(P, coefs, order):
    X = bias_coords(P)
    pw = [np.ones(P)]
    for _ in range(MAX_ORDER):
        pw.append(pw[-1] * X)
    poly = np.zeros((P, P, P))
    for t, (a, b, c) in enumerate(bias_terms(order)):
        mono = (pw[a][:, None, None] * pw[b][None, :, None]) * pw[c][None, None, :]
        poly = poly + coefs[t] * mono
    return poly


def bias(x, mask, key, orders, ranges):
    y = x.copy()
    P = x.shape[1]
    for c in range(x.shape[0]):
        poly = bias_poly(P, bias_coefs(key, c, int(orders[c]), ranges[c]), int(orders[c]))
        y[c] = np.where(mask[c], (x[c].astype(np.float64) * np.exp(poly)).astype(np.float32), x[c])
    return y


def dropout(x, drop):
    y = x.copy()
    for c in range(x.shape[0]):
        if drop[c]:
            y[c] = 0
    return y


def apply_draw(x, draw):
    """all three stages of one patch: draw = None, or a dict with any of "lowres": scales, "bias": (range, order, (k0, k1)),
    "dropout": flags (what Artefact.draw returns)"""
    x = np.asarray(x, np.float32)
    if not draw:
        return x.copy()
    Cv, P = x.shape[:2]
    mask = entry_mask(x)
    if draw.get("lowres") is not None:
        x = lowres(x, mask, [extent(P, s) for s in draw["lowres"]])
    if draw.get("bias") is not None:
        rng, order, key = draw["bias"]
        x = bias(x, mask, key, [order] * Cv, [rng] * Cv)
    if draw.get("dropout") is not None:
        x = dropout(x, draw["dropout"])
    return x


def apply_batch(x, draws):
    return np.stack([apply_draw(xb, d) for xb, d in zip(x, draws)])


def make_data(seed, shape):
    """values in +-3 (a z-scored scan) with about 40 % exact zeros, float32"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-3, 3, shape).astype(np.float32)
    x[rs.uniform(size=shape) < 0.4] = 0
    return np.ascontiguousarray(x, np.float32)
