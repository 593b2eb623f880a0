"""The device rule of n3d_patch_gather_spline and n3d_spline_prefilter (include/n3d.h) restated in numpy, operation by operation, and
the layout of tests/golden/spline.npz (make_golden_spline.py).  No scipy here: the fixture carries scipy's answers.

The crop is flipped on the flipped axes (raw), turned into fp64 B-spline coefficients by the recursive filter along axis 0, then 1,
then 2 (coefficients), and read at the coordinate _elastic_ref.coordinates gives: per axis f = floor(c), the four weights of c - f
(_elastic_ref.weights), the taps f-1 .. f+2 mirrored into the crop, the 64 products summed in the order 16 i0 + 4 i1 + i2.  A voxel
whose nearest crop voxel is 0 (or whose coordinate is outside [0, P-1]) is stored as 0, every other one as the spline value, FLT_MIN
in place of +-0; gain and bias act on the kept voxels in float32."""
import json

import numpy as np

import _elastic_ref as er

FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def constants(P):
    """(z, gain, zn, inv0, anti) in fp64; zn by P - 2 multiplications"""
    z = np.sqrt(np.float64(3.0)) - np.float64(2.0)
    gain = (1.0 - z) * (1.0 - 1.0 / z)
    zn = z
    for _ in range(P - 2):
        zn = zn * z
    return z, gain, zn, 1.0 / (1.0 - zn * zn), z / (z * z - 1.0)


def filter_axis(c, axis):
    """the line recursion applied to every line of the float64 array c along `axis`: a new array"""
    c = np.moveaxis(np.array(c, np.float64), axis, 0)
    P = c.shape[0]
    z, gain, zn, inv0, anti = constants(P)
    c = c * gain
    s = c[0] + zn * c[P - 1]
    zi = z
    for i in range(1, P - 1):
        s = s + zi * (c[i] + zn * c[P - 1 - i])
        zi = zi * z
    c[0] = s * inv0
    for i in range(1, P):
        c[i] = c[i] + z * c[i - 1]
    c[P - 1] = (z * c[P - 2] + c[P - 1]) * anti
    for i in range(P - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return np.moveaxis(c, 0, axis)


def coefficients(raw):
    """(..., P, P, P) float64: the coefficients of every trailing cube of the float32 array raw, axis 0 first"""
    c = np.asarray(raw, np.float32).astype(np.float64)
    for axis in (-3, -2, -1):
        c = filter_axis(c, axis)
    return c


def flipped(x, flips):
    axes = [x.ndim - 3 + a for a in range(3) if flips[a]]
    return np.flip(x, axes) if axes else x


def nearest(P, c):
    """(ok (P, P, P) bool, [r_0, r_1, r_2] int): the bounds test and the nearest voxel in the flipped crop (0 where not ok)"""
    ok = np.all((0.0 <= c) & (c <= float(P - 1)), axis=0)
    return ok, [np.floor(np.where(ok, c[a], 0.0) + 0.5).astype(np.int64) for a in range(3)]


def mask(raw, c):
    """(C, P, P, P) bool: the voxels the rule keeps -- a coordinate inside and a nonzero nearest voxel of that channel"""
    ok, r = nearest(raw.shape[-1], c)
    return ok[None] & (raw[:, r[0], r[1], r[2]] != 0)


def spline_values(coef, c):
    """(C, P, P, P) float64: the 64-tap sums at the coordinates c (those of a voxel outside are the sums at coordinate 0)"""
    P = coef.shape[-1]
    ok = np.all((0.0 <= c) & (c <= float(P - 1)), axis=0)
    cc = np.where(ok[None], c, 0.0)
    f = np.floor(cc)
    u = [er.weights(cc[a] - f[a]) for a in range(3)]
    f = f.astype(np.int64)

    def tap(a, d):
        q = f[a] - 1 + d
        q = np.where(q < 0, -q, q)
        return np.where(q > P - 1, 2 * (P - 1) - q, q)

    idx = [[tap(a, d) for d in range(4)] for a in range(3)]
    acc = np.zeros(coef.shape, np.float64)
    for i0 in range(4):
        for i1 in range(4):
            for i2 in range(4):
                w = (u[0][i0] * u[1][i1]) * u[2][i2]
                acc = acc + w[None] * coef[:, idx[0][i0], idx[1][i1], idx[2][i2]]
    return acc


def resample(patch, c, flips=(0, 0, 0), gain=None, bias=None):
    """what the rule makes of a (C, P, P, P) float32 crop (zero padded where it hangs out of its volume, NOT flipped) at the (3, P, P,
    P) coordinates c"""
    raw = np.ascontiguousarray(flipped(np.asarray(patch, np.float32), flips))
    y = spline_values(coefficients(raw), c).astype(np.float32)
    keep = mask(raw, c)
    y = np.where(y == 0, FLT_MIN, y)
    out = np.where(keep, y, np.float32(0)).astype(np.float32)
    if gain is not None or bias is not None:
        C = raw.shape[0]
        g = np.ones(C, np.float32) if gain is None else np.asarray(gain, np.float64).astype(np.float32)
        b = np.zeros(C, np.float32) if bias is None else np.asarray(bias, np.float64).astype(np.float32)
        v = out * g[:, None, None, None]
        v = v + b[:, None, None, None]
        out = np.where(keep, v, out).astype(np.float32)
    return out


def spline_patch(patch, mode, k, elastic=None, flips=(0, 0, 0), gain=None, bias=None):
    """resample at the coordinates of the warp rule (mode, k) plus the displacement of elastic = None or (cells, lock, key, amp)"""
    return resample(patch, er.coordinates(patch.shape[-1], mode, k, elastic), flips, gain, bias)


# ---- the fixture --------------------------------------------------------------------------------------------------------------

def records(g):
    """[(config {name, P, mode, cells, lock, key, amp, flips, corner, elastic, crop}, k (12,), x3 (2, P, P, P) float32: scipy's
    map_coordinates(order=3, mode="constant") of the flipped crop, unmasked)] of spline.npz"""
    cfg = json.loads(str(g["config"]))["cases"]
    out, o = [], 0
    for c, k in zip(cfg, g["k"]):
        n = 2 * c["P"] ** 3
        out.append((c, k.copy(), g["x3"][o:o + n].reshape((2,) + (c["P"],) * 3)))
        o += n
    assert o == len(g["x3"]) and g["x3"].dtype == np.float32
    return out


def crops(g):
    """[(config {P, corner, flips}, coef (2, P, P, P) float64: scipy's spline_filter(order=3, mode="mirror") of the flipped crop)]"""
    cfg = json.loads(str(g["config"]))["crops"]
    out, o = [], 0
    for c in cfg:
        n = 2 * c["P"] ** 3
        out.append((c, g["coef"][o:o + n].reshape((2,) + (c["P"],) * 3)))
        o += n
    assert o == len(g["coef"]) and g["coef"].dtype == np.float64
    return out


def case_elastic(c):
    return er.case_elastic(c) if c["elastic"] else None
