"""The device rule of n3d_patch_gather_elastic (include/n3d.h, n3d_patch_edesc) restated in numpy, operation by operation, and the
layout of tests/golden/elastic.npz (make_golden_elastic.py).  No scipy here: the fixture carries scipy's answers.

The lattice has G = cells + 3 control points per axis; control value D[a][l] = 2.0 * (float64(w_a) * 2^-32) - 1.0 with w = Philox4x32-10
of the counter (l, 1, 0, 0) under the patch's key, +0.0 on the `lock` outermost layers; the field at patch index j is the tensor
product of the four uniform cubic B-spline weights per axis (weights()) with the 4^3 control points from cell_a = min(floor(j_a *
inv_h), cells - 1) on, summed separably -- axis 2 innermost, every sum left to right from the m = 0 product; the displacement
amp[a] * acc_a is added to the warp rule's coordinate (_warp_ref.coordinates) and everything downstream is _warp_ref's rule."""
import json
from unittest import mock

import numpy as np

import _appearance_ref as ap
import _warp_ref as wr

MAX_CELLS = 8
SIXTH = np.float64(1.0) / np.float64(6.0)


def lattice(cells, lock, key):
    """(3, G, G, G) float64: the control values"""
    G = cells + 3
    D = np.zeros((3, G ** 3), np.float64)
    for l in range(G ** 3):
        w = ap.philox4x32_10((l, 1, 0, 0), key)
        for a in range(3):
            D[a, l] = 2.0 * (np.float64(w[a]) * 2.0 ** -32) - 1.0
    D = D.reshape(3, G, G, G)
    free = np.zeros(G, bool)
    free[lock:G - lock] = True
    keep = free[:, None, None] & free[None, :, None] & free[None, None, :]
    return np.where(keep[None], D, 0.0)


def weights(f):
    """(4, ...) float64: the uniform cubic B-spline weights of f, product by product"""
    f = np.asarray(f, np.float64)
    g = 1.0 - f
    b0 = ((g * g) * g) * SIXTH
    b1 = ((((3.0 * f - 6.0) * f) * f) + 4.0) * SIXTH
    b2 = ((((3.0 - 3.0 * f) * f + 3.0) * f) + 1.0) * SIXTH
    b3 = ((f * f) * f) * SIXTH
    return np.stack([b0, b1, b2, b3])


def inv_h(cells, P):
    return np.float64(cells) / np.float64(P - 1)


def cells_and_weights(P, cells):
    """per patch index 0 .. P-1: (cell (P,) int, weights (4, P)) -- the same on every axis"""
    s = np.arange(P).astype(np.float64) * inv_h(cells, P)
    cell = np.minimum(np.floor(s), np.float64(cells - 1)).astype(np.int64)
    return cell, weights(s - cell.astype(np.float64))


def field(P, cells, lock, key, amp):
    """(3, P, P, P) float64: delta at every patch index j"""
    D = lattice(cells, lock, key)
    amp = np.broadcast_to(np.asarray(amp, np.float64), (3,))
    cell, b = cells_and_weights(P, cells)
    i = np.arange(P)
    out = []
    for a in range(3):
        U = []
        for m0 in range(4):
            T = []
            for m1 in range(4):
                def d(m2):
                    return D[a][(cell + m0)[:, None, None], (cell + m1)[None, :, None], (cell + m2)[None, None, :]]
                w = b[:, None, None, i]
                t = w[0] * d(0)
                t = t + w[1] * d(1)
                t = t + w[2] * d(2)
                T.append(t + w[3] * d(3))
            w = b[:, None, i, None]
            u = w[0] * T[0]
            u = u + w[1] * T[1]
            u = u + w[2] * T[2]
            U.append(u + w[3] * T[3])
        w = b[:, i, None, None]
        acc = w[0] * U[0]
        acc = acc + w[1] * U[1]
        acc = acc + w[2] * U[2]
        acc = acc + w[3] * U[3]
        out.append(amp[a] * acc)
    return np.stack(out)


def coordinates(P, mode, k, elastic=None):
    """(3, P, P, P) float64: c' = c + delta; elastic = None or (cells, lock, key, amp)"""
    c = wr.coordinates(P, mode, k)
    if elastic is None:
        return c
    return c + field(P, *elastic)


def resample(patch, c, order=0, flips=(0, 0, 0), gain=None, bias=None):
    """everything downstream of the coordinate is the warp rule: _warp_ref.warp_patch itself, handed the (3, P, P, P) coordinates c
    in place of the ones it would compute from twelve coefficients"""
    with mock.patch.object(wr, "coordinates", lambda P, mode, k: c):
        return wr.warp_patch(patch, 1, None, order, flips, gain, bias)


def elastic_patch(patch, mode, k, elastic=None, order=0, flips=(0, 0, 0), gain=None, bias=None):
    """what the rule makes of a (C, P, P, P) crop (zero padded where it hangs out of its volume); elastic = None or (cells, lock, key,
    amp); labels go through with order 0 and no gain / bias"""
    return resample(patch, coordinates(patch.shape[-1], mode, k, elastic), order, flips, gain, bias)


# ---- the fixture --------------------------------------------------------------------------------------------------------------

def records(g):
    """[(config {name, P, mode, cells, lock, key, amp, flips, corner}, k (12,), x0 (2, P, P, P) float32: scipy at order 0, x1: scipy
    at order 1, y (1, P, P, P) uint8: scipy's labels at order 0)] of elastic.npz"""
    cfg = json.loads(str(g["config"]))["cases"]
    ks, x0s, x1s, ys = g["k"], g["x0"], g["x1"], g["y"]
    out, o = [], 0
    for c, k in zip(cfg, ks):
        P3 = c["P"] ** 3
        shape = (c["P"],) * 3
        out.append((c, k.copy(), x0s[2 * o:2 * (o + P3)].reshape((2,) + shape).astype(np.float32), x1s[2 * o:2 * (o + P3)].reshape((2,) + shape),
                    ys[o:o + P3].reshape((1,) + shape)))
        o += P3
    assert o == len(ys) and 2 * o == len(x0s) == len(x1s) and x1s.dtype == np.float32
    return out


def case_elastic(c):
    return c["cells"], c["lock"], tuple(c["key"]), tuple(c["amp"])
