"""The device rule of n3d_patch_gather_warp (include/n3d.h, n3d_patch_wdesc) restated in numpy, the host functions
generator.rotation_matrix / warp_transform restated independently, and the layout of tests/golden/warp.npz (make_golden_warp.py).
No scipy here: the fixture carries scipy's answers.

For patch index j of a P^3 crop and the twelve coefficients k:
  mode 0:  c_a = (float64(j_a) + sh[a]) * A[a],  A = k[0:3], sh = k[3:6];
  mode 1:  c_a = ((m[a][0] * j_0 + m[a][1] * j_1) + m[a][2] * j_2) + off[a],  m = k[0:9] row-major, off = k[9:12]
every product and every sum rounded to fp64 on its own; inside <=> 0 <= c_a <= P - 1 on all axes, tested on c itself; the labels
(and the data at order 0) take the voxel floor(c + 0.5); the data at order 1 the eight taps floor(c) + d in lexicographic order of
d, weight (u_0 * u_1) * u_2, acc = acc + weight * float64(x), a tap past P - 1 skipped; a tap index r is P - 1 - r on a flipped axis;
then, on the nonzero values, * gain and + bias in float32, each rounded on its own."""
import json

import numpy as np


def coordinates(P, mode, k):
    """(3, P, P, P) float64: the source coordinate of every patch index"""
    k = np.asarray(k, np.float64)
    j = [g.astype(np.float64) for g in np.meshgrid(*[np.arange(P)] * 3, indexing="ij")]
    if mode == 0:
        return np.stack([(j[a] + k[3 + a]) * k[a] for a in range(3)])
    out = []
    for a in range(3):
        t = k[3 * a] * j[0]
        t = t + k[3 * a + 1] * j[1]
        t = t + k[3 * a + 2] * j[2]
        out.append(t + k[9 + a])
    return np.stack(out)


def warp_patch(patch, mode, k, order=0, flips=(0, 0, 0), gain=None, bias=None):
    """what the rule makes of a (C, P, P, P) crop (zero padded where it hangs out of its volume); order 1 and the intensity map
    are for float32 data -- labels go through with order 0 and no gain / bias"""
    P = patch.shape[-1]
    c = coordinates(P, mode, k)
    ok = np.all((0.0 <= c) & (c <= float(P - 1)), axis=0)

    def src(r, a):
        r = np.clip(r, 0, P - 1)
        return P - 1 - r if flips[a] else r

    if order == 0:
        r = [src(np.floor(np.where(ok, c[a], 0.0) + 0.5).astype(np.int64), a) for a in range(3)]
        out = np.where(ok[None], patch[:, r[0], r[1], r[2]], np.zeros((), patch.dtype))
    else:
        f = np.floor(np.where(ok[None], c, 0.0))
        w = np.where(ok[None], c, 0.0) - f
        f = f.astype(np.int64)
        acc = np.zeros(patch.shape, np.float64)
        for d0 in (0, 1):
            for d1 in (0, 1):
                for d2 in (0, 1):
                    d = (d0, d1, d2)
                    use = ok & (f[0] + d0 <= P - 1) & (f[1] + d1 <= P - 1) & (f[2] + d2 <= P - 1)
                    u = [w[a] if d[a] else 1.0 - w[a] for a in range(3)]
                    wt = (u[0] * u[1]) * u[2]
                    x = patch[:, src(f[0] + d0, 0), src(f[1] + d1, 1), src(f[2] + d2, 2)].astype(np.float64)
                    acc = np.where(use[None], acc + wt[None] * x, acc)
        out = acc.astype(np.float32)
    if gain is not None or bias is not None:
        C = patch.shape[0]
        g = np.ones(C, np.float32) if gain is None else np.asarray(gain, np.float64).astype(np.float32)
        b = np.zeros(C, np.float32) if bias is None else np.asarray(bias, np.float64).astype(np.float32)
        y = out * g[:, None, None, None]            # float32 * float32, rounded to float32
        y = y + b[:, None, None, None]              # ... then the add, rounded again
        out = np.where(out != 0, y, out).astype(np.float32)
    return out


def rotation_matrix(angles_deg):
    """Rz . Ry . Rx, entry by entry (generator.rotation_matrix restated: radians = angle * pi / 180, numpy's sin / cos, products and
    sums left to right)"""
    rad = [np.float64(a) * np.pi / 180.0 for a in angles_deg]
    (cx, cy, cz), (sx, sy, sz) = [np.cos(r) for r in rad], [np.sin(r) for r in rad]
    R = np.zeros((3, 3), np.float64)
    R[0, 0], R[0, 1], R[0, 2] = cz * cy, (cz * sy) * sx - sz * cx, (cz * sy) * cx + sz * sx
    R[1, 0], R[1, 1], R[1, 2] = sz * cy, (sz * sy) * sx + cz * cx, (sz * sy) * cx - cz * sx
    R[2, 0], R[2, 1], R[2, 2] = -sy, cy * sx, cy * cx
    return R


def warp_transform(A, b, R, P):
    """(M, off): M[a][n] = A[a] * R[a][n]; off[a] = A[a] * (p - ((R[a][0] * p + R[a][1] * p) + R[a][2] * p)) + b[a], p = (P - 1) / 2"""
    p = np.float64(P - 1) / np.float64(2)
    M, off = np.zeros((3, 3), np.float64), np.zeros(3, np.float64)
    for a in range(3):
        Rp = (np.float64(R[a][0]) * p + np.float64(R[a][1]) * p) + np.float64(R[a][2]) * p
        off[a] = np.float64(A[a]) * (p - Rp) + np.float64(b[a])
        for n in range(3):
            M[a, n] = np.float64(A[a]) * np.float64(R[a][n])
    return M, off


def coefficients(mode, first, second):
    """the twelve coefficients: mode 0 from (A, sh), mode 1 from (M, off)"""
    if mode == 0:
        return np.concatenate((np.asarray(first, np.float64), np.asarray(second, np.float64), np.zeros(6)))
    return np.concatenate((np.asarray(first, np.float64).reshape(9), np.asarray(second, np.float64)))


# ---- the fixture --------------------------------------------------------------------------------------------------------------

def records(g):
    """[(config {name, P, mode}, k (12,), x0 (2, P, P, P) float32: scipy at order 0, x1: scipy at order 1, y (1, P, P, P) uint8:
    scipy's labels at order 0)] of warp.npz; the inputs are make_golden_warp.warp_inputs(P)"""
    cfg = json.loads(str(g["config"]))["cases"]
    ks, x0s, x1s, ys = g["k"], g["x0"], g["x1"], g["y"]
    out, o = [], 0
    for c, k in zip(cfg, ks):
        P = c["P"]
        P3 = P ** 3
        out.append((c, k.copy(), x0s[2 * o:2 * (o + P3)].reshape(2, P, P, P).astype(np.float32), x1s[2 * o:2 * (o + P3)].reshape(2, P, P, P),
                    ys[o:o + P3].reshape(1, P, P, P)))
        o += P3
    assert o == len(ys) and 2 * o == len(x0s) == len(x1s) and x1s.dtype == np.float32
    return out


def one_step(a, b):
    """|a - b| <= np.spacing(|b|) elementwise for float32 arrays: equal, or neighbours"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64)
