"""The device rule of n3d_patch_gather_aug (include/n3d.h, n3d_patch_adesc) restated in numpy with one index table per axis, and
the layout of tests/golden/augment.npz (make_golden_augment.py).  No scipy here: the fixture carries scipy's answers.

Per axis a of a P^3 patch and patch index j:  c = (float64(j) + sh[a]) * A[a] -- an add, then a multiply, each rounded to fp64;
inside <=> 0 <= c <= P - 1, tested on c itself; source index r = int(floor(c + 0.5)), then P - 1 - r on a flipped axis (the flip was
applied to the source before it was resampled).  A voxel with an outside axis is 0 in the data and in the labels."""
import json

import numpy as np


def axis_table(P, A, sh, identity, flipped):
    """source index of every patch index on one axis, -1 where the coordinate falls outside the patch"""
    j = np.arange(P, dtype=np.float64)
    if identity:
        r = np.arange(P, dtype=np.int64)
    else:
        c = (j + np.float64(sh)) * np.float64(A)
        inside = (0.0 <= c) & (c <= float(P - 1))
        r = np.where(inside, np.floor(np.where(inside, c, 0.0) + 0.5), -1).astype(np.int64)
    if flipped:
        r = np.where(r >= 0, P - 1 - r, -1)
    return r


def augment_patch(patch, A, sh, identity, flips):
    """what do_augment makes of a (C, P, P, P) crop: out[c, i0, i1, i2] = patch[c, r0[i0], r1[i1], r2[i2]], or 0"""
    P = patch.shape[-1]
    tabs = [axis_table(P, A[a], sh[a], identity, bool(flips[a])) for a in range(3)]
    ok = (tabs[0] >= 0)[:, None, None] & (tabs[1] >= 0)[None, :, None] & (tabs[2] >= 0)[None, None, :]
    src = [np.maximum(t, 0) for t in tabs]
    out = patch[:, src[0][:, None, None], src[1][None, :, None], src[2][None, None, :]]
    return np.where(ok[None], out, np.zeros((), patch.dtype))


def params_of(A, b, identity):
    """(A, sh): sh = b / A, the division scipy.ndimage.affine_transform does in numpy (nothing to divide on the identity path)"""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    return (A, np.zeros(3)) if identity else (A, b / A)


# ---- the fixture --------------------------------------------------------------------------------------------------------------

def operator_records(g):
    """[(config, scale or None, flips (3,), A, b, identity, x (2, P, P, P) float32, y (1, P, P, P) uint8)] of augment.npz"""
    cfg = json.loads(str(g["config"]))["ops"]
    table, xs, ys = g["op/table"], g["op/x"], g["op/y"]
    out, ox, oy = [], 0, 0
    for c, row in zip(cfg, table):
        P3 = c["P"] ** 3
        x = xs[ox:ox + 2 * P3].reshape(2, c["P"], c["P"], c["P"]).astype(np.float32)
        y = ys[oy:oy + P3].reshape(1, c["P"], c["P"], c["P"])
        ox, oy = ox + 2 * P3, oy + P3
        scale = None if np.isnan(row[:3]).any() else row[:3].copy()
        out.append((c, scale, row[3:6].astype(np.int64), row[6:9].copy(), row[9:12].copy(), bool(row[12]), x, y))
    assert ox == len(xs) and oy == len(ys)
    return out


def adversarial_records(g):
    """[(P, axis, A, b, src (P,) int: scipy's source index per output index, -1 outside)]"""
    return [(int(t[0]), int(t[1]), float(t[2]), float(t[3]), s[:int(t[0])].astype(np.int64)) for t, s in zip(g["adv/table"], g["adv/src"])]


def generator_records(g):
    """[(config, rows (n, 15) int32: epoch, batch, volume, corner, key (6, or -1), flips (3); scales (n, 3), NaN: none; x, y of the
    first batch)]"""
    cfg = json.loads(str(g["config"]))["gens"]
    return [(c, g["gen%d/rows" % i], g["gen%d/scales" % i], g["gen%d/x8" % i].astype(np.float32) / 8, g["gen%d/y" % i])
            for i, c in enumerate(cfg)]


def key_of_row(k):
    return None if k[0] < 0 else ((int(k[0]), int(k[1])), int(k[2]), int(k[3]), int(k[4]), int(k[5]))
