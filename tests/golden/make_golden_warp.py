#!/usr/bin/env python3
"""Generate tests/golden/warp.npz: scipy.ndimage.affine_transform's own answers (mode="constant", cval=0) for the resampling rule of
n3d_patch_gather_warp (include/n3d.h, n3d_patch_wdesc), on P = 8 and P = 10 inputs (warp_inputs: those of
make_golden_augment.operator_inputs with the second channel made non-negative).

Needs scipy (1.15.3 wrote the committed file) and tests/golden/augment.npz.  Per case: the twelve coefficients as the kernel takes
them and scipy's outputs for the two data channels at order 0 and at order 1 and for the label volume at order 0:

  * matrix cases (mode 1, a 2-D matrix): rotations alone; rotations composed with the non-identity scale maps (A, b) of
    augment.npz's operator cases through warp_transform; exact 90-degree rotations; matrices whose offsets put a coordinate
    exactly on 0, on P - 1 and on k + 0.5; and candidates for telling the two summation orders of the matrix rule apart (below);
  * zoom cases (mode 0, a 1-D matrix): the scale maps of augment.npz's operator and adversarial cases, which scipy resamples by its
    zoom-shift rule c = (j + b / A) * A -- here at order 1 as well.

The two summation orders.  scipy adds the products in axis order and the offset last, ((m0 j0 + m1 j1) + m2 j2) + off; the other
candidate is the offset first, ((off + m0 j0) + m1 j1) + m2 j2.  find_order_cases() constructs rows (m, off) for which the two
land on different sides of a rounding threshold (k + 0.5) or of a bound (0, P - 1) at some voxel -- such inputs exist -- and keeps
scipy's answer: it is the axis-order one in every case found, which main() asserts.

main() also checks what tests/test_warp_ref_host.py asserts: the numpy statement of the rule (tests/_warp_ref.py) equals scipy at
order 0 everywhere, and at order 1 to one float32 step with at most 1 voxel in 1000 differing at all.
Usage:  python tests/golden/make_golden_warp.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _augment_ref as ar  # noqa: E402
import _warp_ref as wr  # noqa: E402
from make_golden_augment import operator_inputs  # noqa: E402

ROTATIONS = [(8, (10.0, -5.0, 3.0)), (10, (-15.0, 15.0, 15.0)), (8, (0.0, 0.0, 12.5)), (10, (7.0, 0.0, 0.0)), (8, (-2.0, 14.0, -9.0)),
             (10, (1e-3, -1e-3, 2e-3))]
SCALED_ANGLES = [(6.0, -11.0, 4.0), (-14.0, 3.0, 9.0), (2.5, 8.0, -13.0)]


def warp_inputs(P):
    """operator_inputs(P) with channel 1 shifted to 0..4: with no negative values a linear interpolation cancels nothing, so scipy's
    order of multiplications ((x * u_0) * u_1) * u_2 and the rule's ((u_0 * u_1) * u_2) * x stay some 1e-16 apart RELATIVELY (a
    signed pattern interpolates to values like -2.4e-11 whose float32 roundings are many steps apart)"""
    data, truth = operator_inputs(P)
    data = data.copy()
    data[1] += 2
    return data, truth


def quarter_turns():
    """exact 90-degree rotations about the centre: entries 0 / +-1, offsets 0 or P - 1 -- every coordinate is an integer"""
    out = []
    for P, rows in ((8, ((0, -1, 0), (1, 0, 0), (0, 0, 1))), (10, ((0, 0, 1), (0, 1, 0), (-1, 0, 0))), (8, ((1, 0, 0), (0, 0, -1), (0, 1, 0))),
                    (10, ((0, 1, 0), (0, 0, 1), (1, 0, 0)))):
        M = np.array(rows, np.float64)
        off = np.array([(P - 1.0) if (M[a] < 0).any() else 0.0 for a in range(3)])
        out.append(("quarter_turn", P, M, off))
    return out


def threshold_cases():
    """a rotation by an exactly representable (c, s) = (0.8, 0.6) / (0.96, 0.28) pair in one plane, with offsets that put the
    coordinate of a chosen voxel exactly on 0, on P - 1 and on k + 0.5"""
    out = []
    for P, (c, s), j, targets in ((8, (0.8, 0.6), (2, 5, 3), (0.0, 7.0, 3.5)), (10, (0.96, 0.28), (7, 1, 4), (9.0, 4.5, 0.0)),
                                  (8, (0.6, -0.8), (1, 1, 6), (6.5, 0.0, 7.0)), (10, (0.28, 0.96), (5, 8, 2), (0.5, 9.0, 8.5))):
        M = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        if P == 10:
            M = M[[2, 0, 1]][:, [2, 0, 1]]
        jj = np.array(j, np.float64)
        off = np.array([t - ((M[a, 0] * jj[0] + M[a, 1] * jj[1]) + M[a, 2] * jj[2]) for a, t in enumerate(targets)])
        out.append(("threshold", P, M, off))
    return out


def _rule(m, off, j, order):
    if order == "axis":
        return ((m[0] * j[0] + m[1] * j[1]) + m[2] * j[2]) + off
    return ((off + m[0] * j[0]) + m[1] * j[1]) + m[2] * j[2]


def _answer(c, P):
    return np.where((c >= 0) & (c <= P - 1), np.floor(np.where((c >= 0) & (c <= P - 1), c, 0.0) + 0.5), -1).astype(np.int64)


def find_order_cases(n_want=4, seed=91):
    """(P, M, off) whose first row separates the two summation orders at some voxel: the row is a slightly shrunk rotation row, the
    offset puts the axis-order sum of a chosen voxel on a threshold, and the case is kept when the offset-first sum of SOME voxel
    answers differently (another voxel, or a bound).  The other two rows are the identity's."""
    rng = np.random.default_rng(seed)
    j = [g.astype(np.float64) for g in np.meshgrid(*[np.arange(10)] * 3, indexing="ij")]
    found, tries = [], 0
    while len(found) < n_want:
        tries += 1
        P = 8 if len(found) % 2 == 0 else 10
        jp = [g[:P, :P, :P] for g in j]
        th = rng.uniform(-0.3, 0.3, 2)
        m = np.array([np.cos(th[0]) * np.cos(th[1]), -np.sin(th[0]), np.sin(th[1])]) * rng.uniform(0.8, 1.2)
        j0 = rng.integers(0, P, 3).astype(np.float64)
        target = float(rng.choice([0.0, P - 1.0])) if tries % 3 == 0 else float(rng.integers(0, P - 1)) + 0.5
        off = target - ((m[0] * j0[0] + m[1] * j0[1]) + m[2] * j0[2])
        a, b = _answer(_rule(m, off, jp, "axis"), P), _answer(_rule(m, off, jp, "offset_first"), P)
        if np.array_equal(a, b):
            continue
        M = np.eye(3)
        M[0] = m
        found.append(("order", P, M, np.array([off, 0.0, 0.0]), int((a != b).sum())))
    return found, tries


def scipy_answers(P, matrix, offset):
    """affine_transform of the two data channels at orders 0 and 1 and of the labels at order 0; matrix: (3, 3), or (3,) -- the
    diagonal, which scipy resamples by its zoom-shift rule"""
    from scipy.ndimage import affine_transform
    data, truth = warp_inputs(P)

    def run(vol, order):
        return affine_transform(vol, matrix, offset=offset, output_shape=(P, P, P), order=order, mode="constant", cval=0)
    return np.stack([run(ch, 0) for ch in data]), np.stack([run(ch, 1) for ch in data]), run(truth[0], 0)[None]


def main():
    g = np.load(os.path.join(HERE, "augment.npz"), allow_pickle=False)
    ops, advs = ar.operator_records(g), ar.adversarial_records(g)
    scales = [(cfg["name"], cfg["P"], A, b) for cfg, _, _, A, b, identity, _, _ in ops if not identity]
    cases = []                                        # (name, P, mode, k, scipy outputs)
    for P, angles in ROTATIONS:
        M, off = wr.warp_transform(np.ones(3), np.zeros(3), wr.rotation_matrix(angles), P)
        cases.append(("rotation_%g_%g_%g" % angles, P, 1, wr.coefficients(1, M, off)))
    for n, (name, P, A, b) in enumerate(scales):
        M, off = wr.warp_transform(A, b, wr.rotation_matrix(SCALED_ANGLES[n % len(SCALED_ANGLES)]), P)
        cases.append(("rotated_" + name, P, 1, wr.coefficients(1, M, off)))
    for name, P, M, off in quarter_turns() + threshold_cases():
        cases.append((name, P, 1, wr.coefficients(1, M, off)))
    order_cases, tries = find_order_cases()
    for name, P, M, off, ndiff in order_cases:
        cases.append((name, P, 1, wr.coefficients(1, M, off)))
        print("order case: P %d row %s off %r -- %d voxels separate the two summation orders" % (P, M[0].tolist(), off[0], ndiff))
    print("(%d candidates tried)" % tries)
    zooms = [("zoom_" + name, P, A, b) for name, P, A, b in scales]
    for n, (P, axis, A, b, _) in enumerate(advs):
        A_, b_ = np.ones(3), np.zeros(3)
        A_[axis], b_[axis] = A, b
        zooms.append(("zoom_adversarial_%d" % n, P, A_, b_))

    config, ks, x0s, x1s, ys = [], [], [], [], []
    differ = total = 0

    def keep(name, P, mode, k, x0, x1, y):
        nonlocal differ, total
        data, truth = warp_inputs(P)
        h0, h1, hy = wr.warp_patch(data, mode, k, 0), wr.warp_patch(data, mode, k, 1), wr.warp_patch(truth, mode, k, 0)
        assert x0.dtype == np.float32 and x1.dtype == np.float32 and y.dtype == np.uint8
        assert np.array_equal(h0, x0) and np.array_equal(hy, y), name        # order 0 and labels: the rule IS scipy's
        assert wr.one_step(h1, x1).all(), name
        differ += int((h1 != x1).sum())
        total += h1.size
        assert np.array_equal(x0, np.round(x0)) and np.abs(x0).max() < 2 ** 15
        config.append({"name": name, "P": P, "mode": mode})
        ks.append(k)
        x0s.append(x0.astype(np.int16).reshape(-1))
        x1s.append(x1.reshape(-1))
        ys.append(y.reshape(-1))
        print("%-34s P %2d mode %d  voxels with a source %4d  interpolated (non-integer) %4d" % (
            name, P, mode, int((x0[0] != 0).sum()), int((x1[0] != np.round(x1[0])).sum())))

    for name, P, mode, k in cases:
        keep(name, P, mode, k, *scipy_answers(P, k[:9].reshape(3, 3), k[9:12]))
    for name, P, A, b in zooms:
        keep(name, P, 0, wr.coefficients(0, A, b / A), *scipy_answers(P, A, b))
    print("order 1: %d of %d voxels differ from the numpy statement (all within one float32 step)" % (differ, total))
    assert differ * 1000 <= total
    out = {"config": np.array(json.dumps({"cases": config})), "k": np.asarray(ks, np.float64), "x0": np.concatenate(x0s),
           "x1": np.concatenate(x1s).astype(np.float32), "y": np.concatenate(ys).astype(np.uint8)}
    path = os.path.join(HERE, "warp.npz")
    np.savez_compressed(path, **out)
    print("wrote %s  (%d cases, %.1f KB)" % (path, len(config), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    sys.exit(main())
