#!/usr/bin/env python3
"""Generate tests/golden/elastic.npz: scipy.ndimage.map_coordinates' own answers (mode="constant", cval=0) at the coordinates the
numpy statement of n3d_patch_gather_elastic's rule (tests/_elastic_ref.py; include/n3d.h, n3d_patch_edesc) gives, on small inputs
(make_golden_warp.warp_inputs(P) as a P^3 volume).

Needs scipy (1.15.3 wrote the committed file).  Per case: the twelve coefficients of the affine part as the kernel takes them, the
lattice parameters (cells, lock, key, amp), the flips and the crop's corner in the config, and scipy's outputs for the two data
channels at order 0 and at order 1 and for the label volume at order 0.  scipy is handed the crop (zero padded where it hangs out
of the volume, flipped on the flipped axes) as float64 and the coordinates c' = c + delta; its "constant" mode gives 0 to a voxel
whose c' lies outside [0, P - 1] on some axis, at either order: the rule's bounds test.

The cases: (P, cells, lock, amp) = (8, 1, 0, 1.5), (12, 2, 0, 2.0), (12, 3, 2, 1.5), (16, 4, 3, 1.8), (16, 8, 0, 0.9), one with per-axis
amp (2.0, 0.0, 1.0), one with flipped axes, one whose corner hangs out of the volume; the affine part is the identity (mode 0) or a
rotation composed with a scale (mode 1).  The lock 3 case is the exception: at cells 4 it has ONE free control point (G = 7, the
middle one), whose weight peaks at (2/3)^3, so it displaces by at most 0.296 * 1.8 = 0.53 voxels and by 0.03 on average -- on
integer coordinates no nearest voxel would change.  Its affine part is therefore a shift of 0.49 voxels per axis, signed like that
point's control value (the key was picked among 400 for the largest smallest component, 0.88): the coordinates sit just below the
rounding threshold and a displacement of 0.01 voxels shows as another source voxel.

main() asserts what keeps a test from passing on a field that does nothing: in every case with amp >= 1.5 and cells <= 4 the nearest
source voxel differs from the non-elastic one for at least 20 % of the voxels, and in every case fewer than 50 % of the voxels
have no source; and what tests/test_elastic_ref_host.py asserts: the restatement equals scipy at order 0, and at order 1 to one
float32 step.
Usage:  python tests/golden/make_golden_elastic.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _elastic_ref as er  # noqa: E402
import _warp_ref as wr  # noqa: E402
from make_golden_warp import warp_inputs  # noqa: E402
from oracle import data_step as ds  # noqa: E402

IDENTITY = None
# (name, P, cells, lock, amp, key, affine: None, (shift,) or (angles, A, b), flips, corner)
CASES = [
    ("p8_cells1", 8, 1, 0, 1.5, (0x243F6A88, 0x85A308D3), IDENTITY, (0, 0, 0), (0, 0, 0)),
    ("p12_cells2", 12, 2, 0, 2.0, (0x13198A2E, 0x03707344), IDENTITY, (0, 0, 0), (0, 0, 0)),
    ("p12_cells3_lock2_rotated", 12, 3, 2, 1.5, (0xA4093822, 0x299F31D0), ((6.0, -11.0, 4.0), (1.1, 0.93, 1.04), (-0.5, 0.4, -0.2)), (0, 0, 0), (0, 0, 0)),
    ("p16_cells4_lock3_shifted", 16, 4, 3, 1.8, (137296677, 3964562569), ((0.49, -0.49, 0.49),), (0, 0, 0), (0, 0, 0)),
    ("p16_cells8_rotated", 16, 8, 0, 0.9, (0x452821E6, 0x38D01377), ((-9.0, 3.0, 12.0), (0.95, 1.08, 0.9), (0.3, -0.6, 0.8)), (0, 0, 0), (0, 0, 0)),
    ("p12_per_axis_amp", 12, 2, 0, (2.0, 0.0, 1.0), (0xBE5466CF, 0x34E90C6C), IDENTITY, (0, 0, 0), (0, 0, 0)),
    ("p8_flipped_rotated", 8, 1, 0, 1.5, (0xC0AC29B7, 0xC97C50DD), ((4.0, 7.0, -5.0), (1.05, 0.97, 1.0), (0.0, 0.25, -0.25)), (1, 0, 1), (0, 0, 0)),
    ("p12_corner_outside", 12, 2, 0, 2.0, (0x3F84D5B5, 0xB5470917), IDENTITY, (0, 0, 0), (-2, 3, -1)),
]


def flipped(x, flips):
    axes = [1 + a for a in range(3) if flips[a]]
    return np.flip(x, axes) if axes else x


def case_inputs(c):
    """(data crop (2, P, P, P) float32, truth crop (1, P, P, P) uint8) of a config entry: the crop of warp_inputs(P) at its corner,
    NOT flipped (the rule flips the tap indices)"""
    data, truth = warp_inputs(c["P"])
    return ds.crop_zero_pad(data, c["corner"], c["P"]), ds.crop_zero_pad(truth, c["corner"], c["P"])


def coefficients(P, affine):
    if affine is None:
        return 0, wr.coefficients(0, np.ones(3), np.zeros(3))
    if len(affine) == 1:
        return 0, wr.coefficients(0, np.ones(3), np.asarray(affine[0], np.float64))
    angles, A, b = affine
    M, off = wr.warp_transform(np.asarray(A, np.float64), np.asarray(b, np.float64), wr.rotation_matrix(angles), P)
    return 1, wr.coefficients(1, M, off)


def scipy_answers(data, truth, c, flips):
    """map_coordinates of the (flipped) crop at the coordinates c: data at orders 0 and 1, labels at order 0"""
    from scipy.ndimage import map_coordinates

    def run(vol, order):
        return map_coordinates(vol.astype(np.float64), c, order=order, mode="constant", cval=0)
    d, t = flipped(data, flips), flipped(truth, flips)
    return (np.stack([run(ch, 0) for ch in d]).astype(np.float32), np.stack([run(ch, 1) for ch in d]).astype(np.float32),
            run(t[0], 0)[None].astype(np.uint8))


def main():
    config, ks, x0s, x1s, ys = [], [], [], [], []
    differ = total = 0
    for name, P, cells, lock, amp, key, affine, flips, corner in CASES:
        mode, k = coefficients(P, affine)
        amp3 = [float(a) for a in np.broadcast_to(np.asarray(amp, np.float64), (3,))]
        cfg = {"name": name, "P": P, "mode": mode, "cells": cells, "lock": lock, "key": list(key), "amp": amp3, "flips": list(flips),
               "corner": list(corner)}
        data, truth = case_inputs(cfg)
        el = er.case_elastic(cfg)
        c0, c1 = er.coordinates(P, mode, k), er.coordinates(P, mode, k, el)
        x0, x1, y = scipy_answers(data, truth, c1, flips)
        # the conditions on the fixture
        ok0, ok1 = (np.all((0.0 <= c) & (c <= P - 1.0), axis=0) for c in (c0, c1))
        near0, near1 = (np.floor(c + 0.5) for c in (c0, c1))
        moved = float(np.mean(np.any(near0 != near1, axis=0) | (ok0 != ok1)))
        nosrc = float(np.mean(~ok1))
        assert nosrc < 0.5, (name, nosrc)
        if min(amp3) >= 1.5 and cells <= 4:
            assert moved >= 0.2, (name, moved)
        assert (np.abs(er.field(P, *el)) <= np.asarray(amp3)[:, None, None, None]).all(), name
        # the restatement against scipy
        h0 = er.elastic_patch(data, mode, k, el, 0, flips)
        h1 = er.elastic_patch(data, mode, k, el, 1, flips)
        hy = er.elastic_patch(truth, mode, k, el, 0, flips)
        assert np.array_equal(h0, x0) and np.array_equal(hy, y), name
        assert wr.one_step(h1, x1).all(), name
        differ += int((h1 != x1).sum())
        total += h1.size
        assert np.array_equal(x0, np.round(x0)) and np.abs(x0).max() < 2 ** 15
        config.append(cfg)
        ks.append(k)
        x0s.append(x0.astype(np.int16).reshape(-1))
        x1s.append(x1.reshape(-1))
        ys.append(y.reshape(-1))
        print("%-26s P %2d cells %d lock %d  moved %4.1f %%  no source %4.1f %%  interpolated (non-integer) %5d" % (
            name, P, cells, lock, 100 * moved, 100 * nosrc, int((x1[0] != np.round(x1[0])).sum())))
    print("order 1: %d of %d voxels differ from the numpy statement (all within one float32 step)" % (differ, total))
    out = {"config": np.array(json.dumps({"cases": config})), "k": np.asarray(ks, np.float64), "x0": np.concatenate(x0s),
           "x1": np.concatenate(x1s).astype(np.float32), "y": np.concatenate(ys).astype(np.uint8)}
    path = os.path.join(HERE, "elastic.npz")
    np.savez_compressed(path, **out)
    print("wrote %s  (%d cases, %.1f KB)" % (path, len(config), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    sys.exit(main())
