#!/usr/bin/env python3
"""Generate tests/golden/spline.npz: scipy's own answers for the cubic B-spline (order 3) interpolation of the patch gather
(n3d_patch_gather_spline / n3d_spline_prefilter, include/n3d.h; the numpy statement is tests/_spline_ref.py).

Needs scipy (1.15.3 wrote the committed file).  The cases are those of make_golden_elastic.py -- P = 8, 12, 16, two channels, a
crop hanging out of the volume, flipped axes, both coordinate modes, every lattice -- each with its displacement, and three of them
(an identity, two rotations, one of those flipped) once more without it.  Per case: scipy.ndimage.map_coordinates(order=3,
mode="constant", cval=0) of the float64 crop (zero padded, flipped on the flipped axes) at the rule's coordinates, as float32 and NOT
masked: the mask is the rule's own addition and the tests apply it.  Per distinct crop: scipy.ndimage.spline_filter(order=3,
mode="mirror", output=float64), the coefficients map_coordinates uses for mode="constant".

main() asserts what tests/test_spline_ref_host.py asserts (the statement within one float32 step of scipy on the kept voxels, the
coefficients within the bound) and what keeps those from being empty: in every case the mask keeps and drops at least 10 % of the
voxels of some channel, scipy is nonzero on most dropped voxels, and most kept voxels lie off the integer grid.
Usage:  python tests/golden/make_golden_spline.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _elastic_ref as er  # noqa: E402
import _spline_ref as sr  # noqa: E402
import _warp_ref as wr  # noqa: E402
from make_golden_elastic import CASES, case_inputs, coefficients  # noqa: E402

PLAIN = ("p12_cells2", "p12_cells3_lock2_rotated", "p8_flipped_rotated")      # also recorded without their displacement


def main():
    from scipy.ndimage import map_coordinates, spline_filter
    config, crops, ks, x3s, coefs = [], [], [], [], []
    worst_coef = 0.0
    differ = total = 0
    for name, P, cells, lock, amp, key, affine, flips, corner in CASES:
        mode, k = coefficients(P, affine)
        amp3 = [float(a) for a in np.broadcast_to(np.asarray(amp, np.float64), (3,))]
        for elastic in ((True, False) if name in PLAIN else (True,)):
            cfg = {"name": name + ("" if elastic else "_plain"), "P": P, "mode": mode, "cells": cells, "lock": lock, "key": list(key),
                   "amp": amp3, "flips": list(flips), "corner": list(corner), "elastic": elastic}
            data, _ = case_inputs(cfg)
            raw = sr.flipped(data, flips).astype(np.float64)
            crop = {"P": P, "corner": list(corner), "flips": list(flips)}
            if crop not in crops:
                crops.append(crop)
                want = np.stack([spline_filter(ch, order=3, output=np.float64, mode="mirror") for ch in raw])
                have = sr.coefficients(raw.astype(np.float32))
                worst_coef = max(worst_coef, float(np.abs(have - want).max() / np.abs(raw).max()))
                coefs.append(want.reshape(-1))
            cfg["crop"] = crops.index(crop)
            c = er.coordinates(P, mode, k, sr.case_elastic(cfg))
            x3 = np.stack([map_coordinates(ch, c, order=3, mode="constant", cval=0) for ch in raw]).astype(np.float32)
            have = sr.resample(data, c, flips)
            keep = sr.mask(raw.astype(np.float32), c)
            assert wr.one_step(have, x3)[keep].all() and not have[~keep].any() and (have[keep] != 0).all(), cfg["name"]
            differ += int((have != x3)[keep].sum())
            total += int(keep.sum())
            frac = keep.reshape(2, -1).mean(axis=1)
            assert ((frac > 0.1) & (frac < 0.9)).any(), (cfg["name"], frac)
            inside = np.broadcast_to(sr.nearest(P, c)[0], keep.shape)
            assert not x3[~inside].any() and (x3[~keep & inside] != 0).mean() > 0.5, cfg["name"]
            if elastic or mode == 1:
                assert (x3[keep] != np.round(x3[keep])).mean() > 0.5, cfg["name"]
            else:       # integer coordinates: the spline interpolates, so scipy returns the crop itself (and rounding noise where it is 0)
                assert np.array_equal(x3[keep], raw.astype(np.float32)[keep]), cfg["name"]
            config.append(cfg)
            ks.append(k)
            x3s.append(x3.reshape(-1))
            print("%-34s P %2d  kept %4.1f / %4.1f %%  scipy nonzero on dropped %4.1f %%  range %.2f .. %.2f" % (
                cfg["name"], P, 100 * frac[0], 100 * frac[1], 100 * (x3[~keep & inside] != 0).mean(), x3.min(), x3.max()))
    print("order 3: %d of %d kept voxels differ from the numpy statement (all within one float32 step)" % (differ, total))
    print("coefficients: largest |statement - spline_filter| / max|x| = %.3e" % worst_coef)
    out = {"config": np.array(json.dumps({"cases": config, "crops": crops})), "k": np.asarray(ks, np.float64),
           "x3": np.concatenate(x3s).astype(np.float32), "coef": np.concatenate(coefs).astype(np.float64)}
    path = os.path.join(HERE, "spline.npz")
    np.savez_compressed(path, **out)
    print("wrote %s  (%d cases, %d crops, %.1f KB)" % (path, len(config), len(crops), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    sys.exit(main())
