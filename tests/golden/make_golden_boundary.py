#!/usr/bin/env python3
"""Generate tests/golden/boundary.npz: scipy's squared distances for the signed distance maps of loss.BoundaryLoss.

Per fixture shape of tests/_boundary_ref.SHAPES the archive holds
  <name>.t      uint8 (B, C, D0, D1, D2): the maps (tests/_boundary_ref.fixture_targets)
  <name>.d2fg   int32: squared Euclidean index distance to the nearest voxel with t = 1; INF (1 << 29) where the map holds none
  <name>.d2bg   int32: the same for t = 0
  <name>.phi    float32: the rule of include/n3d.h applied to THOSE distances -- sqrt(float64(d2_fg)) on the background,
                -(sqrt(float64(d2_bg)) - 1.0) on the foreground, one rounding to float32, 0 where the distance is INF.
The distances are scipy's: distance_transform_edt(mask, return_indices=True) names, for every voxel of the mask, the nearest voxel
outside it; the squared index differences to it are exact integers, summed here in int64.  (scipy's float distances are not used,
and a map without a voxel outside the mask -- where scipy's indices mean nothing -- is recorded as INF by this script's own rule.)
phi of the fixture is what Kervadec's one_hot2dist gives, edt(~m) * ~m - (edt(m) - 1) * m, whenever both kinds of voxel exist: main()
checks that against scipy's own float64 distances after the rounding to float32.

Needs scipy (checked on 1.15.3) and numpy; the tests need neither scipy nor this script.  The archive is written with fixed member
times and order, so a second run gives the same bytes.
Usage:  python tests/golden/make_golden_boundary.py"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def scipy_d2(mask):
    """int64 squared distance from every voxel of `mask` to the nearest voxel outside it (0 outside); INF when nothing is outside"""
    from scipy.ndimage import distance_transform_edt
    import _boundary_ref as br
    if mask.all():
        return np.full(mask.shape, br.INF, np.int64)
    idx = distance_transform_edt(mask, return_indices=True, return_distances=False)
    grid = np.indices(mask.shape)
    return ((idx.astype(np.int64) - grid) ** 2).sum(axis=0)


def build():
    from scipy.ndimage import distance_transform_edt
    import _boundary_ref as br
    arrays = {}
    for name, (shape, _) in br.SHAPES.items():
        B, C = shape[:2]
        t = br.fixture_targets(name)
        d2fg = np.empty(shape, np.int64)
        d2bg = np.empty(shape, np.int64)
        phi = np.empty(shape, np.float32)
        for b in range(B):
            for c in range(C):
                m = t[b, c] != 0
                d2fg[b, c] = scipy_d2(~m)      # on the background: to the nearest foreground voxel
                d2bg[b, c] = scipy_d2(m)
                phi[b, c] = br.phi_rule(m, d2fg[b, c], d2bg[b, c])
                if m.any() and not m.all():
                    one_hot2dist = distance_transform_edt(~m) * ~m - (distance_transform_edt(m) - 1) * m
                    assert np.array_equal(phi[b, c], one_hot2dist.astype(np.float32)), (name, b, c)
        arrays[name + ".t"] = t
        arrays[name + ".d2fg"] = d2fg.astype(np.int32)
        arrays[name + ".d2bg"] = d2bg.astype(np.int32)
        arrays[name + ".phi"] = phi
    return arrays


def save(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    arrays = build()
    path = os.path.join(HERE, "boundary.npz")
    save(path, arrays)
    print("wrote %s: %d arrays, %d bytes" % (path, len(arrays), os.path.getsize(path)))


if __name__ == "__main__":
    main()
