#!/usr/bin/env python3
"""Generate tests/golden/components.npz: scipy's answers for the label clean-up (nas_3d_unet_amd.postprocess).

The reference has no code for this step; the fixture pins the definitions to scipy.ndimage.label:
  * components of `labels != 0` under generate_binary_structure(3, 1 | 2 | 3) = connectivity 6 | 18 | 26; the id of a component is
    the smallest linear index (x * Y + y) * Z + z of its voxels, -1 on background;
  * step A: a component is kept iff size >= min_voxels and (not keep_largest or it is the largest; equal sizes: the smallest id);
    the voxels of the others become 0;
  * step B: e = label-4 voxels in kept components; if 0 < e < et_min_voxels they become 1.
The rules are stated here in this script's own code (np.bincount and plain numpy), not imported from the package.  Needs scipy
(1.15) and numpy; the tests need neither scipy nor this script's main().  Per case the fixture holds the input volume, the ids at
6 / 18 / 26 and, per rule set of RULES, the cleaned volume and the nine statistics.  The archive is written with fixed member
times and order, so a second run gives the same bytes.
Usage:  python tests/golden/make_golden_components.py"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 2718
CONNECTIVITIES = (6, 18, 26)
STAT_KEYS = ("n_components", "n_kept", "voxels_in", "voxels_kept", "largest_size", "largest_id", "et_in", "et_kept", "et_relabelled")
ET_KEPT = 7     # label-4 voxels of the et_rule case that lie in the component step A keeps at min_voxels = 10
# (connectivity, min_voxels, keep_largest, et_min_voxels); every rule set is applied to every case
RULES = ((26, 0, False, 0),                 # every rule off: the output is the input
         (26, 5, False, 0), (6, 3, False, 0), (18, 0, True, 0),
         (26, 0, True, 10 ** 6),            # the largest component only, and whatever label 4 it holds becomes 1
         (6, 2, False, 4), (26, 10 ** 9, False, 0),   # nothing is as large: nothing is kept
         (18, 4, True, 0),
         (26, 10, False, ET_KEPT - 1), (26, 10, False, ET_KEPT), (26, 10, False, ET_KEPT + 1))


def _labels(rng, shape):
    return rng.choice(np.array([1, 2, 4], np.uint8), size=shape)


def serpentine(shape, y):
    """a one-voxel-wide path in the plane `y`: the z lines at even x, joined at alternating ends by one voxel at odd x; it starts
    at (0, y, 0), its smallest linear index"""
    X, _, Z = shape
    m = np.zeros(shape, bool)
    for x in range(0, X, 2):
        m[x, y, :] = True
        if x + 1 < X - 1:
            m[x + 1, y, Z - 1 if (x // 2) % 2 == 0 else 0] = True
    return m


def spiral(n):
    """a one-voxel-wide square spiral in an n x n plane, one empty cell between its arms, from (0, 0) inwards"""
    m = np.zeros((n, n), bool)
    x, y, d = 0, 0, 0
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))
    m[0, 0] = True

    def free(d):
        ax, ay = x + steps[d][0], y + steps[d][1]
        bx, by = ax + steps[d][0], ay + steps[d][1]
        if not (0 <= ax < n and 0 <= ay < n) or m[ax, ay]:
            return False
        return not (0 <= bx < n and 0 <= by < n and m[bx, by])

    while True:
        if not free(d):
            d = (d + 1) % 4
            if not free(d):
                return m
        x, y = x + steps[d][0], y + steps[d][1]
        m[x, y] = True


def component_cases():
    """[(name, labels (X, Y, Z) uint8)], seeded; numpy only.  The device kernels label 8 x 8 x 32 tiles: the cases cross tile faces
    along every axis."""
    rng = np.random.default_rng(SEED)
    z = lambda s: np.zeros(s, np.uint8)
    cases = []
    # odd sizes, ~30 % density: many components, different at 6 / 18 / 26
    box = (13, 9, 21)
    cases.append(("box", np.where(rng.uniform(0, 1, box) < 0.3, _labels(rng, box), 0).astype(np.uint8)))
    # 9 x 1 x 3 tiles: one component that crosses every tile face of its plane many times, speckle two planes away from it
    wide = (70, 5, 66)
    path = serpentine(wide, 2)
    v = np.where(path, np.where(rng.uniform(0, 1, wide) < 0.2, 4, 2), 0).astype(np.uint8)
    sp = rng.uniform(0, 1, wide) < 0.1
    sp[:, 1:4, :] = False
    cases.append(("wide", np.where(sp, _labels(rng, wide), v).astype(np.uint8)))
    # a line of 130 along y: 17 tiles long
    tall = z((3, 130, 4))
    tall[1, :, 2] = 2
    tall[1, 40:44, 2] = 4
    tall[0, rng.uniform(0, 1, 130) < 0.3, 0] = 1
    cases.append(("tall", tall))
    # a long chain of parents: 25 tiles in the plane, the path's smallest index at its outer end
    cases.append(("spiral", np.repeat(np.where(spiral(40), 2, 0).astype(np.uint8)[:, :, None], 3, axis=2)))
    # pairs that touch by a face, by an edge only and by a corner only, each across tile faces (x: 7 | 8, y: 7 | 8, z: 31 | 32)
    diag = z((12, 12, 40))
    for p in ((7, 1, 1), (8, 1, 1), (4, 7, 31), (4, 8, 32), (7, 7, 31), (8, 8, 32)):
        diag[p] = 2
    cases.append(("diag", diag))
    # neighbours in linear index that are no neighbours in space
    wrap = z((4, 5, 6))
    for p in ((1, 1, 5), (1, 2, 0), (2, 4, 5), (3, 0, 0)):
        wrap[p] = 1
    cases.append(("wrap", wrap))
    cases.append(("full", _labels(rng, (17, 9, 40))))
    g = np.indices((10, 9, 35)).sum(axis=0)
    cases.append(("checker", np.where(g % 2 == 0, 2, 0).astype(np.uint8)))
    cases.append(("empty", z(box)))
    single = z(box)
    single[5, 4, 11] = 4
    cases.append(("single", single))
    # two largest components of 8 voxels and a smaller one
    tie = z(box)
    tie[1:3, 1:3, 1:3] = 2
    tie[8:10, 5:7, 12:14] = 1
    tie[5, 4, 6:9] = 4
    cases.append(("tie", tie))
    # label 4 partly in a component that min_voxels = 10 removes: 3 voxels there, ET_KEPT in the large one
    et = z((20, 9, 40))
    et[2:8, 2:7, 10:34] = 2
    et[3, 3, 30:30 + ET_KEPT] = 4
    et[15, 4, 3:6] = 4
    et[15, 5, 3] = 1
    cases.append(("et_rule", et))
    return cases


def first_index_ids(lab):
    """scipy's labels (1 .. n, 0 background) -> the smallest linear index of each label's voxels, -1 on background"""
    _, first = np.unique(lab.ravel(), return_index=True)       # sorted labels; the first occurrence in flat order
    if lab.min() == 0:
        first = first.copy()
        first[0] = -1
    else:
        first = np.concatenate([[-1], first])
    return first[lab].astype(np.int32)


def scipy_ids(mask, connectivity):
    from scipy import ndimage
    lab, _ = ndimage.label(mask, ndimage.generate_binary_structure(3, CONNECTIVITIES.index(connectivity) + 1))
    return first_index_ids(lab)


def clean(labels, ids, min_voxels, keep_largest, et_min_voxels):
    """steps A and B on `labels` with the component ids `ids` -> (cleaned volume, the nine statistics in STAT_KEYS order)"""
    n = labels.size
    fg = ids >= 0
    size = np.bincount(ids[fg], minlength=n)
    et = np.bincount(ids[fg & (labels == 4)], minlength=n)
    roots = np.flatnonzero(size)
    largest_size = int(size[roots].max()) if roots.size else 0
    largest_id = int(roots[size[roots] == largest_size].min()) if roots.size else -1
    keep_root = size[roots] >= min_voxels
    if keep_largest:
        keep_root &= roots == largest_id
    kept = np.zeros(n + 1, bool)             # kept[-1]: background
    kept[roots[keep_root]] = True
    out = np.where(kept[ids], labels, 0).astype(np.uint8)
    e = int(et[roots[keep_root]].sum())
    relabel = 0 < e < et_min_voxels
    if relabel:
        out[out == 4] = 1
    stats = [roots.size, int(keep_root.sum()), int(size.sum()), int(size[roots[keep_root]].sum()), largest_size, largest_id,
             int(et.sum()), e, int(relabel)]
    return out, np.array(stats, np.int64)


def write_npz(path, arrays):
    """np.load reads it like np.savez_compressed's; members sorted and stamped 1980-01-01, so the bytes depend on the arrays only"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    out, names = {}, []
    for name, labels in component_cases():
        names.append(name)
        out[name + "/labels"] = labels
        ids = {c: scipy_ids(labels != 0, c) for c in CONNECTIVITIES}
        counts = []
        for c in CONNECTIVITIES:
            out["%s/ids_%d" % (name, c)] = ids[c]
            counts.append(len(np.unique(ids[c][ids[c] >= 0])))
        for k, (c, mv, kl, em) in enumerate(RULES):
            vol, stats = clean(labels, ids[c], mv, kl, em)
            out["%s/clean_%d" % (name, k)], out["%s/stats_%d" % (name, k)] = vol, stats
        print("%-8s %-14s components at 6 / 18 / 26: %s" % (name, labels.shape, counts))
        if name == "diag":
            assert counts == [5, 4, 3], counts
        if name == "wrap":
            assert counts == [4, 4, 4], counts
        if name in ("wide", "spiral", "tall"):      # the path is one component at every connectivity and starts at voxel (0, y, 0) or the line's end
            path = {"wide": (0, 2, 0), "spiral": (0, 0, 0), "tall": (1, 0, 2)}[name]
            lin = int(np.ravel_multi_index(path, labels.shape))
            for c in CONNECTIVITIES:
                size = int((ids[c] == lin).sum())
                assert size >= {"wide": 2300, "spiral": 3 * 700, "tall": 130}[name], (name, c, size)
                if name != "wide":
                    assert size == int((ids[6] == lin).sum())
        if name == "full":
            assert counts == [1, 1, 1] and (labels != 0).all()
        if name == "checker":
            assert counts == [int((labels != 0).sum()), 1, 1], counts
        if name == "empty":
            assert counts == [0, 0, 0] and out["empty/stats_0"].tolist() == [0, 0, 0, 0, 0, -1, 0, 0, 0]
        if name == "single":
            assert counts == [1, 1, 1]
        if name == "tie":
            s = out["tie/stats_3"]          # (18, 0, True, 0)
            assert s[4] == 8 and s[5] == int(np.ravel_multi_index((1, 1, 1), labels.shape)) and s[1] == 1 and s[3] == 8
            assert (out["tie/clean_3"] != 0).sum() == 8 and (out["tie/clean_3"][1:3, 1:3, 1:3] == 2).all()
        if name == "et_rule":
            for k, relabelled in ((8, 0), (9, 0), (10, 1)):       # et_min_voxels = e - 1, e, e + 1: only e < et_min_voxels relabels
                s = out["et_rule/stats_%d" % k]
                assert s[6] == ET_KEPT + 3 and s[7] == ET_KEPT and s[8] == relabelled, s
            assert (out["et_rule/clean_10"] == 4).sum() == 0 and (out["et_rule/clean_9"] == 4).sum() == ET_KEPT
        assert np.array_equal(out[name + "/clean_0"], labels)
    out["names"] = np.array(names)
    out["rules"] = np.array([[c, mv, int(kl), em] for c, mv, kl, em in RULES], np.int64)
    path = os.path.join(HERE, "components.npz")
    write_npz(path, out)
    size = os.path.getsize(path)
    print("wrote %s  (%d arrays, %.1f KB)" % (path, len(out), size / 1024))
    assert size < 512 * 1024


if __name__ == "__main__":
    sys.exit(main())
