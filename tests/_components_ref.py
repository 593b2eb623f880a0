"""A numpy-only restatement of the label clean-up (include/n3d.h, "Label clean-up"), written from the definitions: what the device
results are compared with besides scipy's fixture (tests/golden/components.npz).

Labelling is iterated minimum propagation: every foreground voxel starts with its own linear index and takes, round after round,
the smallest value among itself and its neighbours -- the volume shifted by every offset of the neighbourhood, voxels shifted in
from outside counting as background -- until a round changes nothing.  A value is always the index of a voxel of the same
component, so each round also replaces a voxel's value by the value of the voxel it names (a path of n voxels settles in about
log n rounds instead of n); the fixed point is the same: every voxel holds its component's smallest index.  The rules are boolean
algebra on np.bincount's sizes."""
import itertools

import numpy as np

CONNECTIVITIES = (6, 18, 26)
STAT_KEYS = ("n_components", "n_kept", "voxels_in", "voxels_kept", "largest_size", "largest_id", "et_in", "et_kept", "et_relabelled")


def offsets(connectivity):
    """the neighbourhood: the offsets in {-1, 0, 1}^3 with 1 .. level nonzero entries (level 1, 2, 3 for 6, 18, 26)"""
    level = CONNECTIVITIES.index(connectivity) + 1
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 1 <= sum(1 for c in o if c) <= level]


def _shifted(shape, off):
    """(destination, source) slices: destination voxel p reads source voxel p + off where that lies inside the volume"""
    dst = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip(off, shape))
    src = tuple(slice(max(0, o), n - max(0, -o)) for o, n in zip(off, shape))
    return dst, src


def label(mask, connectivity=26):
    """(X, Y, Z) array, nonzero = foreground -> int32 (X, Y, Z): the smallest linear index of the voxel's component, -1 on background"""
    mask = np.asarray(mask) != 0
    big = mask.size
    ids = np.where(mask, np.arange(big, dtype=np.int64).reshape(mask.shape), big)
    slices = [_shifted(mask.shape, o) for o in offsets(connectivity)]
    while True:
        new = ids.copy()
        for dst, src in slices:
            np.minimum(new[dst], ids[src], out=new[dst])
        new[~mask] = big
        new = np.append(new.ravel(), big)[new]          # the value of the voxel the value names; background names `big`, which stays
        if np.array_equal(new, ids):
            return np.where(mask, ids, -1).astype(np.int32)
        ids = new


def clean(labels, connectivity=26, min_voxels=0, keep_largest=False, et_min_voxels=0):
    """-> (cleaned uint8 volume, statistics dict with STAT_KEYS)"""
    labels = np.asarray(labels)
    ids = label(labels != 0, connectivity).ravel()
    lab = labels.ravel()
    n = lab.size
    fg = ids >= 0
    size = np.bincount(ids[fg], minlength=n)
    et = np.bincount(ids[fg & (lab == 4)], minlength=n)
    is_root = size > 0
    largest_size = int(size.max()) if n else 0
    largest_id = int(np.argmax(size)) if largest_size else -1       # argmax: the first, i.e. smallest, index among equals
    keep = is_root & (size >= min_voxels)
    if keep_largest:
        keep &= np.arange(n) == largest_id
    kept_voxel = fg & keep[np.where(fg, ids, 0)]
    e = int(et[keep].sum())
    relabel = 0 < e < et_min_voxels
    out = np.where(kept_voxel, lab, 0).astype(np.uint8)
    if relabel:
        out[out == 4] = 1
    stats = dict(zip(STAT_KEYS, (int(is_root.sum()), int(keep.sum()), int(size.sum()), int(size[keep].sum()), largest_size, largest_id,
                                 int(et.sum()), e, bool(relabel))))
    return out.reshape(labels.shape), stats


def stats_row(stats):
    """the statistics as the fixture stores them: nine int64 in STAT_KEYS order"""
    return np.array([int(stats[k]) for k in STAT_KEYS], np.int64)
