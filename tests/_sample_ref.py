"""The rules of n3d_volume_line_index and n3d_patch_sample (include/n3d.h) in numpy and Python integers, operation by operation: the
same Philox4x32-10 words, the same multiply-shift reduction, the same binary search on the line index and the same k-th mask voxel of
the chosen line.  Volumes are (Cv, X, Y, Z) float32 arrays, truths (X, Y, Z) uint8 arrays or None.  Used by the CPU tests (which tie
it to brute force: np.cumsum, np.argwhere) and by the GPU tests (which tie the kernels to it with ==)."""
import functools

import numpy as np

from _appearance_ref import philox4x32_10

MASKS = ("brain", "tumour", 1, 2, 4)
MODE_UNIFORM, MODE_FALLBACK, MODE_BAD_ID = 255, 254, 253


def mask_bits(masks):
    return sum(1 << MASKS.index(m) for m in masks)


def masks_of(vol, truth):
    """the five boolean masks (5, X, Y, Z): some channel nonzero (the bits below the sign: -0.0 is zero, NaN / inf / denormals are
    not); label != 0; label 1; label 2; label 4 -- rows 1 to 4 all False without truth"""
    bits = np.ascontiguousarray(vol, np.float32).view(np.uint32)
    m = np.zeros((5,) + vol.shape[1:], bool)
    m[0] = ((bits & np.uint32(0x7FFFFFFF)) != 0).any(axis=0)
    if truth is not None:
        t = np.asarray(truth).reshape(vol.shape[1:])
        m[1], m[2], m[3], m[4] = t != 0, t == 1, t == 2, t == 4
    return m


def line_index(vol, truth):
    """(5, X*Y + 1) int32: row m, entry l = the number of mask-m voxels in the lines (x, y), x*Y + y < l"""
    Cv, X, Y, Z = vol.shape
    m = masks_of(vol, truth).reshape(5, X * Y, Z)
    out = np.zeros((5, X * Y + 1), np.int64)
    for i in range(5):
        acc = 0
        counts = m[i].sum(axis=1)
        for l in range(X * Y):
            acc += int(counts[l])
            out[i, l + 1] = acc
    return out.astype(np.int32)


def reduce(q, R):
    """a 32-bit word to [0, R): (q * R) >> 32 in Python integers"""
    q, R = int(q), int(R)
    assert 0 <= q <= 0xFFFFFFFF and R >= 1
    return (q * R) >> 32


@functools.lru_cache(maxsize=None)
def draws(N, key):
    """the words of samples 0 .. N-1 under `key`: [(w, u)] with w the block of counter (n, 2, 0, 0) and u that of (n, 3, 0, 0)"""
    return [(philox4x32_10((n, 2, 0, 0), key), philox4x32_10((n, 3, 0, 0), key)) for n in range(N)]


def corner_bounds(D, P):
    """(lo, hi) of one axis: the corners that keep the patch inside a box of D, or the one that centres a smaller box"""
    if D >= P:
        return 0, D - P
    lo = -((P - D) // 2)
    return lo, lo


def select_voxel(masks5, index, m, r):
    """voxel r of mask m by the rule: the line by binary search on the index row, then the (r - row[l])-th set z of that line"""
    _, X, Y, Z = masks5.shape
    row = index[m]
    l = int(np.searchsorted(row, r, side="right")) - 1
    z = int(np.flatnonzero(masks5[m].reshape(X * Y, Z)[l])[r - int(row[l])])
    return l // Y, l % Y, z


def sample(vols, truths, ids, N, P, key, fg_threshold, masks, prepared=None):
    """(cand (N, 4) int32, mode (N,) uint8) of n3d_patch_sample.  masks: the bit word.  prepared: None, or what prepare() gave for
    (vols, truths) -- the masks and line indexes, which do not depend on the other arguments"""
    prepared = prepare(vols, truths) if prepared is None else prepared
    cand, mode = np.zeros((N, 4), np.int32), np.zeros(N, np.uint8)
    for n, (w, u) in enumerate(draws(int(N), (int(key[0]), int(key[1])))):
        v = int(ids[reduce(u[0], len(ids))])
        if not 0 <= v < len(vols):
            cand[n], mode[n] = (v, 0, 0, 0), MODE_BAD_ID
            continue
        masks5, index = prepared[v]
        D = masks5.shape[1:]
        md, vox = MODE_UNIFORM, None
        if u[1] < fg_threshold:
            present = [m for m in range(5) if (masks >> m) & 1 and index[m, -1] > 0]
            md = MODE_FALLBACK
            if present:
                md = present[reduce(u[2], len(present))]
                vox = select_voxel(masks5, index, md, reduce(w[0], int(index[md, -1])))
        c = []
        for a in range(3):
            lo, hi = corner_bounds(D[a], P)
            c.append(min(max(vox[a] - P // 2, lo), hi) if vox is not None else lo + reduce(w[1 + a], hi - lo + 1))
        cand[n], mode[n] = [v] + c, md
    return cand, mode


def prepare(vols, truths):
    return [(masks_of(v, t), line_index(v, t)) for v, t in zip(vols, truths)]


KEY = (0x2545F491, 0x9E3779B9)      # the key the tests fix


def four_volumes(Cv=2):
    """the tests' set: (vols, truths).  0: an axis (5) shorter than every P used; 1: no label 4; 2: no tumour at all; 3: tumour only
    at z = 63, 64, 127, 128 of the 130-long first and last lines.  Data: small integers, about half of them zero, some -0.0, and
    voxels that are nonzero in the LAST channel only."""
    rng = np.random.default_rng(20)
    shapes = ((5, 20, 18), (18, 17, 20), (17, 19, 16), (9, 17, 130))
    vols, truths = [], []
    for n, sh in enumerate(shapes):
        v = rng.integers(-3, 4, (Cv,) + sh).astype(np.float32) * (rng.random((1,) + sh) < 0.5)
        v[:-1][:, rng.random(sh) < 0.2] = 0.0            # brain through the last channel alone, where that one is nonzero
        v[0][rng.random(sh) < 0.1] = -0.0
        t = rng.choice(np.array([0, 0, 0, 1, 2, 4], np.uint8), sh)
        if n == 1:
            t[t == 4] = 2
        elif n == 2:
            t[:] = 0
        elif n == 3:
            t[:] = 0
            t[0, 0, [63, 64, 127, 128]] = (1, 2, 4, 1)
            t[-1, -1, [63, 64, 127, 128]] = (4, 2, 1, 4)
        vols.append(np.ascontiguousarray(v, np.float32))
        truths.append(t)
    return vols, truths


SEVEN = [(4, 5, 6), (4, 5, 7), (10, 20, 4), (11, 4, 20), (20, 20, 20), (19, 4, 4), (12, 12, 12)]


def seven_voxel_volume():
    """(vol, truth): a 24^3 box of brain with exactly the 7 tumour voxels SEVEN (labels 1, 2, 4 in turn), all far enough inside
    that a patch of 8 centred on one is never clamped: corner + 4 is the voxel"""
    D = (24, 24, 24)
    vol, t = np.ones((1,) + D, np.float32), np.zeros(D, np.uint8)
    for n, x in enumerate(SEVEN):
        t[x] = (1, 2, 4)[n % 3]
    return vol, t


def uniformity_counts(cand7000, mode6000):
    """(the hits per voxel of SEVEN among 7000 always-foreground crops of 8, the foreground-centred samples among 6000 at 1/3)"""
    hit = [tuple(c) for c in (np.asarray(cand7000)[:, 1:] + 4).tolist()]
    return [hit.count(x) for x in SEVEN], int((np.asarray(mode6000) == 1).sum())
