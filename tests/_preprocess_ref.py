"""numpy restatement of the reference's preprocessing (preprocess.py:58-66, 77-144; helper.py:5-11) on in-memory int16 arrays: what
the device path (nas_3d_unet_amd.preprocess) is compared with where the fixture (tests/golden/preprocess.npz, made by the
reference's own functions) does not hold the quantity.  tests/test_preprocess_ref_host.py pins it to the fixture bit for bit."""
import numpy as np


def outline(img):
    """cal_outline: (2, 3) -- one voxel of margin around the nonzero voxels; start clamped to 0, end to the SHAPE (not shape - 1)"""
    idx = np.asarray(np.nonzero(img))
    return np.vstack((np.maximum(idx.min(axis=1) - 1, 0), np.minimum(idx.max(axis=1) + 1, img.shape)))


def normalize(img, mean, std, offset=0.1, mul_factor=100):
    """normalize + minmax_normalize: fp64 throughout, written back into the int16 array (truncation toward zero)"""
    out = np.array(img, dtype=np.int16)
    nz = np.nonzero(out)
    z = (out[nz] - np.float64(mean)) / np.float64(std)
    zmin, zmax = np.min(z), np.max(z)
    out[nz] = ((z - zmin) / (zmax - zmin) + offset) * mul_factor
    return out


def dataset_stats(subjects):
    """cal_mean_std's two loops per modality over raw (Cm, X, Y, Z) int16 arrays: counts, integer sums, unrounded fp64 mean and
    std (np.sum's pairwise order per subject, subjects added in order), each (Cm,)"""
    Cm = subjects[0].shape[0]
    count, total, mean, std = np.zeros(Cm, np.int64), np.zeros(Cm, np.int64), np.zeros(Cm), np.zeros(Cm)
    for c in range(Cm):
        brains = [s[c][np.nonzero(s[c])] for s in subjects]
        m = 0
        for b in brains:
            m += np.sum(b)              # int16 -> numpy sums in int64: exact
            count[c] += len(b)
        total[c] = m
        m = m / count[c]
        sq = 0
        for b in brains:
            sq += np.sum((b - m) ** 2)
        mean[c], std[c] = m, np.sqrt(sq / count[c])
    return count, total, mean, std


def rounded(v):
    """round() of an np.float64 is numpy's (scale, rint, unscale), not Python's correctly rounded decimal one"""
    return round(np.float64(v), 4)


def brain_width(normalized):
    """create_h5:63-65 over a subject's normalised modalities (Cm, X, Y, Z)"""
    w = np.array([outline(m) for m in normalized])
    return np.vstack((w.min(axis=0)[0], w.max(axis=0)[1]))


def box_slices(bw, shape):
    """the box the reference reads back (patches.py:140-142): start : end + 1, which numpy clips to the image"""
    return tuple(slice(int(bw[0, a]), min(int(bw[1, a]) + 1, int(shape[a]))) for a in range(3))
