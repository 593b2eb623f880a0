"""The ZScore normalisation rule (include/n3d.h, "a second normalisation", rules 1-5) restated in numpy, operation by operation:
sort, bins and the fixed order of the squared-deviation sum.  Every line below is one fp64 numpy operation (numpy does not
contract), so the device and this file agree bit for bit.  Shared by tests/test_zscore_ref_host.py and tests/test_gpu_zscore.py."""
from collections import namedtuple

import numpy as np

import _preprocess_ref as pr

FLT_MIN = np.float32(np.finfo(np.float32).tiny)           # 0x00800000
BINS, RUNS = 65536, 1024                                  # rule 4: 1024 runs of 64 consecutive bins

Stats = namedtuple("Stats", "count order lower_bound upper_bound n_below n_above sum_in mean std")


def bound(a, q):
    """rule 1 over the sorted int64 counts a: (bound, a[k], a[min(k + 1, n - 1)])"""
    n = len(a)
    vi = np.float64(n - 1) * (np.float64(q) / np.float64(100.0))
    kf = np.floor(vi)
    t = vi - kf
    k = int(kf)
    lo, hi = int(a[k]), int(a[min(k + 1, n - 1)])
    A, B = np.float64(lo), np.float64(hi)
    d = B - A
    return (B - d * (np.float64(1.0) - t) if t >= 0.5 else A + d * t), lo, hi


def modality_stats(vals, lower, upper):
    """rules 1-4 over the nonzero counts of one modality (any integer array, n >= 1)"""
    a = np.sort(np.asarray(vals).astype(np.int64).reshape(-1))
    n = len(a)
    assert n >= 1 and not (a == 0).any()
    (L, l0, l1), (U, u0, u1) = bound(a, lower), bound(a, upper)
    hist = np.bincount(a + 32768, minlength=BINS).astype(np.int64)
    vi = np.arange(BINS, dtype=np.int64) - 32768
    v = vi.astype(np.float64)
    below, above = v < L, v > U
    inside = ~(below | above)
    nL, nU, s_in = int(hist[below].sum()), int(hist[above].sum()), int((hist[inside] * vi[inside]).sum())
    mean = ((np.float64(nL) * L + np.float64(s_in)) + np.float64(nU) * U) / np.float64(n)
    dev = v - mean
    term = np.where(inside, hist.astype(np.float64) * (dev * dev), 0.0)      # + 0.0 leaves a non-negative sum as it is
    rows = term.reshape(RUNS, BINS // RUNS)
    acc = np.zeros(RUNS, np.float64)
    for j in range(BINS // RUNS):                                            # each run in ascending value
        acc = acc + rows[:, j]
    while len(acc) > 1:                                                      # adjacent pairs, ten rounds
        acc = acc[0::2] + acc[1::2]
    ssd = (np.float64(nL) * ((L - mean) * (L - mean)) + acc[0]) + np.float64(nU) * ((U - mean) * (U - mean))
    std = np.sqrt(ssd / np.float64(n))
    return Stats(n, (l0, l1, u0, u1), np.float64(L), np.float64(U), nL, nU, s_in, np.float64(mean), np.float64(std))


def subject_stats(raw, lower, upper):
    return [modality_stats(m[m != 0], lower, upper) for m in raw]


def normalized_modality(m, st):
    """rules 2 and 5 over one whole modality (X, Y, Z) int16 -> float32"""
    w = np.clip(m.astype(np.float64), st.lower_bound, st.upper_bound)
    r = ((w - st.mean) / st.std).astype(np.float32)
    r[r == 0] = FLT_MIN
    r[m == 0] = 0
    return r


def normalize_subject(raw, truth, lower, upper):
    """(box float32 (Cm, bx, by, bz), box truth or None, brain_width (2, 3) int64): the outline rule of the reference scheme"""
    sts = subject_stats(raw, lower, upper)
    full = np.stack([normalized_modality(m, st) for m, st in zip(raw, sts)])
    w = np.array([pr.outline(m) for m in raw])
    bw = np.vstack((w.min(axis=0)[0], w.max(axis=0)[1])).astype(np.int64)
    sl = pr.box_slices(bw, raw.shape[1:])
    return np.ascontiguousarray(full[(slice(None),) + sl]), (None if truth is None else np.ascontiguousarray(truth[sl])), bw
