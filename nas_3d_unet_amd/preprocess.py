"""The reference's preprocessing (preprocess.py:58-66, 77-144) on the device: raw int16 scans to the data set's mean / std
dictionary and to each subject's normalised brain-wise box -- what VolumeSet.add stores and Generator / Trainer / SubjectPredictor
consume.  File access (nibabel, h5) is not built: the caller hands over arrays.

  * cal_mean_std(subjects): two passes over the subjects (resident in HBM in between).  Pass 1: one n3d_brain_scan launch per
    subject adds each modality's count and exact integer sum of the nonzero voxels; ONE host sync; mean = sum / count in fp64.
    Pass 2: n3d_brain_sqdev adds sum (x - mean)^2 in fp64 in a fixed order (no floating-point atomics: two runs give the same
    bits); ONE host sync; std = sqrt(. / count).  Both rounded as the reference's np.float64 values round: numpy's round(., 4).
  * normalize_subject(raw, mean_std, truth): n3d_brain_scan for the per-modality extrema and outlines, ONE host sync for them,
    then one n3d_brain_normalize launch writes the box only: create_h5's brain_width and the crop patches.py:140-142 reads back.

The reference's normalize writes its fp64 result into nibabel's int16 array, so the stored value is truncated toward zero to an
integer 10..110 (background 0); the networks were trained on those values, and this module reproduces them bit for bit.
float32 raw data is refused: the reference's sums are then fp32 pairwise sums whose order cannot be pinned.

A second scheme stands next to it for nets trained from scratch, chosen per call with scheme=ZScore(lower, upper): each
modality's brain voxels are clipped to two of their own percentiles and z-scored (include/n3d.h states the rule operation by
operation).  It needs no dictionary; the box and brain_width are the same; a brain voxel never stores 0 (FLT_MIN stands in), so
the box is nonzero exactly where raw is, which is what every consumer takes as "brain".
  * normalize_subject(raw, None, truth, scheme=ZScore()): n3d_brain_scan, n3d_brain_hist (exact histogram of the counts),
    n3d_brain_robust (order statistics, bounds, mean, std: one record per modality), ONE host sync for the outlines and the
    record, then n3d_brain_zscore writes the box.  subject_stats(raw, scheme) returns what the record holds.

Host logic only; the kernels are n3d_brain_scan, n3d_brain_sqdev, n3d_brain_normalize and n3d_brain_hist, n3d_brain_robust,
n3d_brain_zscore (include/n3d.h)."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import N3DError, check

MODS = ("t1", "t1ce", "flair", "t2")
REC_WORDS = 8       # N3D_BRAIN_REC_WORDS: min value, max value, min index x y z, max index x y z
_I32_MAX, _I32_MIN = 2 ** 31 - 1, -2 ** 31
_REC_INIT = [_I32_MAX, _I32_MIN, _I32_MAX, _I32_MAX, _I32_MAX, -1, -1, -1]

# count, sum: int64 (Cm,); mean, std: UNROUNDED float64 (Cm,)
DatasetStats = namedtuple("DatasetStats", "count sum mean std")

HIST_BINS = 65536   # N3D_BRAIN_HIST_BINS
ROBUST_WORDS = 16   # N3D_BRAIN_ROBUST_WORDS
# one record of n3d_brain_robust, word for word as include/n3d.h lays it out
ROBUST_DTYPE = np.dtype([("count", "<i8"), ("order", "<i8", (4,)), ("n_below", "<i8"), ("n_above", "<i8"), ("sum_in", "<i8"),
                         ("lower", "<f8"), ("upper", "<f8"), ("mean", "<f8"), ("std", "<f8"), ("ssd", "<f8"), ("reserved", "<i8", (3,))])
assert ROBUST_DTYPE.itemsize == 8 * ROBUST_WORDS
# one modality of subject_stats: order = (a[kL], a[kL + 1], a[kU], a[kU + 1]) of the sorted brain counts (indices clamped to n - 1);
# lower_bound, upper_bound, mean, std: np.float64
SubjectStats = namedtuple("SubjectStats", "count order lower_bound upper_bound n_below n_above mean std")


def _device(device):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise N3DError("preprocess: raw scans are processed on a HIP device (got %s); there is no CPU fallback" % dev)
    return dev


def _raw(raw, device, what):
    """(Cm, X, Y, Z) int16 numpy array or tensor -> contiguous device tensor (a device tensor stays where it is: no copy)"""
    r = torch.from_numpy(np.ascontiguousarray(raw)) if isinstance(raw, np.ndarray) else raw
    if not (isinstance(r, torch.Tensor) and r.dim() == 4):
        raise N3DError("%s: raw must be a (C, X, Y, Z) int16 array or tensor" % what)
    if r.dtype != torch.int16:
        raise N3DError("%s: raw must be int16 scanner counts (got %s); float raw data is not built -- the reference sums it in "
                       "fp32 in an order that cannot be reproduced" % (what, r.dtype))
    if min(r.shape) < 1 or int(np.prod(r.shape[1:])) >= 2 ** 31:
        raise N3DError("%s: raw of shape %s: needs 1 <= X * Y * Z < 2^31" % (what, tuple(r.shape)))
    return r.to(device).contiguous()


def _records(n, Cm, device):
    return torch.tensor(_REC_INIT, dtype=torch.int32).repeat(n, Cm, 1).to(device)


def _scan(lib, r, totals, rec):
    Cm, X, Y, Z = (int(s) for s in r.shape)
    check(lib.n3d_brain_scan(K.ptr(r), Cm, X, Y, Z, K.ptr(totals), K.ptr(rec), K.stream_ptr()), "n3d_brain_scan")


def dataset_stats(subjects, mods=MODS, device=None):
    """counts, exact sums and the UNROUNDED fp64 mean and std of every modality over the nonzero voxels of `subjects` (an iterable
    of (Cm, X, Y, Z) int16 arrays or tensors, Cm = len(mods); shapes may differ).  Two host syncs."""
    dev, lib, Cm = _device(device), _lib.load(), len(mods)
    totals = torch.zeros((Cm, 2), dtype=torch.int64, device=dev)
    resident = []
    for s in subjects:
        r = _raw(s, dev, "cal_mean_std")
        if r.shape[0] != Cm:
            raise N3DError("cal_mean_std: a subject has %d modalities, mods names %d" % (r.shape[0], Cm))
        resident.append(r)
    if not resident:
        raise N3DError("cal_mean_std: no subjects")
    recs = _records(len(resident), Cm, dev)
    for i, r in enumerate(resident):
        _scan(lib, r, totals, recs[i])
    t = totals.cpu().numpy()                                   # sync 1
    count, total = t[:, 0].copy(), t[:, 1].copy()
    for c in range(Cm):
        if count[c] == 0:
            raise N3DError("cal_mean_std: modality %s has no nonzero voxel in the data set" % mods[c])
    mean = total.astype(np.float64) / count.astype(np.float64)  # |sum| < 2^53: the conversion is exact, one rounding in the quotient
    mean_d = torch.from_numpy(mean).to(dev)
    acc = torch.zeros(Cm, dtype=torch.float64, device=dev)
    rows = max(int(lib.n3d_brain_sqdev_rows(int(np.prod(r.shape[1:])))) for r in resident)
    ws = torch.empty(Cm * rows, dtype=torch.float64, device=dev)
    for r in resident:
        check(lib.n3d_brain_sqdev(K.ptr(r), Cm, int(np.prod(r.shape[1:])), K.ptr(mean_d), K.ptr(ws), K.ptr(acc), K.stream_ptr()),
              "n3d_brain_sqdev")
    std = np.sqrt(acc.cpu().numpy() / count)                   # sync 2
    return DatasetStats(count, total, mean, std)


def cal_mean_std(subjects, mods=MODS, device=None):
    """preprocess.py:96-144: {'t1_mean': .., 't1_std': .., ...} over the nonzero voxels of every modality, values np.float64 rounded
    as the reference's are (round() of an np.float64 is numpy's rounding); the std is taken about the unrounded mean."""
    st = dataset_stats(subjects, mods, device)
    out = {}
    for c, m in enumerate(mods):
        out["%s_mean" % m] = round(np.float64(st.mean[c]), 4)
        out["%s_std" % m] = round(np.float64(st.std[c]), 4)
    return out


class ZScore:
    """The second normalisation scheme (include/n3d.h, "a second normalisation"): per subject and per modality, the brain voxels'
    counts are clipped to their `lower` and `upper` percentiles (in percent, numpy's linear np.percentile) and z-scored with the
    mean and std of the clipped counts.  ZScore(0, 100) clips nothing: plain z-scoring.  Needs no data-set statistics."""

    def __init__(self, lower=0.5, upper=99.5):
        try:
            lo, hi = float(lower), float(upper)
        except (TypeError, ValueError):
            raise N3DError("ZScore: lower and upper are percentiles in percent (got %r, %r)" % (lower, upper)) from None
        if not (np.isfinite(lo) and np.isfinite(hi) and 0 <= lo < hi <= 100):
            raise N3DError("ZScore: needs finite percentiles 0 <= lower < upper <= 100 (got %r, %r)" % (lower, upper))
        self.lower, self.upper = lo, hi

    def __repr__(self):
        return "ZScore(lower=%r, upper=%r)" % (self.lower, self.upper)


def _truth(truth, X, Y, Z, dev):
    if truth is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(truth)) if isinstance(truth, np.ndarray) else truth
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and tuple(t.shape) in ((X, Y, Z), (1, X, Y, Z))):
        raise N3DError("normalize_subject: truth must be a (X, Y, Z) or (1, X, Y, Z) uint8 label volume matching raw")
    return t.reshape(X, Y, Z).to(dev).contiguous()


def _box(h, shape):
    """create_h5's brain_width (2, 3) and the high corner of the box the reference reads back, from the host copy of the scan's
    records h (Cm, REC_WORDS) int64"""
    start = np.maximum(h[:, 2:5] - 1, 0).min(axis=0)
    end = np.minimum(h[:, 5:8] + 1, shape).max(axis=0)
    return np.vstack((start, end)), np.minimum(end + 1, shape)


def _robust(lib, r, scheme, mods, dev, what):
    """n3d_brain_scan, n3d_brain_hist and n3d_brain_robust of one subject and ONE host sync -> (rec int64 (Cm, REC_WORDS) on the
    host, the records as a ROBUST_DTYPE array (Cm,), the device tensor that holds the records for n3d_brain_zscore)"""
    if not isinstance(scheme, ZScore):
        raise N3DError("%s: scheme must be a preprocess.ZScore (got %r)" % (what, scheme))
    Cm, X, Y, Z = (int(s) for s in r.shape)
    if Cm != len(mods):
        raise N3DError("%s: raw has %d modalities, mods names %d" % (what, Cm, len(mods)))
    # one buffer, one copy each way: Cm robust records, then the scan's records (two int32 per word)
    init = np.zeros(Cm * (ROBUST_WORDS + REC_WORDS // 2), np.int64)
    init[Cm * ROBUST_WORDS:].view(np.int32)[:] = np.tile(np.array(_REC_INIT, np.int32), Cm)
    buf = torch.from_numpy(init).to(dev)
    rob, rec = buf[:Cm * ROBUST_WORDS], buf[Cm * ROBUST_WORDS:].view(torch.int32).view(Cm, REC_WORDS)
    hist = torch.empty((Cm, HIST_BINS), dtype=torch.int32, device=dev)
    _scan(lib, r, torch.zeros((Cm, 2), dtype=torch.int64, device=dev), rec)
    check(lib.n3d_brain_hist(K.ptr(r), Cm, X, Y, Z, K.ptr(rec), K.ptr(hist), K.stream_ptr()), "n3d_brain_hist")
    check(lib.n3d_brain_robust(K.ptr(hist), Cm, scheme.lower, scheme.upper, K.ptr(rob), K.stream_ptr()), "n3d_brain_robust")
    host = buf.cpu().numpy()                                   # the one sync
    h = host[Cm * ROBUST_WORDS:].view(np.int32).reshape(Cm, REC_WORDS).astype(np.int64)
    for c, m in enumerate(mods):
        if h[c, 5] < 0:
            raise N3DError("%s: modality %s has no nonzero voxel" % (what, m))
    return h, host[:Cm * ROBUST_WORDS].view(ROBUST_DTYPE), rob


def subject_stats(raw, scheme, mods=MODS, device=None):
    """what ZScore normalisation of this subject rests on, per modality (a tuple of SubjectStats in the order of mods): the brain
    voxels' count, the four order statistics around the two percentiles, the bounds, the voxels clipped at either end and the mean
    and std of the clipped counts, as n3d_brain_robust formed them.  One host sync."""
    dev, lib = _device(device), _lib.load()
    r = _raw(raw, dev, "subject_stats")
    _, rr, _ = _robust(lib, r, scheme, mods, dev, "subject_stats")
    return tuple(SubjectStats(int(q["count"]), tuple(int(v) for v in q["order"]), np.float64(q["lower"]), np.float64(q["upper"]),
                              int(q["n_below"]), int(q["n_above"]), np.float64(q["mean"]), np.float64(q["std"])) for q in rr)


def _normalize_zscore(lib, r, t, scheme, mods, dev):
    Cm, X, Y, Z = (int(s) for s in r.shape)
    h, rr, rob = _robust(lib, r, scheme, mods, dev, "normalize_subject")
    for c, m in enumerate(mods):
        if rr[c]["count"] < 2:
            raise N3DError("normalize_subject: modality %s has %d nonzero voxel: z-scoring needs at least two" % (m, rr[c]["count"]))
        if not rr[c]["std"] > 0:
            raise N3DError("normalize_subject: modality %s has a single value (%g) after clipping to [%g, %g]: std == 0, the z-score "
                           "is 0 / 0" % (m, rr[c]["mean"], rr[c]["lower"], rr[c]["upper"]))
    brain_width, hi = _box(h, np.array([X, Y, Z], np.int64))
    b = [int(v) for v in hi - brain_width[0]]
    out = torch.empty((Cm, *b), dtype=torch.float32, device=dev)
    t_out = torch.empty(b, dtype=torch.uint8, device=dev) if t is not None else None
    check(lib.n3d_brain_zscore(K.ptr(r), Cm, X, Y, Z, K.ptr(rob), (C.c_int32 * 3)(*[int(v) for v in brain_width[0]]),
                               (C.c_int32 * 3)(*[int(v) for v in hi]), K.ptr(out), K.ptr(t), K.ptr(t_out), K.stream_ptr()),
          "n3d_brain_zscore")
    return out, t_out, brain_width


def normalize_subject(raw, mean_std, truth=None, mods=MODS, device=None, scheme=None):
    """raw (Cm, X, Y, Z) int16, truth (X, Y, Z) or (1, X, Y, Z) uint8 or None -> (box_volume, box_truth, brain_width):
    box_volume (Cm, bx, by, bz) fp32 device tensor, the normalised modalities (create_h5:58-60) cropped to the box the reference
    reads back (patches.py:140-142: start : end + 1, clipped to the image); box_truth the same crop of truth (None without);
    brain_width the (2, 3) int64 array create_h5:63-65 stores -- its end row equals the image size on an axis where the brain
    touches the high face.  One host sync (the outlines decide the size of the box).
    scheme: None -- the reference's rule with the dictionary mean_std; a ZScore -- that rule from the subject alone (mean_std must
    be None), same box, same brain_width, nonzero exactly where raw is."""
    dev, lib = _device(device), _lib.load()
    r = _raw(raw, dev, "normalize_subject")
    Cm, X, Y, Z = (int(s) for s in r.shape)
    if scheme is not None:
        if mean_std is not None:
            raise N3DError("normalize_subject: a scheme takes its statistics from the subject: give mean_std or scheme, not both")
        return _normalize_zscore(lib, r, _truth(truth, X, Y, Z, dev), scheme, mods, dev)
    if mean_std is None:
        raise N3DError("normalize_subject: needs the mean / std dictionary of cal_mean_std, or a scheme (preprocess.ZScore)")
    if Cm != len(mods):
        raise N3DError("normalize_subject: raw has %d modalities, mods names %d" % (Cm, len(mods)))
    ms = np.array([[np.float64(mean_std["%s_mean" % m]), np.float64(mean_std["%s_std" % m])] for m in mods], np.float64)
    t = _truth(truth, X, Y, Z, dev)
    ms_d = torch.from_numpy(ms).to(dev)
    rec = _records(1, Cm, dev)[0]
    _scan(lib, r, torch.zeros((Cm, 2), dtype=torch.int64, device=dev), rec)
    h = rec.cpu().numpy().astype(np.int64)                     # the one sync
    shape = np.array([X, Y, Z], np.int64)
    for c, m in enumerate(mods):
        if h[c, 5] < 0:
            raise N3DError("normalize_subject: modality %s has no nonzero voxel (the reference's np.min raises on the empty "
                           "selection)" % m)
        z = (h[c, :2].astype(np.float64) - ms[c, 0]) / ms[c, 1]
        if not z[1] > z[0]:
            raise N3DError("normalize_subject: modality %s has a single nonzero value (%d): zmax == zmin, the min-max quotient "
                           "is 0 / 0" % (m, h[c, 0]))
    brain_width, hi = _box(h, shape)
    start = brain_width[0]
    b = [int(v) for v in hi - start]
    out = torch.empty((Cm, *b), dtype=torch.float32, device=dev)
    t_out = torch.empty(b, dtype=torch.uint8, device=dev) if t is not None else None
    check(lib.n3d_brain_normalize(K.ptr(r), Cm, X, Y, Z, K.ptr(ms_d), K.ptr(rec), (C.c_int32 * 3)(*[int(v) for v in start]),
                                  (C.c_int32 * 3)(*[int(v) for v in hi]), K.ptr(out), K.ptr(t), K.ptr(t_out), K.stream_ptr()),
          "n3d_brain_normalize")
    return out, t_out, brain_width
