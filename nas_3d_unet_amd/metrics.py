"""The last step of the reference's workflow: a predicted label volume scored against the truth per region -- the Dice,
Sensitivity, Specificity and Hausdorff95 columns of the BraTS portal's CSV that plot.py:151-173 (evaluation_plot / draw_evaluate)
draws -- without the labels leaving the device.  The reference has no code for the metrics; the definitions (include/n3d.h,
"Segmentation metrics") are the portal's and medpy.metric.binary.hd95's at unit voxel spacing:

  * labels uint8 {0, 1, 2, 4}; regions in tr.eval_result()'s order: WT = label != 0, TC = label in {1, 4}, ET = label == 4;
  * TP / FP / FN counted over the full image, TN = voxels - TP - FP - FN; Dice = 2TP / (2TP + FP + FN), Sensitivity = TP / (TP + FN),
    Specificity = TN / (TN + FP), formed here in fp64 from the integers; a zero denominator gives NaN, except Dice = 1 when both
    masks are empty;
  * surface = mask & ~binary_erosion(mask, 6-neighbourhood, border_value=0); HD95 = np.percentile(., 95) of the distances from every
    surface voxel of one mask to the other mask's surface, both directions concatenated; 0 when both masks are empty, NaN when
    exactly one is.  Squared distances are integers, so the device hands over integers only (n, two order statistics, the
    maximum) and finish() below interpolates exactly as numpy does.

score_labels enqueues four kernels' worth of work (n3d_seg_regions, n3d_seg_edt -- three launches --, n3d_seg_sample,
n3d_seg_order) and makes ONE host sync: the copy of a 240-byte record.  Scratch is allocated once per image shape and device and
reused across subjects.  No CPU fallback: a host tensor is an error."""
from __future__ import annotations

import csv
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import N3DError, check

REGIONS = ("WT", "TC", "ET")
CRITERIA = ("Dice", "Sensitivity", "Specificity", "Hausdorff95")
# the portal's column order: per criterion ET, WT, TC
COLUMNS = ("Label",) + tuple("%s_%s" % (c, r) for c in CRITERIA for r in ("ET", "WT", "TC"))
SUMMARY_ROWS = ("Mean", "StdDev", "Median", "25quantile", "75quantile")

INF = 1 << 29            # N3D_SEG_INF
MAX_AXIS = 1024          # N3D_SEG_MAX_AXIS
REC_WORDS, REC_ORDER, REC_BBOX = 30, 9, 21   # N3D_SEG_REC_*
_I32_MAX = 2 ** 31 - 1


# ---- host: pure numpy, needs neither a GPU nor the library

def _ratio(num, den):
    return float(np.float64(num) / np.float64(den)) if den else float("nan")


def hd_from_order(n, d2_lo, d2_hi):
    """np.percentile(sqrt(D), 95) (linear interpolation) from n = len(D) > 0 and the order statistics d2_lo = D[k],
    d2_hi = D[min(k + 1, n - 1)] of the sorted squared distances, k = floor((n - 1) * 0.95): numpy's own operations in its order
    (virtual index (n - 1) * q, gamma = index - floor, then its lerp with the t >= 0.5 form)."""
    vi = np.float64(n - 1) * np.float64(0.95)
    t = vi - np.floor(vi)
    lo, hi = np.sqrt(np.float64(d2_lo)), np.sqrt(np.float64(d2_hi))
    diff = hi - lo
    return float(hi - diff * (1 - t)) if t >= 0.5 else float(lo + diff * t)


def finish(counts, n_voxels, order):
    """counts: (3, 3) integers [region][TP, FP, FN]; n_voxels: voxels of the image; order: (3, 4) integers [region][n, D[k],
    D[k + 1], max D] -> {region: {dice, sensitivity, specificity, hausdorff95, tp, fp, fn, tn, n_surface, hausdorff100}}."""
    counts = np.asarray(counts, dtype=np.int64).reshape(3, 3)
    order = np.asarray(order, dtype=np.int64).reshape(3, 4)
    out = {}
    for r, name in enumerate(REGIONS):
        tp, fp, fn = (int(v) for v in counts[r])
        tn = int(n_voxels) - tp - fp - fn
        n, d_lo, d_hi, d_max = (int(v) for v in order[r])
        pred_empty, truth_empty = tp + fp == 0, tp + fn == 0
        if pred_empty and truth_empty:
            dice, hd95, hd100 = 1.0, 0.0, 0.0
        else:
            dice = _ratio(2 * tp, 2 * tp + fp + fn)
            if pred_empty or truth_empty or n == 0:
                hd95 = hd100 = float("nan")
            else:
                hd95, hd100 = hd_from_order(n, d_lo, d_hi), float(np.sqrt(np.float64(d_max)))
        out[name] = {"dice": dice, "sensitivity": _ratio(tp, tp + fn), "specificity": _ratio(tn, tn + fp), "hausdorff95": hd95,
                     "tp": tp, "fp": fp, "fn": fn, "tn": tn, "n_surface": n, "hausdorff100": hd100}
    return out


def row_of(label, scores):
    """one CSV row (a dict keyed by COLUMNS) from a score_labels result"""
    row = {"Label": label}
    for c in CRITERIA:
        for r in REGIONS:
            row["%s_%s" % (c, r)] = scores[r][c.lower()]
    return row


def summary_rows(rows):
    """the portal's five trailing rows over `rows`, NaN entries left out (an all-NaN column stays NaN)"""
    out = [{"Label": s} for s in SUMMARY_ROWS]
    for col in COLUMNS[1:]:
        v = np.array([r[col] for r in rows], dtype=np.float64)
        v = v[~np.isnan(v)]
        if v.size:
            vals = (v.mean(), v.std(), np.median(v), np.percentile(v, 25), np.percentile(v, 75))
        else:
            vals = (float("nan"),) * 5
        for o, x in zip(out, vals):
            o[col] = float(x)
    return out


def write_csv(path, rows):
    """rows (score_set's) followed by Mean, StdDev, Median, 25quantile, 75quantile: the file evaluation_plot reads (its [:-5]
    strips exactly those five).  NaN is written as an empty field, which pandas reads back as NaN."""
    rows = list(rows)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(COLUMNS)
        for r in rows + summary_rows(rows):
            w.writerow([r["Label"]] + ["" if math.isnan(r[c]) else repr(float(r[c])) for c in COLUMNS[1:]])


# ---- device

class _Workspace:
    def __init__(self, lib, device, full):
        off = (C.c_int64 * 5)()
        nbytes = int(lib.n3d_seg_workspace_bytes(full[0], full[1], full[2], off))
        if nbytes == 0:
            raise N3DError("metrics: image shape %s: needs 1 <= FX * FY * FZ < 2^31" % (tuple(full),))
        n = full[0] * full[1] * full[2]
        self.hist_len = int(off[4])
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.rec = self.buf[off[0]:off[0] + REC_WORDS * 8].view(torch.int64)
        self.flags = self.buf[off[1]:off[1] + n].view(full)
        self.dist = self.buf[off[2]:off[2] + 6 * n * 4].view(torch.int32)
        self.hist = self.buf[off[3]:off[3] + 3 * self.hist_len * 4].view(torch.int32)
        self.rec_init = _rec_init(device)


_workspaces = {}


def _rec_init(device):
    bbox = np.array([_I32_MAX] * 3 + [-1] * 3, dtype=np.int32)
    rec = np.zeros(REC_WORDS, dtype=np.int64)
    rec[REC_BBOX:] = np.tile(bbox, 3).view(np.int64)
    return torch.from_numpy(rec).to(device)


def _i3(v):
    return (C.c_int32 * 3)(*[int(x) for x in v])


def _labels(t, what, name):
    if not (isinstance(t, torch.Tensor) and t.dim() == 3 and t.dtype == torch.uint8 and t.is_cuda):
        raise N3DError("%s: %s must be a (X, Y, Z) uint8 label volume on a HIP device (got %s); there is no CPU fallback" % (
            what, name, "%s %s on %s" % (tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t).__name__))
    if t.numel() == 0:
        raise N3DError("%s: %s is empty: shape %s" % (what, name, tuple(t.shape)))
    return t.contiguous()


def _geometry(pred, truth, origin, what):
    pred, truth = _labels(pred, what, "pred"), _labels(truth, what, "truth")
    if truth.device != pred.device:
        raise N3DError("%s: pred is on %s, truth on %s" % (what, pred.device, truth.device))
    full, box = tuple(int(s) for s in pred.shape), tuple(int(s) for s in truth.shape)
    org = (0, 0, 0) if origin is None else tuple(int(o) for o in origin)
    if len(org) != 3 or any(o < 0 or o + b > f for o, b, f in zip(org, box, full)) or (origin is None and box != full):
        raise N3DError("%s: the truth box %s at %s is not inside the image %s%s" % (
            what, box, org, full, "" if origin is not None else " (no origin: the box must be the image)"))
    if full[0] * full[1] * full[2] >= 2 ** 31:
        raise N3DError("%s: image %s: needs FX * FY * FZ < 2^31" % (what, full))
    return pred, truth, full, box, org


def _regions(lib, pred, truth, full, box, org, flags, rec):
    check(lib.n3d_seg_regions(K.ptr(pred), K.ptr(truth), _i3(full), _i3(box), _i3(org), K.ptr(flags), K.ptr(rec), K.stream_ptr()),
          "n3d_seg_regions")


def surfaces_and_counts(pred, truth, origin=None):
    """pred: (FX, FY, FZ) uint8 device labels; truth: (X, Y, Z) uint8 device labels, the box at `origin` inside the image (None:
    the box is the image) -> (flags uint8 (FX, FY, FZ): bits 0..2 the prediction's surface of WT / TC / ET, bits 3..5 the truth's;
    counts int64 (3, 3) [region][TP, FP, FN]), both on the device.  One launch, no host sync."""
    pred, truth, full, box, org = _geometry(pred, truth, origin, "surfaces_and_counts")
    flags = torch.empty(full, dtype=torch.uint8, device=pred.device)
    rec = _rec_init(pred.device)
    _regions(_lib.load(), pred, truth, full, box, org, flags, rec)
    return flags, rec[:9].view(3, 3)


def edt_sq(mask):
    """mask: (X, Y, Z) uint8 or bool device tensor -> int32 (X, Y, Z): the squared Euclidean distance from every voxel to the
    nearest nonzero voxel of mask (0 on it), INF = 2^29 everywhere for an empty mask.  Exact.  Axes up to 1024."""
    if not (isinstance(mask, torch.Tensor) and mask.dim() == 3 and mask.dtype in (torch.uint8, torch.bool) and mask.is_cuda
            and mask.numel() > 0):
        raise N3DError("edt_sq: mask must be a non-empty (X, Y, Z) uint8 or bool tensor on a HIP device (got %s); there is no CPU "
                     "fallback" % ("%s %s on %s" % (tuple(mask.shape), mask.dtype, mask.device) if isinstance(mask, torch.Tensor)
                                   else type(mask).__name__))
    full = tuple(int(s) for s in mask.shape)
    if full[0] * full[1] * full[2] >= 2 ** 31:
        raise N3DError("edt_sq: mask %s: needs X * Y * Z < 2^31" % (full,))
    flags = (mask != 0).to(torch.uint8).contiguous()
    bbox = torch.tensor([0, 0, 0, full[0] - 1, full[1] - 1, full[2] - 1], dtype=torch.int32, device=mask.device)
    dist = torch.empty(full, dtype=torch.int32, device=mask.device)
    check(_lib.load().n3d_seg_edt(K.ptr(flags), 1, 1, _i3(full), K.ptr(bbox), K.ptr(dist), K.stream_ptr()), "n3d_seg_edt")
    return dist


def score_record(pred, truth, origin=None):
    """the device work of score_labels: -> (record int64 (30,) numpy array as include/n3d.h lays it out, voxels of the image).
    The subject's one host sync is the copy of the record."""
    pred, truth, full, box, org = _geometry(pred, truth, origin, "score_labels")
    if max(full) > MAX_AXIS:
        raise N3DError("score_labels: image %s: the distance transform takes axes up to %d" % (full, MAX_AXIS))
    lib = _lib.load()
    key = (pred.device, full)
    ws = _workspaces.get(key)
    if ws is None:
        _workspaces.clear()            # one shape at a time: the scratch of a full-size image is 24 bytes per voxel
        ws = _workspaces[key] = _Workspace(lib, pred.device, full)
    ws.rec.copy_(ws.rec_init)
    check(lib.n3d_zero(K.ptr(ws.hist), ws.hist.numel() * 4, K.stream_ptr()), "n3d_zero")
    _regions(lib, pred, truth, full, box, org, ws.flags, ws.rec)
    f3 = _i3(full)
    bbox = C.c_void_p(ws.rec.data_ptr() + REC_BBOX * 8)
    check(lib.n3d_seg_edt(K.ptr(ws.flags), 6, 3, f3, bbox, K.ptr(ws.dist), K.stream_ptr()), "n3d_seg_edt")
    check(lib.n3d_seg_sample(K.ptr(ws.flags), f3, bbox, K.ptr(ws.dist), K.ptr(ws.hist), ws.hist_len, K.stream_ptr()), "n3d_seg_sample")
    check(lib.n3d_seg_order(K.ptr(ws.hist), ws.hist_len, K.ptr(ws.rec), K.stream_ptr()), "n3d_seg_order")
    return ws.rec.cpu().numpy(), full[0] * full[1] * full[2]


def score_labels(pred, truth, origin=None):
    """pred: (FX, FY, FZ) uint8 device labels (what the predictors return); truth: (X, Y, Z) uint8 device labels at `origin`
    inside the image (None: the box is the image) -> {region: {"dice", "sensitivity", "specificity", "hausdorff95", "tp", "fp",
    "fn", "tn", "n_surface", "hausdorff100"}} for region in REGIONS.  One host sync."""
    rec, n = score_record(pred, truth, origin)
    return finish(rec[:9].reshape(3, 3), n, rec[REC_ORDER:REC_BBOX].reshape(3, 4))


def score_subject(volumes, index, labels):
    """labels (a predictor's output for volumes[index]) against volumes.truths[index] at volumes.origins[index]"""
    index = int(index)
    if not 0 <= index < len(volumes):
        raise N3DError("score_subject: volume index %d outside the set of %d" % (index, len(volumes)))
    truth = volumes.truths[index]
    if truth is None:
        raise N3DError("score_subject: the set has no truth to score against")
    origin = volumes.origins[index]
    box = tuple(int(s) for s in truth.shape)
    org = (0, 0, 0) if origin is None else tuple(int(o) for o in origin)
    shape = tuple(int(s) for s in getattr(labels, "shape", ()))
    if len(shape) != 3 or any(o + b > f for o, b, f in zip(org, box, shape)) or (origin is None and shape != box):
        raise N3DError("score_subject: labels of shape %s do not hold subject %d's box %s at %s" % (shape, index, box, org))
    return score_labels(labels, truth, origin)


def score_set(predictor, volumes, indices, names=None, **predict_kw):
    """predictor.predict(volumes, i, **predict_kw)[0] scored per index -> rows (dicts keyed by COLUMNS; Label = names[j] or the
    index) for write_csv"""
    indices = list(indices)
    if names is not None and len(names) != len(indices):
        raise N3DError("score_set: %d names for %d indices" % (len(names), len(indices)))
    rows = []
    for j, i in enumerate(indices):
        labels = predictor.predict(volumes, i, **predict_kw)[0]
        rows.append(row_of(str(names[j]) if names is not None else str(i), score_subject(volumes, i, labels)))
    return rows
