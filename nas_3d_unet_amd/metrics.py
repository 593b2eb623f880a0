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
reused across subjects.  No CPU fallback: a host tensor is an error.

Lesion-wise scores (BraTS 2023; include/n3d.h, "Lesion-wise metrics"): the truth's region mask is dilated `dilation` times with the
18-neighbourhood, the 26-connected components of the dilated mask are the lesions, and every lesion is scored against the predicted
components that touch its dilated component; a predicted component that touches none is a false positive, a case of Dice 0 and
HD95 `penalty_hd95`.  lesion_record enqueues n3d_lw_score's fixed 47 launches and makes ONE host sync, the copy of a 14 KB integer
record; finish_lesions folds it in fp64 on the host."""
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
LESION_CRITERIA = ("LesionWise_Dice", "LesionWise_Hausdorff95")
LESION_COLUMNS = tuple("%s_%s" % (c, r) for c in LESION_CRITERIA for r in ("ET", "WT", "TC"))

INF = 1 << 29            # N3D_SEG_INF
MAX_AXIS = 1024          # N3D_SEG_MAX_AXIS
REC_WORDS, REC_ORDER, REC_BBOX = 30, 9, 21   # N3D_SEG_REC_WORDS / N3D_SEG_REC_ORDER / N3D_SEG_REC_BBOX
_I32_MAX = 2 ** 31 - 1
# the lesion-wise limits and record layout of include/n3d.h
LW_MAX_DILATION, LW_MAX_LESIONS, LW_MAX_SURFACE, LW_MAX_AXIS = 5, 64, 1 << 18, 1024   # N3D_LW_MAX_DILATION / N3D_LW_MAX_LESIONS / N3D_LW_MAX_SURFACE / N3D_LW_MAX_AXIS
LW_HEADER_WORDS, LW_ROW_WORDS = 8, 9   # N3D_LW_HEADER_WORDS / N3D_LW_ROW_WORDS
LW_REGION_WORDS = LW_HEADER_WORDS + LW_MAX_LESIONS * LW_ROW_WORDS   # N3D_LW_REGION_WORDS
LW_REC_WORDS = 3 * LW_REGION_WORDS   # N3D_LW_REC_WORDS
LW_PHASES = 35   # N3D_LW_PHASES
LW_REGION_PHASES = ("select", "label_pred", "dilate", "label_truth", "roots", "ranks", "match", "components", "surfaces", "distances", "order")   # N3D_LW_REGION_PHASES names, in order
_LW_OVERFLOW = ((1, "N3D_LW_MAX_LESIONS = %d lesions" % LW_MAX_LESIONS),
                (2, "N3D_LW_MAX_SURFACE = %d surface entries of the truth" % LW_MAX_SURFACE),
                (4, "N3D_LW_MAX_SURFACE = %d surface entries of the prediction" % LW_MAX_SURFACE))


# ---- host: pure numpy, needs neither a GPU nor the library

def _ratio(num, den):
    return float(np.float64(num) / np.float64(den)) if den else float("nan")


def percentile_index(n, q):
    """(k, t) of np.percentile's linear method over n > 0 sorted values: virtual index (n - 1) * (q / 100), k its floor,
    t = index - k (numpy's gamma)"""
    vi = np.float64(n - 1) * (np.float64(q) / np.float64(100.0))
    k = np.floor(vi)
    return int(k), vi - k


def percentile_from_order(n, q, lo, hi):
    """np.percentile(a, q) (linear interpolation) from n = len(a) > 0 and the order statistics lo = a[k], hi = a[min(k + 1, n - 1)]
    of the sorted values, (k, t) = percentile_index(n, q): numpy's own operations in its order (its lerp with the t >= 0.5 form)"""
    t = percentile_index(n, q)[1]
    lo, hi = np.float64(lo), np.float64(hi)
    diff = hi - lo
    return float(hi - diff * (1 - t)) if t >= 0.5 else float(lo + diff * t)


def hd_from_order(n, d2_lo, d2_hi):
    """np.percentile(sqrt(D), 95) from n = len(D) > 0 and the order statistics d2_lo = D[k], d2_hi = D[min(k + 1, n - 1)] of the
    sorted squared distances, k = floor((n - 1) * 0.95) (95 / 100 rounds to the double 0.95)"""
    return percentile_from_order(n, 95, np.sqrt(np.float64(d2_lo)), np.sqrt(np.float64(d2_hi)))


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


def summary_rows(rows, columns=COLUMNS):
    """the portal's five trailing rows over `rows`, NaN entries left out (an all-NaN column stays NaN)"""
    out = [{"Label": s} for s in SUMMARY_ROWS]
    for col in columns[1:]:
        v = np.array([r[col] for r in rows], dtype=np.float64)
        v = v[~np.isnan(v)]
        if v.size:
            vals = (v.mean(), v.std(), np.median(v), np.percentile(v, 25), np.percentile(v, 75))
        else:
            vals = (float("nan"),) * 5
        for o, x in zip(out, vals):
            o[col] = float(x)
    return out


def write_csv(path, rows, columns=COLUMNS):
    """rows (score_set's) followed by Mean, StdDev, Median, 25quantile, 75quantile: the file evaluation_plot reads (its [:-5]
    strips exactly those five).  NaN is written as an empty field, which pandas reads back as NaN.  columns: COLUMNS, or
    COLUMNS + LESION_COLUMNS for rows of score_set(..., lesionwise=True); keys of a row that are no column are not written."""
    rows, columns = list(rows), tuple(columns)
    if not columns or columns[0] != "Label":
        raise N3DError("write_csv: the first column must be Label (got %s)" % (columns[:1],))
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(columns)
        for r in rows + summary_rows(rows, columns):
            w.writerow([r["Label"]] + ["" if math.isnan(r[c]) else repr(float(r[c])) for c in columns[1:]])


def finish_lesions(record, min_lesion_voxels=50, penalty_hd95=374.0):
    """record: the int64 words of n3d_lw_score (include/n3d.h) -> {region: {"lesionwise_dice", "lesionwise_hausdorff95",
    "n_lesions", "n_kept", "n_fn", "n_fp", "fp_voxels", "lesions": [{"id", "gt_voxels", "pred_voxels", "tp", "n_matched", "dice",
    "hausdorff95", "hausdorff100"}, ...]}}.  Lesions are listed by ascending id, all of them; the kept ones are those with
    gt_voxels > min_lesion_voxels.  A lesion without a matched component has Dice 0 and both distances penalty_hd95.  The sums
    run over the kept lesions in that order, one fp64 addition each; den = kept lesions + false positives; den == 0 gives Dice 1
    and HD95 0.  An overflow bit in the record raises N3DError."""
    if isinstance(min_lesion_voxels, bool) or int(min_lesion_voxels) != min_lesion_voxels or min_lesion_voxels < 0:
        raise N3DError("finish_lesions: min_lesion_voxels %r: must be an integer >= 0" % (min_lesion_voxels,))
    penalty = float(penalty_hd95)
    if math.isnan(penalty) or penalty < 0:
        raise N3DError("finish_lesions: penalty_hd95 %r: must be a number >= 0" % (penalty_hd95,))
    record = np.asarray(record)
    if record.size != LW_REC_WORDS or record.dtype.kind not in "iu":
        raise N3DError("finish_lesions: the record must hold %d integers (got %s of %s)" % (LW_REC_WORDS, record.shape, record.dtype))
    record = record.astype(np.int64).reshape(3, LW_REGION_WORDS)
    out = {}
    for r, name in enumerate(REGIONS):
        n_lesions, _, n_fp, fp_voxels, overflow = (int(v) for v in record[r, :5])
        for bit, what in _LW_OVERFLOW:
            if overflow & bit:
                raise N3DError("finish_lesions: region %s holds more than %s%s" % (
                    name, what, " (%d)" % n_lesions if bit == 1 else ""))
        if not 0 <= n_lesions <= LW_MAX_LESIONS:
            raise N3DError("finish_lesions: region %s: n_lesions %d outside 0 .. %d" % (name, n_lesions, LW_MAX_LESIONS))
        rows = record[r, LW_HEADER_WORDS:].reshape(LW_MAX_LESIONS, LW_ROW_WORDS)
        lesions, n_kept, n_fn = [], 0, 0
        dice_sum, hd_sum = np.float64(0.0), np.float64(0.0)
        for row in rows[:n_lesions]:
            lid, gt, tp, pv, nm, n, d_lo, d_hi, d_max = (int(v) for v in row)
            if nm > 0 and n > 0:
                dice, hd95, hd100 = _ratio(2 * tp, pv + gt), hd_from_order(n, d_lo, d_hi), float(np.sqrt(np.float64(d_max)))
            else:
                dice, hd95, hd100 = 0.0, penalty, penalty
            lesions.append({"id": lid, "gt_voxels": gt, "pred_voxels": pv, "tp": tp, "n_matched": nm, "dice": dice,
                            "hausdorff95": hd95, "hausdorff100": hd100})
            if gt > min_lesion_voxels:
                n_kept += 1
                n_fn += nm == 0
                dice_sum = dice_sum + np.float64(dice)
                hd_sum = hd_sum + np.float64(hd95)
        den = n_kept + n_fp
        if den == 0:
            lw_dice, lw_hd = 1.0, 0.0
        else:
            lw_dice = float(dice_sum / np.float64(den))
            lw_hd = float((hd_sum + np.float64(penalty) * np.float64(n_fp)) / np.float64(den))
        out[name] = {"lesionwise_dice": lw_dice, "lesionwise_hausdorff95": lw_hd, "n_lesions": n_lesions, "n_kept": n_kept,
                     "n_fn": int(n_fn), "n_fp": n_fp, "fp_voxels": fp_voxels, "lesions": lesions}
    return out


def lesion_columns_of(lesion_scores):
    """the six LESION_COLUMNS entries of a finish_lesions result"""
    return {"%s_%s" % (c, r): lesion_scores[r][c.lower()] for c in LESION_CRITERIA for r in REGIONS}


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


class _LesionWorkspace:
    def __init__(self, lib, device, full):
        nbytes = int(lib.n3d_lw_workspace_bytes(full[0], full[1], full[2], None))
        if nbytes == 0:
            raise N3DError("lesion_record: image shape %s: needs 1 <= FX * FY * FZ < 2^31" % (tuple(full),))
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)


_lesion_workspaces = {}


def _check_dilation(dilation, what):
    if isinstance(dilation, bool) or not isinstance(dilation, (int, np.integer)) or not 0 <= dilation <= LW_MAX_DILATION:
        raise N3DError("%s: dilation %r: must be an integer in 0 .. %d" % (what, dilation, LW_MAX_DILATION))
    return int(dilation)


def dilate_mask(mask, iterations=3):
    """mask: (X, Y, Z) uint8 or bool device tensor -> uint8 (X, Y, Z), 1 where scipy.ndimage.binary_dilation(mask != 0,
    generate_binary_structure(3, 2), iterations=iterations) is set (border value 0; 0 iterations: the mask itself as 0 / 1).
    One launch, no host sync.  0 <= iterations <= 5."""
    if not (isinstance(mask, torch.Tensor) and mask.dim() == 3 and mask.dtype in (torch.uint8, torch.bool) and mask.is_cuda
            and mask.numel() > 0):
        raise N3DError("dilate_mask: mask must be a non-empty (X, Y, Z) uint8 or bool tensor on a HIP device (got %s); there is no CPU "
                       "fallback" % ("%s %s on %s" % (tuple(mask.shape), mask.dtype, mask.device) if isinstance(mask, torch.Tensor)
                                     else type(mask).__name__))
    iterations = _check_dilation(iterations, "dilate_mask")
    full = tuple(int(s) for s in mask.shape)
    if full[0] * full[1] * full[2] >= 2 ** 31:
        raise N3DError("dilate_mask: mask %s: needs X * Y * Z < 2^31" % (full,))
    src = (mask.view(torch.uint8) if mask.dtype == torch.bool else mask).contiguous()
    out = torch.empty(full, dtype=torch.uint8, device=mask.device)
    check(_lib.load().n3d_lw_dilate(K.ptr(src), _i3(full), None, iterations, K.ptr(out), K.stream_ptr()), "n3d_lw_dilate")
    return out


def _lesion_setup(pred, truth, origin, dilation):
    pred, truth, full, box, org = _geometry(pred, truth, origin, "lesion_record")
    dilation = _check_dilation(dilation, "lesion_record")
    if max(full) > LW_MAX_AXIS:
        raise N3DError("lesion_record: image %s: the packed surface coordinates take axes up to %d" % (full, LW_MAX_AXIS))
    lib = _lib.load()
    key = (pred.device, full)
    ws = _lesion_workspaces.get(key)
    if ws is None:
        _lesion_workspaces.clear()     # one shape at a time: the scratch of a full-size image is 28 bytes per voxel
        ws = _lesion_workspaces[key] = _LesionWorkspace(lib, pred.device, full)
    return lib, pred, truth, full, box, org, dilation, ws


def lesion_phases(pred, truth, origin=None, dilation=3, first=0, last=LW_PHASES - 1, rec=None):
    """the phases first .. last of n3d_lw_score (include/n3d.h, n3d_lw_phases) on the shared scratch, for timing -> the device
    record (int64, LW_REC_WORDS)"""
    lib, pred, truth, full, box, org, dilation, ws = _lesion_setup(pred, truth, origin, dilation)
    if rec is None:
        rec = torch.empty(LW_REC_WORDS, dtype=torch.int64, device=pred.device)
    check(lib.n3d_lw_phases(int(first), int(last), K.ptr(pred), K.ptr(truth), _i3(full), _i3(box), _i3(org), dilation, K.ptr(ws.buf),
                            K.ptr(rec), K.stream_ptr()), "n3d_lw_phases")
    return rec


def lesion_record(pred, truth, origin=None, dilation=3):
    """the device work of score_lesions: -> (record int64 (LW_REC_WORDS,) numpy array as include/n3d.h lays it out, voxels of the
    image).  The subject's one host sync is the copy of the record."""
    lib, pred, truth, full, box, org, dilation, ws = _lesion_setup(pred, truth, origin, dilation)
    rec = torch.empty(LW_REC_WORDS, dtype=torch.int64, device=pred.device)
    check(lib.n3d_lw_score(K.ptr(pred), K.ptr(truth), _i3(full), _i3(box), _i3(org), dilation, K.ptr(ws.buf), K.ptr(rec), K.stream_ptr()),
          "n3d_lw_score")
    return rec.cpu().numpy(), full[0] * full[1] * full[2]


def score_lesions(pred, truth, origin=None, dilation=3, min_lesion_voxels=50, penalty_hd95=374.0):
    """pred, truth, origin as score_labels -> finish_lesions' result: the BraTS 2023 lesion-wise Dice and Hausdorff95 per region
    with the per-lesion figures.  One host sync."""
    if isinstance(min_lesion_voxels, bool) or int(min_lesion_voxels) != min_lesion_voxels or min_lesion_voxels < 0:
        raise N3DError("score_lesions: min_lesion_voxels %r: must be an integer >= 0" % (min_lesion_voxels,))
    return finish_lesions(lesion_record(pred, truth, origin, dilation)[0], min_lesion_voxels, penalty_hd95)


def score_subject(volumes, index, labels, lesionwise=False, **lesion_kw):
    """labels (a predictor's output for volumes[index]) against volumes.truths[index] at volumes.origins[index].  lesionwise: the
    result also carries the six LESION_COLUMNS (score_lesions with lesion_kw: dilation, min_lesion_voxels, penalty_hd95)."""
    if lesion_kw and not lesionwise:
        raise N3DError("score_subject: %s given without lesionwise=True" % sorted(lesion_kw))
    if set(lesion_kw) - {"dilation", "min_lesion_voxels", "penalty_hd95"}:
        raise N3DError("score_subject: unknown keywords %s" % sorted(set(lesion_kw) - {"dilation", "min_lesion_voxels", "penalty_hd95"}))
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
    scores = score_labels(labels, truth, origin)
    if lesionwise:
        scores.update(lesion_columns_of(score_lesions(labels, truth, origin, **lesion_kw)))
    return scores


def score_set(predictor, volumes, indices, names=None, lesionwise=False, dilation=3, min_lesion_voxels=50, penalty_hd95=374.0,
              **predict_kw):
    """predictor.predict(volumes, i, **predict_kw)[0] scored per index -> rows (dicts keyed by COLUMNS; Label = names[j] or the
    index) for write_csv.  lesionwise: the rows also carry LESION_COLUMNS (write_csv(path, rows, COLUMNS + LESION_COLUMNS)),
    scored with dilation, min_lesion_voxels and penalty_hd95."""
    indices = list(indices)
    if names is not None and len(names) != len(indices):
        raise N3DError("score_set: %d names for %d indices" % (len(names), len(indices)))
    rows = []
    for j, i in enumerate(indices):
        labels = predictor.predict(volumes, i, **predict_kw)[0]
        if lesionwise:
            scores = score_subject(volumes, i, labels, lesionwise=True, dilation=dilation, min_lesion_voxels=min_lesion_voxels,
                                   penalty_hd95=penalty_hd95)
        else:
            scores = score_subject(volumes, i, labels)
        row = row_of(str(names[j]) if names is not None else str(i), scores)
        if lesionwise:
            row.update({c: scores[c] for c in LESION_COLUMNS})
        rows.append(row)
    return rows
