"""The step between prediction (predict.py) and scoring (metrics.py): the predicted label volume is cleaned on the device -- no copy
to the host, no scipy.ndimage.label.  The reference has no code for it; the definitions (include/n3d.h, "Label clean-up") are
scipy's:

  * components of `labels != 0` at connectivity 6 / 18 / 26 = scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3); the id of a
    component is the smallest linear index (x * Y + y) * Z + z of its voxels, -1 on background;
  * step A: a component is kept iff size >= min_voxels and (not keep_largest or it is the largest; equal sizes: the smallest id);
    voxels of the others become 0; if the largest is smaller than min_voxels nothing is kept;
  * step B: e = label-4 voxels in kept components; if 0 < e < et_min_voxels they become 1 (e == et_min_voxels changes nothing).

clean_labels enqueues six launches (n3d_cc_clean) and makes no host sync unless the statistics are asked for (one copy of an
80-byte record).  Scratch is allocated once per image shape and device and reused across subjects: 17 bytes per voxel (parent,
component id, per-root size and label-4 count as int32, a verdict byte).  No CPU fallback: a host tensor is an error."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import N3DError, check

CONNECTIVITIES = (6, 18, 26)
# N3D_CC_REC_*: the record's int64 words
REC_WORDS = 10   # N3D_CC_REC_WORDS
REC_COMPONENTS, REC_KEPT, REC_VOXELS_IN, REC_VOXELS_KEPT, REC_LARGEST_SIZE, REC_LARGEST_ID, REC_ET_IN, REC_ET_KEPT, REC_ET_RELABELLED, \
    REC_PACKED = range(10)   # N3D_CC_REC_COMPONENTS / N3D_CC_REC_KEPT / N3D_CC_REC_VOXELS_IN / N3D_CC_REC_VOXELS_KEPT / N3D_CC_REC_LARGEST_SIZE / N3D_CC_REC_LARGEST_ID / N3D_CC_REC_ET_IN / N3D_CC_REC_ET_KEPT / N3D_CC_REC_ET_RELABELLED / N3D_CC_REC_PACKED
PHASES = ("local", "merge", "flatten", "decide_max", "decide_keep", "apply")     # N3D_CC_PHASES launches, in order
TILED, GLOBAL_ONLY = 0, 1                                                       # N3D_CC_TILED / N3D_CC_GLOBAL_ONLY
STAT_KEYS = ("n_components", "n_kept", "voxels_in", "voxels_kept", "largest_size", "largest_id", "et_in", "et_kept", "et_relabelled")


# ---- host: needs neither a GPU nor the library

def stats_of(record):
    """record: the REC_WORDS int64 words n3d_cc_clean leaves (array, list or tensor on the host) -> the statistics dict"""
    rec = np.asarray(record.cpu() if isinstance(record, torch.Tensor) else record)
    if rec.shape != (REC_WORDS,) or rec.dtype.kind not in "iu":
        raise N3DError("stats_of: the record is %d int64 words (got shape %s %s)" % (REC_WORDS, rec.shape, rec.dtype))
    out = {k: int(rec[i]) for i, k in enumerate(STAT_KEYS)}
    out["et_relabelled"] = bool(out["et_relabelled"])
    return out


def _describe(t):
    return "%s %s on %s" % (tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t).__name__


def _volume(t, what, name, dtypes):
    kinds = " or ".join(str(d).replace("torch.", "") for d in dtypes)
    if isinstance(t, torch.Tensor) and t.dim() == 3 and t.numel() >= 2 ** 31:      # the int32 component ids
        raise N3DError("%s: %s %s: needs X * Y * Z < 2^31" % (what, name, tuple(t.shape)))
    if not (isinstance(t, torch.Tensor) and t.dim() == 3 and t.dtype in dtypes and t.is_cuda):
        raise N3DError("%s: %s must be a (X, Y, Z) %s volume on a HIP device (got %s); there is no CPU fallback" % (
            what, name, kinds, _describe(t)))
    if t.numel() == 0:
        raise N3DError("%s: %s is empty: shape %s" % (what, name, tuple(t.shape)))
    return t.contiguous(), tuple(int(s) for s in t.shape)


def _connectivity(connectivity, what):
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity not in CONNECTIVITIES:
        raise N3DError("%s: connectivity must be 6, 18 or 26 (got %r)" % (what, connectivity))
    return connectivity


def _rules(what, connectivity=26, min_voxels=0, keep_largest=False, et_min_voxels=0):
    _connectivity(connectivity, what)
    for name, v in (("min_voxels", min_voxels), ("et_min_voxels", et_min_voxels)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 or v >= 2 ** 63:
            raise N3DError("%s: %s must be an integer >= 0 (got %r)" % (what, name, v))
    return dict(connectivity=connectivity, min_voxels=int(min_voxels), keep_largest=bool(keep_largest), et_min_voxels=int(et_min_voxels))


def _i3(v):
    return (C.c_int32 * 3)(*[int(x) for x in v])


# ---- device

class _Workspace:
    def __init__(self, lib, device, full):
        off = (C.c_int64 * 6)()
        nbytes = int(lib.n3d_cc_workspace_bytes(full[0], full[1], full[2], off))
        if nbytes == 0:
            raise N3DError("postprocess: image shape %s: needs 1 <= X * Y * Z < 2^31" % (tuple(full),))
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.rec = self.buf[off[5]:off[5] + REC_WORDS * 8].view(torch.int64)


_workspaces = {}


def _workspace(lib, device, full):
    key = (device, full)
    ws = _workspaces.get(key)
    if ws is None:
        _workspaces.clear()            # one shape at a time: the scratch of a full-size image is 17 bytes per voxel
        ws = _workspaces[key] = _Workspace(lib, device, full)
    return ws


def label_components(mask, connectivity=26):
    """mask: (X, Y, Z) uint8 or bool device tensor -> int32 (X, Y, Z): per voxel the id of its component of `mask != 0` -- the
    smallest linear index among the component's voxels --, -1 on background.  Three launches, no host sync."""
    _connectivity(connectivity, "label_components")
    mask, full = _volume(mask, "label_components", "mask", (torch.uint8, torch.bool))
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    parent = torch.empty(full, dtype=torch.int32, device=mask.device)
    comp = torch.empty(full, dtype=torch.int32, device=mask.device)
    check(_lib.load().n3d_cc_label(K.ptr(mask), _i3(full), connectivity, K.ptr(parent), K.ptr(comp), K.stream_ptr()), "n3d_cc_label")
    return comp


def run_phases(labels, out, first=0, last=len(PHASES) - 1, variant=TILED, **rules):
    """n3d_cc_phases: the launches first .. last of the pipeline on the shape's scratch, writing `out` (tools/postprocess_probe.py
    times them one by one; GLOBAL_ONLY is the variant without the LDS tile phase, same results) -> the record as it lies in the
    scratch (a view: the next call overwrites it)"""
    r = _rules("run_phases", **rules)
    labels, full = _volume(labels, "run_phases", "labels", (torch.uint8,))
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.shape == labels.shape and out.device == labels.device
            and out.is_contiguous()):
        raise N3DError("run_phases: out must be a contiguous uint8 volume like labels (got %s)" % _describe(out))
    lib = _lib.load()
    ws = _workspace(lib, labels.device, full)
    check(lib.n3d_cc_phases(int(variant), int(first), int(last), K.ptr(labels), _i3(full), r["connectivity"], r["min_voxels"],
                            int(r["keep_largest"]), r["et_min_voxels"], K.ptr(ws.buf), K.ptr(out), K.stream_ptr()), "n3d_cc_phases")
    return ws.rec


def clean_record(labels, **rules):
    """the device work of clean_labels: -> (cleaned uint8 volume, record: int64 (REC_WORDS,) device tensor, a copy of its own).
    No host sync."""
    r = _rules("clean_labels", **rules)
    labels, full = _volume(labels, "clean_labels", "labels", (torch.uint8,))
    lib = _lib.load()
    ws = _workspace(lib, labels.device, full)
    out = torch.empty(full, dtype=torch.uint8, device=labels.device)
    check(lib.n3d_cc_clean(K.ptr(labels), _i3(full), r["connectivity"], r["min_voxels"], int(r["keep_largest"]), r["et_min_voxels"],
                           K.ptr(ws.buf), K.ptr(out), K.stream_ptr()), "n3d_cc_clean")
    return out, ws.rec.clone()


def clean_labels(labels, connectivity=26, min_voxels=0, keep_largest=False, et_min_voxels=0, return_stats=False):
    """labels: (X, Y, Z) uint8 device label volume (what the predictors return) -> a new uint8 volume, the input untouched: steps A
    and B of the module text.  With every rule off the output equals the input.  No host sync, unless return_stats: then
    (volume, dict with STAT_KEYS) -- one copy of the 80-byte record."""
    out, rec = clean_record(labels, connectivity=connectivity, min_voxels=min_voxels, keep_largest=keep_largest,
                            et_min_voxels=et_min_voxels)
    return (out, stats_of(rec)) if return_stats else out


class CleanedPredictor:
    """predictor.predict(volumes, index, **kw) with element 0 of its result, the labels, replaced by clean_labels(labels, **rules);
    the rest comes back unchanged -- so metrics.score_set(CleanedPredictor(tr.predictor(...), min_voxels=...), vs, ids) scores
    cleaned volumes.  last_stats: the last subject's record on the device (None before the first); stats() syncs and decodes it."""

    def __init__(self, predictor, **rules):
        if not callable(getattr(predictor, "predict", None)):
            raise N3DError("CleanedPredictor: the predictor needs a predict(volumes, index, **kw) method (got %s)" % type(predictor).__name__)
        unknown = sorted(set(rules) - {"connectivity", "min_voxels", "keep_largest", "et_min_voxels"})
        if unknown:
            raise N3DError("CleanedPredictor: unknown rule%s %s (connectivity, min_voxels, keep_largest, et_min_voxels)" % (
                "s" if len(unknown) > 1 else "", ", ".join(unknown)))
        self.predictor, self.rules, self.last_stats = predictor, _rules("CleanedPredictor", **rules), None

    def predict(self, volumes, index, **kw):
        result = self.predictor.predict(volumes, index, **kw)
        if not isinstance(result, (tuple, list)) or len(result) == 0:
            raise N3DError("CleanedPredictor: predict must return a sequence that starts with the labels (got %s)" % type(result).__name__)
        cleaned, self.last_stats = clean_record(result[0], **self.rules)
        return (cleaned,) + tuple(result[1:])

    def stats(self):
        if self.last_stats is None:
            raise N3DError("CleanedPredictor.stats: no subject has been predicted yet")
        return stats_of(self.last_stats)
