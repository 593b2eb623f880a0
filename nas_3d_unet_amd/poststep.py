"""Step after the hot path (prediction.py:120-170): stitch the per-patch predictions of the searched net
into the brain-wide volume with mean blending (patches.py:172-207), place it in the full image, and fuse the three
sigmoid channels into a label volume -- on the device, from the layout the net produces (no host round trip per patch
as in prediction.py:132-138).  Host logic here: argument plumbing only."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import N3DError, PatchDesc, StitchEntry, check


def stitch(patches, corners, box_shape, full_shape=None, origin=(0, 0, 0)):
    """patches: (B, C, P, P, P) fp32 device tensor (any layout the ops produce); corners: B corners on the brain-wide grid;
    box_shape: (X, Y, Z) of the brain-wide box; full_shape/origin: optional full image the box is written into
    (prediction.py:141-147).  Returns a float64 (C, FX, FY, FZ) device tensor."""
    if not (isinstance(patches, torch.Tensor) and patches.is_cuda and patches.dtype == torch.float32 and patches.dim() == 5):
        raise N3DError("stitch: patches must be a (B, C, P, P, P) fp32 tensor on a HIP device")
    B, Cc, P = int(patches.shape[0]), int(patches.shape[1]), int(patches.shape[2])
    if patches.shape[3] != P or patches.shape[4] != P:
        raise N3DError("stitch: cubic patches expected")
    if len(corners) != B:
        raise N3DError("stitch: one corner per patch")
    st = K._bcv_strides(patches)
    if st is None:
        patches = patches.contiguous()
        st = K._bcv_strides(patches)
    sb, sc, sv = st
    X, Y, Z = (int(v) for v in box_shape)
    FX, FY, FZ = (int(v) for v in (full_shape if full_shape is not None else box_shape))
    cor = torch.tensor([[int(c) for c in cr] for cr in corners], dtype=torch.int32, device=patches.device)
    out = torch.zeros((Cc, FX, FY, FZ), dtype=torch.float64, device=patches.device)
    check(_lib.load().n3d_stitch(K.ptr(patches), sb, sc, sv, Cc, P, K.ptr(cor), B, X, Y, Z, K.ptr(out), FX, FY, FZ, int(origin[0]), int(origin[1]),
                                 int(origin[2]), K.stream_ptr()), "n3d_stitch")
    return out


def tumor_labels(pred, threshold=0.5, inclusive_label=False):
    """pred: (3, X, Y, Z) float64 device tensor (stitch output) -> uint8 (X, Y, Z) labels {0, 1, 2, 4} (prediction.py:150-170)"""
    if not (isinstance(pred, torch.Tensor) and pred.is_cuda and pred.dtype == torch.float64 and pred.dim() == 4 and pred.shape[0] == 3
            and pred.is_contiguous()):
        raise N3DError("tumor_labels: pred must be a contiguous (3, X, Y, Z) float64 tensor on a HIP device")
    out = torch.empty(tuple(pred.shape[1:]), dtype=torch.uint8, device=pred.device)
    check(_lib.load().n3d_tumor_labels(K.ptr(pred), out.numel(), float(threshold), 1 if inclusive_label else 0, K.ptr(out), K.stream_ptr()),
          "n3d_tumor_labels")
    return out


# ---- the same stitch for a whole subject, chunk by chunk (predict.SubjectPredictor): running buffers instead of a patch list
IDENTITY = ([0, 1, 2], [False, False, False])


def entry_table(entries, device):
    """entries: [(corner, (perm, flip) the patch was gathered with, slot)] in list order -> the device table n3d_stitch_add reads
    (n3d_stitch_entry records as bytes; one host -> device copy).  slot: the patch's index in the tensor; < 0: a dead patch."""
    recs = (StitchEntry * max(len(entries), 1))()
    for i, (corner, (perm, flip), slot) in enumerate(entries):
        if sorted(int(a) for a in perm) != [0, 1, 2]:
            raise N3DError("stitch entries: perm must be a permutation of (0, 1, 2), got %s" % (list(perm),))
        recs[i] = StitchEntry(PatchDesc((C.c_int32 * 3)(*[int(c) for c in corner]), (C.c_int32 * 3)(*[int(a) for a in perm]),
                                        (C.c_int32 * 3)(*[int(bool(f)) for f in flip])), int(slot))
    return torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(device)


def stitch_buffers(channels, box_shape, device):
    """the zeroed running buffers of one subject: (sum float64 (C, X, Y, Z), cnt int32 (X, Y, Z))"""
    X, Y, Z = (int(v) for v in box_shape)
    return (torch.zeros((int(channels), X, Y, Z), dtype=torch.float64, device=device),
            torch.zeros((X, Y, Z), dtype=torch.int32, device=device))


def _running(sum_, cnt, cover=torch.int32, what="int32 (X, Y, Z) count"):
    if not (isinstance(sum_, torch.Tensor) and sum_.is_cuda and sum_.dtype == torch.float64 and sum_.dim() == 4 and sum_.is_contiguous()
            and isinstance(cnt, torch.Tensor) and cnt.device == sum_.device and cnt.dtype == cover and cnt.is_contiguous()
            and tuple(cnt.shape) == tuple(sum_.shape[1:])):
        raise N3DError("stitch: running buffers are a contiguous float64 (C, X, Y, Z) sum and %s on one HIP device" % what)
    return tuple(int(v) for v in sum_.shape)


def _add_args(name, patches, table, first, count, lo, hi, sum_, Cc):
    """what n3d_stitch_add and n3d_stitch_add_w share -> (the patch tensor the pointer is into, for the caller to hold through the
    launch; P; the leading arguments patches .. n; (lo, hi))"""
    es = C.sizeof(StitchEntry)
    if not (isinstance(table, torch.Tensor) and table.dtype == torch.uint8 and table.device == sum_.device and table.is_contiguous()
            and first >= 0 and count >= 1 and (first + count) * es <= table.numel()):
        raise N3DError("%s: records [%d, %d) are not in the entry table" % (name, first, first + count))
    if isinstance(patches, tuple):
        pp, (sb, sc, sv), B, P = None, (0, 0, 0), 0, int(patches[1])
    else:
        if not (isinstance(patches, torch.Tensor) and patches.device == sum_.device and patches.dtype == torch.float32 and patches.dim() == 5
                and patches.shape[1] == Cc and patches.shape[2] == patches.shape[3] == patches.shape[4]):
            raise N3DError("%s: patches must be a (B, %d, P, P, P) fp32 tensor on the buffers' device" % (name, Cc))
        st = K._bcv_strides(patches)
        if st is None:
            patches = patches.contiguous()
            st = K._bcv_strides(patches)
        pp, (sb, sc, sv), B, P = K.ptr(patches), st, int(patches.shape[0]), int(patches.shape[2])
    head = (pp, sb, sc, sv, Cc, P, B, table.data_ptr() + first * es, int(count))
    return patches, P, head, ((C.c_int32 * 3)(*[int(v) for v in lo]), (C.c_int32 * 3)(*[int(v) for v in hi]))


def stitch_add(patches, table, first, count, lo, hi, sum_, cnt):
    """add the records [first, first + count) of an entry_table to the running buffers (n3d_stitch_add).  patches: the chunk's
    (B, C, P, P, P) fp32 predictions in any layout the ops produce, or (None, P) when every record of the range is dead; lo / hi:
    the bounding box [lo, hi) of those records' patches on the brain-wide grid (the launch covers it, clipped to the box)."""
    Cc, X, Y, Z = _running(sum_, cnt)
    patches, _, head, box = _add_args("stitch_add", patches, table, first, count, lo, hi, sum_, Cc)
    check(_lib.load().n3d_stitch_add(*head, *box, X, Y, Z, K.ptr(sum_), K.ptr(cnt), K.stream_ptr()), "n3d_stitch_add")


def _finish_args(name, sum_, X, Y, Z, full_shape, want_probs, want_labels, mask_vol):
    """what n3d_stitch_finish and n3d_stitch_finish_w share: ((FX, FY, FZ), Cv, probs, labels), the outputs freshly allocated"""
    if not (want_probs or want_labels):
        raise N3DError("%s: neither probabilities nor labels asked for" % name)
    full = tuple(int(v) for v in (full_shape if full_shape is not None else (X, Y, Z)))
    Cv = 0
    if mask_vol is not None:
        if not (isinstance(mask_vol, torch.Tensor) and mask_vol.device == sum_.device and mask_vol.dtype == torch.float32 and mask_vol.dim() == 4
                and mask_vol.is_contiguous() and tuple(mask_vol.shape[1:]) == (X, Y, Z)):
            raise N3DError("%s: mask_vol must be the subject's contiguous (Cv, %d, %d, %d) fp32 box on the buffers' device" % (name, X, Y, Z))
        Cv = int(mask_vol.shape[0])
    probs = torch.empty((int(sum_.shape[0]),) + full, dtype=torch.float64, device=sum_.device) if want_probs else None
    labels = torch.empty(full, dtype=torch.uint8, device=sum_.device) if want_labels else None
    return full, Cv, probs, labels


def stitch_finish(sum_, cnt, full_shape=None, origin=(0, 0, 0), want_probs=True, want_labels=True, threshold=0.5, inclusive_label=False,
                  mask_vol=None):
    """one pass over the full image (n3d_stitch_finish) -> (labels uint8 (FX, FY, FZ) or None, probs float64 (C, FX, FY, FZ) or
    None): the mean sum / max(cnt, 1) of the box placed at `origin`, and / or tumor_labels of that mean; mask_vol: the subject's
    (Cv, X, Y, Z) fp32 box -- labels are 0 where all of its channels are (the skull mask, prediction.py:83-96)."""
    Cc, X, Y, Z = _running(sum_, cnt)
    (FX, FY, FZ), Cv, probs, labels = _finish_args("stitch_finish", sum_, X, Y, Z, full_shape, want_probs, want_labels, mask_vol)
    check(_lib.load().n3d_stitch_finish(K.ptr(sum_), K.ptr(cnt), Cc, X, Y, Z, K.ptr(probs), K.ptr(labels), float(threshold),
                                        1 if inclusive_label else 0, K.ptr(mask_vol), Cv, FX, FY, FZ, int(origin[0]), int(origin[1]),
                                        int(origin[2]), K.stream_ptr()), "n3d_stitch_finish")
    return labels, probs


# ---- the same with an importance weight per covering patch (sliding-window inference with Gaussian blending): a separable
# profile over the position inside the patch, and a running fp64 weight sum in place of the count
def blend_profile(P, kind="gaussian", sigma_scale=0.125):
    """the float64 (P,) profile of a patch of P voxels per axis; a patch prediction is weighted by profile[l0] * profile[l1] *
    profile[l2] at the local voxel l.  "gaussian": exp(-0.5 * ((i - (P - 1) / 2) / (sigma_scale * P)) ** 2), not normalised (the
    weights of nnU-Net and of MONAI's sliding_window_inference(mode="gaussian"), sigma = P / 8); "mean": ones; an array: the
    profile itself.  Whatever comes out must be 1-D of length P, finite, strictly positive and exactly symmetric (profile[i] ==
    profile[P-1-i]: the kernel takes the weight on the volume's grid, whatever isometry the patch was gathered with)."""
    P = int(P)
    if isinstance(kind, str):
        if kind == "gaussian":
            if not float(sigma_scale) > 0:
                raise N3DError("blend_profile: sigma_scale must be positive, got %r" % (sigma_scale,))
            i = np.arange(P, dtype=np.float64)
            prof = np.exp(-0.5 * ((i - (P - 1) / 2) / (float(sigma_scale) * P)) ** 2)
        elif kind == "mean":
            prof = np.ones(P, dtype=np.float64)
        else:
            raise N3DError("blend_profile: unknown kind %r (\"gaussian\", \"mean\" or an array of %d weights)" % (kind, P))
    else:
        try:
            prof = np.array(kind, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise N3DError("blend_profile: not a profile: %s" % e)
    if prof.ndim != 1 or len(prof) != P:
        raise N3DError("blend_profile: the profile of a patch of %d is 1-D of length %d, got shape %s" % (P, P, prof.shape))
    if not (np.isfinite(prof).all() and (prof > 0).all()):
        raise N3DError("blend_profile: the weights must be finite and strictly positive")
    if not np.array_equal(prof, prof[::-1]):
        raise N3DError("blend_profile: the profile must be exactly symmetric (profile[i] == profile[P-1-i])")
    return prof


def stitch_buffers_w(channels, box_shape, device):
    """the zeroed running buffers of one subject: (sum float64 (C, X, Y, Z), wsum float64 (X, Y, Z))"""
    X, Y, Z = (int(v) for v in box_shape)
    return (torch.zeros((int(channels), X, Y, Z), dtype=torch.float64, device=device),
            torch.zeros((X, Y, Z), dtype=torch.float64, device=device))


def _running_w(sum_, wsum):
    return _running(sum_, wsum, torch.float64, "float64 (X, Y, Z) weight sum")


def stitch_add_w(patches, table, first, count, lo, hi, profile_dev, sum_, wsum):
    """stitch_add with the weight profile[l0] * profile[l1] * profile[l2] per covering record (n3d_stitch_add_w).  profile_dev: a
    blend_profile on the buffers' device, float64 (P,)."""
    Cc, X, Y, Z = _running_w(sum_, wsum)
    patches, P, head, box = _add_args("stitch_add_w", patches, table, first, count, lo, hi, sum_, Cc)
    if not (isinstance(profile_dev, torch.Tensor) and profile_dev.device == sum_.device and profile_dev.dtype == torch.float64
            and profile_dev.is_contiguous() and tuple(profile_dev.shape) == (P,)):
        raise N3DError("stitch_add_w: the profile must be a contiguous float64 (%d,) tensor on the buffers' device" % P)
    check(_lib.load().n3d_stitch_add_w(*head, K.ptr(profile_dev), *box, X, Y, Z, K.ptr(sum_), K.ptr(wsum), K.stream_ptr()), "n3d_stitch_add_w")


def stitch_finish_w(sum_, wsum, full_shape=None, origin=(0, 0, 0), want_probs=True, want_labels=True, threshold=0.5,
                    inclusive_label=False, mask_vol=None):
    """stitch_finish on the weighted buffers (n3d_stitch_finish_w): the mean is sum / wsum where wsum > 0, else 0"""
    Cc, X, Y, Z = _running_w(sum_, wsum)
    (FX, FY, FZ), Cv, probs, labels = _finish_args("stitch_finish_w", sum_, X, Y, Z, full_shape, want_probs, want_labels, mask_vol)
    check(_lib.load().n3d_stitch_finish_w(K.ptr(sum_), K.ptr(wsum), Cc, X, Y, Z, K.ptr(probs), K.ptr(labels), float(threshold),
                                          1 if inclusive_label else 0, K.ptr(mask_vol), Cv, FX, FY, FZ, int(origin[0]), int(origin[1]),
                                          int(origin[2]), K.stream_ptr()), "n3d_stitch_finish_w")
    return labels, probs


# ---- whole-image prediction (predict.ImagePredictor; prediction.py:102-119): the passes around the one forward
def _i3(v, what):
    v = [int(a) for a in v]
    if len(v) != 3:
        raise N3DError("%s: expected three values, got %s" % (what, v))
    return (C.c_int32 * 3)(*v)


def _image_y(y, padded, what):
    """the net's (1, C, PX, PY, PZ) fp32 prediction -> (tensor, channels, channel stride, voxel stride)"""
    if not (isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 5 and y.shape[0] == 1
            and tuple(int(s) for s in y.shape[2:]) == tuple(int(p) for p in padded)):
        raise N3DError("%s: y must be a (1, C, %d, %d, %d) fp32 tensor on a HIP device" % ((what,) + tuple(int(p) for p in padded)))
    st = K._bcv_strides(y)
    if st is None:
        y = y.contiguous()
        st = K._bcv_strides(y)
    return y, int(y.shape[1]), st[1], st[2]


def _image_sum(sum_, Cc, full, device, what):
    if not (isinstance(sum_, torch.Tensor) and sum_.device == device and sum_.dtype == torch.float64 and sum_.is_contiguous()
            and tuple(sum_.shape) == (Cc,) + tuple(int(f) for f in full)):
        raise N3DError("%s: the running sum is a contiguous float64 (%d, %d, %d, %d) tensor on y's device" % ((what, Cc) + tuple(int(f) for f in full)))


def _image_box(box, device, what):
    if not (isinstance(box, torch.Tensor) and box.device == device and box.dtype == torch.float32 and box.dim() == 4 and box.is_contiguous()):
        raise N3DError("%s: the subject's box must be a contiguous (Cv, bx, by, bz) fp32 tensor on the HIP device" % what)
    return tuple(int(s) for s in box.shape)


def image_embed(box, origin, full_shape, padded_shape, flip=(False, False, False), out=None):
    """the subject's (Cv, bx, by, bz) box at `origin` inside the (FX, FY, FZ) image -> the net's input (1, Cv, PX, PY, PZ) in NDHWC
    storage: the image mirrored along the axes of `flip`, zero-padded at the high end (n3d_image_embed).  out: written in place
    (every voxel is written; a pitch gap is left as it is)."""
    if not (isinstance(box, torch.Tensor) and box.is_cuda):
        raise N3DError("image_embed: the box lives on a HIP device; there is no CPU fallback")
    Cv, bx, by, bz = _image_box(box, box.device, "image_embed")
    PX, PY, PZ = (int(p) for p in padded_shape)
    if out is None:
        out = K.empty_ndhwc(1, Cv, PX, PY, PZ, box.device, torch.float32)
    if not (isinstance(out, torch.Tensor) and out.device == box.device and out.dtype == torch.float32 and tuple(out.shape) == (1, Cv, PX, PY, PZ)):
        raise N3DError("image_embed: out must be a (1, %d, %d, %d, %d) fp32 tensor on the box's device" % (Cv, PX, PY, PZ))
    ld = K._pitch_of(out)
    if ld is None:
        raise N3DError("image_embed: out must be in NDHWC (channels-last) storage, as K.empty_ndhwc gives it")
    check(_lib.load().n3d_image_embed(K.ptr(box), Cv, bx, by, bz, _i3(origin, "origin"), _i3(full_shape, "full_shape"),
                                      _i3(padded_shape, "padded_shape"), _i3([bool(f) for f in flip], "flip"), K.ptr(out), ld, K.stream_ptr()),
          "n3d_image_embed")
    return out


def image_add(y, full_shape, padded_shape, flip, sum_=None):
    """one key of an ensemble that is not its last (n3d_image_add): y un-flipped and cropped to the image is written into (sum_ None:
    a fresh buffer, the first key) or added to the fp64 running sum (C, FX, FY, FZ), which is returned"""
    y, Cc, sc, sv = _image_y(y, padded_shape, "image_add")
    first = sum_ is None
    if first:
        sum_ = torch.empty((Cc,) + tuple(int(f) for f in full_shape), dtype=torch.float64, device=y.device)
    _image_sum(sum_, Cc, full_shape, y.device, "image_add")
    check(_lib.load().n3d_image_add(K.ptr(y), sc, sv, Cc, _i3(full_shape, "full_shape"), _i3(padded_shape, "padded_shape"),
                                    _i3([bool(f) for f in flip], "flip"), K.ptr(sum_), 1 if first else 0, K.stream_ptr()), "n3d_image_add")
    return sum_


def image_finish(y, full_shape, padded_shape, flip=(False, False, False), sum_=None, n_keys=1, want_probs=True, want_labels=True,
                 threshold=0.5, inclusive_label=False, mask_box=None, origin=(0, 0, 0)):
    """the last (or only) key: one pass over the image (n3d_image_finish) -> (labels uint8 (FX, FY, FZ) or None, probs float64
    (C, FX, FY, FZ) or None).  mean = (sum_ + y) / n_keys with y un-flipped and cropped (n_keys == 1: no sum_, exactly y);
    mask_box: the subject's (Cv, bx, by, bz) box at `origin` -- labels are 0 where all of its channels are and outside it."""
    y, Cc, sc, sv = _image_y(y, padded_shape, "image_finish")
    if not (want_probs or want_labels):
        raise N3DError("image_finish: neither probabilities nor labels asked for")
    if (sum_ is None) != (int(n_keys) == 1):
        raise N3DError("image_finish: a running sum goes with more than one key, and only with it")
    if sum_ is not None:
        _image_sum(sum_, Cc, full_shape, y.device, "image_finish")
    Cv = bx = by = bz = 0
    if mask_box is not None:
        Cv, bx, by, bz = _image_box(mask_box, y.device, "image_finish")
    full = tuple(int(f) for f in full_shape)
    probs = torch.empty((Cc,) + full, dtype=torch.float64, device=y.device) if want_probs else None
    labels = torch.empty(full, dtype=torch.uint8, device=y.device) if want_labels else None
    check(_lib.load().n3d_image_finish(K.ptr(y), sc, sv, Cc, _i3(full, "full_shape"), _i3(padded_shape, "padded_shape"),
                                       _i3([bool(f) for f in flip], "flip"), K.ptr(sum_), int(n_keys), K.ptr(probs), K.ptr(labels),
                                       float(threshold), 1 if inclusive_label else 0, K.ptr(mask_box), Cv, bx, by, bz, _i3(origin, "origin"),
                                       K.stream_ptr()), "n3d_image_finish")
    return labels, probs
