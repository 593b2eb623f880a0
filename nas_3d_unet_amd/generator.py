"""The reference's training / validation generator (generator.py:68-217) on the device.

The reference builds, every epoch, the list of candidate patches of every volume (patches.py:76-95), crops EACH candidate on the
host to decide whether it is used (add_data's filters: not all four modalities zero; with skip_health, not all labels zero --
generator.py:195-217), once to count the epoch's steps and once more during the epoch.  Here:

  * VolumeSet keeps the brain-wise boxes resident in HBM with two summed-area tables per volume (n3d_volume_sat, built once
    at load), so that one n3d_patch_qualify launch answers both filters for every candidate of an epoch (8 lookups per table
    and candidate, whatever the patch size or overlap); add_subject takes a raw int16 scan there (preprocess.normalize_subject);
  * Generator reproduces the reference class's epoch exactly, random stream included: the overlap drawn per epoch, the candidate
    order, the shuffle and pop() from the end, one isometry key per KEPT patch, the batch boundaries and the smaller last batch,
    steps_per_epoch -- and produces each batch with ONE n3d_patch_gather launch (patches of different volumes in one batch), no
    host sync and no host -> device copy per batch;
  * augment=True (the reference's scale / flip distortion, augment.py:50-67, applied to the crop ahead of the isometry) draws
    from numpy's generator exactly as the reference does and composes the resampling into the same single launch
    (n3d_patch_gather_aug): draw_augment, scale_affine, resample_transform and resample_params below are the reference's and
    nilearn's fp64 host arithmetic; the resampler is scipy.ndimage.affine_transform's rule for a diagonal matrix (order 0, mode
    "constant") restated -- nilearn itself was never run against this package;
  * augment_rotation / augment_interpolation / augment_intensity_scale / augment_intensity_shift (none of them the reference's)
    add a small rotation about the patch centre, linear interpolation of the data (the truth stays nearest neighbour) and a
    per-modality intensity scale and shift of the brain voxels, still in ONE launch per batch (n3d_patch_gather_warp):
    rotation_matrix, warp_transform and draw_warp below are their host arithmetic and draws.

  * augment_elastic (elastic.Elastic; not the reference's either) adds a non-rigid displacement to the gather's coordinate: a cubic
    B-spline free-form deformation whose control values the device generates from a key drawn per patch, still in ONE launch per
    batch (n3d_patch_gather_elastic).

  * augment_appearance (appearance.Appearance; not the reference's either) adds Gaussian noise, Gaussian blur, contrast and gamma of
    the brain voxels, applied to the gathered batch in place by n3d_patch_appearance (1 to 10 launches, no host sync).

  * augment_artefact (artefact.Artefact; not the reference's either) adds simulated low resolution, a multiplicative bias field and
    modality dropout, applied to the gathered batch in place by n3d_patch_artefact after the appearance transforms (1 to 4
    launches, no host sync).

  * sampling (sampling.RandomCrop; not the reference's either) replaces the candidate grid by crops drawn on the device, uniformly
    or centred on a random voxel of a mask (n3d_volume_line_index once per volume, ONE n3d_patch_sample launch per epoch); the
    drawn table takes the grid's place, so qualification, the epoch's order and every gather above are what they were.

Host logic only; the kernels are n3d_volume_sat, n3d_patch_qualify, n3d_patch_gather, n3d_patch_gather_aug,
n3d_patch_gather_warp, n3d_patch_gather_elastic, n3d_patch_appearance, n3d_patch_artefact, n3d_volume_line_index and n3d_patch_sample
(include/n3d.h).
"""
from __future__ import annotations

import ctypes as C
import inspect
import random

import numpy as np
import torch

from . import _lib, appearance, datastep, predict, preprocess
from . import artefact as artefact_mod
from . import elastic as elastic_mod
from . import sampling as sampling_mod
from . import spline as spline_mod
from . import kernels as K
from ._lib import AugDesc, ElasticDesc, GatherDesc, N3DError, PatchDesc, PatchVolume, WarpDesc, check

# augment.py:95-100 draws from list(set(...)): that (deterministic) order, NOT the sorted one of datastep.random_permutation_key
KEYS = list(datastep.generate_permutation_keys())
LABELS = [1, 2, 4]
MAX_BATCH = 64      # N3D_PATCH_MAX_BATCH
AUG_MAX_BATCH = 32  # N3D_PATCH_AUG_MAX_BATCH: the widened descriptors of an augmented batch travel in 4 KB of kernel arguments
WARP_MAX_BATCH = 16  # N3D_PATCH_WARP_MAX_BATCH
WARP_MAX_CHANNELS = 4  # gain[4], bias[4] of n3d_patch_wdesc
ELASTIC_MAX_BATCH = elastic_mod.MAX_BATCH  # N3D_PATCH_ELASTIC_MAX_BATCH
INTERPOLATION_ORDER = {"nearest": 0, "linear": 1, "spline3": spline_mod.ORDER}   # augment_interpolation -> order of n3d_patch_wdesc

_ISO = {None: ([0, 1, 2], [False, False, False])}


def _isometry(key):
    iso = _ISO.get(key)
    if iso is None:
        iso = _ISO[key] = datastep.isometry_of_key(key)
    return iso


def draw_overlap(patch_overlap, rng):
    """generator.py:127: no draw for None / 0; a drawn 0 still selects the fixed-overlap strategy (patching() tests `is None`)"""
    return patch_overlap if not patch_overlap else rng.randint(0, patch_overlap)


def candidate_table(boxes, indices_list, patch, overlap=None, both_ps=False):
    """(N, 4) int32 rows (volume index, corner x, y, z): for each index of indices_list in order, each corner of
    patching(box, patch, overlap, both_ps) in order (patches.py:76-95)"""
    parts = [np.zeros((0, 4), np.int64)]
    for i in indices_list:
        c = predict.patching(tuple(boxes[i]), (patch, patch, patch), overlap, both_ps)
        parts.append(np.concatenate((np.full((len(c), 1), i, np.int64), c), axis=1))
    return np.ascontiguousarray(np.concatenate(parts).astype(np.int32))


def kept_mask(flags, skip_health):
    """add_data's filters (generator.py:202-207) on qualification flags (bit 0: some modality nonzero, bit 1: some label nonzero)"""
    f = np.asarray(flags)
    keep = (f & 1) != 0
    if skip_health:
        keep &= (f & 2) != 0
    return keep


def draw_augment(np_rng, distortion_factor=0.25, flip=True):
    """do_augment's draws (augment.py:26-39,55-57) from an np.random-like object, in the reference's order: the per-axis scale
    np_rng.normal(1, distortion_factor, 3) unless distortion_factor is None, then one np_rng.choice([True, False]) per axis if
    `flip`.  Returns (scale (3,) float64 or None, list of flipped axes -- None without `flip`)."""
    scale = np_rng.normal(1, distortion_factor, 3) if distortion_factor is not None else None
    axes = [a for a in range(3) if np_rng.choice([True, False])] if flip else None
    return scale, axes


def check_affine(affine):
    """the data set's affine as a (4, 4) float64 array (None: identity); its 3x3 part must be diagonal -- what the gather resamples
    is one source voxel per axis index"""
    M = np.eye(4) if affine is None else np.array(affine, dtype=np.float64)
    if M.shape != (4, 4) or not np.isfinite(M).all():
        raise N3DError("Generator: affine must be a finite 4x4 array (got shape %s)" % (M.shape,))
    if not np.all(np.diag(np.diag(M[:3, :3])) == M[:3, :3]):
        raise N3DError("Generator: augment=True supports affines whose 3x3 part is diagonal; got\n%s" % M)
    return M


def scale_affine(affine, P, scale):
    """scale_image (augment.py:8-13) of a P^3 image with affine `affine`: the affine of the rescaled image"""
    M, s, n = np.asarray(affine, dtype=np.float64), np.asarray(scale), np.array((P, P, P))
    N = M.copy()
    N[:3, :3] = M[:3, :3] * s                                       # column a scaled by s[a]
    N[:3, 3] = M[:3, 3] + (n * np.diag(M)[:3] * (1 - s)) / 2        # ... around the centre, in this order of operations
    return N


def resample_transform(affine, P, scale):
    """what nilearn's resample_to_img(scale_image(img, scale), img) hands to scipy for a P^3 image: (A, b, identity).  identity:
    no scale was drawn, or np.allclose(affine, scaled affine) -- nilearn returns the image as it is (A = 1, b = 0 then).  Otherwise
    T = inv(scaled affine) . affine, A = diag(T[:3, :3]) (scipy's 1-D matrix), b = T[:3, 3] (its offset).  A singular scaled affine
    raises numpy.linalg.LinAlgError as in the reference; a T that is not diagonal raises N3DError."""
    M = np.asarray(affine, dtype=np.float64)
    if scale is None:
        return np.ones(3), np.zeros(3), True
    N = scale_affine(M, P, scale)
    if np.allclose(M, N):
        return np.ones(3), np.zeros(3), True
    T = np.linalg.inv(N).dot(M)
    if not np.all(np.diag(np.diag(T[:3, :3])) == T[:3, :3]):
        raise N3DError("Generator: the resampling matrix of scale %s under this affine is not diagonal" % (scale,))
    return np.diag(T[:3, :3]).copy(), T[:3, 3].copy(), False


def resample_params(affine, P, scale):
    """(A, sh, identity) of n3d_patch_adesc: resample_transform with sh = b / A, the division scipy.ndimage.affine_transform does
    in numpy before its zoom-shift loop"""
    A, b, identity = resample_transform(affine, P, scale)
    return A, b / A, identity


def rotation_matrix(angles_deg):
    """R = Rz . Ry . Rx of the three angles (about axes 0, 1, 2, in degrees) as a (3, 3) float64 array.  The radians are
    angle * pi / 180 in this order, sines and cosines are numpy's, and every entry is the written-out product below, evaluated left
    to right in fp64 (no matrix product: a BLAS may fuse or reorder)."""
    ax, ay, az = (np.float64(a) * np.pi / 180.0 for a in angles_deg)
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                     [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                     [-sy, cy * sx, cy * cx]], dtype=np.float64)


def warp_transform(A, b, R, P):
    """(M, off) of n3d_patch_wdesc's matrix rule for a P^3 patch: the output index is rotated by R about the patch's voxel centre
    p = (P - 1) / 2 on every axis, then the reference's scale map c -> A * c + b (resample_transform; A = 1, b = 0 when no scale was
    drawn or nilearn would return the image as it is) is applied:  M = A[:, None] * R,  off = A * (p - R p) + b, with
    R p = (R[:, 0] * p + R[:, 1] * p) + R[:, 2] * p, elementwise fp64.  The rotation is in VOXEL space: the affine's diagonal enters
    through (A, b) only, so under an anisotropic affine the rotation is not rigid in world space (BraTS is 1 mm isotropic)."""
    A, b, R = np.asarray(A, np.float64), np.asarray(b, np.float64), np.asarray(R, np.float64)
    if R.shape != (3, 3) or A.shape != (3,) or b.shape != (3,):
        raise N3DError("warp_transform: A and b are (3,), R is (3, 3)")
    p = np.float64(P - 1) / 2
    Rp = (R[:, 0] * p + R[:, 1] * p) + R[:, 2] * p
    return A[:, None] * R, A * (p - Rp) + b


def draw_warp(np_rng, rotation=None, intensity_scale=None, intensity_shift=None, Cv=4):
    """the draws of the rotation and the intensity map of one kept patch from an np.random-like object, in this order:
    np_rng.uniform(-r, r, 3) if `rotation` is not None (r: a scalar or three per-axis maxima, degrees), then
    np_rng.uniform(1 - g, 1 + g, Cv) if `intensity_scale` (g) is not None, then np_rng.normal(0, s, Cv) if `intensity_shift` (s) is
    not None.  An option that is None draws nothing.  Returns (angles, gain, bias), None where nothing was drawn."""
    angles = gain = bias = None
    if rotation is not None:
        r = np.asarray(rotation, np.float64)
        angles = np_rng.uniform(-r, r, 3)
    if intensity_scale is not None:
        gain = np_rng.uniform(1 - intensity_scale, 1 + intensity_scale, Cv)
    if intensity_shift is not None:
        bias = np_rng.normal(0, intensity_shift, Cv)
    return angles, gain, bias


def epoch_order(flags, batch_size, rng, skip_health=True, shuffle=True, permute=False, augment=None, warp=None, appearance=None,
                elastic=None, artefact=None):
    """generator.py:170-217 on qualification flags: yields each batch as a list of (candidate index, isometry key or None).
    The candidate order is shuffled at the first next() (rng.shuffle, if `shuffle`), then pop()ped from the end; a kept candidate
    draws its key (rng.choice over KEYS, if `permute`) when it is popped; a batch is yielded when full, or when the list is empty.
    skip_health: the caller's skip_health AND the set has truth (without truth the reference skips nothing as healthy).
    augment: None, or (np_rng, distortion_factor, flip): a kept candidate then draws draw_augment(...) just before its key
    (generator.py:208-214), and the batch entries are (candidate index, key, (scale, flipped axes)).
    warp: None, or (np_rng, rotation, intensity_scale, intensity_shift, Cv): a kept candidate then draws draw_warp(...) right after
    draw_augment and before its key, and the entries gain a fourth element (angles, gain, bias).
    appearance: None, or (np_rng, an appearance.Appearance, Cv): a kept candidate then makes Appearance.draw(np_rng, Cv)'s calls right
    after draw_warp's (after draw_augment's without warp) and before its key, and the entries gain a last element, that draw.
    elastic: None, or (np_rng, an elastic.Elastic): a kept candidate then makes Elastic.draw(np_rng)'s calls right after draw_warp's
    (after draw_augment's without warp) and before Appearance.draw's and its key, and the entries gain one element ahead of the
    appearance one: the drawn key (k0, k1), or None for a patch that is not deformed.
    artefact: None, or (np_rng, an artefact.Artefact, Cv): a kept candidate then makes Artefact.draw(np_rng, Cv)'s calls right after
    Appearance.draw's (after whatever precedes those without appearance) and before its key, and the entries gain one element at
    the very end, that draw -- behind the appearance one."""
    if warp is not None and augment is None:
        raise N3DError("epoch_order: the warp draws follow draw_augment's: warp needs augment")
    if appearance is not None and augment is None:
        raise N3DError("epoch_order: the appearance draws follow draw_augment's: appearance needs augment")
    if elastic is not None and augment is None:
        raise N3DError("epoch_order: the elastic draws follow draw_augment's: elastic needs augment")
    if artefact is not None and augment is None:
        raise N3DError("epoch_order: the artefact draws follow draw_augment's: artefact needs augment")
    keep = kept_mask(flags, skip_health).tolist()
    order = list(range(len(keep)))
    if shuffle:
        rng.shuffle(order)
    batch = []
    while order:
        i = order.pop()
        if keep[i]:
            aug = (draw_augment(*augment),) if augment is not None else ()      # drawn before the key
            wrp = (draw_warp(*warp),) if warp is not None else ()               # ... and these between the two
            ela = (elastic[1].draw(elastic[0]),) if elastic is not None else ()  # ... then these
            app = (appearance[1].draw(appearance[0], appearance[2]),) if appearance is not None else ()      # ... then these
            art = (artefact[1].draw(artefact[0], artefact[2]),) if artefact is not None else ()              # ... and these last
            batch.append((i, rng.choice(KEYS) if permute else None) + aug + wrp + ela + app + art)
        if len(batch) == batch_size or (not order and batch):
            yield batch
            batch = []


class VolumeSet:
    """Brain-wise boxes resident in HBM, each with its summed-area tables, and the device table of their records."""

    def __init__(self, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise N3DError("VolumeSet: volumes live on a HIP device (got %s); there is no CPU fallback" % self.device)
        self.volumes, self.truths, self.tables, self.boxes = [], [], [], []
        self.origins, self.full_shapes = [], []     # per volume: the box's corner in its image and the image's shape (add_subject), else None
        self.channels = None
        self.has_truth = None
        self.records = None        # device table of n3d_patch_volume records (rebuilt by add)
        self.line_indexes = []     # per volume: its n3d_volume_line_index table, built by line_index(i) when first asked for
        self.index_ptrs = None     # device array of their addresses, 0 where none is built (rebuilt by index_table)
        self._index_ptrs_of = None
        self._spline_scratch = {}  # (B, Cv, P) -> the scratch of n3d_patch_gather_spline, allocated at the first such batch and reused

    def __len__(self):
        return len(self.volumes)

    def box(self, i):
        return self.boxes[i]

    def add(self, vol, truth=None):
        """vol: (Cv, X, Y, Z) fp32 brain-wise box (numpy or tensor); truth: (X, Y, Z) or (1, X, Y, Z) uint8 raw labels {0,1,2,4}.
        Copies both to the device, builds the volume's tables (n3d_volume_sat) and returns its index."""
        v = torch.from_numpy(np.ascontiguousarray(vol)) if isinstance(vol, np.ndarray) else vol
        if not (isinstance(v, torch.Tensor) and v.dim() == 4 and v.dtype == torch.float32):
            raise N3DError("VolumeSet.add: vol must be a (C, X, Y, Z) float32 array or tensor")
        Cv, X, Y, Z = (int(s) for s in v.shape)
        if self.channels is not None and Cv != self.channels:
            raise N3DError("VolumeSet.add: every volume of a set has the same channels (%d, got %d)" % (self.channels, Cv))
        if self.has_truth is not None and (truth is not None) != self.has_truth:
            raise N3DError("VolumeSet.add: either every volume of a set has truth or none does")
        t = None
        if truth is not None:
            t = torch.from_numpy(np.ascontiguousarray(truth)) if isinstance(truth, np.ndarray) else truth
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and tuple(t.shape) in ((X, Y, Z), (1, X, Y, Z))):
                raise N3DError("VolumeSet.add: truth must be a (X, Y, Z) or (1, X, Y, Z) uint8 label volume matching vol")
            t = t.reshape(X, Y, Z).to(self.device).contiguous()
        v = v.to(self.device).contiguous()
        sat = torch.empty((X + 1, Y + 1, Z + 1, 2), dtype=torch.int32, device=self.device)
        check(_lib.load().n3d_volume_sat(K.ptr(v), Cv, K.ptr(t), X, Y, Z, K.ptr(sat), K.stream_ptr()), "n3d_volume_sat")
        self.volumes.append(v)
        self.truths.append(t)
        self.tables.append(sat)
        self.boxes.append((X, Y, Z))
        self.origins.append(None)
        self.full_shapes.append(None)
        self.channels, self.has_truth = Cv, truth is not None
        recs = (PatchVolume * len(self.volumes))()
        for i, (vv, tt, ss, b) in enumerate(zip(self.volumes, self.truths, self.tables, self.boxes)):
            recs[i] = PatchVolume(vv.data_ptr(), tt.data_ptr() if tt is not None else None, ss.data_ptr(), (C.c_int32 * 3)(*b), 0)
        self.records = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(self.device)
        return len(self.volumes) - 1

    def add_subject(self, raw, truth, mean_std=None, mods=preprocess.MODS, scheme=None):
        """raw: (Cm, X, Y, Z) int16 scanner counts (numpy or tensor); truth: (X, Y, Z) / (1, X, Y, Z) uint8 or None; mean_std: the
        dictionary of preprocess.cal_mean_std, or scheme: a preprocess.ZScore, which needs no dictionary (one of the two).
        Normalises and crops on the device (preprocess.normalize_subject), add()s the box
        and notes where it sits: origins[i] (brain_width[0]) and full_shapes[i] are what SubjectPredictor.predict takes as
        origin / full_shape.  Returns the volume's index."""
        if mean_std is None and scheme is None:
            raise N3DError("VolumeSet.add_subject: needs mean_std (preprocess.cal_mean_std) or scheme (preprocess.ZScore)")
        vol, t, brain_width = preprocess.normalize_subject(raw, mean_std, truth, mods, self.device, scheme)
        i = self.add(vol, t)
        self.origins[i] = tuple(int(v) for v in brain_width[0])
        self.full_shapes[i] = tuple(int(v) for v in raw.shape[-3:])
        return i

    def table(self, i):
        """volume i's summed-area tables: (X+1, Y+1, Z+1, 2) int32, (modality mask, label mask), zero planes at the low ends"""
        return self.tables[i]

    def qualify(self, vol_ids, corners, patch):
        """flags (uint8 device tensor, one per candidate) of the patches [corner, corner + patch) of volumes vol_ids: bit 0 some
        modality is nonzero, bit 1 some label is nonzero (0 wholly outside the volume, and for an index outside the set)"""
        ids = np.asarray(vol_ids, dtype=np.int64).reshape(-1)
        cs = np.asarray(corners, dtype=np.int64).reshape(-1, 3)
        if len(ids) != len(cs):
            raise N3DError("VolumeSet.qualify: one volume index per corner")
        table = np.concatenate((ids[:, None], cs), axis=1)
        if table.size and (table.min() < -2 ** 31 or table.max() >= 2 ** 31):
            raise N3DError("VolumeSet.qualify: indices and corners are int32")
        return self.qualify_table(np.ascontiguousarray(table.astype(np.int32)), patch)

    def qualify_table(self, table, patch):
        """qualify() on an (N, 4) int32 table of (volume index, corner): one host -> device copy, one n3d_patch_qualify launch"""
        if not (isinstance(table, np.ndarray) and table.dtype == np.int32 and table.ndim == 2 and table.shape[1] == 4
                and table.flags.c_contiguous):
            raise N3DError("VolumeSet.qualify_table: expected a C-contiguous (N, 4) int32 array")
        N = int(table.shape[0])
        flags = torch.empty(N, dtype=torch.uint8, device=self.device)
        if N:
            cand = torch.from_numpy(table).to(self.device)
            check(_lib.load().n3d_patch_qualify(K.ptr(self.records), len(self), K.ptr(cand), N, int(patch), K.ptr(flags),
                                                K.stream_ptr()), "n3d_patch_qualify")
        return flags

    def line_index(self, i):
        """volume i's line index: (5, X*Y + 1) int32, row m the exclusive prefix counts of mask m's voxels per (x, y) line
        (include/n3d.h, n3d_volume_line_index; masks: sampling.MASKS).  Built on first use (two launches), then kept."""
        if not 0 <= int(i) < len(self):
            raise N3DError("VolumeSet.line_index: no volume %r in a set of %d" % (i, len(self)))
        i = int(i)
        self.line_indexes += [None] * (len(self) - len(self.line_indexes))
        if self.line_indexes[i] is None:
            X, Y, Z = self.boxes[i]
            index = torch.empty((len(sampling_mod.MASKS), X * Y + 1), dtype=torch.int32, device=self.device)
            check(_lib.load().n3d_volume_line_index(K.ptr(self.volumes[i]), self.channels, K.ptr(self.truths[i]), X, Y, Z, K.ptr(index),
                                                    K.stream_ptr()), "n3d_volume_line_index")
            self.line_indexes[i] = index
        return self.line_indexes[i]

    def index_table(self):
        """the device array of the set's line-index addresses (0: not built), rebuilt when a volume or an index was added"""
        have = [t.data_ptr() if t is not None else 0 for t in self.line_indexes] + [0] * (len(self) - len(self.line_indexes))
        if self._index_ptrs_of != have:
            self.index_ptrs = torch.tensor(have, dtype=torch.int64).to(self.device)
            self._index_ptrs_of = have
        return self.index_ptrs

    def sample(self, ids, n, patch, key, foreground=1 / 3, masks=("tumour",)):
        """n crops of edge `patch` from the volumes `ids` (an index may repeat: it is drawn that much more often), by the rule of
        include/n3d.h, n3d_patch_sample: a uniform corner, or with probability `foreground` the corner centring the patch on a
        uniformly random voxel of one of `masks` (sampling.MASKS).  key: the Philox key (k0, k1).  Returns (cand, mode): the device
        (n, 4) int32 table qualify_table / patch_batch understand and the device uint8 modes (the mask 0..4, 255 uniform, 254 no
        requested mask in the volume).  Builds the missing line indexes, then ONE n3d_patch_sample launch and no sync."""
        ids = [int(i) for i in ids]
        if not ids or not all(0 <= i < len(self) for i in ids):
            raise N3DError("VolumeSet.sample: ids are indices of the set's %d volumes, at least one (got %r)" % (len(self), ids))
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= n <= sampling_mod.MAX_SAMPLES:
            raise N3DError("VolumeSet.sample: n is an integer in 0 .. %d (N3D_SAMPLE_MAX; got %r)" % (sampling_mod.MAX_SAMPLES, n))
        bits, thr = sampling_mod.mask_bits(masks, "VolumeSet.sample"), sampling_mod.fg_threshold(foreground, "VolumeSet.sample")
        if thr and bits & ~1 and not self.has_truth:
            raise N3DError("VolumeSet.sample: a set without truth has the mask \"brain\" only (got %r)" % (masks,))
        for i in sorted(set(ids)):
            self.line_index(i)
        n = int(n)
        cand = torch.empty((n, 4), dtype=torch.int32, device=self.device)
        mode = torch.empty(n, dtype=torch.uint8, device=self.device)
        dev_ids = torch.tensor(ids, dtype=torch.int32).to(self.device)
        check(_lib.load().n3d_patch_sample(K.ptr(self.records), K.ptr(self.index_table()), len(self), self.channels, K.ptr(dev_ids),
                                           len(ids), n, int(patch), int(key[0]), int(key[1]), thr, bits, K.ptr(cand), K.ptr(mode),
                                           K.stream_ptr()), "n3d_patch_sample")
        return cand, mode

    def fits(self, out, B, patch, target_dtype):
        """out = (x, t) can take a batch of B patches in place: x (B, Cv, P, P, P) fp32 in NDHWC storage on the set's device, t
        (B, 3, P, P, P) contiguous of target_dtype (ignored without truth)"""
        if out is None or len(out) < 2 or out[0] is None:
            return False
        x, t = out[0], out[1]
        P = int(patch)
        if not (isinstance(x, torch.Tensor) and x.device == self.device and x.dtype == torch.float32
                and tuple(x.shape) == (B, self.channels, P, P, P)):
            return False
        ld = K._pitch_of(x)
        if ld is None or x.data_ptr() % 16 or (ld % 4 and self.channels % 4 == 0):
            return False
        if not self.has_truth:
            return True
        return (isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == target_dtype and t.is_contiguous()
                and tuple(t.shape) == (B, 3, P, P, P))

    def _warp_descs(self, refs, P, augment, warp):
        """the n3d_patch_wdesc table of a warped batch (patch_batch): entry i takes its flips and its scale map (A, sh) from augment[i]
        and its matrix, interpolation order and intensity map from warp[i]; a None entry changes nothing"""
        B = len(refs)
        if warp is None:
            warp = [None] * B
        if len(warp) != B or (augment is not None and len(augment) != B):
            raise N3DError("VolumeSet.patch_batch: one warp entry (or None) and one augmentation (or None) per ref")
        if B > WARP_MAX_BATCH:
            raise N3DError("VolumeSet.patch_batch: a warped batch holds at most %d patches (N3D_PATCH_WARP_MAX_BATCH)" % WARP_MAX_BATCH)
        descs = (WarpDesc * B)()
        for i, (v, corner, key) in enumerate(refs):
            perm, flip = _isometry(key)
            g = GatherDesc(PatchDesc((C.c_int32 * 3)(*[int(c) for c in corner]), (C.c_int32 * 3)(*perm),
                                     (C.c_int32 * 3)(*[int(f) for f in flip])), int(v))
            a = augment[i] if augment is not None and augment[i] is not None else ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), True, None)
            A, sh, identity, axes = a
            aflip = [int(n in axes) for n in range(3)] if axes else [0, 0, 0]
            matrix, order, gain, bias = warp[i] if warp[i] is not None else (None, 0, None, None)
            if int(order) not in (0, 1, 3):
                raise N3DError("VolumeSet.patch_batch: the interpolation order is 0 (nearest), 1 (linear) or 3 (cubic B-spline)")
            if matrix is not None:
                M, off = (np.asarray(m, np.float64) for m in matrix)
                if M.shape != (3, 3) or off.shape != (3,):
                    raise N3DError("VolumeSet.patch_batch: a warp entry's matrix is (M (3, 3), off (3,)) as warp_transform gives them")
                mode, k = 1, [float(m) for m in M.reshape(-1)] + [float(o) for o in off]
            elif identity:
                mode, k = 0, [1.0] * 3 + [0.0] * 9
            else:
                mode, k = 0, [float(n) for n in A] + [float(h) for h in sh] + [0.0] * 6
            intensity = gain is not None or bias is not None
            if intensity and self.channels > WARP_MAX_CHANNELS:
                raise N3DError("VolumeSet.patch_batch: the intensity map supports at most %d channels (the set has %d)" % (
                    WARP_MAX_CHANNELS, self.channels))
            gn, bs = [1.0] * 4, [0.0] * 4
            if gain is not None:
                gn[:self.channels] = [float(x) for x in np.asarray(gain, np.float64).reshape(self.channels)]
            if bias is not None:
                bs[:self.channels] = [float(x) for x in np.asarray(bias, np.float64).reshape(self.channels)]
            descs[i] = WarpDesc(g, (C.c_int32 * 3)(*aflip), mode, int(order), int(intensity), (C.c_double * 12)(*k),
                                (C.c_float * 4)(*gn), (C.c_float * 4)(*bs))
        orders = {int(d.order) for d in descs}
        if 3 in orders and len(orders) > 1:
            raise N3DError("VolumeSet.patch_batch: order 3 (cubic B-spline) takes the whole batch through its own launches: every warp "
                           "entry of the batch has order 3, or none (got the orders %s)" % sorted(orders))
        return descs

    def _elastic_descs(self, refs, P, augment, warp, elastic):
        """the n3d_patch_edesc table of a batch with a deformed patch (patch_batch): entry i is _warp_descs' record plus elastic[i] =
        (cells, lock, key, amp); a None entry leaves the patch to the warp rule alone"""
        B = len(refs)
        if len(elastic) != B:
            raise N3DError("VolumeSet.patch_batch: one elastic entry (or None) per ref")
        if B > ELASTIC_MAX_BATCH:
            raise N3DError("VolumeSet.patch_batch: a batch with an elastic deformation holds at most %d patches "
                           "(N3D_PATCH_ELASTIC_MAX_BATCH)" % ELASTIC_MAX_BATCH)
        wdescs = self._warp_descs(refs, P, augment, warp)
        descs = (ElasticDesc * B)()
        for i, e in enumerate(elastic):
            if e is None:
                descs[i] = ElasticDesc(wdescs[i], 0, 1, 0, (C.c_uint32 * 2)(0, 0), 0, (C.c_double * 3)(0.0, 0.0, 0.0), 0.0)
                continue
            cells, lock, key, amp = e
            elastic_mod.check_lattice(cells, lock, "VolumeSet.patch_batch")
            amp = np.broadcast_to(np.asarray(amp, np.float64), (3,))
            if not np.isfinite(amp).all() or (amp < 0).any():
                raise N3DError("VolumeSet.patch_batch: an elastic entry's amp is finite and >= 0 (got %r)" % (e[3],))
            descs[i] = ElasticDesc(wdescs[i], 1, int(cells), int(lock), (C.c_uint32 * 2)(int(key[0]), int(key[1])), 0,
                                   (C.c_double * 3)(*[float(a) for a in amp]), float(elastic_mod.inv_h(cells, P)))
        return descs

    def patch_batch(self, refs, patch, inclusive_label=False, target_dtype=torch.float32, out=None, augment=None, warp=None, elastic=None):
        """One batch whose patches come from any volumes of the set: refs = [(volume index, corner, isometry key or None)].
        What datastep.patch_batch makes of each patch on its own volume, bit for bit, in ONE n3d_patch_gather launch on the current
        stream.  Returns (x, t): x (B, Cv, P, P, P) fp32 in NDHWC storage, t (B, 3, P, P, P) of target_dtype (None without truth).
        out=(x, t): written in place (NDHWC x, contiguous t; t's dtype then decides the target dtype), as datastep.patch_batch.
        augment: None, or one entry per ref -- None, or (A, sh, identity, flipped axes) as resample_params gives them: the crop
        of that ref is flipped on those axes and resampled (include/n3d.h, n3d_patch_adesc) ahead of its isometry.  With some
        entry not None the batch is ONE n3d_patch_gather_aug launch (at most 32 patches); otherwise exactly the launch above.
        warp: None, or one entry per ref -- None, or (matrix or None, order, gain or None, bias or None): matrix = (M, off) as
        warp_transform gives them (the rotation composed with the ref's scale map (A, b): it replaces the ref's (A, sh), which hold
        b / A and not b; the flipped axes of augment still apply), order 0 / 1 = nearest / linear interpolation of the data (the truth
        stays nearest), gain / bias = Cv factors / offsets applied to the nonzero voxels (include/n3d.h, n3d_patch_wdesc).  With
        some entry not None the batch is ONE n3d_patch_gather_warp launch (at most 16 patches): the matrix rule for the entries
        with a matrix, the zoom-shift rule with the entry's (A, sh) otherwise.  Otherwise the launches are exactly the ones above.
        elastic: None, or one entry per ref -- None, or (cells, lock, key, amp): the cubic B-spline displacement of include/n3d.h,
        n3d_patch_edesc (cells per axis, locked border layers, the Philox key (k0, k1) of the control values, the largest displacement
        in voxels -- a scalar or one per axis) is added to that ref's coordinate, whatever augment and warp make of it.  With some entry
        not None the batch is ONE n3d_patch_gather_elastic launch (at most 8 patches).  Otherwise the launches are exactly the ones
        above.
        Order 3 in a warp entry: the data is interpolated by a cubic B-spline, scipy's map_coordinates(order=3, mode="constant") on the
        crop, stored as 0 where order 0 would read 0 (include/n3d.h, n3d_patch_gather_spline).  Then EVERY entry of the batch has
        order 3 (a None entry counts as order 0; mixing raises), the batch holds at most 8 patches of at least 4 voxels an edge and is
        five launches (crop, three prefilter passes, gather), with or without elastic entries, over a scratch of 12 bytes per voxel and
        channel that the set allocates at the first batch of a (B, Cv, P) and reuses."""
        if target_dtype not in (torch.float32, torch.uint8):
            raise N3DError("VolumeSet.patch_batch: targets are float32 or uint8")
        B, P = len(refs), int(patch)
        if B < 1 or not self.volumes:
            raise N3DError("VolumeSet.patch_batch: need at least one patch of a non-empty set")
        deformed = elastic is not None and any(e is not None for e in elastic)
        warped = deformed or (warp is not None and any(w is not None for w in warp))
        augmented = not warped and augment is not None and any(a is not None for a in augment)
        if augmented and len(augment) != B:
            raise N3DError("VolumeSet.patch_batch: one augmentation (or None) per ref")
        if augmented and B > AUG_MAX_BATCH:
            raise N3DError("VolumeSet.patch_batch: an augmented batch holds at most %d patches (N3D_PATCH_AUG_MAX_BATCH)" % AUG_MAX_BATCH)
        spline = warp is not None and any(w is not None and int(w[1]) == spline_mod.ORDER for w in warp)
        if spline:
            if B > ELASTIC_MAX_BATCH:
                raise N3DError("VolumeSet.patch_batch: a batch interpolated at order 3 holds at most %d patches "
                               "(N3D_PATCH_ELASTIC_MAX_BATCH)" % ELASTIC_MAX_BATCH)
            if P < spline_mod.MIN_PATCH:
                raise N3DError("VolumeSet.patch_batch: order 3 needs a patch of at least %d voxels an edge (got %d)" % (spline_mod.MIN_PATCH, P))
            descs = self._elastic_descs(refs, P, augment, warp, elastic if elastic is not None else [None] * B)
        elif deformed:
            descs = self._elastic_descs(refs, P, augment, warp, elastic)
        else:
            descs = self._warp_descs(refs, P, augment, warp) if warped else ((AugDesc if augmented else GatherDesc) * B)()
        for i, (v, corner, key) in enumerate(() if warped else refs):
            perm, flip = _isometry(key)
            g = GatherDesc(PatchDesc((C.c_int32 * 3)(*[int(c) for c in corner]), (C.c_int32 * 3)(*perm),
                                     (C.c_int32 * 3)(*[int(f) for f in flip])), int(v))
            if not augmented:
                descs[i] = g
                continue
            A, sh, identity, axes = augment[i] if augment[i] is not None else ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), True, None)
            aflip = [int(a in axes) for a in range(3)] if axes else [0, 0, 0]
            descs[i] = AugDesc(g, (C.c_int32 * 3)(*aflip), int(bool(identity)), (C.c_double * 3)(*[float(a) for a in A]),
                               (C.c_double * 3)(*[float(h) for h in sh]))
        Cv = self.channels
        if out is not None:
            x, t = out
            if not self.has_truth:
                t = None
            if not (isinstance(x, torch.Tensor) and x.device == self.device and x.dtype == torch.float32 and tuple(x.shape) == (B, Cv, P, P, P)):
                raise N3DError(f"VolumeSet.patch_batch: out[0] must be a ({B}, {Cv}, {P}, {P}, {P}) fp32 tensor on {self.device}")
            if t is not None:
                if not (isinstance(t, torch.Tensor) and t.device == self.device and t.is_contiguous() and t.dtype in (torch.float32, torch.uint8)
                        and tuple(t.shape) == (B, 3, P, P, P)):
                    raise N3DError(f"VolumeSet.patch_batch: out[1] must be a contiguous ({B}, 3, {P}, {P}, {P}) float32 or uint8 tensor on {self.device}")
                target_dtype = t.dtype
            xv = K.as_view(x)
            if xv.t is not x:
                raise N3DError("VolumeSet.patch_batch: out[0] must be in NDHWC (channels-last) storage, as K.empty_ndhwc / "
                               "Trainer.input_buffers() give it")
        else:
            x = K.empty_ndhwc(B, Cv, P, P, P, self.device, torch.float32)
            t = torch.empty((B, 3, P, P, P), dtype=target_dtype, device=self.device) if self.has_truth else None
            xv = K.as_view(x)
        flags = (_lib.PATCH_INCLUSIVE if inclusive_label else 0) | (_lib.PATCH_T_U8 if target_dtype == torch.uint8 else 0)
        if spline:
            lib = _lib.load()
            scratch = self._spline_scratch.get((B, Cv, P))
            if scratch is None:
                scratch = self._spline_scratch[(B, Cv, P)] = torch.empty(int(lib.n3d_patch_spline_scratch_bytes(B, Cv, P)), dtype=torch.uint8,
                                                                         device=self.device)
            check(lib.n3d_patch_gather_spline(K.ptr(self.records), len(self), Cv, descs, B, P, flags, K.ptr(scratch), scratch.numel(), xv.p,
                                              xv.ld, K.ptr(t), K.stream_ptr()), "n3d_patch_gather_spline")
        elif deformed:
            check(_lib.load().n3d_patch_gather_elastic(K.ptr(self.records), len(self), Cv, descs, B, P, flags, xv.p, xv.ld, K.ptr(t),
                                                       K.stream_ptr()), "n3d_patch_gather_elastic")
        elif warped:
            check(_lib.load().n3d_patch_gather_warp(K.ptr(self.records), len(self), Cv, descs, B, P, flags, xv.p, xv.ld, K.ptr(t),
                                                    K.stream_ptr()), "n3d_patch_gather_warp")
        elif augmented:
            check(_lib.load().n3d_patch_gather_aug(K.ptr(self.records), len(self), Cv, descs, B, P, flags, xv.p, xv.ld, K.ptr(t),
                                                   K.stream_ptr()), "n3d_patch_gather_aug")
        else:
            check(_lib.load().n3d_patch_gather(K.ptr(self.records), len(self), Cv, descs, B, P, flags, xv.p, xv.ld, K.ptr(t),
                                               K.stream_ptr()), "n3d_patch_gather")
        return x, t


class Generator:
    """generator.py:68-217 (class Generator) over a VolumeSet.  The reference's signature, except: `data_file` is a VolumeSet (its
    indices are the reference's h5 key indices); spe_file is gone; affine_file is `affine`, the 4x4 array itself (np.load of that
    file; None: the identity); labels is None or [1, 2, 4]; patches are cubic.  rng: any random.Random-like object (default: the
    `random` module, as the reference) -- it sees exactly the reference's calls: randint (overlap, per epoch_init), shuffle (per
    epoch), choice (one key per kept patch with permute).

    augment=True: the reference's scale / flip distortion of every kept patch (augment.py:50-67), ahead of its isometry: a scale
    drawn per axis around the patch centre (augment_distortion_factor: the standard deviation around 1, None: no scale), axis flips
    (augment_flip), data and truth resampled alike with nearest neighbour.  np_rng: any np.random-like object (default: the
    np.random module, as the reference -- its global generator, NOT `random`): it sees normal(1, factor, 3) and then three
    choice([True, False]) per kept patch, just before rng's key draw.  The affine's 3x3 part must be diagonal and batch_size at
    most 32 (N3D_PATCH_AUG_MAX_BATCH); a `data_file` whose patch_batch takes no `augment` raises NotImplementedError at
    construction.  The resampler is scipy.ndimage.affine_transform's rule as nilearn calls it (order 0, mode "constant"),
    restated in the kernel; nilearn itself was never run against it.

    Beyond the reference, all acting only with augment=True (setting one with augment=False raises N3DError) and all composed into
    the batch's single launch (n3d_patch_gather_warp; batch_size at most 16, N3D_PATCH_WARP_MAX_BATCH):
    augment_rotation=r (degrees; a scalar or three per-axis maxima): a rotation Rz.Ry.Rx by angles uniform in [-r, r] about the
    patch's voxel centre, in voxel space, ahead of the scale map (rotation_matrix, warp_transform);
    augment_interpolation="linear": the data is interpolated linearly over the eight voxels around the coordinate; the truth stays
    nearest neighbour;
    augment_interpolation="spline3": the data is interpolated by a cubic B-spline -- scipy's map_coordinates(order=3, mode="constant")
    on the crop, nnU-Net's / batchgenerators' / TorchIO's default -- and stored as exactly 0 where nearest neighbour would read 0, so
    the background stays background; no clamping, the spline overshoots at edges as scipy's does; the truth stays nearest neighbour.
    The draws are those of "linear".  Every batch is then n3d_patch_gather_spline's five launches (include/n3d.h) over a scratch of 12
    bytes per voxel and channel that the volume set keeps; batch_size at most 8 (N3D_PATCH_ELASTIC_MAX_BATCH), patches of at least
    4 voxels an edge;
    augment_intensity_scale=g / augment_intensity_shift=s: every modality's NONZERO voxels are multiplied by a factor uniform in
    [1 - g, 1 + g] and shifted by a normal(0, s) offset, per patch and modality (at most 4 channels); background stays exactly 0.
    np_rng then sees, per kept patch and after draw_augment's calls: uniform(-r, r, 3), uniform(1 - g, 1 + g, Cv), normal(0, s, Cv),
    each only if its option is set (draw_warp), and then rng's key draw.  With all four at their defaults the generator makes the
    calls, launches and bits it made without them.

    augment_appearance=appearance.Appearance(...): Gaussian noise, Gaussian blur, contrast and gamma of the brain voxels of the
    gathered data (include/n3d.h, n3d_appear_desc), applied in place by n3d_patch_appearance after the batch's gather and before it is
    yielded -- in the trainer's input buffers when the batch went there; the truth is never touched.  Also only with augment=True
    (else N3DError); batch_size at most 16 (N3D_APPEAR_MAX_BATCH), at most 4 channels.  np_rng sees Appearance.draw's calls per
    kept patch right after draw_warp's and before rng's key draw.  It composes with every option above; left None, the generator
    makes the calls, draws, launches and bits it made without it.

    augment_artefact=artefact.Artefact(...): simulated low resolution, a multiplicative bias field and modality dropout of the
    gathered data (include/n3d.h, n3d_patch_artefact), applied in place by n3d_patch_artefact after the appearance transforms and
    before the batch is yielded -- in the trainer's input buffers when the batch went there; the truth is never touched.  Also only
    with augment=True (else N3DError); batch_size at most 16 (N3D_APPEAR_MAX_BATCH), at most 4 channels, patches of 2 to 256 voxels
    an edge.  np_rng sees Artefact.draw's calls per kept patch right after Appearance.draw's and before rng's key draw.  It composes
    with every option above; left None, the generator makes the calls, draws, launches and bits it made without it.

    augment_elastic=elastic.Elastic(...): a non-rigid displacement of the crop, added to the coordinate the options above give
    (include/n3d.h, n3d_patch_edesc): a cubic B-spline free-form deformation on a lattice of cells + 3 control points per axis whose
    values the device generates from a key drawn per patch; data and truth move alike.  Also only with augment=True (else N3DError);
    batch_size at most 8 (N3D_PATCH_ELASTIC_MAX_BATCH); Elastic.check(patch) -- the folding bound -- runs at construction; a
    `data_file` whose patch_batch takes no `elastic` raises NotImplementedError.  np_rng sees Elastic.draw's calls per kept patch
    right after draw_warp's and before Appearance.draw's: uniform(), and for a deformed patch randint(0, 2**32, 2, dtype=np.uint32).
    A batch with a deformed patch is ONE n3d_patch_gather_elastic launch, any other batch the launch it was without the option.  It
    composes with every option above; left None, the generator makes the calls, draws, launches and bits it made without it.

    sampling=sampling.RandomCrop(patches_per_epoch, foreground, masks): the epoch's candidates are not the grid's but crops drawn on
    the device (include/n3d.h, n3d_patch_sample): patches_per_epoch of them over indices_list, each a uniformly random corner or,
    with probability `foreground`, the corner centring the patch on a uniformly random voxel of one of `masks`.  patch_overlap and
    both_ps describe the grid and raise N3DError with it, and so does a mask other than "brain" on a set without truth.
    epoch_init() then draws the epoch's key from np_rng -- randint(0, 2**32, 2, dtype=np.uint32), ahead of every other draw of the
    epoch --, builds the line indexes that are missing, makes ONE n3d_patch_sample launch, copies the table and the modes to the
    host (candidates, sample_modes, sample_key) and qualifies the table as it does the grid's: skip_health and the empty-patch
    filter keep their meaning, n_patches and steps_per_epoch follow from the flags.  epoch() calls epoch_init() after its last
    batch, so every epoch has fresh crops.  Left None, the generator makes the calls, draws, launches and bits it made without it.

    epoch_init(): one n3d_patch_qualify launch and one device -> host copy of the candidates' flag bytes.
    epoch(out=None): a generator of (x, t) device tensors (t None without truth), one n3d_patch_gather launch per batch
    (n3d_patch_gather_aug with augment) on the current stream.  out: a tuple (x, t) or a zero-argument callable returning one (e.g. trainer.input_buffers), evaluated per
    batch; a batch is written into it when it fits (shape, dtype, NDHWC x), else -- None entries, the smaller last batch -- into
    fresh tensors.  A batch written into a trainer's buffers is overwritten by the next next(): step on it first."""

    def __init__(self, indices_list, volumes, patch_shape, patch_overlap=None, batch_size=1, labels=None, augment=False, permute=False,
                 shuffle_index_list=True, skip_health=True, inclusive_label=False, both_ps=False, target_dtype=torch.float32, rng=None,
                 augment_flip=True, augment_distortion_factor=0.25, affine=None, np_rng=None, augment_rotation=None,
                 augment_interpolation="nearest", augment_intensity_scale=None, augment_intensity_shift=None, augment_appearance=None,
                 augment_artefact=None, augment_elastic=None, sampling=None):
        if labels is not None and list(labels) != LABELS:
            raise N3DError("Generator: labels must be None or [1, 2, 4] (the three BraTS regions the kernels expand)")
        ps = [patch_shape] * 3 if isinstance(patch_shape, int) else [int(p) for p in patch_shape]
        if len(ps) != 3 or len(set(ps)) != 1 or ps[0] < 1:
            raise N3DError("Generator: patches are cubic (got %s)" % (patch_shape,))
        if not 1 <= int(batch_size) <= MAX_BATCH:
            raise N3DError("Generator: batch_size must be 1..%d" % MAX_BATCH)
        if target_dtype not in (torch.float32, torch.uint8):
            raise N3DError("Generator: targets are float32 or uint8")
        if augment and int(batch_size) > AUG_MAX_BATCH:
            raise N3DError("Generator: batch_size must be 1..%d with augment=True (N3D_PATCH_AUG_MAX_BATCH)" % AUG_MAX_BATCH)
        if augment_interpolation not in INTERPOLATION_ORDER:
            raise N3DError("Generator: augment_interpolation is 'nearest', 'linear' or 'spline3' (got %r)" % (augment_interpolation,))
        intensity = augment_intensity_scale is not None or augment_intensity_shift is not None
        warped = augment_rotation is not None or augment_interpolation != "nearest" or intensity
        if warped and not augment:
            raise N3DError("Generator: augment_rotation, augment_interpolation and augment_intensity_scale / _shift act only with "
                           "augment=True")
        if warped and int(batch_size) > WARP_MAX_BATCH:
            raise N3DError("Generator: batch_size must be 1..%d with a rotation, linear interpolation or an intensity map "
                           "(N3D_PATCH_WARP_MAX_BATCH)" % WARP_MAX_BATCH)
        if augment_interpolation == "spline3":
            if int(batch_size) > ELASTIC_MAX_BATCH:
                raise N3DError("Generator: batch_size must be 1..%d with augment_interpolation='spline3' (N3D_PATCH_ELASTIC_MAX_BATCH)"
                               % ELASTIC_MAX_BATCH)
            if ps[0] < spline_mod.MIN_PATCH:
                raise N3DError("Generator: augment_interpolation='spline3' needs patches of at least %d voxels an edge (got %d)" % (
                    spline_mod.MIN_PATCH, ps[0]))
        if augment_rotation is not None:
            r = np.asarray(augment_rotation, np.float64)
            if r.shape not in ((), (3,)) or not np.isfinite(r).all() or (r < 0).any():
                raise N3DError("Generator: augment_rotation is a maximum angle in degrees, a scalar or one per axis (got %r)" % (
                    augment_rotation,))
        for name, val in (("augment_intensity_scale", augment_intensity_scale), ("augment_intensity_shift", augment_intensity_shift)):
            if val is not None and not (np.ndim(val) == 0 and np.isfinite(val) and val >= 0):
                raise N3DError("Generator: %s is a non-negative number (got %r)" % (name, val))
        if augment_appearance is not None:
            if not isinstance(augment_appearance, appearance.Appearance):
                raise N3DError("Generator: augment_appearance is an appearance.Appearance (got %r)" % (augment_appearance,))
            if not augment:
                raise N3DError("Generator: augment_appearance acts only with augment=True")
            if int(batch_size) > appearance.MAX_BATCH:
                raise N3DError("Generator: batch_size must be 1..%d with augment_appearance (N3D_APPEAR_MAX_BATCH)" % appearance.MAX_BATCH)
            channels = getattr(volumes, "channels", None)
            if channels is not None and channels > appearance.MAX_CHANNELS:
                raise N3DError("Generator: augment_appearance supports at most %d channels (the set has %d)" % (
                    appearance.MAX_CHANNELS, channels))
        self.augment_appearance = augment_appearance
        if augment_artefact is not None:
            if not isinstance(augment_artefact, artefact_mod.Artefact):
                raise N3DError("Generator: augment_artefact is an artefact.Artefact (got %r)" % (augment_artefact,))
            if not augment:
                raise N3DError("Generator: augment_artefact acts only with augment=True")
            if int(batch_size) > artefact_mod.MAX_BATCH:
                raise N3DError("Generator: batch_size must be 1..%d with augment_artefact (N3D_APPEAR_MAX_BATCH)" % artefact_mod.MAX_BATCH)
            if not 2 <= ps[0] <= artefact_mod.MAX_PATCH:
                raise N3DError("Generator: augment_artefact supports patches of 2..%d voxels an edge (N3D_APPEAR_MAX_PATCH; got %d)" % (
                    artefact_mod.MAX_PATCH, ps[0]))
            channels = getattr(volumes, "channels", None)
            if channels is not None and channels > artefact_mod.MAX_CHANNELS:
                raise N3DError("Generator: augment_artefact supports at most %d channels (the set has %d)" % (
                    artefact_mod.MAX_CHANNELS, channels))
        self.augment_artefact = augment_artefact
        if augment_elastic is not None:
            if not isinstance(augment_elastic, elastic_mod.Elastic):
                raise N3DError("Generator: augment_elastic is an elastic.Elastic (got %r)" % (augment_elastic,))
            if not augment:
                raise N3DError("Generator: augment_elastic acts only with augment=True")
            if int(batch_size) > ELASTIC_MAX_BATCH:
                raise N3DError("Generator: batch_size must be 1..%d with augment_elastic (N3D_PATCH_ELASTIC_MAX_BATCH)" % ELASTIC_MAX_BATCH)
            augment_elastic.check(ps[0])
        self.augment_elastic = augment_elastic
        if sampling is not None:
            if not isinstance(sampling, sampling_mod.RandomCrop):
                raise N3DError("Generator: sampling is a sampling.RandomCrop (got %r)" % (sampling,))
            if patch_overlap is not None or both_ps:
                raise N3DError("Generator: patch_overlap and both_ps describe the candidate grid, which sampling replaces")
            if not callable(getattr(volumes, "sample", None)):
                raise NotImplementedError("Generator: sampling needs a volume set that draws crops on the device (VolumeSet.sample); "
                                          "%s has none" % type(volumes).__name__)
            if sampling.needs_truth() and not getattr(volumes, "has_truth", False):
                raise N3DError("Generator: sampling from the masks %r needs a volume set with truth (without it there is \"brain\" only)"
                               % (sampling.masks,))
        self.sampling = sampling
        self.sample_key = self.sample_modes = None
        self.affine = check_affine(affine) if augment else affine
        if augment:
            # fail here, not in the middle of an epoch with draws already consumed: the batches are made by volumes.patch_batch,
            # and a volume set that stands in for VolumeSet may not have the augmented gather
            gather = getattr(volumes, "patch_batch", None)
            if gather is None or "augment" not in inspect.signature(gather).parameters:
                raise NotImplementedError("Generator: augment=True needs a volume set whose patch_batch(..., augment=) resamples in "
                                          "the gather (VolumeSet); %s has none" % type(volumes).__name__)
            if warped and "warp" not in inspect.signature(gather).parameters:
                raise NotImplementedError("Generator: augment_rotation / augment_interpolation / augment_intensity_* need a volume set "
                                          "whose patch_batch(..., warp=) resamples in the gather (VolumeSet); %s has none"
                                          % type(volumes).__name__)
            if augment_elastic is not None and "elastic" not in inspect.signature(gather).parameters:
                raise NotImplementedError("Generator: augment_elastic needs a volume set whose patch_batch(..., elastic=) deforms in the "
                                          "gather (VolumeSet); %s has none" % type(volumes).__name__)
            channels = getattr(volumes, "channels", None)
            if intensity and channels is not None and channels > WARP_MAX_CHANNELS:
                raise N3DError("Generator: the intensity map supports at most %d channels (the set has %d)" % (WARP_MAX_CHANNELS, channels))
        self.augment = bool(augment)
        self.augment_flip = augment_flip
        self.augment_distortion_factor = augment_distortion_factor
        self.np_rng = np.random if np_rng is None else np_rng
        self.warped = warped
        self.augment_rotation = augment_rotation
        self.augment_interpolation = augment_interpolation
        self.augment_intensity_scale = augment_intensity_scale
        self.augment_intensity_shift = augment_intensity_shift
        self.indices_list = list(indices_list)
        self.volumes = volumes
        self.patch_shape = ps
        self.patch = ps[0]
        self.patch_overlap = patch_overlap
        self.batch_size = int(batch_size)
        self.labels = labels
        self.permute = permute
        self.shuffle_index_list = shuffle_index_list
        self.skip_health = skip_health
        self.inclusive_label = inclusive_label
        self.both_ps = both_ps
        self.target_dtype = target_dtype
        self.rng = random if rng is None else rng
        self.epoch_init()

    def epoch_init(self):
        """generator.py:118-168: draw the epoch's overlap, list the candidates, qualify them on the device, count the kept ones"""
        if self.sampling is not None:
            return self._sampled_epoch_init()
        ov = draw_overlap(self.patch_overlap, self.rng)
        if ov is not None and ov >= self.patch:
            raise N3DError("Generator: drawn overlap %d >= patch %d -- the reference divides by zero here (patches.py:59-67: the "
                           "fixed-overlap pitch patch - overlap is %d; np.mgrid step 0)" % (ov, self.patch, self.patch - ov))
        self.overlap = ov
        self.candidates = candidate_table([self.volumes.box(i) for i in range(len(self.volumes))], self.indices_list, self.patch,
                                          ov, self.both_ps)
        self.flags = self.volumes.qualify_table(self.candidates, self.patch).cpu().numpy()
        self.n_patches = int(kept_mask(self.flags, self._skip_health()).sum())
        self.steps_per_epoch = -(-self.n_patches // self.batch_size)

    def _sampled_epoch_init(self):
        """epoch_init() with sampling: the epoch's key, one n3d_patch_sample launch over indices_list, the table and the modes to the
        host, then the grid's qualification"""
        c = self.sampling
        self.overlap = None
        self.sample_key = c.draw(self.np_rng)
        cand, mode = self.volumes.sample(self.indices_list, c.patches_per_epoch, self.patch, self.sample_key, c.foreground, c.masks)
        self.candidates = cand.cpu().numpy()
        self.sample_modes = mode.cpu().numpy()
        self.flags = self.volumes.qualify_table(self.candidates, self.patch).cpu().numpy()
        self.n_patches = int(kept_mask(self.flags, self._skip_health()).sum())
        self.steps_per_epoch = -(-self.n_patches // self.batch_size)

    def _skip_health(self):
        # np.all(None == 0) is False (generator.py:206): without truth nothing is skipped as healthy
        return bool(self.skip_health) and bool(self.volumes.has_truth)

    def epoch(self, out=None):
        cand = self.candidates
        draws = (self.np_rng, self.augment_distortion_factor, self.augment_flip) if self.augment else None
        if self.warped:
            yield from self._warped_epoch(out, draws)
            return
        for batch in epoch_order(self.flags, self.batch_size, self.rng, self._skip_health(), self.shuffle_index_list, self.permute,
                                 augment=draws, appearance=self._appearance_draws(), **self._elastic_draws(), **self._artefact_draws()):
            o = out() if callable(out) else out
            B = len(batch)
            refs = [(cand[e[0], 0], cand[e[0], 1:], e[1]) for e in batch]
            aug = [resample_params(self.affine, self.patch, e[2][0]) + (e[2][1],) for e in batch] if self.augment else None
            fit = o if self.volumes.fits(o, B, self.patch, self.target_dtype) else None
            yield self._appear(self.volumes.patch_batch(refs, self.patch, self.inclusive_label, self.target_dtype, out=fit, augment=aug,
                                                        **self._elastic_entries(batch, 3)), batch)
        if self.patch_overlap or self.sampling is not None:
            self.epoch_init()

    def _appearance_draws(self):
        a = self.augment_appearance
        return (self.np_rng, a, self.volumes.channels) if a is not None else None

    def _artefact_draws(self):
        """epoch_order's `artefact` argument: absent without the option, so that a stand-in epoch_order sees today's call"""
        a = self.augment_artefact
        return {"artefact": (self.np_rng, a, self.volumes.channels)} if a is not None else {}

    def _elastic_draws(self):
        """epoch_order's `elastic` argument: absent without the option, so that a stand-in epoch_order sees today's call"""
        return {"elastic": (self.np_rng, self.augment_elastic)} if self.augment_elastic is not None else {}

    def _elastic_entries(self, batch, at):
        """patch_batch's `elastic` argument from element `at` of the batch's entries: absent without the option"""
        if self.augment_elastic is None:
            return {}
        return {"elastic": [self.augment_elastic.entry(e[at]) for e in batch]}

    def _appear(self, xt, batch):
        """the batch's appearance draws and then its artefact draws applied to the gathered x where it lies -- the trainer's input
        buffers when the batch went there; the truth is never touched.  The artefact draw is the last element of an entry; the
        appearance draw is the last one without it and the one before it with it."""
        art = self.augment_artefact is not None
        if self.augment_appearance is not None:
            self.augment_appearance.apply(xt[0], [e[-2 if art else -1] for e in batch])
        if art:
            self.augment_artefact.apply(xt[0], [e[-1] for e in batch])
        return xt

    def _warped_epoch(self, out, draws):
        """epoch() with one of the rotation / interpolation / intensity options set: every batch is one n3d_patch_gather_warp launch"""
        cand, P = self.candidates, self.patch
        order = INTERPOLATION_ORDER[self.augment_interpolation]
        wdraws = (self.np_rng, self.augment_rotation, self.augment_intensity_scale, self.augment_intensity_shift, self.volumes.channels)
        for batch in epoch_order(self.flags, self.batch_size, self.rng, self._skip_health(), self.shuffle_index_list, self.permute,
                                 augment=draws, warp=wdraws, appearance=self._appearance_draws(), **self._elastic_draws(),
                                 **self._artefact_draws()):
            o = out() if callable(out) else out
            B = len(batch)
            refs = [(cand[e[0], 0], cand[e[0], 1:], e[1]) for e in batch]
            aug, warp = [], []
            for (scale, axes), (angles, gain, bias) in (e[2:4] for e in batch):
                A, b, identity = resample_transform(self.affine, P, scale)
                aug.append((A, b / A, identity, axes))
                matrix = warp_transform(A, b, rotation_matrix(angles), P) if angles is not None else None
                warp.append((matrix, order, gain, bias))
            fit = o if self.volumes.fits(o, B, P, self.target_dtype) else None
            yield self._appear(self.volumes.patch_batch(refs, P, self.inclusive_label, self.target_dtype, out=fit, augment=aug, warp=warp,
                                                        **self._elastic_entries(batch, 4)), batch)
        if self.patch_overlap or self.sampling is not None:
            self.epoch_init()
