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
    host sync and no host -> device copy per batch.

Host logic only; the kernels are n3d_volume_sat, n3d_patch_qualify and n3d_patch_gather (include/n3d.h).
"""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import torch

from . import _lib, datastep, predict, preprocess
from . import kernels as K
from ._lib import GatherDesc, N3DError, PatchDesc, PatchVolume, check

# augment.py:95-100 draws from list(set(...)): that (deterministic) order, NOT the sorted one of datastep.random_permutation_key
KEYS = list(datastep.generate_permutation_keys())
LABELS = [1, 2, 4]
MAX_BATCH = 64      # N3D_PATCH_MAX_BATCH

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


def epoch_order(flags, batch_size, rng, skip_health=True, shuffle=True, permute=False):
    """generator.py:170-217 on qualification flags: yields each batch as a list of (candidate index, isometry key or None).
    The candidate order is shuffled at the first next() (rng.shuffle, if `shuffle`), then pop()ped from the end; a kept candidate
    draws its key (rng.choice over KEYS, if `permute`) when it is popped; a batch is yielded when full, or when the list is empty.
    skip_health: the caller's skip_health AND the set has truth (without truth the reference skips nothing as healthy)."""
    keep = kept_mask(flags, skip_health).tolist()
    order = list(range(len(keep)))
    if shuffle:
        rng.shuffle(order)
    batch = []
    while order:
        i = order.pop()
        if keep[i]:
            batch.append((i, rng.choice(KEYS) if permute else None))
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

    def add_subject(self, raw, truth, mean_std, mods=preprocess.MODS):
        """raw: (Cm, X, Y, Z) int16 scanner counts (numpy or tensor); truth: (X, Y, Z) / (1, X, Y, Z) uint8 or None; mean_std: the
        dictionary of preprocess.cal_mean_std.  Normalises and crops on the device (preprocess.normalize_subject), add()s the box
        and notes where it sits: origins[i] (brain_width[0]) and full_shapes[i] are what SubjectPredictor.predict takes as
        origin / full_shape.  Returns the volume's index."""
        vol, t, brain_width = preprocess.normalize_subject(raw, mean_std, truth, mods, self.device)
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

    def patch_batch(self, refs, patch, inclusive_label=False, target_dtype=torch.float32, out=None):
        """One batch whose patches come from any volumes of the set: refs = [(volume index, corner, isometry key or None)].
        What datastep.patch_batch makes of each patch on its own volume, bit for bit, in ONE n3d_patch_gather launch on the current
        stream.  Returns (x, t): x (B, Cv, P, P, P) fp32 in NDHWC storage, t (B, 3, P, P, P) of target_dtype (None without truth).
        out=(x, t): written in place (NDHWC x, contiguous t; t's dtype then decides the target dtype), as datastep.patch_batch."""
        if target_dtype not in (torch.float32, torch.uint8):
            raise N3DError("VolumeSet.patch_batch: targets are float32 or uint8")
        B, P = len(refs), int(patch)
        if B < 1 or not self.volumes:
            raise N3DError("VolumeSet.patch_batch: need at least one patch of a non-empty set")
        descs = (GatherDesc * B)()
        for i, (v, corner, key) in enumerate(refs):
            perm, flip = _isometry(key)
            descs[i] = GatherDesc(PatchDesc((C.c_int32 * 3)(*[int(c) for c in corner]), (C.c_int32 * 3)(*perm),
                                            (C.c_int32 * 3)(*[int(f) for f in flip])), int(v))
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
        check(_lib.load().n3d_patch_gather(K.ptr(self.records), len(self), Cv, descs, B, P, flags, xv.p, xv.ld, K.ptr(t),
                                           K.stream_ptr()), "n3d_patch_gather")
        return x, t


class Generator:
    """generator.py:68-217 (class Generator) over a VolumeSet.  The reference's signature, except: `data_file` is a VolumeSet (its
    indices are the reference's h5 key indices); the file-only arguments (affine_file, spe_file, augment_flip,
    augment_distortion_factor) are gone; augment=True (nilearn distortions) is not built; labels is None or [1, 2, 4]; patches are
    cubic.  rng: any random.Random-like object (default: the `random` module, as the reference) -- it sees exactly the reference's
    calls: randint (overlap, per epoch_init), shuffle (per epoch), choice (one key per kept patch with permute).

    epoch_init(): one n3d_patch_qualify launch and one device -> host copy of the candidates' flag bytes.
    epoch(out=None): a generator of (x, t) device tensors (t None without truth), one n3d_patch_gather launch per batch on the
    current stream.  out: a tuple (x, t) or a zero-argument callable returning one (e.g. trainer.input_buffers), evaluated per
    batch; a batch is written into it when it fits (shape, dtype, NDHWC x), else -- None entries, the smaller last batch -- into
    fresh tensors.  A batch written into a trainer's buffers is overwritten by the next next(): step on it first."""

    def __init__(self, indices_list, volumes, patch_shape, patch_overlap=None, batch_size=1, labels=None, augment=False, permute=False,
                 shuffle_index_list=True, skip_health=True, inclusive_label=False, both_ps=False, target_dtype=torch.float32, rng=None):
        if augment:
            raise NotImplementedError("Generator: augment=True (the nilearn scale / flip distortions, augment.py:50-67) is not built")
        if labels is not None and list(labels) != LABELS:
            raise N3DError("Generator: labels must be None or [1, 2, 4] (the three BraTS regions the kernels expand)")
        ps = [patch_shape] * 3 if isinstance(patch_shape, int) else [int(p) for p in patch_shape]
        if len(ps) != 3 or len(set(ps)) != 1 or ps[0] < 1:
            raise N3DError("Generator: patches are cubic (got %s)" % (patch_shape,))
        if not 1 <= int(batch_size) <= MAX_BATCH:
            raise N3DError("Generator: batch_size must be 1..%d" % MAX_BATCH)
        if target_dtype not in (torch.float32, torch.uint8):
            raise N3DError("Generator: targets are float32 or uint8")
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

    def _skip_health(self):
        # np.all(None == 0) is False (generator.py:206): without truth nothing is skipped as healthy
        return bool(self.skip_health) and bool(self.volumes.has_truth)

    def epoch(self, out=None):
        cand = self.candidates
        for batch in epoch_order(self.flags, self.batch_size, self.rng, self._skip_health(), self.shuffle_index_list, self.permute):
            o = out() if callable(out) else out
            B = len(batch)
            refs = [(cand[i, 0], cand[i, 1:], key) for i, key in batch]
            fit = o if self.volumes.fits(o, B, self.patch, self.target_dtype) else None
            yield self.volumes.patch_batch(refs, self.patch, self.inclusive_label, self.target_dtype, out=fit)
        if self.patch_overlap:
            self.epoch_init()
