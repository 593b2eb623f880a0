"""Whole-volume inference (prediction.py:120-148): patch corners of the reference's two patching strategies
(patches.py:9-70), BATCHED forward passes of the searched net on patches cropped on the device (the reference runs them
one by one through the host, prediction.py:132-138), device stitching and label fusion.  Host logic only; the kernels
are n3d_patch_batch, the net's own ops, n3d_stitch and n3d_tumor_labels.

SubjectPredictor is the subject-level pass (prediction.py:64-170) over a generator.VolumeSet: empty patches never reach the net
(n3d_patch_qualify), the forward is one captured graph replayed per chunk, chunks are stitched as they come (n3d_stitch_add, which
also brings the prediction of an isometry of the patch back) and one pass fuses mean, labels and skull mask (n3d_stitch_finish)."""
from __future__ import annotations

import collections
import contextlib
import types

import numpy as np
import torch

from . import datastep, poststep
from . import kernels as K
from ._lib import N3DError


def _corner_lattice(first, pitch, count):
    """All corners first + i * pitch, i < count per axis (first axis slowest), truncated towards zero: the lattice np.mgrid walks for
    the reference (patches.py:72-74).  first / pitch may be fractional -- the reference spreads the patches evenly with a real-valued
    pitch and lets the integer cast place them."""
    axes = [first[d] + np.arange(int(count[d])) * pitch[d] for d in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)


def _even_cover(img, patch):
    """The auto-fitting strategy of patches.py:9-34 in closed form, all three axes at once.  An axis needs n = ceil(img / patch) patches.
    n = 1: the one patch is centred (it overhangs by patch - img, the odd voxel on the low side).  n > 1: the n patches share their
    total excess n * patch - img evenly, i.e. neighbours overlap by excess / (n - 1) and the pitch is patch - that; what is left
    over after the real-valued division (zero up to rounding, and the reference keeps the rounding) is split around the image like
    the overhang.  Returns (first corner, pitch, count) per axis."""
    img, patch = img.astype(np.float64), patch.astype(np.float64)
    n = np.ceil(img / patch)
    lone = n == 1
    gaps = np.where(lone, 1.0, n - 1.0)
    share = np.floor(n * patch - img) / gaps                      # overlap between neighbours (n > 1)
    rest = n * patch - (n - 1.0) * share - img                    # excess the even split leaves
    first = np.where(lone, (-(patch - img)) // 2, (-rest) // 2)
    pitch = np.where(lone, patch, patch - share)
    # the reference walks mgrid[first : first + n * pitch : pitch]: ceil(((first + n * pitch) - first) / pitch) corners
    count = np.ceil(((first + n * pitch) - first) / pitch)
    return first, pitch, count


def _fixed_overlap_cover(img, patch, ov):
    """The given-overlap strategy of patches.py:59-67: pitch patch - ov, as many patches as it takes, the overhang split around the image"""
    img, patch, ov = img.astype(np.float64), patch.astype(np.float64), ov.astype(np.float64)
    pitch = patch - ov
    n = np.ceil(img / pitch)
    first = (-(patch * n - (n - 1.0) * ov - img)) // 2
    count = np.ceil(((first + n * pitch) - first) / pitch)
    return first, pitch, count


def patching(img_shape, patch_shape, overlap=None, both_ps=False):
    """bottom-left patch corners as the reference's patches.patching lists them (patches.py:36-70): the evenly spread cover followed
    by the centred cube; with `overlap` the centred cube followed by the fixed-overlap cover; with both_ps the first list, then the second."""
    img, patch = np.asarray(img_shape), np.asarray(patch_shape)
    centre = ((img - patch) // 2).reshape(1, 3).astype(np.int64)
    even = np.concatenate((_corner_lattice(*_even_cover(img, patch)), centre))
    if overlap is None:
        return even
    ov = np.full(3, overlap) if isinstance(overlap, int) else np.asarray(overlap)
    fixed = np.concatenate((centre, _corner_lattice(*_fixed_overlap_cover(img, patch, ov))))
    return np.concatenate((even, fixed)) if both_ps else fixed


class Predictor:
    """prediction.py:120-170 on the device: `volume` is the brain-wide crop (C, X, Y, Z) resident in HBM."""

    def __init__(self, model, patch=64, batch=8):
        self.model, self.patch, self.batch = model, int(patch), int(batch)

    @torch.no_grad()
    def predict(self, volume, overlap=None, both_ps=False, full_shape=None, origin=(0, 0, 0)):
        """-> float64 (n_labels, FX, FY, FZ) probabilities (the brain-wide box stitched and placed in the full image)"""
        if not (isinstance(volume, torch.Tensor) and volume.is_cuda and volume.dim() == 4):
            raise N3DError("Predictor: volume must be a (C, X, Y, Z) tensor on a HIP device")
        P = self.patch
        box = tuple(int(s) for s in volume.shape[1:])
        corners = [tuple(int(v) for v in c) for c in patching(box, (P, P, P), overlap, both_ps)]
        was_training = self.model.training
        self.model.eval()
        preds = []
        try:
            for i in range(0, len(corners), self.batch):
                chunk = corners[i:i + self.batch]
                x, _ = datastep.patch_batch(volume, None, chunk, [None] * len(chunk), P)
                y = self.model(x)
                # an all-zero patch is not run through the model by the reference: its prediction is zeros (prediction.py:133-135)
                empty = (x.abs().amax(dim=(1, 2, 3, 4)) == 0).view(-1, 1, 1, 1, 1)
                preds.append(torch.where(empty, torch.zeros_like(y), y))
        finally:
            self.model.train(was_training)
        return poststep.stitch(torch.cat(preds), corners, box, full_shape, origin)

    def tumor(self, volume, threshold=0.5, inclusive_label=True, **kw):
        return poststep.tumor_labels(self.predict(volume, **kw), threshold, inclusive_label)


# ---- subject-level inference ------------------------------------------------------------------------------------------------
# corner, key: per entry, its index into the corner list / the key list (key-major: for key in keys: for corner in corners);
# slot: per entry, its patch's index in its chunk's tensor, -1 for a dead entry; chunks: the forwards, in order
SubjectPlan = collections.namedtuple("SubjectPlan", "corner key slot chunks")
# refs: the `batch` entries gathered into the chunk's input slots (the unused slots of a short last chunk repeat its first live
# entry; no table entry points at them); the table entries [first, last) are added once the chunk has run
Chunk = collections.namedtuple("Chunk", "refs first last")


def plan_subject(dead, n_keys, batch):
    """The entry list and chunks of one subject.  dead: one flag per corner (an all-zero patch -- dead under every key, an isometry
    moves zeros onto zeros); every (corner, key) pair is one covering patch of a single stitch.  Live entries are chunked `batch` at
    a time in list order; a chunk's table range runs from its first live entry up to the next chunk's, so the dead entries ride with
    a neighbouring chunk and the table order IS the list order (the first chunk starts at 0, the last one ends at the end).
    No live entry: no chunk (and nothing to add: the mean is 0 everywhere)."""
    dead = np.asarray(dead, dtype=bool).reshape(-1)
    nc, nk, batch = len(dead), int(n_keys), int(batch)
    if nk < 1 or batch < 1:
        raise N3DError("plan_subject: need at least one key and a batch of at least 1")
    corner = np.tile(np.arange(nc, dtype=np.int64), nk)
    key = np.repeat(np.arange(nk, dtype=np.int64), nc)
    live = np.flatnonzero(~dead[corner])
    slot = np.full(nc * nk, -1, dtype=np.int32)
    slot[live] = np.arange(len(live), dtype=np.int32) % batch
    chunks = []
    for k in range(0, len(live), batch):
        mine = [int(e) for e in live[k:k + batch]]
        refs = mine + [mine[0]] * (batch - len(mine))
        first = 0 if k == 0 else mine[0]
        last = int(live[k + batch]) if k + batch < len(live) else nc * nk
        chunks.append(Chunk(refs, first, last))
    return SubjectPlan(corner, key, slot, chunks)


class SubjectPredictor:
    """prediction.py:64-170 for one subject of a generator.VolumeSet, on the device end to end.

    predict(volumes, index, ...) -> (labels uint8 (FX, FY, FZ), probs float64 (n_labels, FX, FY, FZ) or None).
    One n3d_patch_qualify launch and one read of its flag bytes per subject (the only host sync) mark the all-zero patches; they are
    never gathered and never run (the reference's rule, prediction.py:133-135) -- they only count as covering.  The live
    (corner, key) entries go `batch` at a time: VolumeSet.patch_batch writes the chunk into the static input buffer, the net runs
    -- graph=True: ONE captured graph of the forward in eval mode, weight packing included, replayed for every chunk of every
    subject whatever its box -- and n3d_stitch_add adds the chunk to the subject's running fp64 sums, inverting each entry's
    isometry on the way.  n3d_stitch_finish then writes the labels (skull mask included) and, only if asked for, the fp64 image.
    keys: isometry keys of datastep.generate_permutation_keys() (None: the identity); the prediction is the mean over every
    (corner, key) patch, for a net trained with `permute`.

    stats: entries / live / chunks of the last subject; captures / replays / forwards since the predictor was made."""

    def __init__(self, model, patch=64, batch=8, graph=True, _net=None, _padded=False):
        self.model, self.patch, self.batch, self.use_graph = model, int(patch), int(batch), bool(graph)
        if not 1 <= self.batch <= 64:
            raise N3DError("SubjectPredictor: batch must be 1..64 (N3D_PATCH_MAX_BATCH)")
        # a trainer hands over the module its step trains (Trainer.predictor): the model itself, or its zero-padded twin
        self._net, self._padded = _net, bool(_padded)
        self.stats = types.SimpleNamespace(entries=0, live=0, chunks=0, captures=0, replays=0, forwards=0)
        self._ctx = None          # weight packing of this pass (the trainers' contexts stay as their steps left them)
        self._x = self._t = self._y = None
        self._graph = None
        self._sig = None          # (device, parameter storage pointers, input channels) the buffers and the graph were made for

    # -- the forward ------------------------------------------------------------------------------
    def _modules(self):
        seen = {}
        for root in (self.model, self._net):
            if root is not None:
                for m in root.modules():
                    seen.setdefault(id(m), m)
        return list(seen.values())

    def _run(self, x):
        if self._net is None:
            return self.model(x)
        from . import fused, unet
        with fused.padded_switches() if self._padded else contextlib.nullcontext():
            return unet.run(self._net, x)

    def _pass(self, x):
        """one forward on the current stream: weight packing (one launch, once the jobs are known), the net"""
        with torch.no_grad(), K.step_context(self._ctx):
            self._ctx.pack_all()
            y = self._run(x)
        if not self._ctx.frozen:
            self._ctx.freeze()
        return y

    def _signature(self, device, channels):
        net = self._net if self._net is not None else self.model
        return (device, int(channels), tuple(p.data_ptr() for p in net.parameters()))

    def _prepare(self, volumes):
        """the static buffers and (graph=True) the captured forward, made again when the weights have moved to other storage"""
        net = self._net if self._net is not None else self.model
        device = next(net.parameters()).device
        if device != volumes.device:
            raise N3DError("SubjectPredictor: the model is on %s, the volumes on %s" % (device, volumes.device))
        sig = self._signature(device, volumes.channels)
        if sig == self._sig:
            return
        B, P = self.batch, self.patch
        self._ctx = K.StepContext(device)
        self._x = K.empty_ndhwc(B, volumes.channels, P, P, P, device, torch.float32).zero_()
        self._graph = self._y = self._t = None
        if self.use_graph:
            from .train import capture_stream
            s = capture_stream(device)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):      # allocator, net plan, packing jobs
                    self._pass(self._x)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                self._y = self._pass(self._x)
            self._graph = g
            self.stats.captures += 1
        self._sig = sig

    def _forward(self):
        self.stats.forwards += 1
        if self._graph is not None:
            self._graph.replay()
            self.stats.replays += 1
            return self._y
        return self._pass(self._x)

    # -- one subject ------------------------------------------------------------------------------
    def predict(self, volumes, index, overlap=None, both_ps=False, keys=(None,), full_shape=None, origin=(0, 0, 0), threshold=0.5,
                inclusive_label=True, skull_mask=True, want_probs=False):
        index, P, B = int(index), self.patch, self.batch
        if not 0 <= index < len(volumes):
            raise N3DError("SubjectPredictor: volume index %d outside the set of %d" % (index, len(volumes)))
        keys = list(keys)
        if not keys:
            raise N3DError("SubjectPredictor: need at least one isometry key (None: the identity)")
        isos = [poststep.IDENTITY if k is None else datastep.isometry_of_key(k) for k in keys]
        box = tuple(volumes.box(index))
        corners = patching(box, (P, P, P), overlap, both_ps)
        mods = self._modules()
        was = [m.training for m in mods]
        try:
            for m in mods:
                m.training = False
            self._prepare(volumes)
            # the subject's one host sync: which corners are dead (bit 0 clear: every modality zero)
            flags = volumes.qualify([index] * len(corners), corners, P).cpu().numpy()
            plan = plan_subject((flags & 1) == 0, len(keys), B)
            n = len(plan.slot)
            table = poststep.entry_table([(corners[c], isos[k], s) for c, k, s in zip(plan.corner, plan.key, plan.slot)], volumes.device)
            if volumes.has_truth and self._t is None:
                self._t = torch.empty((B, 3, P, P, P), dtype=torch.uint8, device=volumes.device)   # (the gather's labels: not used)
            n_out = None
            sum_ = cnt = None
            for ch in plan.chunks:
                volumes.patch_batch([(index, corners[plan.corner[e]], keys[plan.key[e]]) for e in ch.refs], P, out=(self._x, self._t))
                y = self._forward()
                if sum_ is None:
                    n_out = int(y.shape[1])
                    sum_, cnt = poststep.stitch_buffers(n_out, box, volumes.device)
                cs = corners[plan.corner[ch.first:ch.last]]
                poststep.stitch_add(y, table, ch.first, ch.last - ch.first, cs.min(axis=0), cs.max(axis=0) + P, sum_, cnt)
            if sum_ is None:
                # no live patch: the prediction is 0 everywhere (the head's channel count is then the net's to tell)
                net = self._net if self._net is not None else self.model
                sum_, cnt = poststep.stitch_buffers(int(net.last_conv[0].conv.weight.shape[0]), box, volumes.device)
            self.stats.entries, self.stats.live, self.stats.chunks = n, int((plan.slot >= 0).sum()), len(plan.chunks)
        finally:
            for m, w in zip(mods, was):
                m.training = w
        return poststep.stitch_finish(sum_, cnt, full_shape, origin, want_probs, True, threshold, inclusive_label,
                                      volumes.volumes[index] if skull_mask else None)
