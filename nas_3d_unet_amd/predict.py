"""Whole-volume inference (prediction.py:120-148): patch corners of the reference's two patching strategies
(patches.py:9-70), BATCHED forward passes of the searched net on patches cropped on the device (the reference runs them
one by one through the host, prediction.py:132-138), device stitching and label fusion.  Host logic only; the kernels
are n3d_patch_batch, the net's own ops, n3d_stitch and n3d_tumor_labels.

SubjectPredictor is the subject-level pass (prediction.py:64-170) over a generator.VolumeSet: empty patches never reach the net
(n3d_patch_qualify), the forward is one captured graph replayed per chunk, chunks are stitched as they come (n3d_stitch_add, which
also brings the prediction of an isometry of the patch back) and one pass fuses mean, labels and skull mask (n3d_stitch_finish).
blend="gaussian" weights a patch prediction by the position inside the patch (n3d_stitch_add_w / n3d_stitch_finish_w), and
EnsemblePredictor lets several SubjectPredictors add into the same running buffers.

ImagePredictor is the reference's other mode (prediction.py:102-119, predict(no_patch=True)): ONE forward per subject on the whole
image zero-padded at the high end (n3d_image_embed), cropped, averaged over flips and fused into labels in one pass
(n3d_image_finish).  Both predictors share the forward -- eval mode, weight packing, the captured graph -- through _ForwardHost."""
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


class _ForwardHost:
    """What the subject-level predictors share: the forward of the model (or of the module a trainer's step trains) in eval mode on a
    static input buffer, weight packing included -- graph=True: captured once per signature (device, input shape, parameter
    storage) and replayed -- and the counters captures / replays / forwards of `stats`."""
    _what = "predictor"

    def _init_forward(self, model, graph, _net, _padded):
        self.model, self.use_graph = model, bool(graph)
        # a trainer hands over the module its step trains (Trainer.predictor): the model itself, or its zero-padded twin
        self._net, self._padded = _net, bool(_padded)
        self._ctx = None          # weight packing of this pass (the trainers' contexts stay as their steps left them)
        self._x = self._t = self._y = None
        self._graph = None
        self._sig = None          # (device, input shape key, parameter storage pointers) the buffers and the graph were made for

    def _modules(self):
        seen = {}
        for root in (self.model, self._net):
            if root is not None:
                for m in root.modules():
                    seen.setdefault(id(m), m)
        return list(seen.values())

    @contextlib.contextmanager
    def _eval_mode(self):
        """every module of the model (and of the trainer's module) in eval mode; the caller's modes come back"""
        mods = self._modules()
        was = [m.training for m in mods]
        try:
            for m in mods:
                m.training = False
            yield
        finally:
            for m, w in zip(mods, was):
                m.training = w

    def _the_net(self):
        return self._net if self._net is not None else self.model

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
        return (device, channels if isinstance(channels, tuple) else int(channels), tuple(p.data_ptr() for p in self._the_net().parameters()))

    def _device_for(self, volumes):
        device = next(self._the_net().parameters()).device
        if device != volumes.device:
            raise N3DError("%s: the model is on %s, the volumes on %s" % (self._what, device, volumes.device))
        return device

    def _drop_forward(self):
        """let go of the graph and the static buffers (before their successors are allocated: a full-size set is large)"""
        self._graph = self._y = self._t = self._x = self._ctx = None
        self._sig = None

    def _make_forward(self, device, x, sig):
        """a fresh packing context on the static input x and (graph=True) the captured forward"""
        self._ctx = K.StepContext(device)
        self._x = x
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


class SubjectPredictor(_ForwardHost):
    """prediction.py:64-170 for one subject of a generator.VolumeSet, on the device end to end.

    predict(volumes, index, ...) -> (labels uint8 (FX, FY, FZ), probs float64 (n_labels, FX, FY, FZ) or None).
    One n3d_patch_qualify launch and one read of its flag bytes per subject (the only host sync) mark the all-zero patches; they are
    never gathered and never run (the reference's rule, prediction.py:133-135) -- they only count as covering.  The live
    (corner, key) entries go `batch` at a time: VolumeSet.patch_batch writes the chunk into the static input buffer, the net runs
    -- graph=True: ONE captured graph of the forward in eval mode, weight packing included, replayed for every chunk of every
    subject whatever its box -- and n3d_stitch_add adds the chunk to the subject's running fp64 sums, inverting each entry's
    isometry on the way.  n3d_stitch_finish then writes the labels (skull mask included) and, only if asked for, the fp64 image.
    keys: isometry keys of datastep.generate_permutation_keys() (None: the identity); the prediction is the mean over every
    (corner, key) patch, for a net trained with `permute`.  blend: "mean" (that mean; the default), "gaussian" or an array of `patch`
    weights (poststep.blend_profile) -- the weighted mean, same plan, same forward, n3d_stitch_add_w / n3d_stitch_finish_w.

    stats: entries / live / chunks of the last subject; captures / replays / forwards since the predictor was made."""
    _what = "SubjectPredictor"

    def __init__(self, model, patch=64, batch=8, graph=True, _net=None, _padded=False):
        self.patch, self.batch = int(patch), int(batch)
        if not 1 <= self.batch <= 64:
            raise N3DError("SubjectPredictor: batch must be 1..64 (N3D_PATCH_MAX_BATCH)")
        self._init_forward(model, graph, _net, _padded)
        self._profiles = _Profiles()
        self.stats = types.SimpleNamespace(entries=0, live=0, chunks=0, captures=0, replays=0, forwards=0)

    def _prepare(self, volumes):
        """the static buffers and (graph=True) the captured forward, made again when the weights have moved to other storage"""
        device = self._device_for(volumes)
        sig = self._signature(device, volumes.channels)
        if sig == self._sig:
            return
        B, P = self.batch, self.patch
        self._make_forward(device, K.empty_ndhwc(B, volumes.channels, P, P, P, device, torch.float32).zero_(), sig)

    # -- one subject: plan (plan_entries), accumulate into running buffers, finish (finish_subject) ----------------------------
    def _accumulate(self, volumes, sub, profile, bufs):
        """this predictor's share of a subject: the live entries of `sub` go through the net `batch` at a time and every chunk is
        added to the running buffers -- `bufs`, or fresh ones when it is None (made at the first chunk, which tells the head's
        channel count; no live entry: None comes back).  profile None: (sum, cnt) and n3d_stitch_add; a device profile: (sum,
        wsum) and n3d_stitch_add_w.  Call inside _eval_mode(), after _prepare()."""
        index, P, B, corners, keys = sub.index, self.patch, self.batch, sub.corners, sub.keys
        plan = plan_subject(sub.dead, len(keys), B)
        table = poststep.entry_table([(corners[c], sub.isos[k], s) for c, k, s in zip(plan.corner, plan.key, plan.slot)], volumes.device)
        if volumes.has_truth and self._t is None:
            self._t = torch.empty((B, 3, P, P, P), dtype=torch.uint8, device=volumes.device)   # (the gather's labels: not used)
        for ch in plan.chunks:
            volumes.patch_batch([(index, corners[plan.corner[e]], keys[plan.key[e]]) for e in ch.refs], P, out=(self._x, self._t))
            y = self._forward()
            if bufs is None:
                bufs = (poststep.stitch_buffers if profile is None else poststep.stitch_buffers_w)(int(y.shape[1]), sub.box, volumes.device)
            cs = corners[plan.corner[ch.first:ch.last]]
            if profile is None:
                poststep.stitch_add(y, table, ch.first, ch.last - ch.first, cs.min(axis=0), cs.max(axis=0) + P, *bufs)
            else:
                poststep.stitch_add_w(y, table, ch.first, ch.last - ch.first, cs.min(axis=0), cs.max(axis=0) + P, profile, *bufs)
        self.stats.entries, self.stats.live, self.stats.chunks = len(plan.slot), int((plan.slot >= 0).sum()), len(plan.chunks)
        return bufs

    def predict(self, volumes, index, overlap=None, both_ps=False, keys=(None,), full_shape=None, origin=(0, 0, 0), threshold=0.5,
                inclusive_label=True, skull_mask=True, want_probs=False, blend="mean", sigma_scale=0.125):
        """blend: "mean" (every covering patch counts the same: the reference's stitch), "gaussian" or a length-`patch` array
        (poststep.blend_profile: a patch prediction is weighted by its position inside the patch; sigma_scale: the Gaussian's)."""
        sub = plan_entries(self._what, volumes, index, self.patch, overlap, both_ps, keys)
        profile = self._profiles.on_device(self.patch, blend, sigma_scale, volumes.device)
        with self._eval_mode():
            self._prepare(volumes)
            sub = qualify_entries(volumes, sub, self.patch)
            bufs = self._accumulate(volumes, sub, profile, None)
        return finish_subject(self, volumes, sub, profile, bufs, full_shape, origin, threshold, inclusive_label, skull_mask, want_probs)


# the entries of one subject before they are chunked: the corner list, the key list with its isometries, one dead flag per corner
SubjectEntries = collections.namedtuple("SubjectEntries", "index box corners keys isos dead")


def plan_entries(what, volumes, index, P, overlap, both_ps, keys):
    """the corner list and key list of subject `index` (host work only; `dead` is qualify_entries' to fill in)"""
    index = int(index)
    if not 0 <= index < len(volumes):
        raise N3DError("%s: volume index %d outside the set of %d" % (what, index, len(volumes)))
    keys = list(keys)
    if not keys:
        raise N3DError("%s: need at least one isometry key (None: the identity)" % what)
    isos = [poststep.IDENTITY if k is None else datastep.isometry_of_key(k) for k in keys]
    box = tuple(volumes.box(index))
    return SubjectEntries(index, box, patching(box, (P, P, P), overlap, both_ps), keys, isos, None)


def qualify_entries(volumes, sub, P):
    """the subject's one host sync: which corners are dead (bit 0 of n3d_patch_qualify's flags clear: every modality zero) -- one
    launch and one read of its flag bytes"""
    flags = volumes.qualify([sub.index] * len(sub.corners), sub.corners, P).cpu().numpy()
    return sub._replace(dead=(flags & 1) == 0)


def finish_subject(member, volumes, sub, profile, bufs, full_shape, origin, threshold, inclusive_label, skull_mask, want_probs):
    """the one finishing pass over the running buffers -> (labels, probs or None)"""
    if bufs is None:
        # no live patch: the prediction is 0 everywhere (the head's channel count is then the net's to tell)
        n_out = int(member._the_net().last_conv[0].conv.weight.shape[0])
        bufs = (poststep.stitch_buffers if profile is None else poststep.stitch_buffers_w)(n_out, sub.box, volumes.device)
    finish = poststep.stitch_finish if profile is None else poststep.stitch_finish_w
    return finish(*bufs, full_shape, origin, want_probs, True, threshold, inclusive_label, volumes.volumes[sub.index] if skull_mask else None)


class _Profiles:
    """the blend profiles a predictor has used, on the device: uploaded once per profile and kept"""

    def __init__(self):
        self._dev = {}

    def on_device(self, P, blend, sigma_scale, device):
        """None for "mean" (the unweighted kernels), else the float64 (P,) device tensor of poststep.blend_profile"""
        if isinstance(blend, str) and blend == "mean":
            return None
        prof = poststep.blend_profile(P, blend, sigma_scale)       # (an unknown name raises here)
        key = (torch.device(device), prof.tobytes())
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(prof).to(device)
        return self._dev[key]


class EnsemblePredictor:
    """Several SubjectPredictors -- the models of the cross-validation folds, say (Trainer.predictor of several trainers) --
    averaged in the same running buffers: the prediction is the (weighted) mean over every (member, corner, key) patch.

    predict(volumes, index, ...) takes SubjectPredictor.predict's keywords and returns what it returns.  The subject's entry list
    is planned once -- one qualification launch and one host sync for all members -- then member 0 adds all its chunks in list
    order, then member 1 into the same buffers, and so on (each with its own `batch` and captured forward), and ONE finishing
    pass divides.  A dead patch counts as covering once per member.  EnsemblePredictor([sp]) is sp, bit for bit.

    stats: members; entries / live (per member) and qualifies (qualification syncs) of the last subject."""
    _what = "EnsemblePredictor"

    def __init__(self, members):
        members = list(members)
        if not members or not all(isinstance(m, SubjectPredictor) for m in members):
            raise N3DError("EnsemblePredictor: members must be a non-empty list of SubjectPredictors")
        if len({m.patch for m in members}) != 1:
            raise N3DError("EnsemblePredictor: the members must share one patch size, got %s" % ([m.patch for m in members],))
        self.members, self.patch = members, members[0].patch
        self._profiles = _Profiles()
        self.stats = types.SimpleNamespace(members=len(members), entries=0, live=0, qualifies=0)

    def predict(self, volumes, index, overlap=None, both_ps=False, keys=(None,), full_shape=None, origin=(0, 0, 0), threshold=0.5,
                inclusive_label=True, skull_mask=True, want_probs=False, blend="mean", sigma_scale=0.125):
        sub = plan_entries(self._what, volumes, index, self.patch, overlap, both_ps, keys)
        profile = self._profiles.on_device(self.patch, blend, sigma_scale, volumes.device)
        for m in self.members:
            m._device_for(volumes)            # every member on the volumes' device, before anything runs
        bufs, self.stats.qualifies = None, 0
        for m in self.members:
            with m._eval_mode():
                m._prepare(volumes)
                if sub.dead is None:
                    sub = qualify_entries(volumes, sub, self.patch)
                    self.stats.qualifies += 1
                bufs = m._accumulate(volumes, sub, profile, bufs)
        self.stats.entries, self.stats.live = self.members[0].stats.entries, self.members[0].stats.live
        return finish_subject(self.members[0], volumes, sub, profile, bufs, full_shape, origin, threshold, inclusive_label, skull_mask,
                              want_probs)


# ---- whole-image inference ---------------------------------------------------------------------------------------------------
def _u_net(net):
    """the module that holds stems, cells and head: the net itself, or the supernet's kernel (nas.py:101)"""
    return getattr(net, "kernel", net)


def net_halvings(net):
    """how many times the net halves its input grid: stem1 and every down cell (searched.py:72,78-83), i.e. depth + 1"""
    return len(_u_net(net).down_cells) + 1


def image_pad(full_shape, halvings, pad=None):
    """voxels of zero padding at the high end of each axis of a whole-image forward, D = 2 ** halvings (the net must halve the
    padded grid `halvings` times and double it back onto the skips).  Default: D - F % D, 1..D voxels on EVERY axis -- an axis that
    is a multiple of D already gets D more: that is the reference's literal (0, 16), (0, 16), (0, 5) at 240 x 240 x 155
    (prediction.py:116), and since zero padding enters the GroupNorm statistics the amount is part of the result.  An explicit
    `pad` must make every padded axis a multiple of D."""
    D = 2 ** int(halvings)
    full = tuple(int(f) for f in full_shape)
    if len(full) != 3 or min(full) < 1:
        raise N3DError("image_pad: full_shape must be three positive sizes, got %s" % (full_shape,))
    if pad is None:
        return tuple(D - f % D for f in full)
    pad = tuple(int(p) for p in pad)
    if len(pad) != 3 or min(pad) < 0 or any((f + p) % D for f, p in zip(full, pad)):
        raise N3DError("image_pad: pad %s does not bring every axis of %s to a multiple of %d (the net halves the grid %d times)"
                       % (pad, full, D, int(halvings)))
    return pad


def image_flip_of_key(key):
    """the per-axis flip of a whole-image key: None (no flip) or a flip-only key of datastep.generate_permutation_keys() -- rotate
    (0, 0), transpose 0.  An image that is not a cube has no other isometries onto its own grid."""
    if key is None:
        return (False, False, False)
    try:
        ok = key in datastep.generate_permutation_keys() and tuple(key[0]) == (0, 0) and key[4] == 0
    except (TypeError, IndexError):
        ok = False
    if not ok:
        raise N3DError("ImagePredictor: key %r is not None or a flip-only key ((0, 0), fx, fy, fz, 0): rotations and the transpose "
                       "do not map a non-cubic image onto its own grid" % (key,))
    perm, flip = datastep.isometry_of_key(key)
    assert perm == [0, 1, 2]
    return tuple(bool(f) for f in flip)


def image_tensor_fits(voxels, pitch, elem_bytes=4):
    """may a (voxels x pitch) activation tensor go through the forward?  The MFMA conv kernels for multiples of 16 channels address
    their operands through buffer resources of 2^31 - 1 bytes with lane byte offsets formed in 32-bit int ((voxel * pitch +
    channel) * 4; conv_mfma.hip -- they decline from 2^30 bytes on, conv_bf16.hip's from 2^31 - 1), and the gather and
    weight-gradient kernels count voxels in 32 bits (conv_generic.hip): voxels < 2^31 and voxels * pitch * elem_bytes < 2^31 keep
    every such offset in range, whichever kernel the plan picks (an fp32 element index then stays below 2^29)."""
    voxels, pitch = int(voxels), int(pitch)
    return voxels < 2 ** 31 and voxels * pitch * int(elem_bytes) < 2 ** 31


def image_forward_tensors(net, in_channels, padded_shape):
    """[(name, voxels, channel pitch)] of the widest tensor at each stage of the eval forward at batch 1 on `padded_shape`: the input
    (padded to a quad), the stems, and per cell its preprocessed inputs (node width) and its output buffer (n_nodes x node width:
    the nodes are channel slices of it, or its node planes -- the same bytes).  Channel counts that are not multiples of 4 count as
    their zero-padded twin's (unet.PaddedTwin)."""
    net = _u_net(net)
    pad4 = lambda c: (int(c) + 3) // 4 * 4

    def vox(level):
        return int(np.prod([-(-int(p) // 2 ** level) for p in padded_shape]))

    out_c = lambda conv_ops: pad4(conv_ops.conv.weight.shape[0])
    res = [("input", vox(0), pad4(in_channels)), ("stem0", vox(0), out_c(net.stem0)), ("stem1", vox(1), out_c(net.stem1))]
    level = 1
    for i, cell in enumerate(net.down_cells):
        res.append(("down_cells.%d inputs" % i, vox(level), pad4(cell.c_node)))
        level += 1
        res.append(("down_cells.%d" % i, vox(level), pad4(cell.c_node) * int(cell.n_nodes)))
    for i, cell in enumerate(net.up_cells):
        res.append(("up_cells.%d inputs" % i, vox(level), pad4(cell.c_node)))
        level -= 1
        res.append(("up_cells.%d" % i, vox(level), pad4(cell.c_node) * int(cell.n_nodes)))
    res.append(("head", vox(0), int(net.last_conv[0].conv.weight.shape[0])))
    return res


def check_image_size(net, in_channels, padded_shape):
    """raise N3DError, with the numbers, unless every tensor of the forward on `padded_shape` passes image_tensor_fits (fp32
    elements: the bf16 configuration stores some of them in half the bytes, the bound is kept at the fp32 figure)"""
    for name, voxels, pitch in image_forward_tensors(net, in_channels, padded_shape):
        if not image_tensor_fits(voxels, pitch):
            raise N3DError("ImagePredictor: %s on a padded image of %s is %d voxels x %d channels x 4 bytes = %d bytes; the conv kernels "
                           "index a tensor with 32-bit byte offsets and need it below 2^31 = %d (a narrower net, or the patch path)"
                           % (name, tuple(int(p) for p in padded_shape), voxels, pitch, voxels * pitch * 4, 2 ** 31))


class ImagePredictor(_ForwardHost):
    """prediction.py:102-119 (`fs_pred`, predict(no_patch=True)) for one subject of a generator.VolumeSet, on the device end to end.

    predict(volumes, index, ...) -> (labels uint8 (FX, FY, FZ), probs float64 (n_labels, FX, FY, FZ) or None), as SubjectPredictor.
    The subject's box is written into the full image zero-padded at the high end (n3d_image_embed; pad: image_pad's rule), the
    net runs ONCE per key on it -- graph=True: one captured graph of the forward in eval mode, weight packing included, for the
    most recent padded shape (one entry: a full-size set of activations is large; another shape, or weights in other storage,
    captures again) -- and n3d_image_finish crops, averages over the keys, and writes labels (skull mask included) and, only if
    asked for, the fp64 image.  keys: None or flip-only keys (image_flip_of_key); every key but the last goes through
    n3d_image_add.  An all-zero subject runs no forward (prediction.py:114-115): the far corner of its summed-area table says so,
    the subject's one host sync.

    stats: captures / replays / forwards since the predictor was made."""
    _what = "ImagePredictor"

    def __init__(self, model, graph=True, _net=None, _padded=False):
        self._init_forward(model, graph, _net, _padded)
        self.stats = types.SimpleNamespace(captures=0, replays=0, forwards=0)

    def _prepare(self, volumes, padded):
        device = self._device_for(volumes)
        sig = self._signature(device, (int(volumes.channels),) + tuple(padded))
        if sig == self._sig:
            return
        self._drop_forward()
        # zeroed once, for the warm-up passes: n3d_image_embed then writes every voxel of it per key
        self._make_forward(device, K.zeros_ndhwc(1, volumes.channels, *padded, device, torch.float32), sig)

    def predict(self, volumes, index, full_shape=None, origin=None, pad=None, keys=(None,), threshold=0.5, inclusive_label=True,
                skull_mask=True, want_probs=False):
        index = int(index)
        if not 0 <= index < len(volumes):
            raise N3DError("ImagePredictor: volume index %d outside the set of %d" % (index, len(volumes)))
        flips = [image_flip_of_key(k) for k in keys]
        if not flips:
            raise N3DError("ImagePredictor: need at least one key (None: no flip)")
        box = tuple(volumes.box(index))
        if full_shape is None:
            full_shape = volumes.full_shapes[index]
        if origin is None:
            origin = volumes.origins[index]
        full = tuple(int(f) for f in full_shape) if full_shape is not None else box      # neither recorded nor given: the box is the image
        org = tuple(int(o) for o in origin) if origin is not None else (0, 0, 0)
        if len(full) != 3 or len(org) != 3 or any(o < 0 or o + b > f for o, b, f in zip(org, box, full)):
            raise N3DError("ImagePredictor: the box %s at %s is not inside the image %s" % (box, org, full))
        net = self._the_net()
        widths = image_pad(full, net_halvings(net), pad)
        padded = tuple(f + w for f, w in zip(full, widths))
        vol = volumes.volumes[index]
        self._device_for(volumes)
        check_image_size(net, volumes.channels, padded)      # before anything is allocated or launched
        # the subject's one host sync: how many voxels of the box have a nonzero modality (the table's far corner)
        if int(volumes.table(index)[-1, -1, -1, 0]) == 0:
            n_out = int(_u_net(net).last_conv[0].conv.weight.shape[0])
            labels = torch.zeros(full, dtype=torch.uint8, device=volumes.device)
            return labels, (torch.zeros((n_out,) + full, dtype=torch.float64, device=volumes.device) if want_probs else None)
        with self._eval_mode():
            self._prepare(volumes, padded)
            sum_ = None
            for k, flip in enumerate(flips):
                poststep.image_embed(vol, org, full, padded, flip, out=self._x)
                y = self._forward()
                if k + 1 < len(flips):
                    sum_ = poststep.image_add(y, full, padded, flip, sum_)
            return poststep.image_finish(y, full, padded, flip, sum_, len(flips), want_probs, True, threshold, inclusive_label,
                                         vol if skull_mask else None, org)
