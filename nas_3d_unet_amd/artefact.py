"""Acquisition artefacts of a gathered batch on the device: simulated low resolution, a multiplicative bias field and modality
dropout (none of it the reference's; the rules are nnU-Net v2's SimulateLowResolutionTransform, TorchIO's RandomBiasField and the
BraTS missing-modality recipes, restated in include/n3d.h under n3d_patch_artefact and tied to torch's fp64 interpolate and numpy
by tests/test_artefact_ref_host.py).

Host logic only: the draws of a patch (Artefact.draw) and the descriptor arrays; the kernels are behind n3d_patch_artefact.
Generator(augment=True, augment_artefact=Artefact(...)) makes the draws per kept patch and applies them to every batch it yields,
after the appearance transforms."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import N3DError, check

MAX_BATCH = 16     # N3D_APPEAR_MAX_BATCH
MAX_PATCH = 256    # N3D_APPEAR_MAX_PATCH
MAX_ORDER = 3      # N3D_ARTEFACT_MAX_ORDER
MAX_CHANNELS = 4


def extent(P, scale):
    """the extent a P-wide axis is sampled down to at `scale`: max(1, round(P * scale)) with Python's round (to even on a tie), as
    batchgeneratorsv2 forms it"""
    return max(1, round(P * float(scale)))


class ArtefactTable:
    """the HOST descriptor arrays of n3d_patch_artefact for B patches (include/n3d.h): stages [B][3], n [B][4], order [B][4],
    range [B][4], key [B][2], drop [B][4]; zeroed -- no stage acts"""

    def __init__(self, B):
        self.B = B
        self.stages = (C.c_int32 * (3 * B))()
        self.n = (C.c_int32 * (4 * B))()
        self.order = (C.c_int32 * (4 * B))()
        self.range = (C.c_double * (4 * B))()
        self.key = (C.c_uint32 * (2 * B))()
        self.drop = (C.c_int32 * (4 * B))()

    def args(self):
        return self.stages, self.n, self.order, self.range, self.key, self.drop


def _probability(name, p):
    if not (np.ndim(p) == 0 and np.isfinite(p) and 0 <= p <= 1):
        raise N3DError("Artefact: %s is a probability (got %r)" % (name, p))
    return float(p)


class Artefact:
    """lowres: (lo, hi) of the scale a channel is sampled down to and back, 0 < lo <= hi <= 1, drawn per channel for the channels
    that a p_lowres_channel draw selects; bias: the range of the bias field's polynomial coefficients (uniform in [-bias, bias)),
    bias_order its order (0 .. 3); dropout: the probability that a channel of the patch is zeroed (never all of them).  p_*: the
    probability that a patch gets the transform.  An option left None draws nothing and does nothing."""

    def __init__(self, lowres=None, bias=None, dropout=None, bias_order=3, p_lowres=0.25, p_lowres_channel=0.5, p_bias=0.15, p_dropout=0.1):
        if lowres is not None:
            try:
                lo, hi = (float(a) for a in lowres)
            except (TypeError, ValueError):
                raise N3DError("Artefact: lowres is a (lo, hi) range of scales (got %r)" % (lowres,)) from None
            if not (np.isfinite(lo) and np.isfinite(hi) and 0 < lo <= hi <= 1):
                raise N3DError("Artefact: lowres needs 0 < lo <= hi <= 1 (got %r)" % (lowres,))
            lowres = (lo, hi)
        if bias is not None:
            if not (np.ndim(bias) == 0 and np.isfinite(bias) and bias >= 0):
                raise N3DError("Artefact: bias is a finite non-negative coefficient range (got %r)" % (bias,))
            bias = float(bias)
        if isinstance(bias_order, bool) or not isinstance(bias_order, (int, np.integer)) or not 0 <= bias_order <= MAX_ORDER:
            raise N3DError("Artefact: bias_order is an integer 0 .. %d (N3D_ARTEFACT_MAX_ORDER; got %r)" % (MAX_ORDER, bias_order))
        if dropout is not None:
            dropout = _probability("dropout", dropout)
        self.lowres, self.bias, self.bias_order, self.dropout = lowres, bias, int(bias_order), dropout
        self.p_lowres, self.p_lowres_channel = _probability("p_lowres", p_lowres), _probability("p_lowres_channel", p_lowres_channel)
        self.p_bias, self.p_dropout = _probability("p_bias", p_bias), _probability("p_dropout", p_dropout)
        self._scratch = {}

    def draw(self, np_rng, Cv):
        """the draws of ONE patch from an np.random-like object.  For each option that is set, in the order lowres, bias, dropout:
        np_rng.uniform(), the transform being active iff that value is < p; only if active, its parameters: lowres
        np_rng.uniform(size=Cv) (a channel is selected iff its value is < p_lowres_channel) and then np_rng.uniform(lo, hi, Cv); bias
        np_rng.randint(0, 2**32, 2, dtype=np.uint32) (the Philox key); dropout np_rng.uniform(size=Cv) (a channel falls iff its value
        is < dropout) and, only if every channel fell, np_rng.randint(0, Cv): that channel is kept.  Returns a dict of the active
        transforms: "lowres": (Cv,) float64 scales, 1.0 for a channel that was not selected; "bias": (range, order, (k0, k1));
        "dropout": (Cv,) bool."""
        d = {}
        if self.lowres is not None and np_rng.uniform() < self.p_lowres:
            chosen = np.asarray(np_rng.uniform(size=Cv)) < self.p_lowres_channel
            scale = np.asarray(np_rng.uniform(self.lowres[0], self.lowres[1], Cv), np.float64)
            d["lowres"] = np.where(chosen, scale, 1.0)
        if self.bias is not None and np_rng.uniform() < self.p_bias:
            key = np_rng.randint(0, 2 ** 32, 2, dtype=np.uint32)
            d["bias"] = (self.bias, self.bias_order, (int(key[0]), int(key[1])))
        if self.dropout is not None and np_rng.uniform() < self.p_dropout:
            drop = np.array(np.asarray(np_rng.uniform(size=Cv)) < self.dropout)
            if drop.all():
                drop[int(np_rng.randint(0, Cv))] = False
            d["dropout"] = drop
        return d

    @staticmethod
    def descriptors(draws, Cv, P):
        """the descriptor arrays of a batch (ArtefactTable): one entry of `draws` per patch, a dict as draw() returns it or None;
        n[c] = extent(P, scale[c])"""
        t = ArtefactTable(len(draws))
        for b, d in enumerate(draws):
            if not d:
                continue
            if d.get("lowres") is not None:
                v = np.asarray(d["lowres"], np.float64).reshape(-1)
                if v.shape != (Cv,) or not np.isfinite(v).all():
                    raise N3DError("Artefact.apply: patch %d: lowres takes one finite scale per channel (%d, got %r)" % (b, Cv, d["lowres"]))
                t.stages[3 * b] = 1
                for c in range(Cv):
                    t.n[4 * b + c] = extent(P, v[c])        # outside 1 .. P: the entry point refuses it
            if d.get("bias") is not None:
                rng, order, key = d["bias"]
                t.stages[3 * b + 1] = 1
                t.key[2 * b], t.key[2 * b + 1] = int(key[0]), int(key[1])
                for c in range(Cv):
                    t.order[4 * b + c], t.range[4 * b + c] = int(order), float(rng)
            if d.get("dropout") is not None:
                v = np.asarray(d["dropout"]).reshape(-1)
                if v.shape != (Cv,):
                    raise N3DError("Artefact.apply: patch %d: dropout takes one flag per channel (%d, got %d)" % (b, Cv, v.size))
                if v.all():
                    raise N3DError("Artefact.apply: patch %d: dropout never drops every channel" % b)
                t.stages[3 * b + 2] = 1
                for c in range(Cv):
                    t.drop[4 * b + c] = int(bool(v[c]))
        return t

    def apply(self, x, draws):
        """x: (B, Cv, P, P, P) fp32 device tensor in NDHWC storage (K.empty_ndhwc, Trainer.input_buffers(), VolumeSet.patch_batch),
        transformed IN PLACE on the current stream by n3d_patch_artefact; draws: one entry per patch, a draw() dict or None.
        Returns x.  No host sync; with no active transform in the batch nothing is launched."""
        if not (isinstance(x, torch.Tensor) and x.dim() == 5):
            raise N3DError("Artefact.apply: expected a 5-D (B, Cv, P, P, P) tensor")
        if not x.is_cuda:
            raise N3DError("Artefact.apply: the batch is on %s: the transforms only run on a HIP (gfx950) device; there is no CPU "
                           "fallback" % x.device)
        if x.dtype != torch.float32:
            raise N3DError("Artefact.apply: fp32 expected, got %s" % x.dtype)
        B, Cv, P = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        ld = K._pitch_of(x)
        if ld is None or x.shape[3] != P or x.shape[4] != P or x.data_ptr() % 4:
            raise N3DError("Artefact.apply: the batch must be cubic patches in NDHWC (channels-last) storage, as K.empty_ndhwc / "
                           "Trainer.input_buffers() give it")
        if len(draws) != B:
            raise N3DError("Artefact.apply: one draw (or None) per patch (%d, got %d)" % (B, len(draws)))
        if not any(draws):
            return x
        table = self.descriptors(draws, Cv, P)
        lib = _lib.load()
        key = (B, Cv, P, x.device)
        scratch = self._scratch.get(key)
        if scratch is None:
            scratch = self._scratch[key] = torch.empty(max(int(lib.n3d_patch_artefact_scratch(B, Cv, P)), 16), dtype=torch.uint8, device=x.device)
        check(lib.n3d_patch_artefact(K.ptr(x), ld, B, Cv, P, *table.args(), K.ptr(scratch), scratch.numel(), K.stream_ptr()), "n3d_patch_artefact")
        return x
