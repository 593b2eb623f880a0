"""Appearance augmentation of a gathered batch on the device: Gaussian noise, Gaussian blur, contrast and gamma with retained
statistics on the brain voxels (none of it the reference's; the rules are batchgenerators' / nnU-Net's, restated in include/n3d.h
under n3d_appear_desc and pinned to scipy / numpy by tests/golden/appearance.npz).

Host logic only: the draws of a patch (Appearance.draw), the blur's kernel weights (numpy: the device evaluates no exp) and the
descriptor table; the kernels are behind n3d_patch_appearance.  Generator(augment=True, augment_appearance=Appearance(...)) makes
the draws per kept patch and applies them to every batch it yields."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import AppearDesc, N3DError, check

MAX_BATCH = 16     # N3D_APPEAR_MAX_BATCH
MAX_CHANNELS = 4
MAX_RADIUS = 6     # N3D_APPEAR_MAX_RADIUS


def blur_radius(sigma):
    """scipy.ndimage's radius at truncate = 4"""
    return int(4.0 * np.float64(sigma) + 0.5)


def blur_weights(sigma):
    """(r, w[0 .. r]) of n3d_appear_desc: r = int(4 sigma + 0.5), w[k] = exp(-0.5 / sigma^2 * k^2) / (their sum over -r .. r), in numpy
    exactly as scipy.ndimage builds its kernel; r = 0 (sigma < 0.125) is the identity"""
    sigma = np.float64(sigma)
    r = blur_radius(sigma)
    if r == 0:
        return 0, np.ones(1)
    k = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    w = w / w.sum()
    return r, w[r:].copy()


def _range(name, v):
    try:
        lo, hi = (float(a) for a in v)
    except (TypeError, ValueError):
        raise N3DError("Appearance: %s is a (lo, hi) range (got %r)" % (name, v)) from None
    if not (np.isfinite(lo) and np.isfinite(hi) and 0 <= lo <= hi):
        raise N3DError("Appearance: %s needs finite 0 <= lo <= hi (got %r)" % (name, v))
    return lo, hi


class Appearance:
    """noise: the largest sigma of the additive Gaussian noise (drawn uniform in [0, noise]); blur: (lo, hi) of the Gaussian blur's
    sigma in voxels, per channel; contrast: (lo, hi) of the contrast factor, per channel; gamma: (lo, hi) of the exponent, per
    channel.  p_*: the probability that a patch gets the transform.  An option left None draws nothing and does nothing."""

    def __init__(self, noise=None, blur=None, contrast=None, gamma=None, p_noise=0.1, p_blur=0.2, p_contrast=0.15, p_gamma=0.3):
        if noise is not None:
            if not (np.ndim(noise) == 0 and np.isfinite(noise) and noise >= 0):
                raise N3DError("Appearance: noise is a finite non-negative sigma (got %r)" % (noise,))
            noise = float(noise)
        blur = _range("blur", blur) if blur is not None else None
        if blur is not None and blur_radius(blur[1]) > MAX_RADIUS:
            raise N3DError("Appearance: blur sigma %g needs radius %d, beyond N3D_APPEAR_MAX_RADIUS = %d (sigma < 1.625)" % (
                blur[1], blur_radius(blur[1]), MAX_RADIUS))
        contrast = _range("contrast", contrast) if contrast is not None else None
        gamma = _range("gamma", gamma) if gamma is not None else None
        for name, p in (("p_noise", p_noise), ("p_blur", p_blur), ("p_contrast", p_contrast), ("p_gamma", p_gamma)):
            if not (np.ndim(p) == 0 and np.isfinite(p) and 0 <= p <= 1):
                raise N3DError("Appearance: %s is a probability (got %r)" % (name, p))
        self.noise, self.blur, self.contrast, self.gamma = noise, blur, contrast, gamma
        self.p_noise, self.p_blur, self.p_contrast, self.p_gamma = float(p_noise), float(p_blur), float(p_contrast), float(p_gamma)
        self._scratch = {}

    def draw(self, np_rng, Cv):
        """the draws of ONE patch from an np.random-like object.  For each option that is set, in the order noise, blur, contrast,
        gamma: np_rng.uniform(), the transform being active iff that value is < p; only if active, its parameters: noise
        np_rng.uniform(0, noise) and then np_rng.randint(0, 2**32, 2, dtype=np.uint32) (the Philox key); blur / contrast / gamma
        np_rng.uniform(lo, hi, Cv).  Returns a dict of the active transforms: "noise": (sigma, (k0, k1)), "blur" / "contrast" /
        "gamma": (Cv,) float64."""
        d = {}
        if self.noise is not None and np_rng.uniform() < self.p_noise:
            sigma = np_rng.uniform(0, self.noise)
            key = np_rng.randint(0, 2 ** 32, 2, dtype=np.uint32)
            d["noise"] = (float(sigma), (int(key[0]), int(key[1])))
        for name, rng, p in (("blur", self.blur, self.p_blur), ("contrast", self.contrast, self.p_contrast), ("gamma", self.gamma, self.p_gamma)):
            if rng is not None and np_rng.uniform() < p:
                d[name] = np.asarray(np_rng.uniform(rng[0], rng[1], Cv), np.float64)
        return d

    @staticmethod
    def descriptors(draws, Cv):
        """the n3d_appear_desc table of a batch: one entry of `draws` per patch, a dict as draw() returns it or None"""
        descs = (AppearDesc * len(draws))()
        for b, d in enumerate(draws):
            if not d:
                continue
            rec = descs[b]
            if d.get("noise") is not None:
                sigma, key = d["noise"]
                rec.noise, rec.sigma = 1, float(sigma)
                rec.key[0], rec.key[1] = int(key[0]), int(key[1])
            for name, field in (("blur", None), ("contrast", rec.factor), ("gamma", rec.gamma_c)):
                if d.get(name) is None:
                    continue
                v = np.asarray(d[name], np.float64).reshape(-1)
                if v.shape != (Cv,):
                    raise N3DError("Appearance.apply: patch %d: %s takes one value per channel (%d, got %d)" % (b, name, Cv, v.size))
                setattr(rec, name, 1)
                for c in range(Cv):
                    if name == "blur":
                        if not (np.isfinite(v[c]) and v[c] >= 0):
                            raise N3DError("Appearance.apply: patch %d: a blur sigma is finite and non-negative (got %r)" % (b, v[c]))
                        r, w = blur_weights(v[c])
                        rec.radius[c] = r               # beyond N3D_APPEAR_MAX_RADIUS: the entry point refuses it
                        for k in range(min(r, MAX_RADIUS) + 1):
                            rec.weights[c][k] = float(w[k])
                    else:
                        field[c] = float(v[c])
        return descs

    def apply(self, x, draws):
        """x: (B, Cv, P, P, P) fp32 device tensor in NDHWC storage (K.empty_ndhwc, Trainer.input_buffers(), VolumeSet.patch_batch),
        transformed IN PLACE on the current stream by n3d_patch_appearance; draws: one entry per patch, a draw() dict or None.
        Returns x.  No host sync; with no active transform in the batch nothing is launched."""
        if not (isinstance(x, torch.Tensor) and x.dim() == 5):
            raise N3DError("Appearance.apply: expected a 5-D (B, Cv, P, P, P) tensor")
        if not x.is_cuda:
            raise N3DError("Appearance.apply: the batch is on %s: the transforms only run on a HIP (gfx950) device; there is no CPU "
                           "fallback" % x.device)
        if x.dtype != torch.float32:
            raise N3DError("Appearance.apply: fp32 expected, got %s" % x.dtype)
        B, Cv, P = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        ld = K._pitch_of(x)
        if ld is None or x.shape[3] != P or x.shape[4] != P or x.data_ptr() % 4:
            raise N3DError("Appearance.apply: the batch must be cubic patches in NDHWC (channels-last) storage, as K.empty_ndhwc / "
                           "Trainer.input_buffers() give it")
        if len(draws) != B:
            raise N3DError("Appearance.apply: one draw (or None) per patch (%d, got %d)" % (B, len(draws)))
        if not any(draws):
            return x
        descs = self.descriptors(draws, Cv)
        lib = _lib.load()
        key = (B, Cv, P, x.device)
        scratch = self._scratch.get(key)
        if scratch is None:
            scratch = self._scratch[key] = torch.empty(max(int(lib.n3d_patch_appearance_scratch(B, Cv, P)), 8), dtype=torch.uint8, device=x.device)
        check(lib.n3d_patch_appearance(K.ptr(x), ld, B, Cv, P, descs, K.ptr(scratch), scratch.numel(), K.stream_ptr()), "n3d_patch_appearance")
        return x
