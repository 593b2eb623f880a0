"""Random and foreground-centred crops drawn on the device (none of it the reference's; nnU-Net's oversampled foreground, MONAI's
RandCropByPosNegLabel / RandCropByLabelClasses, TorchIO's LabelSampler; the rule is stated in include/n3d.h under n3d_patch_sample).

Host logic only: the options and their limits.  The kernels are behind n3d_volume_line_index and n3d_patch_sample, reached through
VolumeSet.line_index and VolumeSet.sample (generator.py).  Generator(..., sampling=RandomCrop(...)) draws one key per epoch and
replaces the candidate grid by one n3d_patch_sample launch; everything downstream of the candidate table stays what it was."""
from __future__ import annotations

import numpy as np

from ._lib import N3DError

MASKS = ("brain", "tumour", 1, 2, 4)   # N3D_SAMPLE_MASKS: mask m is bit m of n3d_patch_sample's `masks`
MAX_SAMPLES = 1 << 24                   # N3D_SAMPLE_MAX
MODE_UNIFORM, MODE_FALLBACK, MODE_BAD_ID = 255, 254, 253   # N3D_SAMPLE_MODE_UNIFORM / N3D_SAMPLE_MODE_FALLBACK / N3D_SAMPLE_MODE_BAD_ID


def mask_bits(masks, who="RandomCrop"):
    """the `masks` word of n3d_patch_sample for an iterable of mask names ("brain", "tumour", 1, 2, 4)"""
    if isinstance(masks, (str, int, np.integer)):
        raise N3DError("%s: masks is a tuple of mask names out of %r (got %r)" % (who, MASKS, masks))
    bits = 0
    for m in masks:
        if isinstance(m, bool) or not isinstance(m, (str, int, np.integer)) or m not in MASKS:
            raise N3DError("%s: a mask is one of %r (got %r)" % (who, MASKS, m))
        bits |= 1 << MASKS.index(m)
    return bits


def fg_threshold(foreground, who="RandomCrop"):
    """the probability of a foreground-centred sample as n3d_patch_sample takes it: int(round(foreground * 2**32)), in [0, 2**32]"""
    if isinstance(foreground, bool) or not (np.ndim(foreground) == 0 and np.isfinite(foreground) and 0 <= foreground <= 1):
        raise N3DError("%s: foreground is a probability (got %r)" % (who, foreground))
    return int(round(float(foreground) * 2 ** 32))


class RandomCrop:
    """patches_per_epoch: the number of crops drawn per epoch (1 .. 2^24; the empty-patch and skip_health filters then apply to them
    as they do to the grid's candidates); foreground: the probability that a crop is centred on a voxel of a mask -- the decision is
    per sample, there is no per-batch guarantee; masks: the masks a foreground crop chooses from, uniformly among those present in the
    drawn volume: "brain" (some modality nonzero), "tumour" (label != 0), 1, 2, 4 (that label).  masks=(1, 2, 4) is nnU-Net's
    class-uniform choice, masks=("tumour",) MONAI's positive / negative crop."""

    def __init__(self, patches_per_epoch, foreground=1 / 3, masks=("tumour",)):
        n = patches_per_epoch
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= MAX_SAMPLES:
            raise N3DError("RandomCrop: patches_per_epoch is an integer in 1 .. %d (got %r)" % (MAX_SAMPLES, n))
        self.fg_threshold = fg_threshold(foreground)
        self.mask_bits = mask_bits(masks)
        if self.mask_bits == 0 and self.fg_threshold > 0:
            raise N3DError("RandomCrop: foreground > 0 needs at least one mask")
        self.patches_per_epoch, self.foreground, self.masks = int(n), float(foreground), tuple(masks)

    def needs_truth(self):
        """some mask other than "brain" is requested: the set must hold truth"""
        return bool(self.mask_bits & ~1)

    def draw(self, np_rng):
        """the draw of ONE epoch from an np.random-like object: np_rng.randint(0, 2**32, 2, dtype=np.uint32), the Philox key of the
        epoch's samples (the call Elastic.draw makes for a patch).  Returns (k0, k1)."""
        key = np_rng.randint(0, 2 ** 32, 2, dtype=np.uint32)
        return int(key[0]), int(key[1])
