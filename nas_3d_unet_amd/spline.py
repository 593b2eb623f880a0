"""Cubic B-spline (order 3) interpolation of the data in the patch gather: what scipy.ndimage.map_coordinates(order=3, mode="constant")
makes of the crop (none of it the reference's; the default resampler of nnU-Net / batchgenerators / TorchIO; the rule is stated in
include/n3d.h under n3d_patch_gather_spline and pinned to scipy by tests/golden/spline.npz).

The gather is reached through VolumeSet.patch_batch(..., warp=[(matrix, 3, gain, bias), ...]) and
Generator(augment=True, augment_interpolation="spline3").  Here: the prefilter's five constants as the C entry point computes them,
and the prefilter alone (n3d_spline_prefilter) on a tensor of cubes."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import kernels as K
from ._lib import N3DError, check

ORDER = 3
MIN_PATCH = 4          # the taps f-1 .. f+2 are mirrored into the crop


def constants(P):
    """(z, gain, zn, inv0, anti) of a line of P samples, in fp64: z = sqrt(3) - 2, gain = (1 - z) * (1 - 1 / z), zn = z multiplied up
    to P - 1 factors one by one (not pow), inv0 = 1 / (1 - zn * zn), anti = z / (z * z - 1)"""
    if P < MIN_PATCH:
        raise N3DError("spline: a line has at least %d samples (got %d)" % (MIN_PATCH, P))
    z = np.sqrt(np.float64(3.0)) - np.float64(2.0)
    gain = (1.0 - z) * (1.0 - 1.0 / z)
    zn = z
    for _ in range(P - 2):
        zn = zn * z
    return z, gain, zn, 1.0 / (1.0 - zn * zn), z / (z * z - 1.0)


def prefilter(x):
    """the fp64 B-spline coefficients of x (..., P, P, P): a contiguous fp32 tensor on the device, every trailing cube filtered on its
    own along axis 0, then 1, then 2 with mirror boundaries (three launches on the current stream)"""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() >= 3
            and x.shape[-1] == x.shape[-2] == x.shape[-3] and x.numel() > 0):
        raise N3DError("spline.prefilter: x is a contiguous fp32 device tensor (..., P, P, P)")
    P = int(x.shape[-1])
    if P < MIN_PATCH:
        raise N3DError("spline.prefilter: P must be at least %d (got %d)" % (MIN_PATCH, P))
    coef = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    check(_lib.load().n3d_spline_prefilter(K.ptr(x), x.numel() // P ** 3, P, K.ptr(coef), K.stream_ptr()), "n3d_spline_prefilter")
    return coef
