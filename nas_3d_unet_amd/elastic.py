"""Elastic deformation in the patch gather: a free-form deformation on a coarse lattice of uniform cubic B-splines whose control
values the device generates from an 8-byte key (none of it the reference's; the transform is batchgenerators' / TorchIO's
RandomElasticDeformation / MONAI's Rand3DElastic; the rule is stated in include/n3d.h under n3d_patch_edesc and pinned to scipy by
tests/golden/elastic.npz).

Host logic only: the options, their limits and the draws of a patch; the kernel is behind n3d_patch_gather_elastic, reached through
VolumeSet.patch_batch(..., elastic=).  Generator(augment=True, augment_elastic=Elastic(...)) makes the draws per kept patch and
composes the displacement into every batch's single gather launch."""
from __future__ import annotations

import numpy as np

from ._lib import N3DError

MAX_BATCH = 8      # N3D_PATCH_ELASTIC_MAX_BATCH
MAX_CELLS = 8      # N3D_PATCH_ELASTIC_MAX_CELLS
MAX_LOCK = 3


def check_lattice(cells, lock, who="Elastic"):
    """1 <= cells <= 8, 0 <= lock <= 3 and at least one free control point per axis: (cells + 3) - 2 * lock >= 1"""
    for name, v in (("cells", cells), ("lock", lock)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise N3DError("%s: %s is an integer (got %r)" % (who, name, v))
    if not 1 <= cells <= MAX_CELLS:
        raise N3DError("%s: cells must be 1..%d (got %d)" % (who, MAX_CELLS, cells))
    if not 0 <= lock <= MAX_LOCK:
        raise N3DError("%s: lock must be 0..%d (got %d)" % (who, MAX_LOCK, lock))
    if cells + 3 - 2 * lock < 1:
        raise N3DError("%s: lock %d leaves no free control point on a lattice of %d per axis (cells %d)" % (who, lock, cells + 3, cells))


def inv_h(cells, P):
    """n / (P - 1) in fp64: the lattice coordinate of patch index j is j * inv_h"""
    if P < 2:
        raise N3DError("Elastic: the lattice spans the patch indices 0 .. P - 1: P must be at least 2 (got %d)" % P)
    return np.float64(cells) / np.float64(P - 1)


class Elastic:
    """cells: lattice cells per axis (1..8; the lattice has cells + 3 control points per axis); displacement: the largest
    displacement in voxels, a scalar or three per-axis maxima (amp of n3d_patch_edesc: every control value is uniform in
    [-displacement, displacement)); p: the probability that a patch is deformed; lock: the control points within `lock` of the
    lattice's border are 0 (2: TorchIO's locked_borders; 3: the patch's faces do not move)."""

    def __init__(self, cells=4, displacement=2.0, p=0.2, lock=2):
        check_lattice(cells, lock)
        if not (np.ndim(p) == 0 and np.isfinite(p) and 0 <= p <= 1):
            raise N3DError("Elastic: p is a probability (got %r)" % (p,))
        try:
            d = np.asarray(displacement, np.float64)
        except (TypeError, ValueError):
            raise N3DError("Elastic: displacement is a number or three per-axis maxima (got %r)" % (displacement,)) from None
        if d.shape not in ((), (3,)) or not np.isfinite(d).all() or (d < 0).any():
            raise N3DError("Elastic: displacement is finite and >= 0, a scalar or one per axis (got %r)" % (displacement,))
        self.cells, self.lock, self.p = int(cells), int(lock), float(p)
        self.amp = tuple(float(a) for a in np.broadcast_to(d, (3,)))

    def check(self, P):
        """the folding bound: the field's slope is at most 2 * displacement / h with h = (P - 1) / cells the lattice spacing in
        voxels, so the map is one-to-one for displacement < h / 2; raises N3DError otherwise"""
        bound = (int(P) - 1) / (2.0 * self.cells)
        if not max(self.amp) < bound:
            raise N3DError("Elastic: displacement %g >= (P - 1) / (2 * cells) = (%d - 1) / (2 * %d) = %g voxels: the deformation could "
                           "fold" % (max(self.amp), int(P), self.cells, bound))

    def draw(self, np_rng):
        """the draws of ONE patch from an np.random-like object: np_rng.uniform(), the transform being active iff that value is < p;
        only if active, np_rng.randint(0, 2**32, 2, dtype=np.uint32) (the Philox key of the control values).  Returns the key
        (k0, k1), or None for a patch that is not deformed."""
        if not np_rng.uniform() < self.p:
            return None
        key = np_rng.randint(0, 2 ** 32, 2, dtype=np.uint32)
        return int(key[0]), int(key[1])

    def entry(self, key):
        """patch_batch's `elastic` entry of a draw: None, or (cells, lock, key, amp)"""
        return None if key is None else (self.cells, self.lock, key, self.amp)
