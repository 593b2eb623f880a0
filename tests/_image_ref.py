"""numpy restatement of the whole-image passes (n3d_image_embed / n3d_image_add / n3d_image_finish; prediction.py:102-119) and the
seeded subject of tests/golden/fullimage.npz.  Sums run in fp64, one key after the other, as the kernels' do."""
import numpy as np

from oracle import post_step as ps

# ---- the fixture's subject (tests/golden/make_golden_fullimage.py): regenerated from the seed, only outputs are stored
FIX_SEED = 20261018
FIX_FULL, FIX_BOX, FIX_ORIGIN = (48, 40, 27), (37, 30, 20), (6, 5, 4)
FIX_DEPTH, FIX_GENE = 4, "G_ALL"
FIX_PAD = (16, 24, 5)          # 2 ** (depth + 1) - F % 2 ** (depth + 1): the depth-4 net halves its grid five times
TOL = 2e-5                     # test_gpu_nets.py's bound on this net's probabilities


def fixture_box(seed=FIX_SEED, box=FIX_BOX):
    """(4, bx, by, bz) float32: N(0, 1) everywhere but a slab and a sprinkling of voxels where every modality is zero"""
    rng = np.random.default_rng(seed)
    vol = rng.standard_normal((4,) + tuple(box)).astype(np.float32)
    vol[:, 9:12, :, :5] = 0
    holes = rng.uniform(0, 1, box) < 0.03
    vol[:, holes] = 0
    return vol


def place(box, origin, full):
    """the (Cv, FX, FY, FZ) image with the box at `origin`, zeros around it"""
    img = np.zeros((box.shape[0],) + tuple(full), dtype=box.dtype)
    o = origin
    img[:, o[0]:o[0] + box.shape[1], o[1]:o[1] + box.shape[2], o[2]:o[2] + box.shape[3]] = box
    return img


def _flip(a, flip):
    axes = tuple(1 + i for i in range(3) if flip[i])
    return np.flip(a, axes) if axes else a


def embed(box, origin, full, padded, flip=(False, False, False)):
    """(Cv, PX, PY, PZ): the image mirrored within [0, F) along the axes of `flip`, zero-padded at the high end"""
    img = _flip(place(box, origin, full), flip)
    return np.pad(img, [(0, 0)] + [(0, int(p) - int(f)) for p, f in zip(padded, full)], "constant", constant_values=0)


def unflip_crop(y, full, flip):
    """the prediction (C, PX, PY, PZ) of an image embedded under `flip`, back on the image's own grid"""
    return _flip(y[:, :full[0], :full[1], :full[2]], flip)


def add(sum_, y, full, flip):
    """one key that is not the last: the first one writes, the others add (fp64)"""
    t = unflip_crop(y, full, flip).astype(np.float64)
    return t.copy() if sum_ is None else sum_ + t


def finish(y, full, flip=(False, False, False), sum_=None, n_keys=1, threshold=0.5, inclusive=True, mask_box=None, origin=(0, 0, 0)):
    """(labels uint8 (FX, FY, FZ), probs float64 (C, FX, FY, FZ)): mean = (sum + y) / K in key order (K == 1: exactly y), labels
    fused from the mean and zeroed where every channel of the box is zero and outside the box"""
    t = unflip_crop(y, full, flip).astype(np.float64)
    assert (sum_ is None) == (n_keys == 1)
    mean = t.copy() if sum_ is None else (sum_ + t) / float(n_keys)
    labels = ps.tumor_labels(mean, threshold, inclusive) if mean.shape[0] == 3 else None
    if labels is not None and mask_box is not None:
        labels = labels * skull(mask_box, origin, full)
    return labels, mean


def skull(box, origin, full):
    return np.any(place(box, origin, full) != 0, axis=0).astype(np.uint8)
