#!/usr/bin/env python3
"""Generate tests/golden/metrics.npz: scipy's and numpy's answers for the segmentation metrics (nas_3d_unet_amd.metrics).

The reference has no code for these metrics; the fixture pins the definitions to the libraries they are written in:
  * surfaces:  mask & ~scipy.ndimage.binary_erosion(mask, generate_binary_structure(3, 1), border_value=0);
  * squared distances: scipy.ndimage.distance_transform_edt(~surface, return_indices=True) -- the integer squared distance to
    the nearest surface voxel it names, never the square of its float distance;
  * HD95: np.percentile(sqrt(D), 95), D the distances of both directions concatenated.
Needs scipy (1.15) and numpy; the tests need neither scipy nor this script's main().  Per case the fixture holds the inputs
(pred, truth, origin; origin -1: none, the box is the image) and flags, counts, the sorted squared distances of every region, the
order statistics, HD95 and HD100; per shape one mask with its full squared-distance volume (metrics.edt_sq).
Usage:  python tests/golden/make_golden_metrics.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# (13, 9, 21) with a (9, 7, 12) box at (2, 1, 5): odd sizes, box != image, truth addressed through the origin;
# (70, 5, 66): an axis longer than a wave in x and in z, and a 5-long axis; (3, 130, 4): a line longer than 128 in y, tiny other axes
SMALL, WIDE, TALL = (13, 9, 21), (70, 5, 66), (3, 130, 4)
BOX, ORIGIN = (9, 7, 12), (2, 1, 5)
SEED = 5150
INF = 1 << 29
REGION_LABELS = ((1, 2, 4), (1, 4), (4,))    # WT, TC, ET


def blob(shape, centre, radius, labels=(2, 1, 4)):
    """nested ellipsoids: labels[0] out to `radius`, labels[1] to 0.65 of it, labels[2] to 0.4 (centre, radius: fractions of shape)"""
    g = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    d = np.sqrt(sum(((g[a] - centre[a] * (shape[a] - 1)) / max(radius[a] * shape[a], 0.5)) ** 2 for a in range(3)))
    return np.select([d <= 0.4, d <= 0.65, d <= 1.0], [labels[2], labels[1], labels[0]], 0).astype(np.uint8)


def speckle(vol, rng, n):
    """n isolated voxels of random labels {1, 2, 4}: single-voxel components, all surface"""
    out = vol.copy()
    for _ in range(n):
        out[tuple(int(rng.integers(0, s)) for s in vol.shape)] = rng.choice(np.array([1, 2, 4], np.uint8))
    return out


def metric_cases():
    """[(name, pred (FX, FY, FZ) uint8, truth (X, Y, Z) uint8, origin or None)], seeded"""
    rng = np.random.default_rng(SEED)
    z = lambda s: np.zeros(s, np.uint8)
    cases = []
    # truth addressed through the origin; the prediction also has voxels outside the truth's box
    cases.append(("box", speckle(blob(SMALL, (0.5, 0.5, 0.5), (0.35, 0.4, 0.3)), rng, 6),
                  speckle(blob(BOX, (0.45, 0.5, 0.55), (0.4, 0.45, 0.4)), rng, 3), ORIGIN))
    cases.append(("wide", speckle(blob(WIDE, (0.5, 0.5, 0.45), (0.3, 0.6, 0.3)), rng, 10),
                  speckle(blob(WIDE, (0.45, 0.4, 0.5), (0.33, 0.5, 0.27)), rng, 10), None))
    cases.append(("tall", speckle(blob(TALL, (0.5, 0.5, 0.5), (0.6, 0.35, 0.6)), rng, 5),
                  speckle(blob(TALL, (0.5, 0.45, 0.4), (0.5, 0.4, 0.5)), rng, 5), None))
    # both masks reach every face of the image: edge voxels are surface
    cases.append(("faces", blob(SMALL, (0.5, 0.5, 0.5), (0.9, 0.9, 0.9)), blob(SMALL, (0.4, 0.6, 0.5), (0.8, 0.9, 0.85)), None))
    single_p, single_t = z(SMALL), z(SMALL)
    single_p[3, 4, 5] = 4
    single_t[9, 2, 17] = 4
    cases.append(("single", single_p, single_t, None))
    # a full-image mask (WT and TC; its surface is the shell), ET empty in the prediction only
    cases.append(("full", np.full(SMALL, 1, np.uint8), blob(SMALL, (0.5, 0.5, 0.5), (0.3, 0.35, 0.3)), None))
    eq = cases[1][2]
    cases.append(("equal", eq.copy(), eq.copy(), None))
    cases.append(("both_empty", z(SMALL), z(SMALL), None))
    cases.append(("pred_empty", z(SMALL), blob(BOX, (0.5, 0.5, 0.5), (0.4, 0.4, 0.4)), ORIGIN))
    cases.append(("truth_empty", blob(SMALL, (0.5, 0.5, 0.5), (0.3, 0.3, 0.3)), z(SMALL), None))
    # labels without 4: ET empty on both sides while WT and TC are not
    cases.append(("no_et", blob(SMALL, (0.5, 0.4, 0.5), (0.3, 0.4, 0.3), (2, 1, 1)), blob(SMALL, (0.5, 0.5, 0.55), (0.35, 0.4, 0.3), (2, 2, 1)), None))
    # two blobs far apart in the truth, one of them missed: the distances are bimodal and the percentile falls between distinct values
    two_t = np.maximum(blob(WIDE, (0.15, 0.5, 0.2), (0.1, 0.5, 0.12)), blob(WIDE, (0.8, 0.5, 0.8), (0.06, 0.4, 0.06)))
    cases.append(("two_blobs", blob(WIDE, (0.16, 0.5, 0.22), (0.1, 0.5, 0.11)), two_t, None))
    return cases


def edt_cases():
    """[(name, mask (X, Y, Z) uint8)]: one per shape, the nonzero labels of the first three cases' predictions"""
    return [("edt_" + n, (p != 0).astype(np.uint8)) for n, p, _, _ in metric_cases()[:3]]


def embed(truth, full, origin):
    out = np.zeros(full, np.uint8)
    o = (0, 0, 0) if origin is None else origin
    out[tuple(slice(a, a + b) for a, b in zip(o, truth.shape))] = truth
    return out


def k_of(n):
    return int(np.floor(np.float64(n - 1) * np.float64(0.95)))


def order_of(D):
    """(n, D[k], D[min(k + 1, n - 1)], max D) of a sorted integer array; zeros for an empty one"""
    n = len(D)
    if n == 0:
        return [0, 0, 0, 0]
    k = k_of(n)
    return [n, int(D[k]), int(D[min(k + 1, n - 1)]), int(D[-1])]


def _scipy_surface(mask):
    from scipy import ndimage
    return mask & ~ndimage.binary_erosion(mask, ndimage.generate_binary_structure(3, 1), border_value=0)


def _scipy_d2(surface):
    from scipy import ndimage
    if not surface.any():
        return np.full(surface.shape, INF, np.int64)
    _, idx = ndimage.distance_transform_edt(~surface, return_indices=True)
    g = np.meshgrid(*[np.arange(n) for n in surface.shape], indexing="ij")
    return sum((idx[a].astype(np.int64) - g[a]) ** 2 for a in range(3))


def scipy_answers(pred, truth, origin):
    t = embed(truth, pred.shape, origin)
    flags = np.zeros(pred.shape, np.uint8)
    counts, order, Ds, hd95, hd100 = [], [], [], [], []
    for r, labs in enumerate(REGION_LABELS):
        mp, mt = np.isin(pred, labs), np.isin(t, labs)
        counts.append([int((mp & mt).sum()), int((mp & ~mt).sum()), int((~mp & mt).sum())])
        sp, st = _scipy_surface(mp), _scipy_surface(mt)
        flags |= (sp.astype(np.uint8) << r) | (st.astype(np.uint8) << (3 + r))
        if mp.any() and mt.any():
            D = np.sort(np.concatenate([_scipy_d2(st)[sp], _scipy_d2(sp)[st]]))
            dist = np.sqrt(D.astype(np.float64))
            hd95.append(np.percentile(dist, 95))
            hd100.append(dist.max())
        else:
            D = np.zeros(0, np.int64)
            both = not mp.any() and not mt.any()
            hd95.append(0.0 if both else np.nan)
            hd100.append(0.0 if both else np.nan)
        Ds.append(D.astype(np.int64))
        order.append(order_of(D))
    return flags, np.array(counts, np.int64), np.array(order, np.int64), Ds, np.array(hd95, np.float64), np.array(hd100, np.float64)


def main():
    out, ts = {}, []
    names = []
    for name, pred, truth, origin in metric_cases():
        flags, counts, order, Ds, hd95, hd100 = scipy_answers(pred, truth, origin)
        names.append(name)
        out[name + "/pred"], out[name + "/truth"] = pred, truth
        out[name + "/origin"] = np.array(origin if origin is not None else (-1, -1, -1), np.int32)
        out[name + "/flags"], out[name + "/counts"], out[name + "/order"] = flags, counts, order
        out[name + "/hd95"], out[name + "/hd100"] = hd95, hd100
        for r in range(3):
            out["%s/d2_%d" % (name, r)] = Ds[r]
            if order[r, 0]:
                vi = np.float64(order[r, 0] - 1) * np.float64(0.95)
                ts.append(float(vi - np.floor(vi)))
        print("%-12s %-12s counts %s order %s hd95 %s" % (name, pred.shape, counts.tolist(), order.tolist(), hd95.tolist()))
    assert any(t >= 0.5 for t in ts) and any(0 < t < 0.5 for t in ts), ts
    assert any(o[1] != o[2] for n in names for o in out[n + "/order"]), "no case interpolates between distinct values"
    out["names"] = np.array(names)
    for name, mask in edt_cases():
        out[name + "/mask"] = mask
        out[name + "/d2"] = _scipy_d2(mask.astype(bool)).astype(np.int32)
    out["edt_names"] = np.array([n for n, _ in edt_cases()])
    path = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote %s  (%d arrays, %.1f KB)" % (path, len(out), size / 1024))
    assert size < 256 * 1024


if __name__ == "__main__":
    sys.exit(main())
