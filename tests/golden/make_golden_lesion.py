#!/usr/bin/env python3
"""Generate tests/golden/lesion.npz: scipy's answers for the lesion-wise metrics (nas_3d_unet_amd.metrics.score_lesions; include/n3d.h,
"Lesion-wise metrics") -- the BraTS 2023 lesion-wise Dice and Hausdorff95.

The reference has no code for this step, and neither the organisers' script nor cc3d is at hand; the fixture pins the definition to
scipy.ndimage and claims nothing else.  Per region (WT = label != 0, TC = label in {1, 4}, ET = label == 4):
  * Gd = binary_dilation(G, generate_binary_structure(3, 2), iterations=d) (border value 0; d = 0: G itself);
  * lesions = label(Gd, generate_binary_structure(3, 3)); a lesion's id is the smallest linear index of its DILATED component, the
    lesions are listed by ascending id, lesion l owns G & (component l);
  * predicted components = label(P, generate_binary_structure(3, 3)); component c matches lesion l iff some voxel lies in both;
  * per lesion gt_voxels, tp = |P & G_l|, pred_voxels / n_matched over the matched components, and the squared surface distances
    between the union of the matched components and G_l (surfaces and distances as make_golden_metrics.py has them) -> n, D[k],
    D[k + 1], max D; the components that match nothing are the false positives.
  * folded: kept = lesions with gt_voxels > min_lesion_voxels; an unmatched kept lesion is Dice 0, HD95 penalty; den = kept + n_fp;
    dice = sum / den, hd95 = (sum + penalty * n_fp) / den, one fp64 addition per lesion in id order; den == 0: 1.0 and 0.0.  HD95 of a
    lesion is np.percentile(sqrt(D), 95) on the distances themselves.
The rules are stated here in this script's own code.  Needs scipy (1.15) and numpy; the tests need neither scipy nor this script's
main().  Per case the fixture holds the inputs, the dilated WT mask for d = 0 .. 5, the full record at d = 3 (and at further d for
some cases), and the folded floats for FOLDS.  Fixed member times and order: a second run gives the same bytes.
Usage:  python tests/golden/make_golden_lesion.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_components import first_index_ids, write_npz          # noqa: E402
from make_golden_metrics import REGION_LABELS, _scipy_d2, _scipy_surface, embed, order_of   # noqa: E402

MAX_LESIONS, HEADER_WORDS, ROW_WORDS = 64, 8, 9
REGION_WORDS = HEADER_WORDS + MAX_LESIONS * ROW_WORDS
DILATION = 3
FOLDS = ((50, 374.0), (5, 374.0), (0, 100.0))             # (min_lesion_voxels, penalty_hd95)
EXTRA_DILATIONS = {"gaps": (0, 1, 5), "box": (5,), "diagonal": (2,), "rim": (2,)}
BOX_FULL, BOX, BOX_ORIGIN = (13, 9, 21), (9, 7, 12), (2, 1, 5)
DIAG_A, DIAG_B, DIAG_C = (4, 4, 2), (9, 9, 7), (15, 15, 2)   # B = A + (5, 5, 5): the dilations touch by corners only; C is apart


def grid_points(n):
    """the first n points, in linear-index order, of the 5 x 5 x 3 grid with pitch 8 inside (40, 40, 24)"""
    pts = [(x, y, z) for x in range(3, 40, 8) for y in range(3, 40, 8) for z in range(3, 24, 8)]
    return pts[:n]


def cap_case(n):
    """n single-voxel lesions 8 apart (label 4: all three regions) in (40, 40, 24); the prediction hits every fourth one exactly,
    lies one voxel beside every fourth other one, and has one stray voxel"""
    truth, pred = np.zeros((40, 40, 24), np.uint8), np.zeros((40, 40, 24), np.uint8)
    for i, p in enumerate(grid_points(n)):
        truth[p] = 4
        if i % 4 == 0:
            pred[p] = 4
        elif i % 4 == 1:
            pred[p[0] + 1, p[1], p[2]] = 4
    pred[39, 39, 23] = 2
    return pred, truth


def lesion_cases():
    """[(name, pred (FX, FY, FZ) uint8, truth (X, Y, Z) uint8, origin or None)]; numpy only"""
    z = lambda s: np.zeros(s, np.uint8)
    cases = []
    # blobs on a z line, 6 and then 7 empty voxels between them: {A, B} is one lesion, C another; C crosses z = 32
    t, p = z((12, 11, 45)), z((12, 11, 45))
    t[4:7, 4:7, 8:11] = 4
    t[4:7, 4:7, 17:20] = 1
    t[4:7, 4:7, 27:34] = 2
    p[5:8, 4:7, 8:11] = 4
    p[4:7, 3:6, 28:33] = 2
    p[1, 1, 40] = 1
    cases.append(("gaps", p, t, None))
    # single voxels: the polyhedron's extent and corner-only contact of two dilations
    t, p = z((21, 19, 13)), z((21, 19, 13))
    t[DIAG_A], t[DIAG_B], t[DIAG_C] = 2, 4, 1
    p[DIAG_A[0] + 3, DIAG_A[1] + 3, DIAG_A[2]] = 2          # inside A's dilation
    p[DIAG_A[0] + 3, DIAG_A[1] + 3, DIAG_A[2] + 1] = 2      # 6-connected to it, outside the dilation itself
    p[DIAG_C[0] + 3, DIAG_C[1] + 3, DIAG_C[2] + 1] = 1      # beside C's dilation only: a false positive
    p[DIAG_B] = 4
    cases.append(("diagonal", p, t, None))
    # one predicted bar through two lesions
    t, p = z((11, 10, 34)), z((11, 10, 34))
    t[3:7, 3:7, 3:7] = 2
    t[3:7, 3:7, 23:27] = 4
    p[5, 5, 5:26] = 4
    cases.append(("bridge", p, t, None))
    # a predicted component in the dilation rim only
    t, p = z((11, 10, 15)), z((11, 10, 15))
    t[3:7, 3:7, 3:7] = 4
    p[3:7, 3:7, 9] = 4
    cases.append(("rim", p, t, None))
    # a 60-voxel lesion, a 3-voxel lesion; three false positives (one a single voxel) and a component that matches the small one only
    t, p = z((25, 12, 30)), z((25, 12, 30))
    t[2:6, 2:7, 2:5] = 2
    t[12, 6, 20:23] = 2
    p[3:6, 2:7, 2:6] = 2
    p[12, 6, 24] = 2
    p[20, 2, 2] = 2
    p[20, 8, 10:12] = 1
    p[20, 2, 25:28] = 4
    cases.append(("fps", p, t, None))
    # lesions of exactly 5 and 6 voxels, 7 empty voxels apart
    t, p = z((9, 15, 10)), z((9, 15, 10))
    t[3, 3, 2:7] = 4
    t[3, 11, 2:8] = 4
    p[3, 3, 3:7] = 4
    p[3:5, 11, 2:8] = 4
    cases.append(("threshold", p, t, None))
    # truth in a box: a lesion on the box's faces, one whose dilation the image border clips
    t, p = z(BOX), z(BOX_FULL)
    t[0:2, 2:4, 0:2] = 4
    t[7:9, 5:7, 10:12] = 1
    p[1:4, 3:5, 4:7] = 4
    p[10:13, 6:9, 16:19] = 1
    p[0, 0, 20] = 2
    cases.append(("box", p, t, BOX_ORIGIN))
    # labels 1 / 2 / 4: WT one lesion, TC and ET two
    t, p = z((13, 11, 23)), z((13, 11, 23))
    t[3:10, 3:8, 3:20] = 2
    t[4:7, 4:7, 4:7] = 1
    t[4:6, 4:6, 4:6] = 4
    t[4:6, 4:6, 14:16] = 4
    p[2:9, 3:8, 4:19] = 2
    p[4:6, 4:6, 5:7] = 4
    p[4:6, 4:7, 14:17] = 1
    cases.append(("nested", p, t, None))
    blob = z(BOX_FULL)
    blob[4:8, 3:6, 8:13] = 4
    blob[5, 4, 9:11] = 1
    cases.append(("both_empty", z(BOX_FULL), z(BOX_FULL), None))
    cases.append(("pred_empty", z(BOX_FULL), blob[2:11, 1:8, 5:17].copy(), BOX_ORIGIN))
    cases.append(("truth_empty", blob.copy(), z(BOX_FULL), None))
    cases.append(("cap64",) + cap_case(64) + (None,))
    return cases


def scipy_dilate(mask, d):
    from scipy import ndimage
    return ndimage.binary_dilation(mask, ndimage.generate_binary_structure(3, 2), iterations=d) if d else mask.copy()


def scipy_ids26(mask):
    from scipy import ndimage
    lab, _ = ndimage.label(mask, ndimage.generate_binary_structure(3, 3))
    return first_index_ids(lab)


def scipy_region(P, G, d):
    """-> (header [n_lesions, n_pred_components, n_fp, fp_voxels], rows [[id, gt, tp, pred, n_matched, n, Dk, Dk1, Dmax]], the
    sorted distances per lesion)"""
    idg, idp = scipy_ids26(scipy_dilate(G, d)), scipy_ids26(P)
    sp, sg = _scipy_surface(P), _scipy_surface(G)
    rows, Ds, matched_any = [], [], set()
    for lid in np.unique(idg[idg >= 0]):
        comp = idg == lid
        Gl = G & comp
        assert Gl.any()
        matched = np.unique(idp[comp & P])
        matched_any.update(int(c) for c in matched)
        Pl = np.isin(idp, matched) & P
        if len(matched):
            a, b = sp & Pl, sg & Gl
            assert np.array_equal(a, _scipy_surface(Pl)) and np.array_equal(b, _scipy_surface(Gl))
            D = np.sort(np.concatenate([_scipy_d2(b)[a], _scipy_d2(a)[b]])).astype(np.int64)
        else:
            D = np.zeros(0, np.int64)
        rows.append([int(lid), int(Gl.sum()), int((P & Gl).sum()), int(Pl.sum()), len(matched)] + order_of(D))
        Ds.append(D)
    comps = np.unique(idp[idp >= 0])
    fps = [int(c) for c in comps if int(c) not in matched_any]
    header = [len(rows), len(comps), len(fps), int(sum((idp == c).sum() for c in fps))]
    return header, rows, Ds


def scipy_record(pred, truth, origin, d):
    t = embed(truth, pred.shape, origin)
    rec = np.zeros((3, REGION_WORDS), np.int64)
    Ds = []
    for r, labs in enumerate(REGION_LABELS):
        header, rows, D = scipy_region(np.isin(pred, labs), np.isin(t, labs), d)
        assert len(rows) <= MAX_LESIONS
        rec[r, :4] = header
        if rows:
            rec[r, HEADER_WORDS:HEADER_WORDS + ROW_WORDS * len(rows)] = np.array(rows, np.int64).ravel()
        Ds.append(D)
    return rec.ravel(), Ds


def fold(rec, Ds, min_lesion_voxels, penalty):
    """-> float64 (3, 2): [region][lesion-wise Dice, lesion-wise HD95]"""
    out = np.zeros((3, 2), np.float64)
    rec = rec.reshape(3, REGION_WORDS)
    for r in range(3):
        n_lesions, n_fp = int(rec[r, 0]), int(rec[r, 2])
        dice_sum, hd_sum, kept = np.float64(0), np.float64(0), 0
        for l in range(n_lesions):
            _, gt, tp, pv, nm = (int(v) for v in rec[r, HEADER_WORDS + ROW_WORDS * l:][:5])
            if gt <= min_lesion_voxels:
                continue
            kept += 1
            if nm:
                dice_sum = dice_sum + np.float64(2 * tp) / np.float64(pv + gt)
                hd_sum = hd_sum + np.percentile(np.sqrt(Ds[r][l].astype(np.float64)), 95)
            else:
                hd_sum = hd_sum + np.float64(penalty)
        den = kept + n_fp
        out[r] = (1.0, 0.0) if den == 0 else (dice_sum / np.float64(den), (hd_sum + np.float64(penalty) * np.float64(n_fp)) / np.float64(den))
    return out


def region_rows(rec, r):
    rec = rec.reshape(3, REGION_WORDS)
    n = int(rec[r, 0])
    return rec[r, :HEADER_WORDS], rec[r, HEADER_WORDS:HEADER_WORDS + ROW_WORDS * n].reshape(n, ROW_WORDS)


def main():
    out, names = {}, []
    for name, pred, truth, origin in lesion_cases():
        names.append(name)
        out[name + "/pred"], out[name + "/truth"] = pred, truth
        out[name + "/origin"] = np.array(origin if origin is not None else (-1, -1, -1), np.int32)
        wt = embed(truth, pred.shape, origin) != 0
        dil = np.stack([scipy_dilate(wt, d) for d in range(6)]).astype(np.uint8)
        out[name + "/dilated"] = dil
        rec, Ds = scipy_record(pred, truth, origin, DILATION)
        out[name + "/record"] = rec
        for d in EXTRA_DILATIONS.get(name, ()):
            out["%s/record_d%d" % (name, d)] = scipy_record(pred, truth, origin, d)[0]
        folded = [fold(rec, Ds, mv, pen) for mv, pen in FOLDS]
        for i, f in enumerate(folded):
            out["%s/folded_%d" % (name, i)] = f
        (h0, w0), (h1, w1), (h2, w2) = (region_rows(rec, r) for r in range(3))
        print("%-12s %-13s lesions %s comps %s fp %s  WT rows %s  folded(50) %s" % (
            name, pred.shape, [int(h[0]) for h in (h0, h1, h2)], [int(h[1]) for h in (h0, h1, h2)], [int(h[2]) for h in (h0, h1, h2)],
            w0[:3].tolist(), folded[0].tolist()))
        # ---- the property each case is built for
        if name == "gaps":
            assert h0[0] == 2 and w0[0, 1] == 27 + 27 and w0[1, 1] == 63 and (truth[5, 5, 11:17] == 0).all() and (truth[5, 5, 20:27] == 0).all()
            assert truth[5, 5, 31] and truth[5, 5, 32]                                   # the line crosses z = 32
            assert w0[0, 0] < w0[1, 0] and h0[2] == 1                                    # ascending ids; the stray voxel
            r1 = region_rows(out["gaps/record_d1"], 0)[0]
            assert r1[0] == 3                                                            # at d = 1 the three blobs are three lesions
        if name == "diagonal":
            a = DIAG_A
            assert dil[3][a[0] + 3, a[1] + 3, a[2]] and not dil[3][a[0] + 3, a[1] + 3, a[2] + 1]
            assert dil[3][a[0], a[1], 0] and dil[3][a[0] + 2, a[1] + 2, a[2] + 2] and not dil[3][a[0] + 3, a[1] + 2, a[2] + 2]
            one = np.zeros_like(wt)
            one[DIAG_A] = True
            da = scipy_dilate(one, 3)
            one[DIAG_A], one[DIAG_B] = False, True
            db = scipy_dilate(one, 3)
            assert da.sum() < 263 and db.sum() == 263                                    # A's is clipped at z = 0
            assert not (da & db).any()
            from scipy import ndimage
            assert not (ndimage.binary_dilation(da, ndimage.generate_binary_structure(3, 2)) & db).any()   # no face or edge contact
            assert (ndimage.binary_dilation(da, ndimage.generate_binary_structure(3, 3)) & db).any()       # a corner contact
            assert h0[0] == 2 and w0[0, 1] == 2 and w0[1, 1] == 1                        # {A, B} one lesion, C another
            assert w0[0, 4] == 2 and w0[0, 3] == 3 and h0[2] == 1                        # the pair component counts whole; one FP
        if name == "bridge":
            assert h0[0] == 2 and h0[1] == 1 and h0[2] == 0 and (w0[:, 3] == 21).all() and (w0[:, 4] == 1).all()
        if name == "rim":
            assert h0[0] == 1 and w0[0, 2] == 0 and w0[0, 4] == 1 and w0[0, 5] > 0 and w0[0, 6] >= 4 and h0[2] == 0
            assert folded[0][0, 0] == 0.0 and 2.0 <= folded[0][0, 1] < 10.0              # tp 0, Dice 0, a real HD95 and not the penalty
            assert region_rows(out["rim/record_d2"], 0)[0][2] == 1                       # at d = 2 the rim ends one voxel short
        if name == "fps":
            assert h0[0] == 2 and h0[1] == 5 and h0[2] == 3 and h0[3] == 1 + 2 + 3 and w0[:, 1].tolist() == [60, 3] and w0[1, 4] == 1
            # at 50 and 5 the small lesion is dropped and its component is neither scored nor a false positive: den = 1 + 3
            d50 = 2.0 * w0[0, 2] / (w0[0, 3] + w0[0, 1]) / 4
            assert folded[0][0, 0] == d50 and folded[1][0, 0] == d50 and folded[2][0, 0] != d50
        if name == "threshold":
            assert h0[0] == 2 and w0[:, 1].tolist() == [5, 6]
            assert folded[1][0, 0] == (2.0 * w0[1, 2] / (w0[1, 3] + 6))                   # at 5: only the 6-voxel lesion
            assert folded[2][0, 0] == (np.float64(2.0 * w0[0, 2]) / (w0[0, 3] + 5) + np.float64(2.0 * w0[1, 2]) / (w0[1, 3] + 6)) / 2
        if name == "box":
            assert h0[0] == 2 and truth[0, 2, 0] and dil[3][0, 3, 5] and dil[3][2, 3, 2]     # on the box's faces, grown beyond them
            assert truth[8, 6, 11] and dil[3][12, 8, 16] and dil[3][:, :, 20].sum() == 0   # B's dilation ends at the image's x and y faces
            assert h0[2] == 1
        if name == "nested":
            assert h0[0] == 1 and h1[0] == 2 and h2[0] == 2
        if name == "both_empty":
            assert not rec.any() and all((f == [[1.0, 0.0]] * 3).all() for f in folded)
        if name == "pred_empty":
            assert h0[0] == 1 and h0[1] == 0 and w0[0, 4] == 0 and w0[0, 5] == 0 and folded[0][0].tolist() == [0.0, 374.0]
            assert folded[2][0].tolist() == [0.0, 100.0]
        if name == "truth_empty":
            assert h0[0] == 0 and h0[1] == 1 and h0[2] == 1 and folded[0][0].tolist() == [0.0, 374.0]
        if name == "cap64":
            assert h0[0] == h1[0] == h2[0] == 64 and (np.diff(w0[:, 0]) > 0).all() and (w0[:, 1] == 1).all() and h0[1] == 33 and h0[2] == 1
    pred65, truth65 = cap_case(65)
    assert scipy_region(pred65 != 0, truth65 != 0, DILATION)[0][0] == 65
    out["names"] = np.array(names)
    out["folds"] = np.array(FOLDS, np.float64)
    path = os.path.join(HERE, "lesion.npz")
    write_npz(path, out)
    size = os.path.getsize(path)
    print("wrote %s  (%d arrays, %.1f KB)" % (path, len(out), size / 1024))
    assert size < 256 * 1024


if __name__ == "__main__":
    sys.exit(main())
