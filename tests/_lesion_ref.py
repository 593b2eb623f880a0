"""numpy-only restatement of the lesion-wise metrics (nas_3d_unet_amd.metrics.score_lesions; include/n3d.h, "Lesion-wise metrics"),
written from the definition and not from the kernels: the dilation as ORs of the shifted copies of the mask (one dilation by the
offsets with max|o| <= d and |ox| + |oy| + |oz| <= 2 d -- 263 of them at d = 3 -- clipped at the image border), components by
propagating the minimum linear index along the 26-neighbour pairs of the foreground voxels to a fixed point, surfaces and squared
distances as tests/_metrics_ref.py has them (shifted ANDs, brute force over point pairs), order statistics by sorting.  The floats
come from metrics.finish_lesions, the same host function the device path ends in.  tests/test_lesion_ref_host.py holds it to
scipy's answers (tests/golden/lesion.npz)."""
import itertools

import numpy as np

import _metrics_ref as MR
from nas_3d_unet_amd import metrics as M

MAX_LESIONS, HEADER_WORDS, ROW_WORDS = 64, 8, 9
REGION_WORDS = HEADER_WORDS + MAX_LESIONS * ROW_WORDS
REC_WORDS = 3 * REGION_WORDS
OVERFLOW_LESIONS = 1


def offsets(d):
    """the offsets d dilations by the 18-neighbourhood reach"""
    return [o for o in itertools.product(range(-d, d + 1), repeat=3) if abs(o[0]) + abs(o[1]) + abs(o[2]) <= 2 * d]


def dilate(mask, d):
    """bool (X, Y, Z): OR of the copies of mask shifted by offsets(d), nothing entering from outside the image"""
    mask = np.asarray(mask) != 0
    p = np.pad(mask, d)
    out = np.zeros(mask.shape, bool)
    X, Y, Z = mask.shape
    for ox, oy, oz in offsets(d):
        out |= p[d - ox:d - ox + X, d - oy:d - oy + Y, d - oz:d - oz + Z]
    return out


def label26(mask):
    """int32 (X, Y, Z): per foreground voxel the smallest linear index of its 26-connected component, -1 on background"""
    mask = np.asarray(mask) != 0
    pts = np.argwhere(mask)                                  # in linear-index order
    lin = np.ravel_multi_index(pts.T, mask.shape) if len(pts) else np.zeros(0, np.int64)
    a_all, b_all = [], []
    for o in itertools.product((-1, 0, 1), repeat=3):
        if o <= (0, 0, 0):
            continue                                         # the forward half: every pair once
        q = pts + np.array(o)
        ok = np.all((q >= 0) & (q < np.array(mask.shape)), axis=1)
        idx = np.flatnonzero(ok)
        qlin = np.ravel_multi_index(q[ok].T, mask.shape)
        pos = np.searchsorted(lin, qlin)
        hit = (pos < len(lin)) & (lin[np.minimum(pos, len(lin) - 1)] == qlin) if len(lin) else np.zeros(0, bool)
        a_all.append(idx[hit])
        b_all.append(pos[hit])
    a, b = (np.concatenate(a_all), np.concatenate(b_all)) if a_all else (np.zeros(0, np.int64),) * 2
    lab = lin.copy()
    while True:
        m = np.minimum(lab[a], lab[b])
        new = lab.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        if np.array_equal(new, lab):
            break
        lab = new
    out = np.full(mask.shape, -1, np.int32)
    out[mask] = lab
    return out


def region(P, G, d):
    """-> (header int64 (8,), rows [[id, gt_voxels, tp, pred_voxels, n_matched, n, D[k], D[k + 1], max D]] by ascending id)"""
    idg, idp = label26(dilate(G, d)), label26(P)
    sp, sg = MR.surface(P), MR.surface(G)
    rows, matched_any = [], set()
    for lid in np.unique(idg[idg >= 0]):
        comp = idg == lid
        Gl = G & comp
        matched = np.unique(idp[comp & P])
        matched_any.update(matched.tolist())
        Pl = np.isin(idp, matched) & P
        a, b = np.argwhere(sp & Pl), np.argwhere(sg & Gl)
        D = np.sort(np.concatenate([MR.d2_to(a, b), MR.d2_to(b, a)])) if len(a) and len(b) else np.zeros(0, np.int64)
        rows.append([int(lid), int(Gl.sum()), int((P & Gl).sum()), int(Pl.sum()), len(matched)] + MR.order_of(D))
    comps, sizes = np.unique(idp[idp >= 0], return_counts=True)
    fp = [int(s) for c, s in zip(comps.tolist(), sizes.tolist()) if c not in matched_any]
    header = np.zeros(HEADER_WORDS, np.int64)
    header[:4] = [len(rows), len(comps), len(fp), sum(fp)]
    return header, rows


def record(pred, truth, origin=None, dilation=3):
    """the int64 record of n3d_lw_score, (REC_WORDS,).  More than MAX_LESIONS lesions in a region: the overflow bit, n_lesions and
    nothing else of that region."""
    pred = np.asarray(pred)
    t = MR.embed(np.asarray(truth), pred.shape, origin)
    rec = np.zeros((3, REGION_WORDS), np.int64)
    for r, (mp, mt) in enumerate(zip(MR.region_masks(pred), MR.region_masks(t))):
        header, rows = region(mp, mt, dilation)
        if len(rows) > MAX_LESIONS:
            rec[r, 0], rec[r, 4] = len(rows), OVERFLOW_LESIONS
            continue
        rec[r, :HEADER_WORDS] = header
        if rows:
            rec[r, HEADER_WORDS:HEADER_WORDS + ROW_WORDS * len(rows)] = np.array(rows, np.int64).ravel()
    return rec.ravel()


def score(pred, truth, origin=None, dilation=3, **fold):
    return M.finish_lesions(record(pred, truth, origin, dilation), **fold)


def folded(scores):
    """float64 (3, 2): [region][lesion-wise Dice, lesion-wise HD95] of a finish_lesions result"""
    return np.array([[scores[r]["lesionwise_dice"], scores[r]["lesionwise_hausdorff95"]] for r in M.REGIONS], np.float64)
