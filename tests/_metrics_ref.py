"""numpy-only restatement of the segmentation metrics (nas_3d_unet_amd.metrics; include/n3d.h, "Segmentation metrics"), written
from the definitions and not from the kernels: surfaces by shifted ANDs on a zero-padded array, squared distances by brute
force over point pairs, counts by boolean sums, order statistics by sorting; the floats come from metrics.finish, the same host
function the device path ends in.  tests/test_metrics_ref_host.py holds it to scipy's answers (tests/golden/metrics.npz)."""
import numpy as np

from nas_3d_unet_amd import metrics as M

INF = 1 << 29
REGION_LABELS = ((1, 2, 4), (1, 4), (4,))    # WT, TC, ET


def embed(truth, full, origin):
    """the truth in the image: zero outside its box"""
    out = np.zeros(full, np.uint8)
    o = (0, 0, 0) if origin is None else tuple(int(v) for v in origin)
    out[tuple(slice(a, a + b) for a, b in zip(o, truth.shape))] = truth
    return out


def region_masks(labels):
    return [np.isin(labels, labs) for labs in REGION_LABELS]


def surface(mask):
    """a mask voxel with a 6-neighbour that is unset or outside the image"""
    p = np.pad(mask.astype(bool), 1)
    inner = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return mask.astype(bool) & ~inner


def d2_to(points, sources):
    """for every row of points (n, 3) the squared distance to the nearest row of sources (m, 3), int64; INF without sources"""
    if len(sources) == 0:
        return np.full(len(points), INF, np.int64)
    out = np.empty(len(points), np.int64)
    src = sources.astype(np.int64)
    for a in range(0, len(points), 512):
        p = points[a:a + 512].astype(np.int64)
        out[a:a + 512] = ((p[:, None, :] - src[None, :, :]) ** 2).sum(axis=2).min(axis=1)
    return out


def edt_sq(mask):
    """squared distance from every voxel to the nearest nonzero voxel of mask, int32 (X, Y, Z); INF everywhere for an empty mask"""
    mask = np.asarray(mask) != 0
    pts = np.argwhere(np.ones(mask.shape, bool))
    return d2_to(pts, np.argwhere(mask)).reshape(mask.shape).astype(np.int32)


def order_of(D):
    """(n, D[k], D[min(k + 1, n - 1)], max D), k = floor((n - 1) * 0.95) in fp64, of a SORTED integer array; zeros when empty"""
    n = len(D)
    if n == 0:
        return [0, 0, 0, 0]
    k = int(np.floor(np.float64(n - 1) * np.float64(0.95)))
    return [n, int(D[k]), int(D[min(k + 1, n - 1)]), int(D[-1])]


def interp_t(n):
    vi = np.float64(n - 1) * np.float64(0.95)
    return float(vi - np.floor(vi))


def score(pred, truth, origin=None):
    """-> dict(flags uint8 (FX, FY, FZ), counts int64 (3, 3), order int64 (3, 4), d2 [sorted int64 array per region],
    bbox int64 (3, 6) (lo, hi inclusive of the union of both surfaces; {INT32_MAX x 3, -1 x 3} without surface),
    scores = metrics.finish(counts, voxels, order))"""
    pred = np.asarray(pred)
    t = embed(np.asarray(truth), pred.shape, origin)
    flags = np.zeros(pred.shape, np.uint8)
    counts, order, d2, bbox = [], [], [], []
    for r, (mp, mt) in enumerate(zip(region_masks(pred), region_masks(t))):
        counts.append([int((mp & mt).sum()), int((mp & ~mt).sum()), int((~mp & mt).sum())])
        sp, st = surface(mp), surface(mt)
        flags |= (sp.astype(np.uint8) << r) | (st.astype(np.uint8) << (3 + r))
        pp, pt = np.argwhere(sp), np.argwhere(st)
        D = np.sort(np.concatenate([d2_to(pp, pt), d2_to(pt, pp)]))
        D = D[D < INF]              # one side empty: no distance is defined
        d2.append(D)
        order.append(order_of(D))
        both = np.concatenate([pp, pt])
        bbox.append(both.min(axis=0).tolist() + both.max(axis=0).tolist() if len(both) else [2 ** 31 - 1] * 3 + [-1] * 3)
    counts, order = np.array(counts, np.int64), np.array(order, np.int64)
    return dict(flags=flags, counts=counts, order=order, d2=d2, bbox=np.array(bbox, np.int64),
                scores=M.finish(counts, pred.size, order))


def same_scores(a, b):
    """two metrics.finish results: every integer equal, every float the same bits or both NaN"""
    for r in M.REGIONS:
        for k, v in a[r].items():
            w = b[r][k]
            if isinstance(v, float) and np.isnan(v):
                assert isinstance(w, float) and np.isnan(w), (r, k, v, w)
            else:
                assert type(v) is type(w) and v == w, (r, k, v, w)
    return True
