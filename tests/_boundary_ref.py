"""Reference of loss.BoundaryLoss (include/n3d.h, "Boundary loss") on the CPU.

The transform, in numpy: for a binary map t, d2_fg(v) / d2_bg(v) = the smallest squared Euclidean index distance from v to a voxel with
t = 1 / t = 0 -- exact integers, by separable minima, one axis after the other,

    f0[v] = 0 on a source, INF elsewhere;    f_{a+1}[.., i, ..] = min_j f_a[.., j, ..] + (i - j)^2

(the squared Euclidean distance separates over the axes, and min commutes with the sum) -- and then

    t(v) = 0:  phi = float32(sqrt(float64(d2_fg)))
    t(v) = 1:  phi = float32(-(sqrt(float64(d2_bg)) - 1.0))
    phi = 0 where the wanted distance has no source in the patch (an empty map, a full map).

This is scipy.ndimage.distance_transform_edt under Kervadec's one_hot2dist; tests/test_boundary_ref_host.py holds the statement to
scipy's recorded distances (tests/golden/boundary.npz) with `==`.  `squared_distances_chunked` is the same statement with a bounded
temporary (lines of 1024 voxels), and `squared_distances_from_points` a second one -- the brute-force minimum over a short list of
voxels -- for maps as large as 1024 x 1024 x 1 (`points_case`, `sparse_case`); tests/test_gpu_sdt_extents.py compares the device with
both.

The loss, in fp64: base (tests/_loss_ref.py) + w * mean_bcv (p * phi), and
    d loss / d z = (k2 t + k0 + k_phi phi) p (1 - p) + kb (p - t),   k_phi = w / (B C N)."""
from collections import namedtuple

import numpy as np
import torch

import _loss_ref as lr

INF = 1 << 29      # "no source"; no distance of a patch reaches it

# fixture shapes -> the case of every map, in (b, c) order (`fixture_targets` builds them with `make_case`)
SHAPES = {
    "cube16": ((2, 3, 16, 16, 16), ["empty", "full", "voxel_interior", "two_blobs", "speckle_50", "full_but_one"]),
    "box": ((1, 3, 8, 12, 20), ["nested_wt", "nested_tc", "nested_et"]),
    "long": ((1, 3, 4, 4, 130), ["speckle_02", "voxel_corner", "two_blobs"]),
    "line7": ((1, 1, 1, 1, 7), ["speckle_50"]),
}


SEED = 1618


def fixture_targets(name):
    """the uint8 maps of fixture shape `name`; the nested regions of a shape share one seed"""
    shape, cases = SHAPES[name]
    k = list(SHAPES).index(name)
    assert len(cases) == shape[0] * shape[1]
    return np.stack([make_case(c, shape[2:], SEED + (0 if c.startswith("nested") else 10 * k + i)) for i, c in enumerate(cases)]).reshape(shape)


CORNERS = tuple("corner_%d" % k for k in range(8))
FACES = tuple("face_%d" % a for a in range(3))


def corner(shape, k):
    """voxel index of corner k of `shape`: the far end of axis a where bit a of k is set"""
    return tuple(s - 1 if (k >> a) & 1 else 0 for a, s in enumerate(shape))


def _ball(shape, centre, radius):
    g = np.indices(shape)
    return sum((g[a] - centre[a]) ** 2 for a in range(3)) <= radius * radius


def make_case(name, shape, seed):
    """uint8 map of a named case on `shape` (D0, D1, D2)"""
    rng = np.random.default_rng(seed)
    t = np.zeros(shape, np.uint8)
    mid = tuple(s // 2 for s in shape)
    ext = max(shape)
    if name == "empty":
        pass
    elif name == "full":
        t[:] = 1
    elif name == "voxel_interior":
        t[mid] = 1
    elif name == "voxel_corner":
        t[0, 0, 0] = 1
    elif name == "two_blobs":
        lo = tuple(s // 4 for s in shape)
        hi = tuple(s - 1 - s // 5 for s in shape)
        t[_ball(shape, lo, max(1.5, ext / 8))] = 1
        t[_ball(shape, hi, max(1.0, ext / 11))] = 1
    elif name == "speckle_50":
        t[:] = rng.uniform(0, 1, shape) < 0.5
    elif name == "speckle_02":
        t[:] = rng.uniform(0, 1, shape) < 0.02
    elif name == "full_but_one":
        t[:] = 1
        t[tuple(min(s - 1, s // 3 + 1) for s in shape)] = 0
    elif name in ("nested_wt", "nested_tc", "nested_et"):      # ET inside TC inside WT (one centre, shrinking radii), seed shared
        r = {"nested_wt": 0.42, "nested_tc": 0.3, "nested_et": 0.17}[name] * ext
        g = np.indices(shape)
        t[sum(((g[a] - mid[a]) * (ext / shape[a])) ** 2 for a in range(3)) <= r * r] = 1
    elif name == "speckle_98":
        t[:] = rng.uniform(0, 1, shape) < 0.98
    elif name in CORNERS:                  # one voxel at corner k: bit a of k picks the far end of axis a
        t[corner(shape, int(name[-1]))] = 1
    elif name in FACES:                    # the plane index[a] == 0: distances grow to L - 1 along axis a and every parabola survives
        sel = [slice(None)] * 3
        sel[int(name[-1])] = 0
        t[tuple(sel)] = 1
    elif name == "ramp":                   # a diagonal front: the envelope build pops on almost every step
        g = np.indices(shape)
        t[g[0] + g[1] + g[2] < sum(shape) // 3] = 1
    elif name == "comb":                   # every 7th plane along axis 0
        t[::7] = 1
    else:
        raise ValueError(name)
    return t


def squared_distances(t):
    """(d2_fg, d2_bg) of a binary map of any rank, int64; INF where the map holds no such voxel"""
    t = np.asarray(t) != 0
    out = []
    for src in (t, ~t):
        f = np.where(src, 0, INF).astype(np.int64)
        for axis in range(f.ndim):
            L = f.shape[axis]
            i = np.arange(L)
            d2 = (i[:, None] - i[None, :]) ** 2                  # [i][j]
            g = np.moveaxis(f, axis, -1)
            g = (g[..., None, :] + d2).min(axis=-1)              # [..][i] = min_j f[..][j] + (i - j)^2
            f = np.moveaxis(g, -1, axis)
        out.append(np.where(f >= INF, INF, f))
    return out[0], out[1]


def squared_distances_chunked(t, max_bytes=32 << 20):
    """`squared_distances` with the (rows, L, L) int64 temporary of every axis pass held to max_bytes: the lines of a pass are taken in
    slabs of max_bytes // (8 L^2) along the leading axis of the (lines, L) view.  Same statement, same integers."""
    t = np.asarray(t) != 0
    out = []
    for src in (t, ~t):
        f = np.where(src, 0, INF).astype(np.int64)
        for axis in range(f.ndim):
            L = f.shape[axis]
            rows = max_bytes // (8 * L * L)
            if rows < 1:
                raise ValueError("a line of %d voxels needs a temporary of %d bytes (max_bytes = %d)" % (L, 8 * L * L, max_bytes))
            i = np.arange(L)
            d2 = (i[:, None] - i[None, :]) ** 2                  # [i][j]
            g = np.ascontiguousarray(np.moveaxis(f, axis, -1))
            lines = g.reshape(-1, L)
            for r0 in range(0, lines.shape[0], rows):
                slab = lines[r0:r0 + rows]
                slab[:] = (slab[:, None, :] + d2).min(axis=-1)   # (the right side is complete before the slab is written)
            f = np.moveaxis(g, -1, axis)
        out.append(np.where(f >= INF, INF, f))
    return out[0], out[1]


MAX_POINTS = 64


def squared_distances_from_points(shape, points, max_bytes=32 << 20):
    """int64 array of `shape`: the smallest squared index distance from every voxel to one of `points` (at most MAX_POINTS index
    tuples) -- the brute-force minimum over the list, not separated by axis; INF for an empty list.  Voxels are taken in chunks
    whose (voxels, points) int64 temporary stays under max_bytes."""
    pts = np.asarray(points, np.int64).reshape(-1, len(shape))
    assert len(pts) <= MAX_POINTS and all((0 <= pts[:, a]).all() and (pts[:, a] < s).all() for a, s in enumerate(shape))
    n = int(np.prod(shape))
    out = np.full(n, INF, np.int64)
    if len(pts):
        step = max(1, max_bytes // (8 * len(pts)))
        for v0 in range(0, n, step):
            idx = np.unravel_index(np.arange(v0, min(n, v0 + step)), shape)
            out[v0:v0 + step] = sum((idx[a][:, None] - pts[None, :, a]) ** 2 for a in range(len(shape))).min(axis=1)
    return out.reshape(shape)


def sparse_points(shape, k, seed):
    """k distinct voxels of `shape`, no two of them 6-neighbours (asserted).  Where the shape has room the first three sit as far
    apart as the patch allows -- (0, 0, 0), (1, D1 - 1, D2 - 1), (D0 - 1, 0, 0): neighbouring parabolas with very different offsets,
    the large products of the device's envelope comparison -- and the rest are drawn uniformly."""
    rng = np.random.default_rng(seed)
    pts = []
    cand = [(0, 0, 0), (min(1, shape[0] - 1), shape[1] - 1, shape[2] - 1), (shape[0] - 1, 0, 0)]
    tries = 0
    while len(pts) < k:
        p = cand.pop(0) if cand else tuple(int(rng.integers(0, s)) for s in shape)
        if all(sum(abs(a - b) for a, b in zip(p, q)) >= 2 for q in pts):
            pts.append(p)
        tries += 1
        assert tries < 100 * k + 100, "no room for %d non-adjacent voxels in %s" % (k, (shape,))
    assert len(set(pts)) == k and all(sum(abs(a - b) for a, b in zip(p, q)) >= 2 for n, p in enumerate(pts) for q in pts[:n])
    return pts


def points_case(shape, pts, foreground=True):
    """(t uint8, phi float32) of the map whose foreground (or, with foreground=False, background) is exactly the voxels `pts`, mutually
    non-adjacent (asserted), by the points statement.  The far side is the brute force over the list.  Each listed voxel has a
    6-neighbour inside the patch, of the other kind since no two of the list are adjacent: its own squared distance is 1 and its phi is
    -(1 - 1) as foreground, 1 as background."""
    assert max(shape) > 1 and 1 <= len(pts) <= MAX_POINTS
    assert len(set(pts)) == len(pts) and all(sum(abs(a - b) for a, b in zip(p, q)) >= 2 for n, p in enumerate(pts) for q in pts[:n])
    t = np.zeros(shape, np.uint8)
    t[tuple(np.array(pts).T)] = 1
    far = squared_distances_from_points(shape, pts)
    near = np.where(t != 0, 1, 0).astype(np.int64)          # the few: 1 to a neighbour of the other kind; the many: 0, themselves
    if foreground:
        return t, phi_rule(t, far, near)
    return 1 - t, phi_rule(1 - t, near, far)


def sparse_case(name, shape, k, seed):
    """(t, phi) of `sparse_fg` -- k mutually non-adjacent foreground voxels (sparse_points) -- or of `sparse_bg`, its complement"""
    assert name in ("sparse_fg", "sparse_bg")
    return points_case(shape, sparse_points(shape, k, seed), name == "sparse_fg")


def phi_rule(t, d2_fg, d2_bg):
    """the float32 map from the exact squared distances: one fp64 square root and one rounding per voxel"""
    t = np.asarray(t) != 0
    phi = np.zeros(t.shape, np.float32)
    bg = ~t & (d2_fg < INF)
    fg = t & (d2_bg < INF)
    phi[bg] = np.float32(np.sqrt(d2_fg[bg].astype(np.float64)))
    phi[fg] = np.float32(-(np.sqrt(d2_bg[fg].astype(np.float64)) - 1.0))
    return phi


def signed_distance(t):
    """phi of (B, C, D0, D1, D2) targets (any numeric dtype holding {0, 1}), float32"""
    t = np.asarray(t)
    phi = np.empty(t.shape, np.float32)
    for b in range(t.shape[0]):
        for c in range(t.shape[1]):
            phi[b, c] = phi_rule(t[b, c], *squared_distances(t[b, c]))
    return phi


# ---- the loss
Closed = namedtuple("Closed", "loss base bnd mean_abs kphi dz sums w")


def closed_form(z, t, phi, spec, weight):
    """fp64: loss = base + w mean(p phi) with w = float32(weight) (the device scalar), its parts, mean |p phi| (the scale of the
    boundary part's rounding bound), k_phi, d loss / d z, the per-pair sums (A, P, T, CE, sum p phi) and w"""
    with torch.no_grad():
        c = lr.closed_form(z, t, spec)
        w = float(np.float32(weight))
        z, phi = z.detach().double(), phi.detach().double()
        B, Cc = z.shape[:2]
        n = B * Cc * z[0, 0].numel()
        p = torch.sigmoid(z)
        pf = p * phi
        bnd = w * float(pf.sum()) / n
        kphi = w / n
        dz = c.dz + kphi * phi * p * (1 - p)
        sums = torch.cat([c.sums, pf.sum((-1, -2, -3))[..., None]], dim=-1)
        return Closed(float(c.loss) + bnd, float(c.loss), bnd, float(pf.abs().sum()) / n, kphi, dz, sums, w)


def torch_loss(logits, t, phi, spec, weight):
    """the literal formula on logits, differentiable (phi is a constant)"""
    return lr.torch_loss(logits, t, spec) + float(np.float32(weight)) * (torch.sigmoid(logits) * phi).mean()


def head_reference(x, w, b, gate, t, phi, spec, weight):
    """the fused head with the boundary term in fp64: (Closed of the logits, dx, dw, db); operands as _loss_ref.head_reference"""
    x, w, b, t, phi = x.double(), w.double().reshape(w.shape[0], -1), b.double(), t.double(), phi.double()
    xg = x * gate.double()[:, :, None, None, None] if gate is not None else x
    z = torch.einsum("oc,bcdhw->bodhw", w, xg) + b[None, :, None, None, None]
    c = closed_form(z, t, phi, spec, weight)
    dw = torch.einsum("bodhw,bcdhw->oc", c.dz, xg).reshape(w.shape[0], -1, 1, 1, 1)
    db = c.dz.sum((0, 2, 3, 4))
    dx = torch.einsum("oc,bodhw->bcdhw", w, c.dz)
    if gate is not None:
        dx = dx * gate.double()[:, :, None, None, None]
    return c, dx, dw, db


def tumour_targets(batch, shape, seed, dtype=np.float32):
    """tumour-like (B, 3, D0, D1, D2) targets: nested regions WT > TC > ET of a blob, plus speckle in WT; the last class of sample 0
    is empty"""
    rng = np.random.default_rng(seed)
    t = np.zeros((batch, 3) + tuple(shape), np.uint8)
    ext = max(shape)
    for b in range(batch):
        centre = [rng.uniform(0.3, 0.7) * s for s in shape]
        g = np.indices(shape)
        r2 = sum(((g[a] - centre[a]) * (ext / shape[a])) ** 2 for a in range(3))
        for c, frac in enumerate((0.4, 0.27, 0.15)):
            t[b, c] = r2 <= (frac * ext) ** 2
        t[b, 0] |= rng.uniform(0, 1, shape) < 0.01
    t[0, 2] = 0
    return t.astype(dtype)
