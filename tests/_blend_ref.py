"""numpy restatement of the importance-weighted stitch (n3d_stitch_add_w / n3d_stitch_finish_w) and the seeded entry lists its tests
share.  The entries are visited in list order; every product and sum is one fp64 numpy operation in the association the header
states: w = (w0 * w1) * w2, S = S + w * p, W = W + w; mean = S / W where W > 0, else 0."""
import numpy as np

from oracle import data_step as ds

IDENT = ([0, 1, 2], [False, False, False])
KEYS = [None] + ds.permutation_keys()
SHAPE = (3, 17, 14, 15)
SIZES = (7, 1, 13, 2, 26)          # 49 entries: every key once


def iso(key):
    return IDENT if key is None else ds.isometry_of_key(key)


def inverse_iso(p, key):
    """the prediction p of an isometry of a patch, back on the patch's own grid"""
    from nas_3d_unet_amd.datastep import inverse_isometry
    return ds.apply_isometry(p, *inverse_isometry(*iso(key)))


def blend(patches, corners, shape, profile):
    """patches: list of (C, P, P, P) on the volume's grid; corners: list of (3,); shape (C, X, Y, Z); profile (P,) float64 ->
    (S float64 (C, X, Y, Z), W float64 (X, Y, Z)): each patch is sliced against the box and added in list order"""
    w = np.asarray(profile, dtype=np.float64)
    P = len(w)
    w3 = (w[:, None, None] * w[None, :, None]) * w[None, None, :]
    S, W = np.zeros(shape, dtype=np.float64), np.zeros(shape[1:], dtype=np.float64)
    for p, c in zip(patches, corners):
        lo = [max(int(c[a]), 0) for a in range(3)]
        hi = [min(int(c[a]) + P, shape[1 + a]) for a in range(3)]
        if any(h <= l for l, h in zip(lo, hi)):
            continue
        vs = tuple(slice(l, h) for l, h in zip(lo, hi))
        ls = tuple(slice(l - int(c[a]), h - int(c[a])) for a, (l, h) in enumerate(zip(lo, hi)))
        S[(slice(None),) + vs] = S[(slice(None),) + vs] + w3[ls] * p[(slice(None),) + ls].astype(np.float64)
        W[vs] = W[vs] + w3[ls]
    return S, W


def mean(S, W):
    return np.divide(S, W[None], out=np.zeros_like(S), where=(W > 0)[None])


def blend_per_voxel(patches, corners, shape, profile):
    """the same, written as the kernel walks it: per voxel, the covering entries in list order"""
    C, X, Y, Z = shape
    P = len(profile)
    S, W = np.zeros(shape, dtype=np.float64), np.zeros((X, Y, Z), dtype=np.float64)
    for x in range(X):
        for y in range(Y):
            for z in range(Z):
                for p, c in zip(patches, corners):
                    l0, l1, l2 = x - int(c[0]), y - int(c[1]), z - int(c[2])
                    if 0 <= l0 < P and 0 <= l1 < P and 0 <= l2 < P:
                        wt = np.float64(profile[l0]) * np.float64(profile[l1])
                        wt = wt * np.float64(profile[l2])
                        W[x, y, z] = W[x, y, z] + wt
                        for ch in range(C):
                            S[ch, x, y, z] = S[ch, x, y, z] + wt * np.float64(p[ch, l0, l1, l2])
    return S, W


def case(P, with_dead=False, seed=41):
    """49 entries on SHAPE: every isometry key once in a shuffled order, corners that hang over the box on either side; with_dead: a
    quarter of the entries dead, entry 7 (the chunk of one entry in SIZES) among them.  patches[e] is what the net gave for the
    patch as it was gathered (None for a dead entry); on_grid[e] is that prediction brought back onto the volume's grid (zeros for
    a dead entry)."""
    rng = np.random.default_rng(seed)
    n = sum(SIZES)
    keys = [KEYS[i] for i in rng.permutation(len(KEYS))]
    corners = [tuple(int(v) for v in rng.integers(-4, 14, 3)) for _ in range(n)]
    dead = (rng.uniform(0, 1, n) < 0.25).tolist()
    dead[7] = True
    if not with_dead:
        dead = [False] * n
    patches = [None if dead[e] else rng.uniform(0, 1, (3, P, P, P)).astype(np.float32) for e in range(n)]
    on_grid = [np.zeros((3, P, P, P), np.float32) if dead[e] else inverse_iso(patches[e], keys[e]) for e in range(n)]
    return dict(P=P, n=n, keys=keys, corners=corners, dead=dead, patches=patches, on_grid=on_grid)
