"""GPU: the generator's epoch on the device (nas_3d_unet_amd.generator; n3d_volume_sat, n3d_patch_qualify, n3d_patch_gather).
The summed-area tables equal np.cumsum of the masks exactly; qualification equals the brute-force crop test; the multi-volume gather is
bit-identical to n3d_patch_batch; the Generator reproduces the reference's own Generator (tests/golden/generator.npz) batch for
batch; and a Trainer fed by epoch(out=tr.input_buffers) trains exactly like one fed copies of the same batches."""
import ctypes as C
import json
import random

import numpy as np
import pytest
import torch

import golden_common as gc
import make_golden_generator as mg
from oracle import data_step as ds

pytestmark = pytest.mark.gpu

IDENTITY = ((0, 0), 0, 0, 0, 0)


def _masks(vol, truth):
    m0 = ((vol.view(np.uint32) & 0x7fffffff) != 0).any(axis=0)
    m1 = (truth.reshape(vol.shape[1:]) != 0) if truth is not None else np.zeros(vol.shape[1:], bool)
    return m0, m1


def _expected_table(vol, truth):
    X, Y, Z = vol.shape[1:]
    T = np.zeros((X + 1, Y + 1, Z + 1, 2), np.int64)
    for k, m in enumerate(_masks(vol, truth)):
        T[1:, 1:, 1:, k] = m.astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
    return T


def _special_volumes():
    """zero tests on the fp32 bit pattern: -0.0 is zero; NaN, +inf and a denormal are not; a lone voxel in a corner; all zero"""
    rng = np.random.default_rng(41)
    out = []
    v = (rng.standard_normal((4, 13, 11, 9)) * (rng.uniform(0, 1, (4, 13, 11, 9)) < 0.05)).astype(np.float32)
    v[:, 2, 3, 4] = -0.0
    v[1, 5, 5, 5] = np.nan
    v[2, 6, 1, 0] = np.inf
    v[3, 7, 2, 8] = np.float32(1e-40)
    t = rng.choice(np.array([0] * 30 + [1, 2, 4], np.uint8), (13, 11, 9))
    out.append((v, t))
    lone = np.zeros((4, 6, 9, 131), np.float32)           # z longer than two 64-lane chunks
    lone[3, 5, 8, 130] = -1e-42
    tl = np.zeros((6, 9, 131), np.uint8)
    tl[0, 0, 0] = 4
    out.append((lone, tl))
    out.append((np.zeros((4, 5, 7, 3), np.float32), np.zeros((5, 7, 3), np.uint8)))
    out.append(((np.abs(rng.standard_normal((2, 1, 1, 70))) + 1).astype(np.float32), np.ones((1, 1, 70), np.uint8)))
    return out


def test_summed_area_tables_equal_cumsum():
    from nas_3d_unet_amd.generator import VolumeSet
    vols = _special_volumes()
    for with_truth in (True, False):
        by_c = {}
        for v, t in vols:
            by_c.setdefault(v.shape[0], []).append((v, t))
        for group in by_c.values():
            s = VolumeSet()
            for v, t in group:
                i = s.add(v, t if with_truth else None)
                T = s.table(i).cpu().numpy()
                assert T.dtype == np.int32
                np.testing.assert_array_equal(T.astype(np.int64), _expected_table(v, t if with_truth else None))
    # the volumes are copied contiguous and unchanged (bit for bit, NaN included)
    s = VolumeSet()
    s.add(vols[0][0], vols[0][1])
    assert np.array_equal(s.volumes[0].cpu().numpy().view(np.uint32), vols[0][0].view(np.uint32))


def _sparse_volumes():
    rng = np.random.default_rng(43)
    out = []
    for shape in ((17, 13, 11), (9, 14, 20)):
        v = np.zeros((4,) + shape, np.float32)
        for _ in range(6):
            p = [int(rng.integers(0, n)) for n in shape]
            v[int(rng.integers(0, 4)), p[0], p[1], p[2]] = rng.standard_normal()
        v[:, 0, 0, 0] = -0.0
        t = np.zeros(shape, np.uint8)
        for _ in range(3):
            p = [int(rng.integers(0, n)) for n in shape]
            t[p[0], p[1], p[2]] = rng.choice([1, 2, 4])
        out.append((v, t))
    return out


def _corner_sweep(dim, P):
    """fully outside on both sides, straddling each face, one-voxel intersections, inside"""
    vals = {-P - 1, -P, -P + 1, -P + 2, -1, 0, 1, dim // 2, dim - P - 1, dim - P, dim - P + 1, dim - 2, dim - 1, dim, dim + 1}
    return sorted(vals)


def test_qualify_equals_brute_force_crops():
    from nas_3d_unet_amd.generator import VolumeSet
    vols = _sparse_volumes()
    s = VolumeSet()
    for v, t in vols:
        s.add(v, t)
    rng = np.random.default_rng(44)
    seen = set()
    for P in (1, 2, 5, 12, 25):                                      # 25: larger than every volume on some axis
        ids, corners = [], []
        for vi, (v, _) in enumerate(vols):
            sweep = [_corner_sweep(n, P) for n in v.shape[1:]]
            grid = np.stack(np.meshgrid(*sweep, indexing="ij"), -1).reshape(-1, 3)
            if len(grid) > 700:
                grid = grid[rng.choice(len(grid), 700, replace=False)]
            corners += grid.tolist()
            ids += [vi] * len(grid)
        got = s.qualify(ids, corners, P).cpu().numpy()
        want = np.zeros(len(ids), np.uint8)
        for n, (vi, c) in enumerate(zip(ids, corners)):
            v, t = vols[vi]
            want[n] = int(not np.all(ds.crop_zero_pad(v, c, P) == 0)) | (int(not np.all(ds.crop_zero_pad(t[None], c, P) == 0)) << 1)
        np.testing.assert_array_equal(got, want, err_msg="P=%d" % P)
        seen |= set(want.tolist())
    assert seen == {0, 1, 2, 3}
    # a volume index outside the set gives 0, whatever the corner
    got = s.qualify([-1, 2, 1000, 0], [(0, 0, 0)] * 4, 30).cpu().numpy()
    assert got.tolist() == [0, 0, 0, int(s.qualify([0], [(0, 0, 0)], 30).cpu()[0])] and got[3] == 3
    assert s.qualify([], np.zeros((0, 3)), 4).numel() == 0


def _gather_refs(vols, rng, keys):
    return [(int(rng.integers(0, len(vols))), tuple(int(c) for c in rng.integers(-6, 20, 3)), k) for k in keys]


def test_gather_is_bit_identical_to_patch_batch():
    from nas_3d_unet_amd import datastep as hd, kernels as K
    from nas_3d_unet_amd.generator import VolumeSet
    rng = np.random.default_rng(45)
    vols = [(rng.standard_normal((4,) + sh).astype(np.float32), rng.choice(np.array([0, 0, 1, 2, 4], np.uint8), sh))
            for sh in ((20, 17, 23), (15, 22, 18), (24, 19, 16))]
    s = VolumeSet()
    dev = [(torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()) for v, t in vols]
    for v, t in vols:
        s.add(v, t)
    keys = gc.permutation_keys() + [None] * 4
    refs = _gather_refs(vols, rng, keys)
    P = 10
    for lo in range(0, len(refs), 13):
        batch = refs[lo:lo + 13]
        assert len({r[0] for r in batch}) > 1
        for incl in (True, False):
            for tdt in (torch.float32, torch.uint8):
                x, t = s.patch_batch(batch, P, inclusive_label=incl, target_dtype=tdt)
                assert K._pitch_of(x) == 4 and t.dtype == tdt
                parts = [hd.patch_batch(dev[v][0], dev[v][1], [c], [k], P, inclusive_label=incl, target_dtype=tdt) for v, c, k in batch]
                assert torch.equal(x, torch.cat([p[0] for p in parts])) and torch.equal(t, torch.cat([p[1] for p in parts]))
                # out=: pitched x (a 4-channel slice of an 8-channel NDHWC buffer), t's dtype decides
                B = len(batch)
                wide = torch.full((B, P, P, P, 8), 7.0, device="cuda").permute(0, 4, 1, 2, 3)
                ox, ot = wide[:, :4], torch.full((B, 3, P, P, P), 5, dtype=tdt, device="cuda")
                rx, rt = s.patch_batch(batch, P, inclusive_label=incl, target_dtype=torch.float32, out=(ox, ot))
                assert rx is ox and rt is ot and K._pitch_of(ox) == 8
                assert torch.equal(ox, x) and torch.equal(ot, t) and bool((wide[:, 4:] == 7.0).all())


def test_gather_errors():
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd._lib import GatherDesc, N3DError, PatchDesc
    from nas_3d_unet_amd.generator import VolumeSet
    s = VolumeSet()
    s.add(np.ones((4, 8, 8, 8), np.float32), np.zeros((8, 8, 8), np.uint8))
    s.add(np.ones((4, 9, 8, 7), np.float32), np.zeros((9, 8, 7), np.uint8))
    with pytest.raises(N3DError):
        s.patch_batch([(2, (0, 0, 0), None)], 4)                      # volume index out of range
    with pytest.raises(N3DError):
        s.patch_batch([(-1, (0, 0, 0), None)], 4)
    with pytest.raises(N3DError):
        s.patch_batch([(0, (0, 0, 0), None)] * 65, 4)                 # more than 64 descriptors
    with pytest.raises(N3DError):
        s.patch_batch([(0, (0, 0, 0), None)], 4, out=(torch.zeros(1, 4, 4, 4, 4), torch.zeros(1, 3, 4, 4, 4)))   # CPU tensors
    with pytest.raises(N3DError):
        s.patch_batch([(0, (0, 0, 0), None)], 4, out=(torch.zeros(1, 4, 4, 4, 4, device="cuda"), torch.zeros(1, 3, 4, 4, 4, device="cuda")))  # NCDHW x
    # a bad perm straight through the C ABI
    x = K.empty_ndhwc(1, 4, 4, 4, 4, s.device, torch.float32)
    d = (GatherDesc * 1)(GatherDesc(PatchDesc((C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(0, 0, 1), (C.c_int32 * 3)(0, 0, 0)), 0))
    rc = _lib.load().n3d_patch_gather(K.ptr(s.records), len(s), 4, d, 1, 4, 0, K.ptr(x), 4, None, K.stream_ptr())
    assert rc == -1 and b"perm" in _lib.load().n3d_last_error()
    with pytest.raises(N3DError):
        s.add(np.ones((3, 8, 8, 8), np.float32), np.zeros((8, 8, 8), np.uint8))     # another channel count
    with pytest.raises(N3DError):
        s.add(np.ones((4, 8, 8, 8), np.float32))                                    # truth for all or none


def _oracle_batch(volumes, rows, P, inclusive, with_truth):
    xs, ys = [], []
    for r in rows:
        v, corner, k = int(r[1]), [int(c) for c in r[2:5]], [int(c) for c in r[5:]]
        key = IDENTITY if k[0] < 0 else ((k[0], k[1]), k[2], k[3], k[4], k[5])
        vol, truth = volumes[v]
        x, y = ds.data_step(vol, truth if with_truth else np.zeros_like(truth), [corner], [key], P, inclusive)
        xs.append(x)
        ys.append(y)
    return np.concatenate(xs), np.concatenate(ys)


def test_generator_reproduces_the_reference_generator(golden):
    from nas_3d_unet_amd.generator import Generator, VolumeSet
    g = golden("generator")
    volumes = mg.generator_volumes()
    sets = {}
    for with_truth in (True, False):
        sets[with_truth] = VolumeSet()
        for v, t in volumes:
            sets[with_truth].add(v, t if with_truth else None)
    for ci in range(len(mg.generator_cases())):
        k = "case%d" % ci
        cfg = json.loads(str(g[k + "/config"]))
        kw, wt = cfg["kwargs"], cfg["truth"]
        P, B = kw["patch_shape"], kw["batch_size"]
        overlaps = [None if o < 0 else int(o) for o in g[k + "/overlap"]]
        gen = Generator(volumes=sets[wt], labels=[1, 2, 4], rng=random.Random(cfg["seed"]), **kw)
        for e in range(cfg["epochs"]):
            assert gen.overlap == overlaps[e] and gen.steps_per_epoch == int(g[k + "/spe"][e]), (cfg["name"], e)
            rows = g[k + "/epoch%d/rows" % e]
            n = 0
            for b, (x, t) in enumerate(gen.epoch()):
                br = rows[rows[:, 0] == b]
                assert len(br) >= 1 and x.shape[0] == len(br) and (t is None) == (not wt)
                xr, yr = _oracle_batch(volumes, br, P, kw.get("inclusive_label", False), wt)
                assert np.array_equal(x.cpu().numpy(), xr), (cfg["name"], e, b)
                if wt:
                    assert np.array_equal(t.cpu().numpy(), yr), (cfg["name"], e, b)
                if e == 0 and b == 0 and (k + "/epoch0/batch0/x") in g:
                    assert np.array_equal(x.cpu().numpy(), g[k + "/epoch0/batch0/x"])
                    if wt:
                        assert np.array_equal(t.cpu().numpy(), g[k + "/epoch0/batch0/y"].astype(np.float32))
                n += 1
            assert n == int(g[k + "/spe"][e]) and int(rows[:, 0].max()) == n - 1, (cfg["name"], e)
            assert gen.overlap == overlaps[e + 1], (cfg["name"], e)       # redrawn (or kept) after the epoch


def _train_volumes():
    """three brain boxes of 40-48 voxels per axis, a tumour towards one corner: 27 autofit candidates of 32^3, 8 of them healthy"""
    out = []
    for i, shape in enumerate([(44, 40, 48), (40, 46, 42), (48, 42, 40)]):
        rng = np.random.default_rng(10 + i)
        g = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
        c = [n / 2 for n in shape]
        brain = sum(((g[a] - c[a]) / (0.42 * shape[a])) ** 2 for a in range(3)) <= 1.0
        vol = np.where(brain[None], rng.standard_normal((4,) + shape), 0).astype(np.float32)
        tc = [0.78 * n + rng.uniform(-2, 2) for n in shape]
        d = np.sqrt(sum((g[a] - tc[a]) ** 2 for a in range(3)))
        truth = np.where(brain, np.select([d <= 2, d <= 4, d <= 6], [4, 1, 2], 0), 0).astype(np.uint8)[None]
        out.append((vol, truth))
    return out


def test_trainer_fed_by_the_generator_trains_like_one_fed_copies():
    """the searched configuration test_gpu_train.py trains (net_cases()' first searched entry, 32^3, B = 2): a Trainer fed by
    epoch(out=tr.input_buffers) -- the batches written straight into its captured buffers, the smaller last batch into fresh tensors
    (that step runs eagerly) -- takes the same steps bit for bit as a second Trainer fed copies of the same batches"""
    from nas_3d_unet_amd.generator import Generator, VolumeSet
    from nas_3d_unet_amd.train import Trainer
    from test_gpu_nets import build_net
    key, kind, gname, depth, size, batch, adam = [c for c in gc.net_cases() if c[1] == "searched"][0]
    assert (size, batch) == (32, 2)
    s = VolumeSet()
    for v, t in _train_volumes():
        s.add(v, t)
    gen = Generator([0, 1, 2], s, size, batch_size=batch, labels=[1, 2, 4], permute=True, rng=random.Random(1))
    assert gen.n_patches % batch == 1 and gen.n_patches < 27          # ends in a remainder batch; healthy patches dropped
    tr = Trainer(build_net(kind, gname, depth)[0], graph=True)
    losses, copies, in_place = [], [], 0
    for x, t in gen.epoch(out=tr.input_buffers):
        bufs = tr.input_buffers()
        if bufs[0] is not None and x.shape[0] == batch:
            assert x is bufs[0] and t is bufs[1]
            in_place += 1
        copies.append((x.clone(), t.clone()))
        losses.append(float(tr.step(x, t)))
    assert len(losses) == gen.steps_per_epoch and copies[-1][0].shape[0] == 1 and in_place == len(losses) - 2
    tr2 = Trainer(build_net(kind, gname, depth)[0], graph=True)
    losses2 = [float(tr2.step(x, t)) for x, t in copies]
    assert losses == losses2, (losses, losses2)
    assert torch.equal(tr.fp.flat, tr2.fp.flat)
    # a validation epoch through evaluate(): every kept patch is counted once
    val = Generator([0, 1, 2], s, size, batch_size=batch, labels=[1, 2, 4], rng=random.Random(2))
    for x, t in val.epoch():
        tr.evaluate(x, t)
    res = tr.eval_result()
    assert res.n_samples == val.n_patches and res.n_batches == val.steps_per_epoch


def test_drawn_overlap_equal_to_the_patch_raises():
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.generator import Generator, VolumeSet

    class TopDraw:
        def randint(self, a, b):
            return b

    s = VolumeSet()
    s.add(np.ones((4, 20, 20, 20), np.float32), np.ones((20, 20, 20), np.uint8))
    with pytest.raises(N3DError, match="divides by zero"):
        Generator([0], s, 8, patch_overlap=8, rng=TopDraw())
    gen = Generator([0], s, 8, patch_overlap=7, rng=TopDraw())
    assert gen.overlap == 7 and gen.steps_per_epoch == gen.n_patches == len(gen.candidates)
