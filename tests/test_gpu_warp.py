"""GPU: rotation, linear interpolation and the intensity map in the patch gather (n3d_patch_gather_warp; nas_3d_unet_amd.generator
with augment_rotation / augment_interpolation / augment_intensity_scale / augment_intensity_shift).  With descriptors that change
nothing the new entry is n3d_patch_gather bit for bit, and n3d_patch_gather_aug on the transforms of tests/golden/augment.npz; on the
cases of tests/golden/warp.npz it gives scipy's recorded answers (== at order 0 and for the labels, one float32 step at order 1);
everywhere else it equals, with ==, the numpy statement of the rule (tests/_warp_ref.py) that the CPU tests tie to that fixture."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import _augment_ref as ar
import _warp_ref as wr
import golden_common as gc
import make_golden_augment as mga
import make_golden_generator as mg
import make_golden_warp as mgw
from oracle import data_step as ds
from test_gpu_augment import IDENTITY, PLAIN, _face_refs, _fixture_augs, _random_vols

pytestmark = pytest.mark.gpu

NOOP = (None, 0, None, None)          # a warp entry that changes nothing
SHAPES = ((20, 17, 23), (15, 22, 18), (24, 19, 16))


def _coefficients(aug, warp):
    """(mode, k, order, flips, gain, bias) of one patch as VolumeSet.patch_batch composes them"""
    A, sh, identity, axes = aug if aug is not None else PLAIN
    matrix, order, gain, bias = warp if warp is not None else NOOP
    flips = [a in (axes or []) for a in range(3)]
    if matrix is not None:
        return 1, wr.coefficients(1, matrix[0], matrix[1]), order, flips, gain, bias
    if identity:
        return 0, wr.coefficients(0, np.ones(3), np.zeros(3)), order, flips, gain, bias
    return 0, wr.coefficients(0, A, sh), order, flips, gain, bias


def _expected(vols, refs, augs, warps, P, inclusive):
    """the batch by the rule: crop with zero padding -> flip + resample + intensity (the helper) -> isometry -> labels"""
    xs, ys = [], []
    for (v, corner, key), aug, warp in zip(refs, augs, warps):
        vol, truth = vols[v]
        x = ds.crop_zero_pad(vol, corner, P)
        y = ds.crop_zero_pad(truth.reshape((1,) + vol.shape[1:]), corner, P) if truth is not None else np.zeros((1, P, P, P), np.uint8)
        mode, k, order, flips, gain, bias = _coefficients(aug, warp)
        x, y = wr.warp_patch(x, mode, k, order, flips, gain, bias), wr.warp_patch(y, mode, k, 0, flips)
        perm, flip = ds.isometry_of_key(IDENTITY if key is None else key)
        xs.append(ds.apply_isometry(x, perm, flip))
        ys.append(ds.apply_isometry(y, perm, flip))
    return np.asarray(xs, np.float32), ds.expand_labels(np.asarray(ys), inclusive)


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _set_of(vols, truth=True):
    from nas_3d_unet_amd.generator import VolumeSet
    s = VolumeSet()
    for v, t in vols:
        s.add(v, t if truth else None)
    return s


def _mixed_entries(P, B, augs, scale_maps):
    """per patch an augmentation entry (a fixture transform with its flips, or None) and a warp entry: the kinds cycle through
    None, a matrix with either order, the zoom-shift rule with either order, each with and without gain / bias"""
    from nas_3d_unet_amd import generator as G
    rs = np.random.RandomState(100 + P)
    batch_augs, warps = [], []
    for n in range(B):
        aug = None if n % 5 == 4 else augs[(n + P) % len(augs)]
        A, b = scale_maps[(n + P) % len(scale_maps)] if n % 3 else (np.ones(3), np.zeros(3))
        matrix = G.warp_transform(A, b, G.rotation_matrix(rs.uniform(-15, 15, 3)), P)
        gain, bias = rs.uniform(0.9, 1.1, 4), rs.normal(0, 0.1, 4)
        kind = n % 7
        warp = [None, (matrix, 0, None, None), (matrix, 1, gain, bias), (None, 1, gain, None), (None, 0, None, bias),
                (matrix, 1, None, None), (None, 1, None, None)][kind]
        batch_augs.append(aug)
        warps.append(warp)
    return batch_augs, warps


def test_noop_descriptors_equal_patch_gather_and_mode0_equals_patch_gather_aug(golden):
    from nas_3d_unet_amd import kernels as K
    vols = _random_vols(71, SHAPES, 4)
    s = _set_of(vols)
    rng = np.random.default_rng(72)
    keys = gc.permutation_keys()[::4] + [None]
    P = 9
    refs = _face_refs(vols, P, keys, rng)
    B = len(refs)
    assert B == 13 and len({r[0] for r in refs}) == 3
    for incl in (True, False):
        for tdt in (torch.float32, torch.uint8):
            x0, t0 = s.patch_batch(refs, P, inclusive_label=incl, target_dtype=tdt)
            for aug in (None, [PLAIN] * B, [None] * B):
                x1, t1 = s.patch_batch(refs, P, inclusive_label=incl, target_dtype=tdt, augment=aug, warp=[NOOP] * B)
                assert K._pitch_of(x1) == 4 and t1.dtype == tdt
                assert torch.equal(x0, x1) and torch.equal(t0, t1)
            assert bool(x0.any()) and bool(t0.any())
    # a list of None entries is not a warped batch: the launches are today's
    x2, t2 = s.patch_batch(refs, P, warp=[None] * B)
    x0, t0 = s.patch_batch(refs, P)
    assert torch.equal(x0, x2) and torch.equal(t0, t2)
    # mode 0, order 0, no intensity: n3d_patch_gather_aug bit for bit on the transforms (and flips) of augment.npz
    augs = _fixture_augs(golden("augment"))
    assert len(augs) > 16
    for lo in range(0, len(augs), 13):
        part = augs[lo:lo + 13]
        part = part + augs[:13 - len(part)]
        for incl, tdt in ((True, torch.float32), (False, torch.uint8)):
            xa, ta = s.patch_batch(refs, P, inclusive_label=incl, target_dtype=tdt, augment=part)
            xw, tw = s.patch_batch(refs, P, inclusive_label=incl, target_dtype=tdt, augment=part, warp=[NOOP] * 12 + [None])
            assert torch.equal(xa, xw) and torch.equal(ta, tw)
        assert not torch.equal(xa, s.patch_batch(refs, P, target_dtype=torch.uint8)[0])


def test_fixture_cases_at_corner_zero_equal_scipy(golden):
    """warp.npz's inputs as P^3 volumes at corner 0: the device output is scipy's recorded answer -- == at order 0 (channel 0 numbers
    the voxels, so this is the source voxel of every output voxel, the adversarial coordinates included) and for the labels, one
    float32 step at order 1 with at most 1 voxel in 1000 differing.  Cv = 2: the scalar store path, on the tensor's own pitch and on
    a pitch of 5 with the neighbours untouched"""
    from nas_3d_unet_amd import kernels as K
    recs = wr.records(golden("warp"))
    differ = total = 0
    for P in (8, 10):
        data, truth = mgw.warp_inputs(P)
        s = _set_of([(data, truth)])
        mine = [r for r in recs if r[0]["P"] == P]
        assert len(mine) >= 16
        for lo in range(0, len(mine), 15):
            part = mine[lo:lo + 15]
            B = len(part) + 1                                          # the last patch is left as it is
            refs = [(0, (0, 0, 0), None)] * B
            augs = [None if c["mode"] else (k[:3], k[3:6], False, None) for c, k, *_ in part] + [None]
            for order in (0, 1):
                warps = [((k[:9].reshape(3, 3), k[9:12]) if c["mode"] else None, order, None, None) for c, k, *_ in part] + [None]
                for incl, tdt in ((True, torch.float32), (False, torch.uint8)):
                    x, t = s.patch_batch(refs, P, inclusive_label=incl, target_dtype=tdt, augment=augs, warp=warps)
                    xn, tn = x.cpu().numpy(), t.cpu().numpy()
                    assert np.array_equal(xn[-1], data) and np.array_equal(tn[-1], ds.expand_labels(truth[None], incl)[0].astype(tn.dtype))
                    for n, (c, k, x0, x1, y) in enumerate(part):
                        assert np.array_equal(tn[n], ds.expand_labels(y[None], incl)[0].astype(tn.dtype)), c["name"]
                        if order == 0:
                            assert np.array_equal(xn[n], x0), c["name"]
                        else:
                            assert wr.one_step(xn[n], x1).all(), c["name"]
                            assert np.array_equal(_bits32(xn[n]), _bits32(wr.warp_patch(data, c["mode"], k, 1))), c["name"]
                            if tdt == torch.uint8:
                                differ += int((xn[n] != x1).sum())
                                total += x1.size
                # pitch 5 (a 2-channel slice of a 5-channel NDHWC buffer): the neighbours stay untouched
                wide = torch.full((B, P, P, P, 5), 7.0, device="cuda").permute(0, 4, 1, 2, 3)
                ox, ot = wide[:, :2], torch.full((B, 3, P, P, P), 5, dtype=torch.uint8, device="cuda")
                rx, rt = s.patch_batch(refs, P, out=(ox, ot), augment=augs, warp=warps)
                assert rx is ox and rt is ot and K._pitch_of(ox) == 5
                assert torch.equal(ox, x) and torch.equal(ot, t) and bool((wide[:, 2:] == 7.0).all())
    assert total > 40000 and differ * 1000 <= total


def test_mixed_batches_equal_the_helper(golden):
    """Cv = 4 on the aligned pitch (the float4 store), patches of three volumes hanging over every face, every isometry class,
    flips, both coordinate rules and both orders, entries with and without gain / bias and None entries in one batch, at P = 8, 9
    (not a multiple of the wave) and 12 (several workgroups per patch); fp32 and byte targets, inclusive_label on and off; a set
    without truth.  The volumes have a background of zeros: it stays exactly 0 under a bias"""
    from nas_3d_unet_amd import kernels as K
    g = golden("augment")
    augs = _fixture_augs(g)
    scale_maps = [(A, b) for _, _, _, A, b, identity, _, _ in ar.operator_records(g) if not identity]
    vols = []
    for v, t in _random_vols(73, SHAPES, 4):
        X, Y, Z = v.shape[1:]
        gx, gy, gz = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
        outside = ((gx - X / 2) / (0.6 * X)) ** 2 + ((gy - Y / 2) / (0.6 * Y)) ** 2 + ((gz - Z / 2) / (0.6 * Z)) ** 2 > 1
        v[:, outside] = 0
        vols.append((v, t))
    s, bare = _set_of(vols), _set_of(vols, truth=False)
    rng = np.random.default_rng(74)
    for P in (8, 9, 12):
        keys = (gc.permutation_keys()[(P % 4)::4] + [None] * 3)[:15]
        refs = _face_refs(vols, P, keys, rng)
        B = len(refs)
        batch_augs, warps = _mixed_entries(P, B, augs, scale_maps)
        assert any(w is None for w in warps) and any(a is None for a in batch_augs) and any(a is not None and a[3] for a in batch_augs)
        assert {(w[0] is not None, w[1], w[2] is not None) for w in warps if w is not None} >= {
            (True, 0, False), (True, 1, True), (False, 1, True), (False, 0, False), (True, 1, False), (False, 1, False)}
        want = {incl: _expected(vols, refs, batch_augs, warps, P, incl) for incl in (True, False)}
        plain = _expected(vols, refs, batch_augs, [None] * B, P, True)[0]
        assert sum(not np.array_equal(want[True][0][n], plain[n]) for n in range(B)) >= B // 2
        for incl in (True, False):
            for tdt in (torch.float32, torch.uint8):
                x, t = s.patch_batch(refs, P, inclusive_label=incl, target_dtype=tdt, augment=batch_augs, warp=warps)
                assert K._pitch_of(x) == 4 and x.data_ptr() % 16 == 0 and t.dtype == tdt
                assert np.array_equal(_bits32(x.cpu().numpy()), _bits32(want[incl][0]))
                assert np.array_equal(t.cpu().numpy(), want[incl][1].astype(t.cpu().numpy().dtype))
        x, t = bare.patch_batch(refs, P, augment=batch_augs, warp=warps)
        assert t is None and np.array_equal(_bits32(x.cpu().numpy()), _bits32(want[True][0]))
        # the background: where the rule without an intensity map gives 0 the biased batch is 0 too, and nowhere else
        no_map = [None if w is None else (w[0], w[1], None, None) for w in warps]
        x0 = s.patch_batch(refs, P, augment=batch_augs, warp=no_map)[0]
        biased = [n for n, w in enumerate(warps) if w is not None and w[3] is not None]
        assert biased and bool(torch.equal(x[biased] == 0, x0[biased] == 0)) and not torch.equal(x[biased], x0[biased])
        assert 0.05 < float((x0[biased] == 0).float().mean()) < 0.95


def test_a_full_descriptor_table_its_cap_and_the_validation_messages(golden):
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd._lib import GatherDesc, N3DError, PatchDesc, WarpDesc
    from nas_3d_unet_amd.generator import WARP_MAX_BATCH, VolumeSet
    g = golden("augment")
    augs = _fixture_augs(g)
    scale_maps = [(A, b) for _, _, _, A, b, identity, _, _ in ar.operator_records(g) if not identity]
    vols = _random_vols(75, ((14, 12, 13), (11, 15, 12)), 4)
    s = _set_of(vols)
    rng = np.random.default_rng(76)
    P, B = 8, 16
    assert B == WARP_MAX_BATCH
    keys = [gc.permutation_keys()[int(k)] for k in rng.integers(0, 48, B)]
    refs = [(int(rng.integers(0, 2)), tuple(int(c) for c in rng.integers(-4, 9, 3)), k) for k in keys]
    batch_augs, warps = _mixed_entries(P, B, augs, scale_maps)
    x, t = s.patch_batch(refs, P, target_dtype=torch.uint8, augment=batch_augs, warp=warps)
    wx, wy = _expected(vols, refs, batch_augs, warps, P, False)
    assert np.array_equal(_bits32(x.cpu().numpy()), _bits32(wx)) and np.array_equal(t.cpu().numpy(), wy.astype(np.uint8))
    with pytest.raises(N3DError, match="N3D_PATCH_WARP_MAX_BATCH"):
        s.patch_batch(refs + refs[:1], P, augment=batch_augs + batch_augs[:1], warp=warps + [NOOP])
    s.patch_batch(refs + refs[:1], P, augment=batch_augs + batch_augs[:1])       # 17 patches without a warp: n3d_patch_gather_aug, as before
    # intensity on a set with more than 4 channels: refused in Python and by the entry point
    wide = VolumeSet()
    wide.add(np.ones((5, 9, 9, 9), np.float32))
    with pytest.raises(N3DError, match="at most 4 channels"):
        wide.patch_batch([(0, (0, 0, 0), None)], P, warp=[(None, 1, np.ones(5), None)])
    assert wide.patch_batch([(0, (0, 0, 0), None)], P, warp=[(None, 1, None, None)])[0].shape == (1, 5, P, P, P)
    # straight through the C ABI
    lib = _lib.load()
    xo = K.empty_ndhwc(17, 4, P, P, P, s.device, torch.float32)
    x5 = K.empty_ndhwc(1, 5, P, P, P, s.device, torch.float32)
    nan, inf = float("nan"), float("inf")

    def call(descs, n, recs=s, Cv=4, out=xo):
        return lib.n3d_patch_gather_warp(K.ptr(recs.records), len(recs), Cv, descs, n, P, 0, K.ptr(out), Cv, None, K.stream_ptr())

    def desc(perm=(0, 1, 2), vol=0, mode=0, order=0, intensity=0, k=(1.0,) * 3 + (0.0,) * 9, gain=(1.0,) * 4, bias=(0.0,) * 4):
        gd = GatherDesc(PatchDesc((C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*perm), (C.c_int32 * 3)(0, 0, 0)), vol)
        return WarpDesc(gd, (C.c_int32 * 3)(0, 0, 0), mode, order, intensity, (C.c_double * 12)(*k), (C.c_float * 4)(*gain),
                        (C.c_float * 4)(*bias))

    def k_with(i, v, base=(1.0,) * 3 + (0.0,) * 9):
        k = list(base)
        k[i] = v
        return tuple(k)

    assert call((WarpDesc * 17)(*[desc()] * 17), 17) == -1 and b"N3D_PATCH_WARP_MAX_BATCH" in lib.n3d_last_error()
    assert call((WarpDesc * 16)(*[desc()] * 16), 16) == 0
    assert call((WarpDesc * 1)(desc(mode=1, order=1, intensity=1, k=(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0))), 1) == 0
    assert call((WarpDesc * 1)(desc(mode=1, k=(0.0,) * 12)), 1) == 0             # a zero matrix is legal in mode 1: every voxel reads c = off
    assert call((WarpDesc * 1)(desc(order=1)), 1, wide, 5, x5) == 0
    for bad, word in ((desc(perm=(0, 0, 1)), b"perm"), (desc(perm=(0, 1, 3)), b"perm"), (desc(vol=2), b"volume"), (desc(vol=-1), b"volume"),
                      (desc(mode=2), b"mode"), (desc(mode=-1), b"mode"), (desc(order=2), b"order"), (desc(order=-1), b"order"),
                      (desc(k=k_with(1, 0.0)), b"nonzero"), (desc(k=k_with(0, nan)), b"finite"), (desc(k=k_with(4, inf)), b"finite"),
                      (desc(k=k_with(11, nan)), b"finite"), (desc(mode=1, k=k_with(7, -inf)), b"finite"),
                      (desc(gain=(1.0, nan, 1.0, 1.0)), b"gain and bias"), (desc(intensity=1, bias=(0.0, 0.0, 0.0, inf)), b"gain and bias")):
        assert call((WarpDesc * 1)(bad), 1) == -1 and word in lib.n3d_last_error(), lib.n3d_last_error()
    assert call((WarpDesc * 1)(desc(intensity=1)), 1, wide, 5, x5) == -1 and b"at most 4 channels" in lib.n3d_last_error()
    torch.cuda.synchronize()


def _generator_batches(G, s, seeds, kw):
    gen = G.Generator(volumes=s, labels=[1, 2, 4], rng=random.Random(seeds[0]), np_rng=np.random.RandomState(seeds[1]), **kw)
    out = []
    for e in range(2):
        flags, cand = gen.flags.copy(), gen.candidates.copy()
        out.append((flags, cand, [(x.cpu().numpy(), t.cpu().numpy()) for x, t in gen.epoch()]))
    return out


def test_generator_with_every_option_equals_the_helper_on_a_twin_order_and_is_deterministic():
    from nas_3d_unet_amd import generator as G
    volumes = mg.generator_volumes()
    s = _set_of([(v, t) for v, t in volumes])
    vols = [(v, t[0]) for v, t in volumes]
    Cv = volumes[0][0].shape[0]
    P = 8
    kw = dict(indices_list=[3, 0, 1], patch_shape=P, patch_overlap=3, batch_size=3, permute=True, augment=True, affine=mga.BRATS_AFFINE,
              augment_rotation=15, augment_interpolation="linear", augment_intensity_scale=0.1, augment_intensity_shift=0.1)
    runs = [_generator_batches(G, s, (41, 141), kw) for _ in range(2)]
    rng, twin = random.Random(41), np.random.RandomState(141)
    affine = G.check_affine(mga.BRATS_AFFINE)
    seen = 0
    for e, (flags, cand, batches) in enumerate(runs[0]):
        assert G.draw_overlap(3, rng) is not None
        order = list(G.epoch_order(flags, 3, rng, True, True, True, augment=(twin, 0.25, True), warp=(twin, 15, 0.1, 0.1, Cv)))
        assert len(order) == len(batches) >= 2
        for batch, (x, t) in zip(order, batches):
            refs = [(int(cand[i, 0]), tuple(int(c) for c in cand[i, 1:]), key) for i, key, _, _ in batch]
            augs, warps = [], []
            for _, _, (scale, axes), (angles, gain, bias) in batch:
                A, b, identity = G.resample_transform(affine, P, scale)
                augs.append((A, b / A, identity, axes))
                warps.append((wr.warp_transform(A, b, wr.rotation_matrix(angles), P), 1, gain, bias))
            wx, wy = _expected(vols, refs, augs, warps, P, False)
            assert np.array_equal(_bits32(x), _bits32(wx)) and np.array_equal(t, wy.astype(np.float32)), (e, refs)
            assert bool((x != np.round(x)).any())
            seen += len(batch)
    assert seen >= 8
    for (_, _, a), (_, _, b) in zip(*runs):
        assert len(a) == len(b) and all(np.array_equal(_bits32(xa), _bits32(xb)) and np.array_equal(ta, tb) for (xa, ta), (xb, tb) in zip(a, b))


def test_trainer_fed_by_the_warping_generator_trains_like_one_fed_copies():
    """test_gpu_augment's trainer test with the new options: the batches written by n3d_patch_gather_warp straight into the captured
    input buffers train bit for bit like copies of the same batches"""
    from nas_3d_unet_amd.generator import Generator, VolumeSet
    from nas_3d_unet_amd.train import Trainer
    from test_gpu_generator import _train_volumes
    from test_gpu_nets import build_net
    key, kind, gname, depth, size, batch, adam = [c for c in gc.net_cases() if c[1] == "searched"][0]
    assert (size, batch) == (32, 2)
    s = VolumeSet()
    for v, t in _train_volumes():
        s.add(v, t)
    gen = Generator([0, 1, 2], s, size, batch_size=batch, labels=[1, 2, 4], permute=True, rng=random.Random(1), augment=True,
                    affine=mga.BRATS_AFFINE, np_rng=np.random.RandomState(5), augment_rotation=15, augment_interpolation="linear",
                    augment_intensity_scale=0.1, augment_intensity_shift=0.1)
    plain = Generator([0, 1, 2], s, size, batch_size=batch, labels=[1, 2, 4], permute=True, rng=random.Random(1))
    assert gen.n_patches == plain.n_patches and gen.n_patches % batch == 1
    tr = Trainer(build_net(kind, gname, depth)[0], graph=True)
    losses, copies, in_place = [], [], 0
    for (x, t), (px, pt) in zip(gen.epoch(out=tr.input_buffers), plain.epoch()):
        bufs = tr.input_buffers()
        if bufs[0] is not None and x.shape[0] == batch:
            assert x is bufs[0] and t is bufs[1]
            in_place += 1
        assert x.shape == px.shape and not torch.equal(x, px)          # the same candidates and keys, warped
        copies.append((x.clone(), t.clone()))
        losses.append(float(tr.step(x, t)))
    assert len(losses) == gen.steps_per_epoch and copies[-1][0].shape[0] == 1 and in_place == len(losses) - 2
    tr2 = Trainer(build_net(kind, gname, depth)[0], graph=True)
    losses2 = [float(tr2.step(x, t)) for x, t in copies]
    assert losses == losses2, (losses, losses2)
    assert torch.equal(tr.fp.flat, tr2.fp.flat)
