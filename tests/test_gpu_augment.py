"""GPU: the generator's scale / flip augmentation in the patch gather (n3d_patch_gather_aug; nas_3d_unet_amd.generator with
augment=True).  With every patch flagged identity and no flips the new entry is n3d_patch_gather bit for bit; on the reference's
own operator outputs and on the adversarial coordinates of tests/golden/augment.npz it equals the fixture, and everywhere else the
numpy statement of the rule (tests/_augment_ref.py) that the CPU tests tie to the fixture; Generator(augment=True) yields the
reference Generator's batches; a Trainer fed in place trains like one fed copies."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import _augment_ref as ar
import golden_common as gc
import make_golden_augment as mga
import make_golden_generator as mg
from oracle import data_step as ds

pytestmark = pytest.mark.gpu

IDENTITY = ((0, 0), 0, 0, 0, 0)
PLAIN = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), True, None)        # an augmentation entry that changes nothing


def _expected(vols, refs, augs, P, inclusive):
    """the batch as the reference makes it: crop with zero padding -> flip + resample (the helper) -> isometry -> labels"""
    xs, ys = [], []
    for (v, corner, key), aug in zip(refs, augs):
        vol, truth = vols[v]
        x = ds.crop_zero_pad(vol, corner, P)
        y = ds.crop_zero_pad(truth.reshape((1,) + vol.shape[1:]), corner, P) if truth is not None else np.zeros((1, P, P, P), np.uint8)
        if aug is not None:
            A, sh, identity, axes = aug
            flips = [a in (axes or []) for a in range(3)]
            x, y = ar.augment_patch(x, A, sh, identity, flips), ar.augment_patch(y, A, sh, identity, flips)
        perm, flip = ds.isometry_of_key(IDENTITY if key is None else key)
        xs.append(ds.apply_isometry(x, perm, flip))
        ys.append(ds.apply_isometry(y, perm, flip))
    return np.asarray(xs, np.float32), ds.expand_labels(np.asarray(ys), inclusive)


def _fixture_augs(g):
    """(A, sh, identity, flipped axes) of every operator case and (one axis each) every adversarial case of the fixture"""
    out = []
    for cfg, scale, flips, A, b, identity, _, _ in ar.operator_records(g):
        A_, sh = ar.params_of(A, b, identity)
        out.append((A_, sh, identity, [a for a in range(3) if flips[a]]))
    for P, axis, A, b, _ in ar.adversarial_records(g):
        A_, sh = np.ones(3), np.zeros(3)
        A_[axis], sh[axis] = A, np.float64(b) / np.float64(A)
        out.append((A_, sh, False, None))
    return out


def _random_vols(seed, shapes, Cv):
    rng = np.random.default_rng(seed)
    return [(rng.integers(-99, 100, (Cv,) + sh).astype(np.float32), rng.choice(np.array([0, 0, 1, 2, 4], np.uint8), sh)) for sh in shapes]


def _face_refs(vols, P, keys, rng):
    """corners hanging over each of the six faces of some volume, then random ones (some wholly inside, some far out)"""
    refs = []
    for a in range(3):
        for side in (0, 1):
            v = (2 * a + side) % len(vols)
            dims = vols[v][0].shape[1:]
            c = [int(rng.integers(0, max(1, d - P))) for d in dims]
            c[a] = -3 if side == 0 else dims[a] - P + 3
            refs.append((v, tuple(c)))
    while len(refs) < len(keys):
        refs.append((int(rng.integers(0, len(vols))), tuple(int(c) for c in rng.integers(-6, 16, 3))))
    return [(v, c, k) for (v, c), k in zip(refs, keys)]


def test_identity_patches_without_flips_equal_patch_gather():
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd.generator import VolumeSet
    vols = _random_vols(61, ((20, 17, 23), (15, 22, 18), (24, 19, 16)), 4)
    s = VolumeSet()
    for v, t in vols:
        s.add(v, t)
    rng = np.random.default_rng(62)
    keys = gc.permutation_keys()[::4] + [None]
    P = 9
    refs = _face_refs(vols, P, keys, rng)
    B = len(refs)
    assert B == 13 and len({r[0] for r in refs}) == 3
    for incl in (True, False):
        for tdt in (torch.float32, torch.uint8):
            x0, t0 = s.patch_batch(refs, P, inclusive_label=incl, target_dtype=tdt)
            x1, t1 = s.patch_batch(refs, P, inclusive_label=incl, target_dtype=tdt, augment=[PLAIN] * B)
            assert K._pitch_of(x1) == 4 and t1.dtype == tdt
            assert torch.equal(x0, x1) and torch.equal(t0, t1)
            assert bool(x0.any()) and bool(t0.any())
    # a list of None entries is not an augmented batch: the plain launch, as today
    x2, t2 = s.patch_batch(refs, P, augment=[None] * B)
    x0, t0 = s.patch_batch(refs, P)
    assert torch.equal(x0, x2) and torch.equal(t0, t2)


def test_operator_and_adversarial_cases_equal_the_fixture(golden):
    """the reference's inputs as P^3 volumes at corner 0: the device output IS do_augment's recorded output (scipy's answer); for
    the adversarial axes, the source index decoded from the voxel numbers is scipy's table.  Cv = 2: the scalar store path, on the
    tensor's own pitch and on a pitch of 5; one batch mixes identity and resampled patches"""
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd.generator import VolumeSet
    g = golden("augment")
    ops, advs, augs = ar.operator_records(g), ar.adversarial_records(g), _fixture_augs(g)
    for P in (8, 10):
        data, truth = mga.operator_inputs(P)
        s = VolumeSet()
        s.add(data, truth)
        pick = [i for i, r in enumerate(ops) if r[0]["P"] == P] + [len(ops) + i for i, r in enumerate(advs) if r[0] == P]
        batch_augs = [augs[i] for i in pick] + [None]                 # the last patch is left as it is
        B = len(batch_augs)
        assert any(not a[2] for a in batch_augs[:-1])
        refs = [(0, (0, 0, 0), None)] * B
        for incl in (True, False):
            for tdt in (torch.float32, torch.uint8):
                x, t = s.patch_batch(refs, P, inclusive_label=incl, target_dtype=tdt, augment=batch_augs)
                xn, tn = x.cpu().numpy(), t.cpu().numpy()
                assert np.array_equal(xn[-1], data) and np.array_equal(tn[-1], ds.expand_labels(truth[None], incl)[0].astype(tn.dtype))
                for n, i in enumerate(pick):
                    if i < len(ops):
                        want_x, want_y = ops[i][6], ops[i][7]
                        assert np.array_equal(xn[n], want_x), ops[i][0]["name"]
                        assert np.array_equal(tn[n], ds.expand_labels(want_y[None], incl)[0].astype(tn.dtype)), ops[i][0]["name"]
                    else:
                        _, axis, A, b, src = advs[i - len(ops)]
                        ident = xn[n, 0].astype(np.int64) - 1                      # channel 0 numbers the voxels from 1; 0: no source
                        got = np.where(ident >= 0, np.unravel_index(np.maximum(ident, 0), (P, P, P))[axis], -1)
                        shape = [1, 1, 1]
                        shape[axis] = P
                        assert np.array_equal(got, np.broadcast_to(src.reshape(shape), (P, P, P))), (P, axis, A, b)
                        want_x, want_y = _expected([(data, truth)], [refs[n]], [augs[i]], P, incl)
                        assert np.array_equal(xn[n], want_x[0]) and np.array_equal(tn[n], want_y[0].astype(tn.dtype))
        # pitch 5 (a 2-channel slice of a 5-channel NDHWC buffer): the neighbours stay untouched
        wide = torch.full((B, P, P, P, 5), 7.0, device="cuda").permute(0, 4, 1, 2, 3)
        ox, ot = wide[:, :2], torch.full((B, 3, P, P, P), 5, dtype=torch.uint8, device="cuda")
        rx, rt = s.patch_batch(refs, P, out=(ox, ot), augment=batch_augs)
        assert rx is ox and rt is ot and K._pitch_of(ox) == 5
        x, t = s.patch_batch(refs, P, target_dtype=torch.uint8, augment=batch_augs)
        assert torch.equal(ox, x) and torch.equal(ot, t) and bool((wide[:, 2:] == 7.0).all())


def test_mixed_batches_equal_the_helper(golden):
    """Cv = 4 on the aligned pitch (the float4 store), patches of three volumes hanging over every face, every isometry class, the
    fixture's transforms applied at P = 9 (not a multiple of the wave) and 12 (several workgroups per patch), entries without an
    augmentation in the same batch; fp32 and byte targets, inclusive_label on and off; a set without truth"""
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd.generator import VolumeSet
    augs = _fixture_augs(golden("augment"))
    vols = _random_vols(63, ((20, 17, 23), (15, 22, 18), (24, 19, 16)), 4)
    s, bare = VolumeSet(), VolumeSet()
    for v, t in vols:
        s.add(v, t)
        bare.add(v)
    rng = np.random.default_rng(64)
    for P in (9, 12):
        keys = (gc.permutation_keys()[(P % 4)::4] + [None] * 3)[:15]
        refs = _face_refs(vols, P, keys, rng)
        B = len(refs)
        batch_augs = [None if n % 5 == 4 else augs[(n + P) % len(augs)] for n in range(B)]
        assert any(a is None for a in batch_augs) and any(a is not None and a[2] for a in batch_augs)
        want = {incl: _expected(vols, refs, batch_augs, P, incl) for incl in (True, False)}
        assert any(not np.array_equal(want[True][0][n], _expected(vols, [refs[n]], [None], P, True)[0][0]) for n in range(B))
        for incl in (True, False):
            for tdt in (torch.float32, torch.uint8):
                x, t = s.patch_batch(refs, P, inclusive_label=incl, target_dtype=tdt, augment=batch_augs)
                assert K._pitch_of(x) == 4 and x.data_ptr() % 16 == 0 and t.dtype == tdt
                assert np.array_equal(x.cpu().numpy(), want[incl][0])
                assert np.array_equal(t.cpu().numpy(), want[incl][1].astype(t.cpu().numpy().dtype))
        x, t = bare.patch_batch(refs, P, augment=batch_augs)
        assert t is None and np.array_equal(x.cpu().numpy(), want[True][0])


def test_a_full_descriptor_table_and_its_cap(golden):
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd._lib import AugDesc, GatherDesc, N3DError, PatchDesc
    from nas_3d_unet_amd.generator import AUG_MAX_BATCH, VolumeSet
    augs = _fixture_augs(golden("augment"))
    vols = _random_vols(65, ((14, 12, 13), (11, 15, 12)), 4)
    s = VolumeSet()
    for v, t in vols:
        s.add(v, t)
    rng = np.random.default_rng(66)
    P, B = 8, 32
    assert B == AUG_MAX_BATCH
    keys = [gc.permutation_keys()[int(k)] for k in rng.integers(0, 48, B)]
    refs = [(int(rng.integers(0, 2)), tuple(int(c) for c in rng.integers(-4, 9, 3)), k) for k in keys]
    batch_augs = [augs[n % len(augs)] for n in range(B)]
    x, t = s.patch_batch(refs, P, target_dtype=torch.uint8, augment=batch_augs)
    wx, wy = _expected(vols, refs, batch_augs, P, False)
    assert np.array_equal(x.cpu().numpy(), wx) and np.array_equal(t.cpu().numpy(), wy.astype(np.uint8))
    with pytest.raises(N3DError, match="N3D_PATCH_AUG_MAX_BATCH"):
        s.patch_batch(refs + refs[:1], P, augment=batch_augs + batch_augs[:1])
    s.patch_batch(refs + refs[:1], P)                                 # 33 plain patches are one n3d_patch_gather launch, as before
    # straight through the C ABI: the cap, a zero / non-finite A, a non-finite sh, a bad perm, a volume outside the set
    lib = _lib.load()
    xo = K.empty_ndhwc(33, 4, P, P, P, s.device, torch.float32)

    def call(descs, n):
        return lib.n3d_patch_gather_aug(K.ptr(s.records), len(s), 4, descs, n, P, 0, K.ptr(xo), 4, None, K.stream_ptr())

    def desc(perm=(0, 1, 2), vol=0, A=(1.0, 1.0, 1.0), sh=(0.0, 0.0, 0.0), identity=0):
        g = GatherDesc(PatchDesc((C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*perm), (C.c_int32 * 3)(0, 0, 0)), vol)
        return AugDesc(g, (C.c_int32 * 3)(0, 0, 0), identity, (C.c_double * 3)(*A), (C.c_double * 3)(*sh))

    assert call((AugDesc * 33)(*[desc()] * 33), 33) == -1 and b"N3D_PATCH_AUG_MAX_BATCH" in lib.n3d_last_error()
    assert call((AugDesc * 1)(desc()), 1) == 0
    for bad, word in ((desc(A=(1.0, 0.0, 1.0)), b"nonzero"), (desc(A=(float("nan"), 1.0, 1.0)), b"nonzero"),
                      (desc(A=(1.0, 1.0, float("inf")), identity=1), b"nonzero"), (desc(sh=(0.0, float("inf"), 0.0)), b"finite"),
                      (desc(perm=(0, 0, 1)), b"perm"), (desc(vol=2), b"volume"), (desc(vol=-1), b"volume")):
        assert call((AugDesc * 1)(bad), 1) == -1 and word in lib.n3d_last_error(), lib.n3d_last_error()
    torch.cuda.synchronize()


def test_generator_with_augmentation_reproduces_the_reference_generator(golden):
    from nas_3d_unet_amd import generator as G
    volumes = mg.generator_volumes()
    s = G.VolumeSet()
    for v, t in volumes:
        s.add(v, t)
    vols = [(v, t[0]) for v, t in volumes]
    for n, (cfg, rows, scales, x0, y0) in enumerate(ar.generator_records(golden("augment"))):
        kw = cfg["kwargs"]
        P, incl = kw["patch_shape"], kw.get("inclusive_label", False)
        affine = mga.AFFINES[cfg["affine"]]
        if n == 1:                       # np_rng=None: numpy's global generator, as the reference
            np.random.seed(cfg["np_seed"])
            np_rng = None
        else:
            np_rng = np.random.RandomState(cfg["np_seed"])
        gen = G.Generator(volumes=s, labels=[1, 2, 4], rng=random.Random(cfg["seed"]), np_rng=np_rng,
                          affine=None if cfg["affine"] == "identity" else affine, **kw)
        for e in range(cfg["epochs"]):
            assert gen.overlap == cfg["overlap"][e] and gen.steps_per_epoch == cfg["spe"][e], (cfg["name"], e)
            er, es = rows[rows[:, 0] == e], scales[rows[:, 0] == e]
            nb = 0
            for b, (x, t) in enumerate(gen.epoch()):
                sel = er[:, 1] == b
                br, bs = er[sel], es[sel]
                assert len(br) >= 1 and x.shape[0] == len(br)
                refs = [(int(r[2]), tuple(int(c) for c in r[3:6]), ar.key_of_row(r[6:12])) for r in br]
                augs = [G.resample_params(G.check_affine(affine), P, None if np.isnan(sc).any() else sc) +
                        ([a for a in range(3) if r[12 + a]],) for r, sc in zip(br, bs)]
                wx, wy = _expected(vols, refs, augs, P, incl)
                assert np.array_equal(x.cpu().numpy(), wx) and np.array_equal(t.cpu().numpy(), wy.astype(np.float32)), (cfg["name"], e, b)
                if e == 0 and b == 0:
                    assert np.array_equal(x.cpu().numpy(), x0) and np.array_equal(t.cpu().numpy(), y0.astype(np.float32)), cfg["name"]
                nb += 1
            assert nb == cfg["spe"][e] and int(er[:, 1].max()) == nb - 1, (cfg["name"], e)
            assert gen.overlap == cfg["overlap"][e + 1], (cfg["name"], e)


def test_trainer_fed_by_the_augmenting_generator_trains_like_one_fed_copies():
    """test_gpu_generator's trainer test with augment=True: the batches written by n3d_patch_gather_aug straight into the captured
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
                    affine=mga.BRATS_AFFINE, np_rng=np.random.RandomState(5))
    plain = Generator([0, 1, 2], s, size, batch_size=batch, labels=[1, 2, 4], permute=True, rng=random.Random(1))
    assert gen.n_patches == plain.n_patches and gen.n_patches % batch == 1
    tr = Trainer(build_net(kind, gname, depth)[0], graph=True)
    losses, copies, in_place = [], [], 0
    for (x, t), (px, pt) in zip(gen.epoch(out=tr.input_buffers), plain.epoch()):
        bufs = tr.input_buffers()
        if bufs[0] is not None and x.shape[0] == batch:
            assert x is bufs[0] and t is bufs[1]
            in_place += 1
        assert x.shape == px.shape and not torch.equal(x, px)          # the same candidates and keys, distorted
        copies.append((x.clone(), t.clone()))
        losses.append(float(tr.step(x, t)))
    assert len(losses) == gen.steps_per_epoch and copies[-1][0].shape[0] == 1 and in_place == len(losses) - 2
    tr2 = Trainer(build_net(kind, gname, depth)[0], graph=True)
    losses2 = [float(tr2.step(x, t)) for x, t in copies]
    assert losses == losses2, (losses, losses2)
    assert torch.equal(tr.fp.flat, tr2.fp.flat)
