"""GPU: crops drawn on the device (n3d_volume_line_index, n3d_patch_sample; nas_3d_unet_amd.generator with sampling=).  The kernels
are integer work, so every comparison is ==: the line index and the sampled table against the numpy statement (tests/_sample_ref.py)
that the CPU tests tie to np.cumsum, np.argwhere and a known-answer table; the generator's batches against VolumeSet.patch_batch on
the statement's table for the recorded key."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import _sample_ref as sr
import make_golden_augment as mga

pytestmark = pytest.mark.gpu

KEY = sr.KEY
IDS = [0, 1, 2, 3, 1]          # five entries: the reduction is not a shift; volume 1 is drawn twice as often
ALWAYS = 1 << 32
# where a line's 64-voxel chunking or the scan's 1024-line tiles change
LINE_SHAPES = [(1, 1, 1), (3, 5, 63), (3, 5, 64), (3, 5, 65), (2, 3, 130), (32, 32, 7), (33, 31, 5), (25, 41, 3), (70, 70, 9)]


def _lib_k():
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd import kernels as K
    return _lib, _lib.load(), K


def _line_volume(shape, Cv, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    v = rng.integers(-2, 3, (Cv,) + shape).astype(np.float32) * (rng.random((1,) + shape) < 0.6)
    flat = v.reshape(Cv, n)
    for i, x in enumerate((-0.0, np.nan, np.inf, 1e-45)):         # alone in their voxel: the rule decides the count
        at = (i * 7) % n
        flat[:, at] = 0.0
        flat[Cv - 1, at] = x
    return v, rng.choice(np.array([0, 0, 1, 2, 4], np.uint8), shape)


def _device_index(vol, truth):
    _lib, lib, K = _lib_k()
    Cv, X, Y, Z = vol.shape
    v = torch.from_numpy(vol).cuda()
    t = torch.from_numpy(truth).cuda() if truth is not None else None
    out = torch.full((5, X * Y + 1), -7, dtype=torch.int32, device="cuda")          # every entry is written
    rc = lib.n3d_volume_line_index(K.ptr(v), Cv, K.ptr(t), X, Y, Z, K.ptr(out), K.stream_ptr())
    assert rc == 0, lib.n3d_last_error()
    return out.cpu().numpy()


@pytest.mark.parametrize("Cv", [1, 4])
@pytest.mark.parametrize("shape", LINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_line_index_equals_the_statement(shape, Cv):
    vol, truth = _line_volume(shape, Cv, 31 + Cv)
    got = _device_index(vol, truth)
    assert np.array_equal(got, sr.line_index(vol, truth))
    assert np.array_equal(got, _device_index(vol, truth))                        # two runs, the same bits
    bare = _device_index(vol, None)
    assert np.array_equal(bare[0], got[0]) and not bare[1:].any()
    if np.prod(shape) > 28:
        assert got[0, -1] == sr.masks_of(vol, truth)[0].sum() and 0 < got[0, -1] < np.prod(shape)


def test_line_index_refuses_bad_arguments():
    _lib, lib, K = _lib_k()
    v = torch.ones((1, 2, 2, 2), device="cuda")
    out = torch.full((5, 5), -7, dtype=torch.int32, device="cuda")
    for args in ((None, 1, None, 2, 2, 2, K.ptr(out)), (K.ptr(v), 1, None, 2, 2, 2, None), (K.ptr(v), 0, None, 2, 2, 2, K.ptr(out)),
                 (K.ptr(v), 1, None, 0, 2, 2, K.ptr(out)), (K.ptr(v), 1, None, 2048, 2048, 512, K.ptr(out))):
        assert lib.n3d_volume_line_index(*args, K.stream_ptr()) == -1 and b"volume_line_index" in lib.n3d_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7).all())


@pytest.fixture(scope="module")
def four():
    """(vols, truths, the statement's masks and indexes, the device set with every index built)"""
    from nas_3d_unet_amd.generator import VolumeSet
    vols, truths = sr.four_volumes()
    s = VolumeSet()
    for v, t in zip(vols, truths):
        s.add(v, t)
    assert s.line_indexes == [] and s.index_ptrs is None                        # add builds none
    prep = sr.prepare(vols, truths)
    for i in range(len(s)):
        assert np.array_equal(s.line_index(i).cpu().numpy(), prep[i][1])
    return vols, truths, prep, s


def _launch(s, ids, N, P, key, thr, bits):
    """n3d_patch_sample straight through the C ABI into sentinel-filled tables"""
    _lib, lib, K = _lib_k()
    cand = torch.full((max(N, 1), 4), -9, dtype=torch.int32, device="cuda")
    mode = torch.full((max(N, 1),), 99, dtype=torch.uint8, device="cuda")
    dev_ids = torch.tensor(ids, dtype=torch.int32).cuda()
    rc = lib.n3d_patch_sample(K.ptr(s.records), K.ptr(s.index_table()), len(s), s.channels, K.ptr(dev_ids), len(ids), N, P, key[0], key[1],
                              thr, bits, K.ptr(cand), K.ptr(mode), K.stream_ptr())
    assert rc == 0, lib.n3d_last_error()
    return cand.cpu().numpy()[:N], mode.cpu().numpy()[:N]


@pytest.mark.parametrize("masks", [("brain",), ("tumour",), (1, 2, 4), (4,)], ids=lambda m: "-".join(map(str, m)))
@pytest.mark.parametrize("P", [8, 16])
def test_sampler_equals_the_statement(four, P, masks):
    vols, truths, prep, s = four
    bits = sr.mask_bits(masks)
    bounds = [[sr.corner_bounds(d, P) for d in v.shape[1:]] for v in vols]
    seen = set()
    for N in (1, 63, 64, 65, 5000):
        for thr in (0, int(round(2 ** 32 / 3)), ALWAYS):
            cand, mode = _launch(s, IDS, N, P, KEY, thr, bits)
            want = sr.sample(vols, truths, IDS, N, P, KEY, thr, bits, prep)
            assert np.array_equal(cand, want[0]) and np.array_equal(mode, want[1]), (N, thr)
            again = _launch(s, IDS, N, P, KEY, thr, bits)
            assert np.array_equal(cand, again[0]) and np.array_equal(mode, again[1])
            for (v, *c), md in zip(cand.tolist(), mode.tolist()):
                assert all(lo <= x <= hi for x, (lo, hi) in zip(c, bounds[v])), (v, c)
                if md < 5:
                    centre = [x + P // 2 for x in c]
                    unclamped = all(lo < x < hi for x, (lo, hi) in zip(c, bounds[v]))
                    assert not unclamped or prep[v][0][md][tuple(centre)], (v, c, md)
                    assert prep[v][0][md][tuple(slice(max(x, 0), x + P) for x in c)].any()       # clamped or not, the patch holds the voxel
                    seen.add((md, unclamped))
            if N >= 63:
                other = _launch(s, IDS, N, P, (KEY[0], KEY[1] ^ 1), thr, bits)
                assert not np.array_equal(other[0], cand)
    assert {m for m, _ in seen} == {sr.MASKS.index(m) for m in masks}
    # the centre check did run: P = 8 leaves room in volume 1, which has every mask but label 4 (its corner must lie strictly inside
    # [lo, hi] on all three axes to be known as unclamped)
    assert P == 16 or masks == (4,) or any(u for _, u in seen)


def test_uniformity_conditions_hold_on_the_device():
    """the CPU half's two conditions under the same key, on the kernel's own output (which also equals the statement): 7000 draws over
    7 tumour voxels each within 6 sigma (29.3) of 1000; 6000 samples at foreground 1/3 within 6 sigma (36.5) of 2000 foreground"""
    from nas_3d_unet_amd.generator import VolumeSet
    vol, t = sr.seven_voxel_volume()
    s = VolumeSet()
    s.add(vol, t)
    s.line_index(0)
    cand, mode = _launch(s, [0], 7000, 8, KEY, ALWAYS, 2)
    _, mode3 = _launch(s, [0], 6000, 8, KEY, int(round(2 ** 32 / 3)), 2)
    counts, share = sr.uniformity_counts(cand, mode3)
    assert (mode == 1).all() and sum(counts) == 7000 and all(abs(c - 1000) <= 6 * 29.3 for c in counts), counts
    assert set(mode3.tolist()) == {1, 255} and abs(share - 2000) <= 6 * 36.5, share
    want = sr.sample([vol], [t], [0], 7000, 8, KEY, ALWAYS, 2)
    assert np.array_equal(cand, want[0]) and np.array_equal(mode, want[1])


def test_ids_outside_the_set_are_marked_and_then_dropped(four):
    vols, truths, prep, s = four
    ids, bits = [7, 0, -2, 3], sr.mask_bits(("tumour",))
    cand, mode = _launch(s, ids, 200, 8, KEY, ALWAYS, bits)
    want = sr.sample(vols, truths, ids, 200, 8, KEY, ALWAYS, bits, prep)
    assert np.array_equal(cand, want[0]) and np.array_equal(mode, want[1])
    bad = mode == 253
    assert 60 < bad.sum() < 140 and set(cand[bad, 0]) == {7, -2} and not cand[bad, 1:].any()
    flags = s.qualify_table(np.ascontiguousarray(cand), 8).cpu().numpy()
    assert not flags[bad].any() and flags[~bad].all()


def test_refusals_return_invalid_and_leave_the_tables_alone(four):
    _lib, lib, K = _lib_k()
    s = four[3]
    cand = torch.full((17, 4), -9, dtype=torch.int32, device="cuda")
    mode = torch.full((16,), 99, dtype=torch.uint8, device="cuda")
    ids = torch.tensor([0, 1, 2, 3], dtype=torch.int32).cuda()
    ok = dict(vols=K.ptr(s.records), index=K.ptr(s.index_table()), nvol=len(s), Cv=s.channels, ids=K.ptr(ids), n_ids=4, N=16, P=8, k0=1, k1=2,
              thr=1 << 31, masks=2, cand=K.ptr(cand), mode=K.ptr(mode))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.n3d_patch_sample(a["vols"], a["index"], a["nvol"], a["Cv"], a["ids"], a["n_ids"], a["N"], a["P"], a["k0"], a["k1"], a["thr"],
                                    a["masks"], a["cand"], a["mode"], K.stream_ptr())

    bad = [dict(masks=0), dict(masks=0, thr=1), dict(masks=32), dict(masks=63), dict(masks=-1), dict(thr=(1 << 32) + 1), dict(n_ids=0),
           dict(n_ids=-1), dict(P=0), dict(N=-1), dict(N=(1 << 24) + 1), dict(vols=None), dict(index=None), dict(ids=None), dict(cand=None),
           dict(mode=None), dict(cand=C.c_void_p(cand.data_ptr() + 4)), dict(cand=C.c_void_p(cand.data_ptr() + 8)),
           dict(ids=C.c_void_p(ids.data_ptr() + 2)), dict(index=C.c_void_p(s.index_table().data_ptr() + 4))]
    for kw in bad:
        assert call(**kw) == -1 and b"patch_sample" in lib.n3d_last_error(), kw
    # N == 0 is legal, launches nothing and reads no table; wrong scalars are refused even then
    assert call(N=0) == 0 and call(N=0, vols=None, index=None, ids=None, cand=None, mode=None) == 0
    assert call(N=0, masks=32) == -1 and call(N=0, P=0) == -1
    torch.cuda.synchronize()
    assert bool((cand == -9).all()) and bool((mode == 99).all())
    # the limits themselves are legal: no mask with no foreground, the threshold 2^32, all five masks
    assert call(masks=0, thr=0) == 0 and call(thr=1 << 32, masks=31) == 0
    torch.cuda.synchronize()
    assert bool((cand[:16] != -9).any()) and bool((cand[16] == -9).all()) and bool((mode != 99).all())


def test_volume_set_sample_builds_indexes_lazily_and_refuses(four):
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.generator import VolumeSet
    vols, truths, prep, _ = four
    s = VolumeSet()
    for v, t in zip(vols, truths):
        s.add(v, t)
    cand, mode = s.sample([1, 3], 100, 8, KEY, foreground=1.0, masks=(1, 2, 4))
    assert [t is not None for t in s.line_indexes] == [False, True, False, True]
    assert s.index_ptrs.cpu().tolist() == [0, s.line_indexes[1].data_ptr(), 0, s.line_indexes[3].data_ptr()]
    want = sr.sample(vols, truths, [1, 3], 100, 8, KEY, ALWAYS, sr.mask_bits((1, 2, 4)), prep)
    assert cand.dtype == torch.int32 and mode.dtype == torch.uint8 and cand.is_cuda
    assert np.array_equal(cand.cpu().numpy(), want[0]) and np.array_equal(mode.cpu().numpy(), want[1])
    kept = s.index_ptrs
    s.sample([3], 4, 8, KEY)
    assert s.index_ptrs is kept and s.line_index(3) is s.line_indexes[3]          # nothing new: nothing rebuilt
    s.sample([0], 4, 8, KEY)
    assert s.index_ptrs is not kept and s.index_ptrs.cpu().tolist()[0] == s.line_indexes[0].data_ptr()
    assert tuple(s.sample([0], 0, 8, KEY)[0].shape) == (0, 4)
    bare = VolumeSet()
    bare.add(vols[0])
    for call in (lambda: s.sample([], 4, 8, KEY), lambda: s.sample([4], 4, 8, KEY), lambda: s.sample([0], -1, 8, KEY),
                 lambda: s.sample([0], 4, 8, KEY, masks=(3,)), lambda: s.sample([0], 4, 8, KEY, foreground=2),
                 lambda: bare.sample([0], 4, 8, KEY, masks=("tumour",)), lambda: s.line_index(4)):
        with pytest.raises(N3DError):
            call()
    c, m = bare.sample([0], 50, 8, KEY, foreground=1.0, masks=("brain",))
    w = sr.sample(vols[:1], [None], [0], 50, 8, KEY, ALWAYS, 1)
    assert np.array_equal(c.cpu().numpy(), w[0]) and np.array_equal(m.cpu().numpy(), w[1]) and (w[1] == 0).all()


class Recording:
    """an np.random-like object that notes the name of every call it passes on"""

    def __init__(self, rs):
        self.rs, self.names = rs, []

    def __getattr__(self, name):
        f = getattr(self.rs, name)

        def call(*a, **k):
            self.names.append(name)
            return f(*a, **k)
        return call


def _bits32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "rotated"])
def test_generator_batches_are_patch_batch_on_the_statements_table(four, augment):
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd.sampling import RandomCrop
    vols, truths, prep, s = four
    P, B, ids = 8, 4, [0, 1, 2, 3]
    bits = sr.mask_bits((4,))
    kw = dict(augment=True, augment_rotation=10, affine=mga.BRATS_AFFINE) if augment else {}
    rec = Recording(np.random.RandomState(77))
    gen = G.Generator(ids, s, P, batch_size=B, labels=[1, 2, 4], rng=random.Random(5), np_rng=rec,
                      sampling=RandomCrop(24, foreground=1.0, masks=(4,)), **kw)
    twin, twin_rng = np.random.RandomState(77), random.Random(5)
    key = tuple(int(k) for k in twin.randint(0, 2 ** 32, 2, dtype=np.uint32))
    assert rec.names == ["randint"] and gen.sample_key == key                    # the key is the epoch's first draw
    cand, mode = sr.sample(vols, truths, ids, 24, P, key, ALWAYS, bits, prep)
    assert np.array_equal(gen.candidates, cand) and np.array_equal(gen.sample_modes, mode)
    assert {4, 254} <= set(mode.tolist()) and 255 not in mode                   # volumes 1 and 2 have no label 4
    flags = s.qualify_table(cand, P).cpu().numpy()
    assert np.array_equal(gen.flags, flags)
    assert gen.n_patches == int(G.kept_mask(flags, True).sum()) >= 12 and gen.steps_per_epoch == -(-gen.n_patches // B)
    affine = G.check_affine(mga.BRATS_AFFINE)
    order = G.epoch_order(flags, B, twin_rng, True, True, False, augment=(twin, 0.25, True) if augment else None,
                          warp=(twin, 10, None, None, s.channels) if augment else None)
    seen = 0
    for (x, t), batch in zip(gen.epoch(), order):
        refs = [(int(cand[e[0], 0]), tuple(int(c) for c in cand[e[0], 1:]), e[1]) for e in batch]
        if augment:
            aug, warp = [], []
            for (scale, axes), (angles, gain, bias) in (e[2:4] for e in batch):
                A, b, identity = G.resample_transform(affine, P, scale)
                aug.append((A, b / A, identity, axes))
                warp.append((G.warp_transform(A, b, G.rotation_matrix(angles), P), 0, gain, bias))
            wx, wt = s.patch_batch(refs, P, augment=aug, warp=warp)
        else:
            wx, wt = s.patch_batch(refs, P)
        assert np.array_equal(_bits32(x), _bits32(wx)) and torch.equal(t, wt), refs
        seen += len(refs)
    assert seen == int(G.kept_mask(flags, True).sum()) and next(order, None) is None
    # the np_rng calls: the key, today's calls per kept patch, and the next epoch's key after the last batch
    per_patch = ["normal", "choice", "choice", "choice", "uniform"] if augment else []
    assert rec.names == ["randint"] + per_patch * seen + ["randint"]
    key2 = tuple(int(k) for k in twin.randint(0, 2 ** 32, 2, dtype=np.uint32))
    cand2, mode2 = sr.sample(vols, truths, ids, 24, P, key2, ALWAYS, bits, prep)
    assert gen.sample_key == key2 != key and not np.array_equal(cand2, cand)
    assert np.array_equal(gen.candidates, cand2) and np.array_equal(gen.sample_modes, mode2)


def test_generator_refuses_what_sampling_replaces(four):
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.generator import VolumeSet
    from nas_3d_unet_amd.sampling import RandomCrop
    vols, truths, prep, s = four
    crop = RandomCrop(24, foreground=1.0, masks=(4,))
    kw = dict(indices_list=[0, 1], volumes=s, patch_shape=8, batch_size=4, labels=[1, 2, 4], np_rng=np.random.RandomState(1))
    with pytest.raises(N3DError, match="grid"):
        G.Generator(patch_overlap=2, sampling=crop, **kw)
    with pytest.raises(N3DError, match="grid"):
        G.Generator(patch_overlap=0, sampling=crop, **kw)
    with pytest.raises(N3DError, match="grid"):
        G.Generator(both_ps=True, sampling=crop, **kw)
    with pytest.raises(N3DError, match="RandomCrop"):
        G.Generator(sampling=(24, 1.0), **kw)
    bare = VolumeSet()
    bare.add(vols[1])
    with pytest.raises(N3DError, match="truth"):
        G.Generator(sampling=crop, **dict(kw, volumes=bare, indices_list=[0]))
    gen = G.Generator(sampling=RandomCrop(10, 0.5, ("brain",)), **dict(kw, volumes=bare, indices_list=[0]))
    assert set(gen.sample_modes.tolist()) == {0, 255} and gen.n_patches == 10       # without truth nothing is skipped as healthy
    x, t = next(gen.epoch())
    assert tuple(x.shape) == (4, 2, 8, 8, 8) and t is None
