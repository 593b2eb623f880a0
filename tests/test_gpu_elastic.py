"""GPU: the elastic deformation in the patch gather (n3d_patch_gather_elastic; nas_3d_unet_amd.generator with augment_elastic).  On the
cases of tests/golden/elastic.npz the kernel gives scipy's recorded answers (== at order 0 and for the labels, one float32 step at
order 1) and, with ==, the numpy statement of the rule (tests/_elastic_ref.py) that the CPU tests tie to that fixture and to an
independent B-spline evaluation; with `elastic` clear or amp = 0 it is n3d_patch_gather_warp bit for bit; everywhere else -- mixed
batches, every option of the generator -- it equals the numpy statement with ==."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import _elastic_ref as er
import _warp_ref as wr
import golden_common as gc
import make_golden_augment as mga
import make_golden_warp as mgw
from oracle import data_step as ds
from test_gpu_augment import IDENTITY, _face_refs, _random_vols
from test_gpu_warp import _bits32, _coefficients, _set_of

pytestmark = pytest.mark.gpu

ISO_KEY = ((0, 1), 1, 0, 1, 1)          # an isometry with a permutation and flips


def _volume(P, Cv):
    """the fixture's inputs as a (Cv, P, P, P) volume: its two channels, then two more (a signed pattern and a small ramp)"""
    data, truth = mgw.warp_inputs(P)
    g = np.meshgrid(*[np.arange(P)] * 3, indexing="ij")
    extra = np.stack([(3 * g[0] + g[1] + 2 * g[2]) % 7 - 3, 0.25 * g[0] + 0.5 * g[2] + 1]).astype(np.float32)
    return np.concatenate((data, extra))[:Cv].copy(), truth[0].copy()


def _expected(vols, refs, augs, warps, elastics, P, inclusive):
    """the batch by the rule: crop with zero padding -> flip + deformed resample + intensity (the helper) -> isometry -> labels"""
    xs, ys = [], []
    for (v, corner, key), aug, warp, el in zip(refs, augs, warps, elastics):
        vol, truth = vols[v]
        x = ds.crop_zero_pad(vol, corner, P)
        y = ds.crop_zero_pad(truth.reshape((1,) + vol.shape[1:]), corner, P) if truth is not None else np.zeros((1, P, P, P), np.uint8)
        mode, k, order, flips, gain, bias = _coefficients(aug, warp)
        c = er.coordinates(P, mode, k, el)
        x, y = er.resample(x, c, order, flips, gain, bias), er.resample(y, c, 0, flips)
        perm, flip = ds.isometry_of_key(IDENTITY if key is None else key)
        xs.append(ds.apply_isometry(x, perm, flip))
        ys.append(ds.apply_isometry(y, perm, flip))
    return np.asarray(xs, np.float32), ds.expand_labels(np.asarray(ys), inclusive)


def _edesc(vol=0, corner=(0, 0, 0), key=None, flips=(0, 0, 0), mode=0, order=0, k=(1.0,) * 3 + (0.0,) * 9, elastic=1, cells=1, lock=0,
           pkey=(1, 2), amp=(1.0, 1.0, 1.0), inv_h=None, P=8, perm=None):
    from nas_3d_unet_amd._lib import ElasticDesc, GatherDesc, PatchDesc, WarpDesc
    p, f = ds.isometry_of_key(IDENTITY if key is None else key)
    gd = GatherDesc(PatchDesc((C.c_int32 * 3)(*corner), (C.c_int32 * 3)(*(perm or p)), (C.c_int32 * 3)(*[int(x) for x in f])), vol)
    w = WarpDesc(gd, (C.c_int32 * 3)(*flips), mode, order, 0, (C.c_double * 12)(*[float(x) for x in k]), (C.c_float * 4)(*[1.0] * 4),
                 (C.c_float * 4)(*[0.0] * 4))
    h = float(er.inv_h(cells, P)) if inv_h is None else inv_h
    return ElasticDesc(w, elastic, cells, lock, (C.c_uint32 * 2)(*pkey), 0, (C.c_double * 3)(*amp), h)


def _launch(s, Cv, descs, P, flags, xld, tdt):
    """n3d_patch_gather_elastic straight through the C ABI into buffers pre-filled with a pattern: (x (B, Cv, P, P, P), the lanes
    between Cv and xld, t (B, 3, P, P, P))"""
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd import kernels as K
    B = len(descs)
    buf = torch.full((B, P, P, P, xld), 7.0, device="cuda")
    t = torch.full((B, 3, P, P, P), 5, dtype=tdt, device="cuda")
    table = (_lib.ElasticDesc * B)(*descs)
    lib = _lib.load()
    rc = lib.n3d_patch_gather_elastic(K.ptr(s.records), len(s), Cv, table, B, P, flags, K.ptr(buf), xld, K.ptr(t), K.stream_ptr())
    assert rc == 0, lib.n3d_last_error()
    return buf[..., :Cv].permute(0, 4, 1, 2, 3).cpu().numpy(), buf[..., Cv:].cpu().numpy(), t.cpu().numpy()


def test_fixture_cases_through_the_c_abi_equal_the_helper_and_scipy(golden):
    """every case of elastic.npz, as patch 0 under the identity isometry and as patch 1 under a permuting, flipping one: == the numpy
    statement at order 0, at order 1 and for the labels; == scipy's recorded answers at order 0 and for the labels, one float32 step
    at order 1.  Cv 4 (the float4 store) and Cv 3, on the channel pitch Cv and on a pitch of 8 whose other lanes stay untouched; float
    and byte targets; inclusive on and off.  P = 12: 1728 voxels, the last workgroup is partial."""
    from nas_3d_unet_amd import _lib
    recs = er.records(golden("elastic"))
    sizes = sorted({c["P"] for c, *_ in recs})
    assert sizes == [8, 12, 16]
    vols = {Cv: [_volume(P, Cv) for P in sizes] for Cv in (4, 3)}
    sets = {Cv: _set_of(vols[Cv]) for Cv in (4, 3)}
    perm, flip = ds.isometry_of_key(ISO_KEY)
    assert list(perm) != [0, 1, 2] and any(flip)
    configs = ((4, 4, torch.float32, True), (4, 8, torch.uint8, False), (3, 3, torch.float32, False), (3, 8, torch.uint8, True))
    for c, k, x0, x1, y in recs:
        P, v, el = c["P"], sizes.index(c["P"]), er.case_elastic(c)
        coords = er.coordinates(P, c["mode"], k, el)
        crop, tcrop = (ds.crop_zero_pad(a, c["corner"], P) for a in (vols[4][v][0], vols[4][v][1][None]))
        want = {order: er.resample(crop, coords, order, c["flips"]) for order in (0, 1)}
        wy = er.resample(tcrop, coords, 0, c["flips"])
        assert np.array_equal(want[0][:2], x0) and wr.one_step(want[1][:2], x1).all() and np.array_equal(wy, y)
        for Cv, xld, tdt, incl in configs:
            flags = (_lib.PATCH_INCLUSIVE if incl else 0) | (_lib.PATCH_T_U8 if tdt == torch.uint8 else 0)
            for order in (0, 1):
                descs = [_edesc(v, c["corner"], key, c["flips"], c["mode"], order, k, 1, el[0], el[1], el[2], el[3], None, P)
                         for key in (None, ISO_KEY)]
                x, rest, t = _launch(sets[Cv], Cv, descs, P, flags, xld, tdt)
                assert (rest == 7.0).all()
                for n, (pm, fl) in enumerate((([0, 1, 2], [False] * 3), (perm, flip))):
                    name = (c["name"], Cv, xld, order, n)
                    assert np.array_equal(_bits32(x[n]), _bits32(ds.apply_isometry(want[order][:Cv], pm, fl))), name
                    assert np.array_equal(t[n], ds.expand_labels(ds.apply_isometry(y, pm, fl)[None], incl)[0].astype(t.dtype)), name
                    if order == 0:
                        assert np.array_equal(x[n][:2], ds.apply_isometry(x0, pm, fl)), name
                    else:
                        assert wr.one_step(x[n][:2], ds.apply_isometry(x1, pm, fl)).all(), name


def _mixed_batch(P, B, seed):
    """per patch an augmentation entry, a warp entry and an elastic entry: elastic on and off, cells 1 .. 8, every lock, per-axis
    amplitudes; matrix and zoom-shift coordinates, both orders, with and without gain / bias"""
    from nas_3d_unet_amd import generator as G
    rs = np.random.RandomState(seed)
    augs, warps, elastics = [], [], []
    lattices = [(1, 0), (2, 0), (3, 2), (4, 3), (8, 0), (5, 1), (2, 1), (7, 3)]
    for n in range(B):
        A, b = (np.ones(3), np.zeros(3)) if n % 3 == 0 else (rs.uniform(0.9, 1.1, 3), rs.uniform(-0.5, 0.5, 3))
        matrix = G.warp_transform(A, b, G.rotation_matrix(rs.uniform(-15, 15, 3)), P)
        gain, bias = rs.uniform(0.9, 1.1, 4), rs.normal(0, 0.1, 4)
        augs.append(None if n % 4 == 3 else (A, b / A, n % 3 == 0, [a for a in range(3) if (n >> a) & 1]))
        warps.append([None, (matrix, 0, None, None), (matrix, 1, gain, bias), (None, 1, gain, None), (matrix, 1, None, None)][n % 5])
        cells, lock = lattices[n % len(lattices)]
        amp = 0.45 * (P - 1) / cells * np.array([1.0, 0.5, 0.0] if n % 4 == 1 else [1.0, 1.0, 1.0])
        elastics.append(None if n % 3 == 2 else (cells, lock, (int(rs.randint(0, 2 ** 31)), int(rs.randint(0, 2 ** 31))), tuple(amp)))
    return augs, warps, elastics


def test_mixed_batches_of_eight_from_two_volumes_equal_the_helper():
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd._lib import N3DError
    vols = []
    for v, t in _random_vols(81, ((20, 17, 23), (15, 22, 18)), 4):
        v[:, :2] = 0                                     # a slab of background: it stays exactly 0 under a bias
        vols.append((v, t))
    s, bare = _set_of(vols), _set_of(vols, truth=False)
    rng = np.random.default_rng(82)
    for P in (12, 9):
        keys = (gc.permutation_keys()[(P % 4)::7] + [None])[:8]
        refs = _face_refs(vols, P, keys, rng)
        B = len(refs)
        assert B == 8 and len({r[0] for r in refs}) == 2
        augs, warps, elastics = _mixed_batch(P, B, 100 + P)
        assert any(e is None for e in elastics) and len({e[0] for e in elastics if e is not None}) >= 4
        want = {incl: _expected(vols, refs, augs, warps, elastics, P, incl) for incl in (True, False)}
        plain = _expected(vols, refs, augs, warps, [None] * B, P, True)[0]
        on = [n for n, e in enumerate(elastics) if e is not None]
        assert all(not np.array_equal(want[True][0][n], plain[n]) for n in on)
        for incl in (True, False):
            for tdt in (torch.float32, torch.uint8):
                x, t = s.patch_batch(refs, P, inclusive_label=incl, target_dtype=tdt, augment=augs, warp=warps, elastic=elastics)
                assert K._pitch_of(x) == 4 and t.dtype == tdt
                assert np.array_equal(_bits32(x.cpu().numpy()), _bits32(want[incl][0]))
                assert np.array_equal(t.cpu().numpy(), want[incl][1].astype(t.cpu().numpy().dtype))
        x, t = bare.patch_batch(refs, P, augment=augs, warp=warps, elastic=elastics)
        assert t is None and np.array_equal(_bits32(x.cpu().numpy()), _bits32(want[True][0]))
        # without warp entries the coordinate is the augmentation's, deformed
        x, t = s.patch_batch(refs, P, augment=augs, elastic=elastics)
        wx, wy = _expected(vols, refs, augs, [None] * B, elastics, P, False)
        assert np.array_equal(_bits32(x.cpu().numpy()), _bits32(wx)) and np.array_equal(t.cpu().numpy(), wy.astype(np.float32))
    with pytest.raises(N3DError, match="N3D_PATCH_ELASTIC_MAX_BATCH"):
        s.patch_batch(refs + refs[:1], P, elastic=elastics + [None])
    s.patch_batch(refs + refs[:1], P, elastic=[None] * 9)                      # nothing deformed: the launch is today's
    with pytest.raises(N3DError, match="one elastic entry"):
        s.patch_batch(refs, P, elastic=elastics[:3])
    with pytest.raises(N3DError, match="cells"):
        s.patch_batch(refs[:1], P, elastic=[(9, 0, (1, 2), 1.0)])


def test_elastic_off_and_zero_amplitude_are_the_warp_launch_bit_for_bit():
    vols = _random_vols(83, ((20, 17, 23), (15, 22, 18)), 4)
    s = _set_of(vols)
    rng = np.random.default_rng(84)
    P = 12
    refs = _face_refs(vols, P, (gc.permutation_keys()[1::7] + [None])[:8], rng)
    augs, warps, _ = _mixed_batch(P, 8, 7)
    real = (2, 0, (5, 6), 2.0)
    elastics = [None, (4, 2, (1, 2), 0.0), None, (8, 0, (3, 4), (0.0, 0.0, 0.0)), None, (1, 0, (9, 9), 0.0), None, real]
    for tdt in (torch.float32, torch.uint8):
        xw, tw = s.patch_batch(refs, P, target_dtype=tdt, augment=augs, warp=warps)
        xe, te = s.patch_batch(refs, P, target_dtype=tdt, augment=augs, warp=warps, elastic=elastics)
        xe2, te2 = s.patch_batch(refs, P, target_dtype=tdt, augment=augs, warp=warps, elastic=elastics)
        a, b, c = (_bits32(x.cpu().numpy()) for x in (xw, xe, xe2))
        assert np.array_equal(a[:7], b[:7]) and torch.equal(tw[:7], te[:7]) and not np.array_equal(a[7], b[7])
        assert np.array_equal(b, c) and torch.equal(te, te2)                   # two runs of the same call
        assert bool(xw.any()) and bool(tw.any())


def test_invalid_arguments_return_invalid_and_launch_nothing():
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd import kernels as K
    P = 8
    s = _set_of([_volume(P, 4)])
    lib = _lib.load()
    out = torch.full((9, P, P, P, 4), 3.0, device="cuda")
    t = torch.full((9, 3, P, P, P), 9, dtype=torch.uint8, device="cuda")
    nan, inf = float("nan"), float("inf")

    def call(descs, flags=_lib.PATCH_T_U8, Cv=4, xld=4):
        table = (_lib.ElasticDesc * len(descs))(*descs)
        return lib.n3d_patch_gather_elastic(K.ptr(s.records), len(s), Cv, table, len(descs), P, flags, K.ptr(out), xld, K.ptr(t), K.stream_ptr())

    k = [1.0] * 3 + [0.0] * 9
    bad = [([_edesc()] * 9, b"N3D_PATCH_ELASTIC_MAX_BATCH"),
           ([_edesc(cells=0)], b"cells"), ([_edesc(cells=9, inv_h=1.0)], b"cells"), ([_edesc(lock=-1)], b"lock"), ([_edesc(lock=4, cells=8)], b"lock"),
           ([_edesc(cells=1, lock=2)], b"no free control point"), ([_edesc(cells=2, lock=3)], b"no free control point"),
           ([_edesc(amp=(1.0, nan, 1.0))], b"amp"), ([_edesc(amp=(inf, 1.0, 1.0))], b"amp"), ([_edesc(amp=(1.0, 1.0, -0.5))], b"amp"),
           ([_edesc(inv_h=nan)], b"inv_h"), ([_edesc(inv_h=inf)], b"inv_h"), ([_edesc(inv_h=-0.125)], b"inv_h"),
           # the lattice is checked on a patch that is not deformed as well
           ([_edesc(elastic=0, cells=0)], b"cells"), ([_edesc(elastic=0, amp=(nan, 0.0, 0.0))], b"amp"),
           # everything n3d_patch_gather_warp checks
           ([_edesc(perm=(0, 0, 1))], b"perm"), ([_edesc(perm=(0, 1, 3))], b"perm"), ([_edesc(vol=1)], b"volume"), ([_edesc(vol=-1)], b"volume"),
           ([_edesc(mode=2)], b"mode"), ([_edesc(order=2)], b"order"), ([_edesc(k=[0.0] + k[1:])], b"nonzero"),
           ([_edesc(k=k[:4] + [inf] + k[5:])], b"finite"), ([_edesc(mode=1, k=k[:11] + [nan])], b"finite"),
           ([_edesc(), _edesc(cells=0)], b"descriptor 1")]
    for descs, word in bad:
        assert call(descs) == -1 and word in lib.n3d_last_error(), (word, lib.n3d_last_error())
        assert b"patch_gather_elastic" in lib.n3d_last_error()
    assert call([_edesc()], flags=4) == -1 and b"flag" in lib.n3d_last_error()
    gain_nan = _edesc()
    gain_nan.w.gain[1] = nan
    assert call([gain_nan]) == -1 and b"gain and bias" in lib.n3d_last_error()
    five = _edesc()
    five.w.intensity = 1
    assert call([five], Cv=5, xld=5) == -1 and b"at most 4 channels" in lib.n3d_last_error()       # refused ahead of any launch
    assert call([_edesc()], Cv=5) == -1 and b"bad args" in lib.n3d_last_error()                        # a pitch below Cv
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((t == 9).all())
    # ... and the limits themselves are legal: 8 patches, cells 8 with lock 3, cells 4 with lock 3, amp 0, inv_h 0
    good = [_edesc(cells=8, lock=3), _edesc(cells=4, lock=3), _edesc(cells=3, lock=2), _edesc(amp=(0.0, 0.0, 0.0)), _edesc(inv_h=0.0),
            _edesc(elastic=0), _edesc(cells=8, lock=0, amp=(0.4, 0.4, 0.4)), _edesc(cells=1, lock=1)]
    assert call(good) == 0
    torch.cuda.synchronize()
    assert bool((out[:8] != 3.0).any()) and bool((out[8] == 3.0).all())


def _volumes_for_the_generator():
    vols = _random_vols(85, ((20, 18, 16), (18, 19, 17)), 4)
    for v, _ in vols:
        v[:, :, :, :3] = 0
    return vols


def _twin_batches(G, gen, kw, rng, twin, e, Cv, P):
    """the restatement driven by epoch_order's entries, on twin random streams: yields (refs, augs, warps, elastics) per batch"""
    affine = G.check_affine(mga.BRATS_AFFINE)
    warped = kw.get("augment_rotation") is not None or kw.get("augment_interpolation", "nearest") != "nearest"
    wdraws = (twin, kw.get("augment_rotation"), None, None, Cv) if warped else None
    order = 1 if kw.get("augment_interpolation") == "linear" else 0
    for batch in G.epoch_order(gen.flags, kw["batch_size"], rng, True, True, kw.get("permute", False), augment=(twin, 0.25, True), warp=wdraws,
                               elastic=(twin, e)):
        refs = [(int(gen.candidates[x[0], 0]), tuple(int(c) for c in gen.candidates[x[0], 1:]), x[1]) for x in batch]
        augs, warps, elastics = [], [], []
        for x in batch:
            scale, axes = x[2]
            A, b, identity = G.resample_transform(affine, P, scale)
            augs.append((A, b / A, identity, axes))
            if warped:
                angles = x[3][0]
                warps.append((wr.warp_transform(A, b, wr.rotation_matrix(angles), P) if angles is not None else None, order, None, None))
            else:
                warps.append(None)
            key = x[4 if warped else 3]
            elastics.append(None if key is None else (e.cells, e.lock, key, e.amp))
        yield refs, augs, warps, elastics


def test_generator_batches_equal_the_helper_with_every_option_and_in_out_buffers():
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd.elastic import Elastic
    vols = _volumes_for_the_generator()
    s = _set_of(vols)
    P, Cv = 8, 4
    e = Elastic(cells=1, displacement=1.5, p=0.5, lock=0)
    base = dict(indices_list=[0, 1], patch_shape=P, patch_overlap=None, batch_size=3, augment=True, affine=mga.BRATS_AFFINE)
    runs = [(dict(base), None), (dict(base, augment_rotation=15, augment_interpolation="linear", permute=True), None),
            (dict(base, permute=True), "out")]
    for n, (kw, out) in enumerate(runs):
        gen = G.Generator(volumes=s, labels=[1, 2, 4], rng=random.Random(51 + n), np_rng=np.random.RandomState(151 + n), augment_elastic=e, **kw)
        bufs = (K.empty_ndhwc(3, Cv, P, P, P, s.device, torch.float32), torch.empty((3, 3, P, P, P), device=s.device)) if out else None
        twins = _twin_batches(G, gen, kw, random.Random(51 + n), np.random.RandomState(151 + n), e, Cv, P)
        seen = deformed = in_place = 0
        for (x, t), (refs, augs, warps, elastics) in zip(gen.epoch(out=bufs), twins):
            if out and len(refs) == 3:
                assert x is bufs[0] and t is bufs[1]
                in_place += 1
            wx, wy = _expected(vols, refs, augs, warps, elastics, P, False)
            assert np.array_equal(_bits32(x.cpu().numpy()), _bits32(wx)) and np.array_equal(t.cpu().numpy(), wy.astype(np.float32)), (n, refs)
            seen += len(refs)
            deformed += sum(el is not None for el in elastics)
        assert seen == gen.n_patches >= 12 and next(twins, None) is None
        assert 0.25 * seen <= deformed <= 0.75 * seen                       # p = 0.5
        assert not out or in_place >= 3


def test_generator_refuses_what_the_option_cannot_do():
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.elastic import Elastic
    s = _set_of(_volumes_for_the_generator())
    e = Elastic(cells=1, displacement=1.5, p=0.5, lock=0)
    kw = dict(indices_list=[0, 1], volumes=s, patch_shape=8, labels=[1, 2, 4], affine=mga.BRATS_AFFINE)
    with pytest.raises(N3DError, match="only with augment=True"):
        G.Generator(batch_size=3, augment_elastic=e, **kw)
    with pytest.raises(N3DError, match="N3D_PATCH_ELASTIC_MAX_BATCH"):
        G.Generator(batch_size=9, augment=True, augment_elastic=e, **kw)
    with pytest.raises(N3DError, match="fold"):
        G.Generator(batch_size=3, augment=True, augment_elastic=Elastic(cells=1, displacement=3.5, lock=0), **kw)
    with pytest.raises(N3DError, match="elastic.Elastic"):
        G.Generator(batch_size=3, augment=True, augment_elastic=(1, 0, 1.5), **kw)

    class NoElastic:
        channels, has_truth = 4, True

        def patch_batch(self, refs, patch, inclusive_label=False, target_dtype=torch.float32, out=None, augment=None, warp=None):
            raise AssertionError("not reached")

    with pytest.raises(NotImplementedError, match="elastic"):
        G.Generator(batch_size=3, augment=True, augment_elastic=e, **dict(kw, volumes=NoElastic()))
    assert G.Generator(batch_size=8, augment=True, augment_elastic=e, **kw).augment_elastic is e
