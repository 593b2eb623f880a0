"""GPU: cubic B-spline (order 3) interpolation in the patch gather (n3d_spline_prefilter, n3d_patch_gather_spline; nas_3d_unet_amd.generator
with augment_interpolation="spline3").  The prefilter equals the numpy statement (tests/_spline_ref.py) bit for bit on both of its
plans; on the cases of tests/golden/spline.npz the gather equals the statement with == on the bits, scipy's recorded answers to one
float32 step where the mask keeps a voxel, and the order-0 launch of the same descriptors in its labels and its zero set; the
generator's batches equal the statement and carry the targets of the "linear" run."""
import random

import numpy as np
import pytest
import torch

import _elastic_ref as er
import _spline_ref as sr
import _warp_ref as wr
import make_golden_augment as mga
from oracle import data_step as ds
from test_gpu_augment import IDENTITY
from test_gpu_elastic import ISO_KEY, _edesc, _launch, _volume, _volumes_for_the_generator
from test_gpu_warp import _bits32, _coefficients, _set_of

pytestmark = pytest.mark.gpu

# no voxel value of the test volumes (integers, and multiples of 0.25 in channel 3) maps to exactly 0: v * gain + bias == 0 would need
# v = -0.4, 0.28, -1.82 or 2.04
GAIN, BIAS = (1.25, 0.9, 1.1, 0.75), (0.5, -0.25, 2.0, -1.53125)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("P,n", [(4, 3), (8, 3), (12, 3), (16, 3), (255, 1), (256, 1), (257, 1)])
def test_prefilter_equals_the_statement_bit_for_bit(P, n):
    """P = 4 (the smallest), 8, 12, 16 on three cubes: 48, 192, 432 and 768 lines against workgroups of 32 -- the last workgroup is
    partial at P = 4 (16 lines) and P = 12 (16 lines), whole at 8 and 16; P = 255 and 256 on one cube: the last size of the LDS plan
    (65 025 lines: a last workgroup of one line) and the first of the in-memory plan, whose workgroups take 64 lines: 65 536 lines at
    P = 256 are whole workgroups, so P = 257 (66 049 = 64 * 1032 + 1 lines) is there for that plan's tail"""
    from nas_3d_unet_amd import spline
    rs = np.random.RandomState(P)
    x = rs.uniform(10, 110, (n, P, P, P)).astype(np.float32)
    x[:, : P // 3] = 0                                       # background next to the data
    x[0, -1, -1, -1] = -37.5
    want = sr.coefficients(x)
    have = spline.prefilter(torch.from_numpy(x).cuda())
    assert have.dtype == torch.float64 and tuple(have.shape) == x.shape
    assert np.array_equal(_bits64(have.cpu().numpy()), _bits64(want))


def _sdesc(intensity, *a, **kw):
    d = _edesc(*a, **kw)
    d.w.order = 3
    if intensity:
        d.w.intensity = 1
        d.w.gain[:] = GAIN
        d.w.bias[:] = BIAS
    return d


def _launch_spline(s, Cv, descs, P, flags, xld, tdt):
    """n3d_patch_gather_spline straight through the C ABI into buffers pre-filled with a pattern: (x (B, Cv, P, P, P), the lanes
    between Cv and xld, t (B, 3, P, P, P))"""
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd import kernels as K
    B = len(descs)
    buf = torch.full((B, P, P, P, xld), 7.0, device="cuda")
    t = torch.full((B, 3, P, P, P), 5, dtype=tdt, device="cuda")
    table = (_lib.ElasticDesc * B)(*descs)
    lib = _lib.load()
    scratch = torch.empty(lib.n3d_patch_spline_scratch_bytes(B, Cv, P), dtype=torch.uint8, device="cuda")
    rc = lib.n3d_patch_gather_spline(K.ptr(s.records), len(s), Cv, table, B, P, flags, K.ptr(scratch), scratch.numel(), K.ptr(buf), xld,
                                     K.ptr(t), K.stream_ptr())
    assert rc == 0, lib.n3d_last_error()
    return buf[..., :Cv].permute(0, 4, 1, 2, 3).cpu().numpy(), buf[..., Cv:].cpu().numpy(), t.cpu().numpy()


def test_fixture_cases_through_the_c_abi_equal_the_statement_scipy_and_the_order_0_launch(golden):
    """every case of spline.npz, as patch 0 under the identity isometry and as patch 1 under a permuting, flipping one.  Cv 4 on pitch 4
    (the float4 store) and Cv 3 on pitch 8 (the spare lanes untouched), each once with float targets, inclusive, no intensity map and
    once with byte targets, not inclusive, with the intensity map.  P = 12: 1728 voxels, the last workgroup is partial."""
    from nas_3d_unet_amd import _lib
    recs = sr.records(golden("spline"))
    sizes = sorted({c["P"] for c, *_ in recs})
    assert sizes == [8, 12, 16]
    vols = {Cv: [_volume(P, Cv) for P in sizes] for Cv in (4, 3)}
    sets = {Cv: _set_of(vols[Cv]) for Cv in (4, 3)}
    perm, flip = ds.isometry_of_key(ISO_KEY)
    configs = ((4, 4, torch.float32, True, False), (3, 8, torch.uint8, False, True), (4, 4, torch.uint8, False, True),
               (3, 8, torch.float32, True, False))
    for c, k, x3 in recs:
        P, v, el = c["P"], sizes.index(c["P"]), sr.case_elastic(c)
        coords = er.coordinates(P, c["mode"], k, el)
        crop = ds.crop_zero_pad(vols[4][v][0], c["corner"], P)
        keep = sr.mask(sr.flipped(crop, c["flips"]), coords)
        lattice = el if el is not None else (1, 0, (0, 0), (0.0, 0.0, 0.0))
        for Cv, xld, tdt, incl, intensity in configs:
            flags = (_lib.PATCH_INCLUSIVE if incl else 0) | (_lib.PATCH_T_U8 if tdt == torch.uint8 else 0)
            want = sr.resample(crop[:Cv], coords, c["flips"], GAIN[:Cv] if intensity else None, BIAS[:Cv] if intensity else None)

            def descs(make, order_of):
                return [make(v, c["corner"], key, c["flips"], c["mode"], order_of, k, int(el is not None), lattice[0], lattice[1], lattice[2],
                             lattice[3], None, P) for key in (None, ISO_KEY)]

            x, rest, t = _launch_spline(sets[Cv], Cv, descs(lambda *a: _sdesc(intensity, *a), 3), P, flags, xld, tdt)
            x0, _, t0 = _launch(sets[Cv], Cv, descs(_edesc, 0), P, flags, xld, tdt)
            assert (rest == 7.0).all()
            assert np.array_equal(t, t0) and np.array_equal(x == 0, x0 == 0) and not np.signbit(x[x == 0]).any(), c["name"]
            for n, (pm, fl) in enumerate((([0, 1, 2], [False] * 3), (perm, flip))):
                name = (c["name"], Cv, n)
                assert np.array_equal(_bits32(x[n]), _bits32(ds.apply_isometry(want, pm, fl))), name
                if not intensity:
                    kp = ds.apply_isometry(keep[:2], pm, fl)
                    assert wr.one_step(x[n][:2], ds.apply_isometry(x3, pm, fl))[kp].all() and kp.any() and not x[n][:2][~kp].any(), name


def test_a_batch_mixing_deformed_and_undeformed_patches(golden):
    """one launch, patch 0 with its displacement and patch 1 (another crop, another isometry) without: `elastic` differs between the
    workgroups of the launch"""
    recs = {c["name"]: (c, k) for c, k, _ in sr.records(golden("spline"))}
    c, k = recs["p12_cells3_lock2_rotated"]
    P, el = c["P"], sr.case_elastic(c)
    vol = _volume(P, 4)
    s = _set_of([vol])
    other = (1, -2, 3)
    descs = [_sdesc(True, 0, c["corner"], None, c["flips"], c["mode"], 3, k, 1, el[0], el[1], el[2], el[3], None, P),
             _sdesc(True, 0, other, ISO_KEY, (0, 1, 0), c["mode"], 3, k, 0, 1, 0, (0, 0), (0.0, 0.0, 0.0), None, P)]
    x, _, t = _launch_spline(s, 4, descs, P, 0, 4, torch.float32)
    perm, flip = ds.isometry_of_key(ISO_KEY)
    want0 = sr.spline_patch(ds.crop_zero_pad(vol[0], c["corner"], P), c["mode"], k, el, c["flips"], GAIN, BIAS)
    want1 = sr.spline_patch(ds.crop_zero_pad(vol[0], other, P), c["mode"], k, None, (0, 1, 0), GAIN, BIAS)
    assert np.array_equal(_bits32(x[0]), _bits32(want0)) and np.array_equal(_bits32(x[1]), _bits32(ds.apply_isometry(want1, perm, flip)))
    plain0 = sr.spline_patch(ds.crop_zero_pad(vol[0], c["corner"], P), c["mode"], k, None, c["flips"], GAIN, BIAS)
    assert not np.array_equal(want0, plain0) and t.any()


def test_refused_arguments_return_invalid_and_leave_the_buffers_untouched():
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd import kernels as K
    P = 8
    s = _set_of([_volume(P, 4)])
    lib = _lib.load()
    out = torch.full((9, P, P, P, 4), 3.0, device="cuda")
    t = torch.full((9, 3, P, P, P), 9, dtype=torch.uint8, device="cuda")
    need = lib.n3d_patch_spline_scratch_bytes(9, 4, P)
    scratch = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")

    def call(descs, P=P, scratch_ptr=K.ptr(scratch), nbytes=None):
        B = len(descs)
        table = (_lib.ElasticDesc * B)(*descs)
        nbytes = lib.n3d_patch_spline_scratch_bytes(B, 4, P) if nbytes is None else nbytes
        return lib.n3d_patch_gather_spline(K.ptr(s.records), len(s), 4, table, B, P, _lib.PATCH_T_U8, scratch_ptr, nbytes, K.ptr(out), 4, K.ptr(t),
                                           K.stream_ptr())

    good = _sdesc(False)
    for order in (0, 1, 2):
        bad = _sdesc(False)
        bad.w.order = order
        assert call([good, bad]) == -1 and b"order must be 3" in lib.n3d_last_error() and b"descriptor 1" in lib.n3d_last_error()
    assert call([good] * 9) == -1 and b"N3D_PATCH_ELASTIC_MAX_BATCH" in lib.n3d_last_error()
    assert call([good], P=3) == -1 and b"at least 4" in lib.n3d_last_error()
    assert call([good], nbytes=12 * 4 * P ** 3 - 1) == -1 and b"scratch" in lib.n3d_last_error()
    assert call([good], scratch_ptr=None) == -1 and b"scratch" in lib.n3d_last_error()
    # what the elastic entry checks is checked here too
    assert call([_sdesc(False, cells=0)]) == -1 and b"cells" in lib.n3d_last_error()
    assert call([_sdesc(False, mode=2)]) == -1 and b"mode" in lib.n3d_last_error()
    assert b"patch_gather_spline" in lib.n3d_last_error()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((t == 9).all()) and bool((scratch == 0x5A).all())
    # the other entry points keep refusing order 3
    table = (_lib.ElasticDesc * 1)(good)
    assert lib.n3d_patch_gather_elastic(K.ptr(s.records), len(s), 4, table, 1, P, 0, K.ptr(out), 4, None, K.stream_ptr()) == -1
    assert b"order must be 0 or 1" in lib.n3d_last_error()
    wtable = (_lib.WarpDesc * 1)(good.w)
    assert lib.n3d_patch_gather_warp(K.ptr(s.records), len(s), 4, wtable, 1, P, 0, K.ptr(out), 4, None, K.stream_ptr()) == -1
    assert b"order must be 0 or 1" in lib.n3d_last_error()
    # ... and the limits themselves are legal: 8 patches, P = 4, the exact scratch
    assert call([good] * 8) == 0
    small = _set_of([_volume(4, 4)])
    o4 = torch.full((1, 4, 4, 4, 4), 3.0, device="cuda")
    table = (_lib.ElasticDesc * 1)(_sdesc(False, elastic=0, P=4))
    assert lib.n3d_patch_gather_spline(K.ptr(small.records), 1, 4, table, 1, 4, 0, K.ptr(scratch), 12 * 4 * 64, K.ptr(o4), 4, None,
                                       K.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((out[:8] != 3.0).any()) and bool((out[8] == 3.0).all())
    want = sr.spline_patch(_volume(4, 4)[0], 0, [1.0] * 3 + [0.0] * 9)
    assert np.array_equal(_bits32(o4.permute(0, 4, 1, 2, 3).cpu().numpy()[0]), _bits32(want))


def _expected(vols, refs, augs, warps, elastics, P, inclusive):
    """the batch by the rule: crop with zero padding -> flip + spline resample + intensity (the statement) -> isometry -> labels"""
    xs, ys = [], []
    for (v, corner, key), aug, warp, el in zip(refs, augs, warps, elastics):
        vol, truth = vols[v]
        mode, k, order, flips, gain, bias = _coefficients(aug, warp)
        assert order == 3
        c = er.coordinates(P, mode, k, el)
        x = sr.resample(ds.crop_zero_pad(vol, corner, P), c, flips, gain, bias)
        y = er.resample(ds.crop_zero_pad(truth.reshape((1,) + vol.shape[1:]), corner, P), c, 0, flips)
        perm, flip = ds.isometry_of_key(IDENTITY if key is None else key)
        xs.append(ds.apply_isometry(x, perm, flip))
        ys.append(ds.apply_isometry(y, perm, flip))
    return np.asarray(xs, np.float32), ds.expand_labels(np.asarray(ys), inclusive)


def test_generator_epoch_equals_the_statement_and_carries_the_targets_of_linear():
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd.elastic import Elastic
    vols = _volumes_for_the_generator()
    s = _set_of(vols)
    P, Cv = 8, 4
    e = Elastic(cells=1, displacement=1.5, p=0.5, lock=0)
    kw = dict(indices_list=[0, 1], patch_shape=P, patch_overlap=None, batch_size=3, augment=True, affine=mga.BRATS_AFFINE,
              augment_rotation=15, augment_interpolation="spline3", augment_intensity_scale=0.1, permute=True)

    def make(**over):
        return G.Generator(volumes=s, labels=[1, 2, 4], rng=random.Random(61), np_rng=np.random.RandomState(161), augment_elastic=e,
                           **dict(kw, **over))

    gen, lin = make(), make(augment_interpolation="linear")
    bufs = (K.empty_ndhwc(3, Cv, P, P, P, s.device, torch.float32), torch.empty((3, 3, P, P, P), device=s.device))
    twin = np.random.RandomState(161)
    affine = G.check_affine(mga.BRATS_AFFINE)
    order = G.epoch_order(gen.flags, 3, random.Random(61), True, True, True, augment=(twin, 0.25, True), warp=(twin, 15, 0.1, None, Cv),
                          elastic=(twin, e))
    seen = deformed = in_place = 0
    for (x, t), (xl, tl), batch in zip(gen.epoch(out=bufs), lin.epoch(), order):
        refs = [(int(gen.candidates[b[0], 0]), tuple(int(c) for c in gen.candidates[b[0], 1:]), b[1]) for b in batch]
        augs, warps, elastics = [], [], []
        for b in batch:
            (scale, axes), (angles, gain, bias), key = b[2], b[3], b[4]
            A, sh, identity = G.resample_transform(affine, P, scale)
            augs.append((A, sh / A, identity, axes))
            warps.append((wr.warp_transform(A, sh, wr.rotation_matrix(angles), P), 3, gain, bias))
            elastics.append(None if key is None else (e.cells, e.lock, key, e.amp))
        in_place += len(refs) == 3 and x is bufs[0] and t is bufs[1]
        wx, wy = _expected(vols, refs, augs, warps, elastics, P, False)
        assert np.array_equal(_bits32(x.cpu().numpy()), _bits32(wx)) and np.array_equal(t.cpu().numpy(), wy.astype(np.float32)), refs
        assert torch.equal(t, tl) and not torch.equal(x, xl)
        seen += len(refs)
        deformed += sum(el is not None for el in elastics)
    assert seen == gen.n_patches >= 12 and next(order, None) is None and in_place >= 3 and 0 < deformed < seen
    assert (3, Cv, P) in s._spline_scratch and len(s._spline_scratch) <= 2          # one scratch per batch shape, reused


def test_a_captured_batch_replays_to_the_same_bits():
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd import kernels as K
    vols = _volumes_for_the_generator()
    s = _set_of(vols)
    P, Cv = 8, 4
    rs = np.random.RandomState(7)
    refs = [(0, (2, 1, 0), None), (1, (-1, 3, 5), ISO_KEY)]
    warps = [(G.warp_transform(np.ones(3), np.zeros(3), G.rotation_matrix(rs.uniform(-15, 15, 3)), P), 3, rs.uniform(0.9, 1.1, 4), None)
             for _ in refs]
    elastics = [(2, 0, (11, 12), 1.2), None]
    x0, t0 = s.patch_batch(refs, P, warp=warps, elastic=elastics)            # also allocates the scratch, outside the capture
    out = (K.empty_ndhwc(2, Cv, P, P, P, s.device, torch.float32), torch.empty((2, 3, P, P, P), device=s.device))
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        s.patch_batch(refs, P, out=out, warp=warps, elastic=elastics)
    for _ in range(2):
        out[0].fill_(-1.0)
        out[1].fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits32(out[0].cpu().numpy()), _bits32(x0.cpu().numpy())) and torch.equal(out[1], t0)
    assert bool((x0 != 0).any()) and bool(t0.any())
