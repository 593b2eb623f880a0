"""GPU: the signed distance transform (n3d_target_sdt, csrc/distance.hip) at the extents where its launcher changes plan.

Why.  tests/test_gpu_boundary.py holds the transform to scipy's recorded answers on four shapes whose y and x extents stop at 16: the
line kernel's load loop never takes a second trip of SDT_LOAD = 32 positions, the L rule of sdt_tshift (L << s <= SDT_STACK) never
decides a launch, and the z kernel's grid never strides.  Here the same comparison -- uint32 views against an exact host statement
(tests/_boundary_ref.py: the separable minima, or the brute-force minimum over a short list of voxels), then a second call that must
give the same bits -- runs at the shapes below.  The transform is integer-exact, so there is no tolerance anywhere in this file.

Plan table, shapes (B, C, D0, D1, D2); T = 1 << shift z columns per tile, ty from D1 (y pass), tx from D0 (x pass).  PLAN below
holds the same rows, and `_tshift`, the launcher's rule restated, asserts every ty / tx when the module is imported.
  shape                               ty tx  reaches
  (1,3,64,64,64)                       6  6  the benchmarked patch: two load chunks, T = 64 in both passes
  (1,1,128,128,32)                     5  5  the L rule decides: T = 32, four load chunks, one z tile
  (1,1,65,33,40)                       6  5  odd extents: y pass with 24 dead columns, x pass with a partial second tile; partial load
                                             chunks (33 = 32 + 1, 65 = 64 + 1)
  (1,2,257,2,5)                        3  3  T = 8
  (1,1,1024,2,4)                       2  2  the 49152-byte dynamic-LDS request (asserted below), L at the limit along x
  (1,1,2,1024,3)                       2  2  L at the limit along y
  (1,1,2,3,1024)                       6  6  a z line of 16 ballot words, 16 z tiles per line pass
  (1,1,3,2,1023) (1,1,3,2,64) (1,1,3,2,65)   6  6  the z line's last-word mask with 63, 64 and 1 valid bits
  (1,1,1024,1024,1)                    0  0  D2 = 1: T = 1, two threads per workgroup; both line extents at the limit; 1048576 lines:
                                             four trips of the z kernel's grid; reference = the points statement
  (2,3,211,209,2)                      1  1  264594 lines: the z kernel's second grid-stride trip, last workgroup with two dead waves
  (1,1,1,1,1) (1,1,7,1,1) (1,1,1,7,1)  0  0  degenerate axes
The three mid-size shapes take the full case list (empty, full, full_but_one, two_blobs, speckle 02 / 50 / 98, corner_0..7,
face_0..2, ramp, comb; at 64^3 three cases per call, as the three channels); the thin shapes take corner_*, the face along the long axis,
speckle_02 and full_but_one; the last-word-mask shapes the cases whose background words reach the mask (full, full_but_one,
speckle_98) and the far corner.  Float / byte targets, the channels-last view and the pitched output run at (1,2,65,33,40) and
(1,2,1024,2,4) -- two channels, since the channels-last view of one channel is the dense tensor; the plan is that of the table's rows.
Then: a stale workspace, a view that is not uniformly strided, the limits (B C = 65535 / 65536, an extent of 1024 / 1025), and the raw
ABI's refusals ahead of any launch.

Result on an MI355X: all 160 cases pass the unmodified library; no defect was found (the 49152-byte launch is accepted, and the limits
of include/n3d.h are those of sdt_shape_ok).  Wall time of the whole file: 16.5 s, nearly all of it the host references (0.3 - 0.5 s
for a call at 64^3 x 3, 128 x 128 x 32 or 1024 x 1024 x 1; the rest are milliseconds each).

Mutation evidence (method of tests/test_gpu_conv_exact.py: each applied alone to a scratch copy of csrc/, this file's 160 cases and the
transform tests of test_gpu_boundary.py -- test_target_sdt_equals_the_fixture, test_signed_distance_is_the_public_function: 33 cases --
run against it; none of the three changes an index, only values):
  1 load loop: chunk j0 > 0 stored at wst[u * nt] in place of wst[(j0 + u) * nt]   here: 104 fail   existing: all pass
      every case of every row with a y or x extent above 32 (64^3, 128 x 128 x 32, 65 x 33 x 40 -- empty maps included: the unloaded
      positions are read as whatever the LDS held --, 257, 1024 along x, along y, 1024^2, 211 x 209, the operand forms, the stale
      workspace); the rows whose only long axis is z, the degenerate axes and the limits pass, as they should
  2 sdt_z_kernel leaves its line loop after the first trip                          here: 11 fail    existing: all pass
      the 264594-line row, and all ten cases of 1024 x 1024 x 1: its 1048576 lines are FOUR trips of the z grid
  3 the envelope build's comparison without the two `long long` casts               here: all pass   existing: all pass
Mutation 3 changes no result, and cannot within N3D_SDT_MAX_AXIS = 1024.  Take o < p < q <= 1023 as the line positions; a finite
field value is at most 2 * 1023^2 (two earlier passes), so |w_p - w_o| (q - p) <= (2 * 1023^2 + p^2)(1023 - p), largest at p = 1:
2 139 106 298, and |w_q - w_p| (p - o) <= (3 * 1023^2 - p^2) p, largest at p = 1022: 2 141 195 266 -- both below 2^31 =
2 147 483 648, by 0.3 %.  The casts are a margin, not a necessity, and no map within the limits can tell them from their absence;
1024 x 1024 x 1 (one earlier pass: products up to 1.17e9) comes as close as a shape of testable size does, with the far-apart voxels
of _boundary_ref.sparse_points."""
import functools

import numpy as np
import pytest
import torch

import _boundary_ref as br
from _util import dev

pytestmark = pytest.mark.gpu

SDT_LOAD, SDT_STACK, MAX_AXIS, MAX_MAPS = 32, 4096, 1024, 65535      # csrc/distance.hip, include/n3d.h


def _tshift(L, D2):
    """sdt_tshift of csrc/distance.hip: the largest power of two T = 1 << s <= 64 with T * L <= SDT_STACK, no more than D2 rounded up"""
    s = 6
    while s > 0 and ((L << s) > SDT_STACK or (1 << (s - 1)) >= D2):
        s -= 1
    return s


PLAN = [      # (shape, ty, tx): the docstring's table
    ((1, 3, 64, 64, 64), 6, 6), ((1, 1, 128, 128, 32), 5, 5), ((1, 1, 65, 33, 40), 6, 5), ((1, 2, 257, 2, 5), 3, 3),
    ((1, 1, 1024, 2, 4), 2, 2), ((1, 1, 2, 1024, 3), 2, 2), ((1, 1, 2, 3, 1024), 6, 6), ((1, 1, 3, 2, 1023), 6, 6),
    ((1, 1, 3, 2, 64), 6, 6), ((1, 1, 3, 2, 65), 6, 6), ((1, 1, 1024, 1024, 1), 0, 0), ((2, 3, 211, 209, 2), 1, 1),
    ((1, 1, 1, 1, 1), 0, 0), ((1, 1, 7, 1, 1), 0, 0), ((1, 1, 1, 7, 1), 0, 0),
    ((1, 2, 65, 33, 40), 6, 5), ((1, 2, 1024, 2, 4), 2, 2),      # the operand forms: the plans of their one-channel rows
]
for _shape, _ty, _tx in PLAN:
    assert (_tshift(_shape[3], _shape[4]), _tshift(_shape[2], _shape[4])) == (_ty, _tx), _shape
    assert max(_shape[2:]) <= MAX_AXIS and _shape[0] * _shape[1] <= MAX_MAPS
    for _L, _s in ((_shape[3], _ty), (_shape[2], _tx)):
        assert _L << _s <= SDT_STACK and _L * (2 << _s) * 6 <= 49152      # the dynamic LDS of a line pass
assert 1024 * (2 << _tshift(1024, 4)) * 6 == 49152                          # (1,1,1024,2,4): the largest request there is
assert (2 * 3 * 211 * 209, -(-2 * 3 * 211 * 209 // 4) > 1 << 16, 2 * 3 * 211 * 209 % 4) == (264594, True, 2)

FULL_LIST = ("empty", "full", "full_but_one", "two_blobs", "speckle_02", "speckle_50", "speckle_98") + br.CORNERS + br.FACES + ("ramp", "comb")


@functools.lru_cache(maxsize=None)
def _case(shape3, case):
    """(t uint8, phi float32) of one map, by the separable statement; read-only"""
    t = br.make_case(case, shape3, 700 + sum(map(ord, case)))
    phi = br.phi_rule(t, *br.squared_distances_chunked(t))
    t.setflags(write=False), phi.setflags(write=False)
    return t, phi


def _maps(shape, cases):
    """(targets, phi) of `shape` (B, C, D0, D1, D2) with the named case per (b, c)"""
    assert len(cases) == shape[0] * shape[1]
    both = [_case(tuple(shape[2:]), c) for c in cases]
    return np.stack([t for t, _ in both]).reshape(shape), np.stack([f for _, f in both]).reshape(shape)


def _same_bits(got, want, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.float32
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, "%s: %d of %d voxels differ, worst |err| %.3g" % (what, bad, got.size, np.abs(got - want).max())
    return got


def _check(tn, want, what=""):
    """the dense call against `want`, and a second call that gives the same bits"""
    from nas_3d_unet_amd import kernels as K
    t = dev(tn)
    out = K.target_sdt(t)
    assert out.is_contiguous() and out.dtype == torch.float32
    got = _same_bits(out, want, what)
    assert np.array_equal(K.target_sdt(t).cpu().numpy().view(np.uint32), got.view(np.uint32)), what + ": the second call differs"


# ---- the mid-size shapes: the full case list ---------------------------------------------------------------------------------------
def test_the_benchmarked_patch_with_nested_regions():
    _check(*_maps((1, 3, 64, 64, 64), ["nested_wt", "nested_tc", "nested_et"]))


_TRIPLES = [FULL_LIST[i:i + 3] for i in range(0, 18, 3)] + [FULL_LIST[18:] + ("voxel_interior",)]


@pytest.mark.parametrize("cases", _TRIPLES, ids="+".join)
def test_the_benchmarked_patch(cases):
    _check(*_maps((1, 3, 64, 64, 64), list(cases)))


@pytest.mark.parametrize("case", FULL_LIST)
@pytest.mark.parametrize("shape", [(1, 1, 128, 128, 32), (1, 1, 65, 33, 40)], ids=["128x128x32", "65x33x40"])
def test_mid_size_shapes(shape, case):
    _check(*_maps(shape, [case]))


# ---- the thin shapes ---------------------------------------------------------------------------------------------------------------
def _thin_cases(axis):
    return br.CORNERS + ("face_%d" % axis, "speckle_02", "full_but_one")


@pytest.mark.parametrize("k", range(6))
def test_eight_columns_per_tile(k):
    cases = _thin_cases(0) + ("speckle_50",)
    _check(*_maps((1, 2, 257, 2, 5), list(cases[2 * k:2 * k + 2])))


THIN = [((1, 1, 1024, 2, 4), 0), ((1, 1, 2, 1024, 3), 1), ((1, 1, 2, 3, 1024), 2)]


@pytest.mark.parametrize("shape,case", [(s, c) for s, a in THIN for c in _thin_cases(a)], ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v[2:])))
def test_an_axis_at_the_limit(shape, case):
    _check(*_maps(shape, [case]))


@pytest.mark.parametrize("case", ["full", "full_but_one", "speckle_98", "speckle_02", "corner_4", "corner_3", "face_2", "empty"])
@pytest.mark.parametrize("D2", [1023, 64, 65])
def test_the_last_word_of_a_z_line(D2, case):
    """63, 64 and 1 valid bits: a background word whose dead bits were not masked puts a background voxel past the line's end"""
    _check(*_maps((1, 1, 3, 2, D2), [case]))


SQUARE = (1024, 1024, 1)


@functools.lru_cache(maxsize=None)
def _square(case):
    if case.startswith("sparse"):
        t, phi = br.sparse_case(case, SQUARE, 64, 31)
    else:
        t, phi = br.points_case(SQUARE, [br.corner(SQUARE, int(case[-1]))])
        assert np.array_equal(t, br.make_case(case, SQUARE, 0))
    t.setflags(write=False), phi.setflags(write=False)
    return t, phi


@pytest.mark.parametrize("case", ("sparse_fg", "sparse_bg") + br.CORNERS)
def test_one_column_per_tile_and_both_line_extents_at_the_limit(case):
    t, phi = _square(case)
    _check(t[None, None], phi[None, None], case)


def test_more_lines_than_one_trip_of_the_z_grid():
    """264594 lines = 66149 workgroups of four, the grid holds 65536: the last 613 workgroups' lines -- the end of the last map -- are a
    second trip, and the very last workgroup has two dead waves"""
    _check(*_maps((2, 3, 211, 209, 2), ["speckle_50", "two_blobs", "ramp", "comb", "speckle_02", "speckle_98"]))


@pytest.mark.parametrize("case", ["empty", "full", "speckle_50", "corner_0", "full_but_one"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 1, 1), (1, 7, 1)], ids=["1x1x1", "7x1x1", "1x7x1"])
def test_degenerate_axes(shape, case):
    _check(*_maps((1, 1) + shape, [case]))


# ---- operand forms -----------------------------------------------------------------------------------------------------------------
FORMS = {(1, 2, 65, 33, 40): ["speckle_50", "two_blobs"], (1, 2, 1024, 2, 4): ["speckle_02", "corner_5"]}


@pytest.mark.parametrize("pitched", [False, True], ids=["dense_out", "pitched_out"])
@pytest.mark.parametrize("strided", [False, True], ids=["dense_t", "strided_t"])
@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["float", "bytes"])
@pytest.mark.parametrize("shape", list(FORMS), ids=["65x33x40", "1024x2x4"])
def test_operand_forms(shape, dtype, strided, pitched):
    from nas_3d_unet_amd import kernels as K
    from test_gpu_boundary import _pitched_out, _strided_targets
    tn, want = _maps(shape, FORMS[shape])
    tn = tn.astype(dtype)
    t = _strided_targets(tn) if strided else dev(tn)
    if pitched:
        buf, out = _pitched_out(shape)
        assert K.target_sdt(t, out=out) is out
        assert float(buf[..., -1].min()) == -777.0 and float(buf[..., -1].max()) == -777.0      # the padding is untouched
    else:
        out = K.target_sdt(t)
    got = _same_bits(out, want)
    assert np.array_equal(K.target_sdt(t).cpu().numpy().view(np.uint32), got.view(np.uint32))


def test_a_result_does_not_depend_on_what_the_workspace_held():
    """one shape, so kernels.target_sdt hands every call the same workspace: fields of a dense map, then no foreground at all (every
    foreground field INF), one far voxel, no background at all"""
    from nas_3d_unet_amd import kernels as K
    shape = (1, 1, 65, 33, 40)
    ws = None
    for case in ("speckle_50", "empty", "corner_7", "full"):
        tn, want = _maps(shape, [case])
        _same_bits(K.target_sdt(dev(tn)), want, case)
        mine = K._sdt_ws[(torch.device("cuda", torch.cuda.current_device()),) + shape]
        assert ws is None or mine is ws
        ws = mine


def test_a_view_that_is_not_uniformly_strided_is_packed_first():
    from nas_3d_unet_amd import kernels as K
    rng = np.random.default_rng(8)
    wide = dev((rng.uniform(0, 1, (1, 2, 9, 10, 25)) < 0.3).astype(np.float32))
    t = wide[..., ::2]                                       # 13 voxels 2 apart in rows of 25: no single voxel stride
    assert K._bcv_strides(t) is None and not t.is_contiguous()
    want = br.signed_distance(t.cpu().numpy())
    _same_bits(K.target_sdt(t), want)
    _same_bits(K.target_sdt(t.contiguous()), want)
    _same_bits(K.target_sdt(t.to(torch.uint8)), want)


# ---- limits ------------------------------------------------------------------------------------------------------------------------
def test_the_map_count_limit():
    from nas_3d_unet_amd import _lib, kernels as K
    tn = (np.arange(MAX_MAPS) % 2).astype(np.uint8).reshape(21845, 3, 1, 1, 1)
    got = K.target_sdt(dev(tn)).cpu().numpy()
    assert got.shape == tn.shape and not got.view(np.uint32).any()      # a one-voxel map holds no voxel of the other kind: +0.0
    assert int(_lib.load().n3d_target_sdt_workspace_bytes(32768, 2, 1, 1, 1)) == 0
    with pytest.raises(K.N3DError, match="65535"):
        K.target_sdt(dev(np.zeros((32768, 2, 1, 1, 1), np.uint8)))


@pytest.mark.parametrize("axis", range(3))
def test_the_extent_limit(axis):
    from nas_3d_unet_amd import _lib, kernels as K
    lib = _lib.load()
    ext = [2, 2, 2]
    ext[axis] = MAX_AXIS
    assert int(lib.n3d_target_sdt_workspace_bytes(1, 1, *ext)) == 2 * 4 * 4 * MAX_AXIS
    ext[axis] = MAX_AXIS + 1
    assert int(lib.n3d_target_sdt_workspace_bytes(1, 1, *ext)) == 0
    with pytest.raises(K.N3DError, match="extents 1..1024"):
        K.target_sdt(dev(np.zeros((1, 1) + tuple(ext), np.uint8)))
    one = [1, 1, 1]
    one[axis] = MAX_AXIS + 1
    assert int(lib.n3d_target_sdt_workspace_bytes(1, 1, *one)) == 0
    with pytest.raises(K.N3DError, match="extents 1..1024"):
        K.target_sdt(dev(np.zeros((1, 1) + tuple(one), np.uint8)))


def test_the_raw_abi_refuses_ahead_of_any_launch():
    """a workspace one byte short: N3D_ERR_WORKSPACE (-4); a null phi: N3D_ERR_INVALID (-1); an extent of 1025: N3D_ERR_UNSUPPORTED
    (-2).  Output and workspace keep their sentinels."""
    from nas_3d_unet_amd import _lib, kernels as K
    lib = _lib.load()
    shape = (1, 1, 4, 5, 6)
    N = 4 * 5 * 6
    tn, want = _maps(shape, ["speckle_50"])
    t = dev(tn.astype(np.float32))
    need = int(lib.n3d_target_sdt_workspace_bytes(*shape))
    assert need == 2 * 4 * N
    phi = torch.full(shape, -777.0, device="cuda")
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")

    def call(out, ws_bytes, D0=4):
        return lib.n3d_target_sdt(K.ptr(t), _lib.F32, N, N, 1, 1, 1, D0, 5, 6, K.ptr(out), N, N, 1, K.ptr(ws), ws_bytes, K.stream_ptr())

    def untouched():
        torch.cuda.synchronize()
        return bool((phi == -777.0).all()) and bool((ws == 0xA5).all())

    assert call(phi, need - 1) == -4 and b"workspace too small" in lib.n3d_last_error() and untouched()
    assert call(None, need) == -1 and b"bad args" in lib.n3d_last_error() and untouched()
    assert call(phi, need, D0=MAX_AXIS + 1) == -2 and b"extents 1..1024" in lib.n3d_last_error() and untouched()
    assert call(phi, need) == 0                                                       # and the same operands, whole, are taken
    _same_bits(phi, want)
