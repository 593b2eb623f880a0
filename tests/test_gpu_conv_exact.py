"""GPU: the convolution family on CHANNEL-SLICE operands with EXACT integer data, through the C ABI wrappers (kernels.py).

Why.  The other kernel-level conv tests hand the kernels dense tensors (ld == C, start of an allocation) and assert
max|err| / max|ref| <= tol against fp32 torch.  Production is the opposite: fused._slice_view gives a cell's convs node k of the
concatenation buffer (pointer + k c, pitch n c), data gradients accumulate back into such slices, relu_src is another slice with a
pitch of its own -- and the dispatch depends on pitch and alignment.  Here every activation operand of every call is a channel slice of
a wider buffer from kernels.empty_ndhwc, and the data are small integers (_conv_exact_ref.py): every product and partial sum is an exact
fp32 number, so a correct kernel returns the fp64 reference BIT FOR BIT whatever its summation order, K-split, MFMA shape or launch
grouping.  Every assertion is torch.equal on whole buffers; there is no tolerance.  The budgets (worst-case sums < 2^24) and the
integrality of every reference are asserted on the CPU (test_conv_exact_ref_host.py).

Placements (operand -> buffer; LAYOUT below).  x: 3 nodes; y: 3 nodes behind 8 foreign channels; dy: 2 nodes; dx: 3 nodes behind 16
channels; relu_src: 3 nodes behind 24 -- five different pitches in one call (C = 4: 12, 20, 8, 28, 36), so a swapped pitch is caught.
  dense  every operand its own dense tensor (the control)
  n0     node 0                  (bf16, C = 4: 16-byte aligned)
  n1     node 1                  (fp32: neighbours on both sides; bf16, C = 4: only 8-byte aligned)
  n2     the last node           (the last record of the allocation; bf16, C = 4: the 16-byte LDS fill of a voxel runs into the next
                                  voxel and, on the last voxel, into the readable slack)
fp32 rows run dense, n1, n2; bf16 rows dense, n0, n1 and, with a 4-channel operand, n2.  Neighbour channels of INPUTS hold 28672 (a kernel
that lets one into a sum is off by thousands); OUTPUT buffers hold -12288 everywhere, also in the slice itself (an element the
kernel leaves out shows), and must come back bit-unchanged outside the slice.  View(t, ld) aliases the buffer (asserted: as_view
does not repack).

Per row: forward with bias, accumulating onto an integer base, with RELU_IN and an input gate; statistics rows (narrow set: their sum
over rows == the exact per-sample sums, no row left unwritten); data gradient plain, accumulating, with relu_src from its own slice,
with an output gate, and all three at once; weight and bias gradient with / without dbias, with RELU_IN and a gate, standalone, with
defer=False and deferred through a StepContext; conv_bwd_both; the same row on the generic path (N3D_NO_MFMA); the C >= 16 rows
with N3D_MM_BF16 (representable operands: the exact result; the +-515 set: the fp64 conv of the RNE-rounded operands).  bf16-stored
outputs are the exact value rounded to nearest even.

Rows (form: _conv_exact_ref.CASES, with the packed-weight layout ids of n3d_conv_pack_info asserted per row):
  fp32   vox64 C = 4 / 8, dilation 1 / 2 (one-plane tiles; D % 4 == 0 rows also reach vox_wgrad; 2- / 4-plane and two-wave tiles at 64^3) . vox_s2 forward with vox_up data
         gradient, C = 8 and the C = 4 two-plane tile . their transposed roles . tile16 dilation 1 / 2 . tile32 dilation 1 / 2 .
         tile16_up as data gradient and as transposed forward . gemm16 K-split 4 and K-split 16 (also the 2^3 row where one MFMA tile spans
         two samples, Ci != Co, stride 2, transposed, 1x1x1) and without K-split where no tile kernel applies (H % 4 != 0) . the gather kernel (3x3x3, 4 -> 12 stride 2, transposed parity classes) .
         the 1x1x1 streaming kernel (4 -> 12, ragged 12 -> 4, stride-2 zero-upsampling data gradient) . conv_point_kernel . depthwise
         gather (stride 1 / 2 / transposed) and the depthwise LDS-tile weight gradient . LDS-tile weight gradients 16 / 32 / 64 channels .
         conv_wgrad16 . the stride-2 MFMA weight gradient (C = 8) and its Co / 4 column-tile form (4 -> 12) . conv_bwd_both on all of them
  bf16   vox64b C = 4 dilation 1 / 2 and C = 8 dilation 1 / 2 on one-plane tiles, C = 4 4-plane tiles (dilation 1; dilation 2 with two
         waves) and C = 8 2-plane tiles at the 64^3 level . vox_s2b / vox_upb and their transposed roles . the gather and streaming forms in the storage mixes
         bf16->bf16, bf16->f32, f32->bf16 . the stride-2 MFMA weight gradient in bf16 and with fp32 x / bf16 dy
The streaming kernel needs 32^3 voxels per sample (k1_dims_ok: 32768), so the 16^3 pointwise shapes of the older lists run
conv_point_kernel / the gather kernel, as rows 30 / 31 do.  The deep-tile vox64 forms (2 / 4 planes, two waves per workgroup) need
>= 4096 tile groups: rows 38 - 40 and 44 - 46 run them at the 64^3 level itself, the smallest shape that reaches them.
Every non-depthwise row is expected to emit statistics rows, in every storage mix and on the generic path: n3d_conv_stats_rows <= 0
fails the row.

Folded launches on shared buffers: n3d_conv_fwdN with four one-wave-tile convs (C = 4, C = 8) reading the four node slices of ONE buffer,
one accumulating; n3d_conv_fwd2 / n3d_conv_bwd_data2 with two pointwise jobs (one launch, asserted through conv_pointwise_counts) and with two
small MFMA jobs whose destinations are two interleaved slices of one buffer (the third node keeps its sentinel); n3d_conv_fwdN with three
of them; n3d_conv_bwd_both2 with both dx in one buffer; n3d_conv_bwd_both of one conv.  That each call took its folded kernel -- one
launch of conv_vox_multi_kernel, conv_gemm16_pair_kernel, conv_gemm16_multi_kernel, conv_bwd16_quad_kernel, conv_bwd16_dual_kernel --
is asserted through kernels.conv_fold_counts (n3d_conv_fold_counts: launch counters of those kernels, added with this file).

Reached kernels (kernel traces of this file on an MI355X): conv_vox64_kernel<4|8, 1, 1|2, 1> and its deep tiles <4,4,1,1>, <4,4,2,2>,
<8,2,1,1>, conv_gemm16_kernel<2,1,1> / <2,2,1>, vox_wgrad_kernel with 2 and 4 staged tiles, conv_vox64b_kernel<4,4,2,2>, <4,4,1,1>,
<8,2,1,1> and <8,1,1,1>, conv_vox_s2_kernel<8,1,1> / <4,2,2>,
conv_vox_up_kernel<8,1> / <4,2>, conv_tile16_kernel<1|2, DG false|true>, conv_tile32_kernel<1|2, false|true>, conv_tile16_up_kernel<1> / <2>,
conv_gemm16_kernel<1,1,4> / <1,1,16>, conv_gemm16_pair_kernel<16>, conv_bwd16_dual_kernel<16>, conv_bwd16_quad_kernel<16>,
conv_vox_multi_kernel<4> / <8>, wgrad_tile16_kernel<1,16> / <2,16> / <1,8>, conv_wgrad16_kernel, vox_wgrad_kernel<4,1> / <8,2> (fp32 and bf16),
vox_wgrad_s2_kernel<8,1> / <4,1> in fp32, bf16 and fp32 x / bf16 dy, conv_k1_kernel and conv_k1_wgrad_kernel in every storage mix,
conv_point_kernel<4,4> / <4,8>, conv_gather_kernel, conv_wgrad_kernel, dw_gather_kernel, dw_wgrad_kernel, dw_wgrad_tile_kernel,
conv_vox64b_kernel<4|8>, conv_vox_s2b_kernel<4,2,1> / <4,1,1> / <8,1,2>, conv_vox_upb_kernel<4,1> / <8,2>.

Dense against pitched.  n3d_conv_pack_info sees geometry and flags only, so the layout ids are those of the dense call by construction;
every fp32 slice with C % 4 == 0 is 16-byte aligned, so the fp32 rows take the same kernel in every placement.  Three forms DO depend on
the placement, all by design and all exact either way:
  * bf16, C = 4, 3x3x3 stride 1: the dense placement (pitch 4, 16-byte aligned) runs the two-voxels-per-slot LDS image
    (conv_vox64b_kernel<.., P2 = true>), every node placement the one-voxel-per-slot image (P2 = false) -- which the dense
    kernel-level tests of test_gpu_bf16.py never reach.  Row 45 runs both images of the 4-plane kernel <4,4,1,1>;
  * the same dense source with >= 4096 4-plane tiles (2 x (64, 128, 128) and larger) runs 8-plane tiles (conv_vox64b_kernel<4,8,..>,
    conv_bf16.hip, vox16_conv_try).  No pitched operand can reach that form and 2 x 64^3 has 2048 tiles, so it stays with the dense
    tests of test_gpu_bf16.py (test_dense_bf16_conv_8_plane_tiles_*);
  * the 1x1x1 streaming kernel stores through its "flat" path only where dld == Cd >= 8 (the dense 4 -> 12 row), per voxel otherwise.
With extras (RELU_IN, gates, relu_src) the vox64 / vox_s2 / vox_up shapes and their bf16 forms run the gather kernel in every placement.
No kernel or eligibility bug was found: all 278 cases pass unchanged library code (9.6 s wall for the whole file on an MI355X, most of
it the fp64 references of the 64^3 rows on the host).

Mutation evidence (each applied alone to a scratch copy of csrc/, this file and the existing kernel-level conv tests -- test_gpu_conv.py,
test_gpu_pointwise.py, test_gpu_pair.py, test_gpu_step_form.py, the kernel-level part of test_gpu_bf16.py: 282 cases -- run against it):
  1 vox64_body tile loader: row address with C in place of a.sld           here: 16 fail (rows 00-03, 38-40 at n1 / n2, both fwdN)       existing: all pass
  2 conv_vox64b_kernel tile loader: voxel offset with C in place of a.sld  here: 11 fail (rows 41-44, every node placement)              existing: all pass
  3 conv_vox64b_kernel store widened to the 16-byte record (C = 4)          here: 12 fail (rows 41 / 42 / 44, all placements)             existing: 10 fail (test_gpu_bf16, dense: the spill races the next voxel's own store)
  4 n3d_conv_bwd_data hands dxld on as rld                                 here: 163 fail (every pitched / generic case with a ReLU mask) existing: all pass
  5 launch_point: the second job given the first job's source pitch        here: 1 fails (the pointwise pair)                            existing: 4 fail (test_gpu_pointwise pair tests)
  6 wgrad_tile16_kernel (fp32): the x operand rounded to bf16               here: 21 fail (rows 08-11, 14-16, all placements)             existing: 19 fail (test_gpu_conv)
  7 vox64_body: the last halo column of a tile not loaded (one tap lost)   here: 17 fail (rows 00 / 02 / 38-40, both fwdN)               existing: 8 fail (test_gpu_conv)
Mutations 1, 2 and 4 -- a pitch confused with a channel count or with another operand's pitch -- pass every older kernel-level test.
"""
import functools

import pytest
import torch

import _conv_exact_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
# operand -> (nodes of its buffer, foreign channels in front of node 0)
LAYOUT = {"x": (3, 0), "y": (3, 8), "dy": (2, 0), "dx": (3, 16), "rs": (3, 24)}
NODE = {"dense": lambda n: 0, "n0": lambda n: 0, "n1": lambda n: 1, "n2": lambda n: n - 1}


def _K():
    from nas_3d_unet_amd import kernels as K
    return K


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """a device fault ends the session: nothing more is started on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU fault, no further test is started: %s" % e, returncode=3)


def _dt(mix):
    a, b = mix.split("->") if "->" in mix else (mix, mix)
    f = {"f32": torch.float32, "bf16": torch.bfloat16}
    return f[a], f[b]


class Slot:
    """a channel slice of a wider NDHWC buffer: buf (B, Ct, D, H, W) logical, t = buf[:, c0:c0 + C], v = View(t, Ct)"""
    __slots__ = ("buf", "t", "v", "c0", "C", "fill")

    def __init__(self, buf, c0, C, fill, value=None):
        K = _K()
        self.buf, self.c0, self.C, self.fill = buf, c0, C, fill
        self.t = buf[:, c0:c0 + C]
        if value is not None:
            self.t.copy_(value.float().to(DEV).to(buf.dtype))
        self.v = K.View(self.t, buf.shape[1])
        a = K.as_view(self.t)
        assert a.t.data_ptr() == self.v.t.data_ptr() == buf.data_ptr() + c0 * buf.element_size() and a.ld == self.v.ld == buf.shape[1], \
            "as_view repacked a slice the test wants in place"


def _buffer(B, Ct, spatial, dtype, fill):
    buf = _K().empty_ndhwc(B, Ct, *spatial, torch.device(DEV), dtype)      # bf16: with its readable slack
    buf.fill_(fill)
    return buf


def _slot(name, pl, B, C, spatial, dtype, fill, value=None):
    n, front = (1, 0) if pl == "dense" else LAYOUT[name]
    return Slot(_buffer(B, front + n * C, spatial, dtype, fill), front + NODE[pl](n) * C, C, fill, value)


def _mismatch(got, want):
    bad = got != want
    idx = tuple(int(v) for v in bad.nonzero()[0])
    return "%d of %d differ, max |diff| %g, first at %s: got %r, want %r" % (
        int(bad.sum()), bad.numel(), float((got.double() - want.double()).abs()[bad].max()), idx, float(got[idx]), float(want[idx]))


def _check(fails, what, slot, want):
    """the whole buffer == its fill with the slice replaced by the exact result (in the buffer's storage type: bf16 = RNE)"""
    exp = torch.full_like(slot.buf, slot.fill)
    exp[:, slot.c0:slot.c0 + slot.C] = want.float().to(DEV).to(slot.buf.dtype)
    if not torch.equal(slot.buf, exp):
        sl = slice(slot.c0, slot.c0 + slot.C)
        inside = not torch.equal(slot.buf[:, sl], exp[:, sl])
        outside = int((slot.buf != exp).sum()) - int((slot.buf[:, sl] != exp[:, sl]).sum())
        fails.append("%s: %s%s" % (what, _mismatch(slot.buf[:, sl], exp[:, sl]) if inside else "slice exact",
                                   "; %d NEIGHBOUR elements overwritten" % outside if outside else ""))


def _eq(fails, what, got, want):
    want = want.float().to(DEV)
    if got.shape != want.shape or not torch.equal(got, want):
        fails.append("%s: %s" % (what, _mismatch(got, want)))


def _geom(c):
    K = _K()
    pad = R.padding(c.k, c.stride, c.dil)
    if c.transposed:
        return K.conv_geom(c.B, *R.out_shape(c), c.cout, c.cin, c.k, c.stride, c.dil, pad, c.depthwise)
    return K.conv_geom(c.B, *c.shape, c.cin, c.cout, c.k, c.stride, c.dil, pad, c.depthwise)


def _layouts(c):
    import ctypes as C
    from nas_3d_unet_amd import _lib
    in_dt, out_dt = _dt(c.mix)
    sb, db = (_lib.SRC_BF16 if in_dt == torch.bfloat16 else 0), (_lib.DST_BF16 if out_dt == torch.bfloat16 else 0)
    sbd, dbd = (_lib.SRC_BF16 if out_dt == torch.bfloat16 else 0), (_lib.DST_BF16 if in_dt == torch.bfloat16 else 0)     # dy -> dx
    g, out = _geom(c), []
    for data_grad, fl in ((c.transposed, sb | db), (not c.transposed, sbd | dbd)):
        lay, cdp, n = C.c_int32(), C.c_int32(), C.c_int64()
        _lib.check(_lib.load().n3d_conv_pack_info(C.byref(g), 1 if data_grad else 0, fl, C.byref(lay), C.byref(cdp), C.byref(n)), "n3d_conv_pack_info")
        out.append(lay.value)
    return tuple(out)


def _dev(t):
    return t.float().to(DEV)


def _sent(t):
    return torch.full_like(t, R.SENT_OUT)


def _placements(c):
    if c.mix == "f32":
        return ["dense", "n1", "n2"]
    return ["dense", "n0", "n1"] + (["n2"] if 4 in (c.cin, c.cout) else [])


# per row: its placements, then node 1 on the generic path (N3D_NO_MFMA) and, for the C >= 16 rows, with N3D_MM_BF16 -- in row order,
# so that the fp64 references of a row are computed once
ROWS = [(i, pl) for i, c in enumerate(R.CASES) for pl in _placements(c) + ["generic"] + (["mm_bf16"] if c.mm else [])]
IDS = [R.case_id(i) for i in range(len(R.CASES))]


def _finish(fails, where):
    torch.cuda.synchronize()
    assert not fails, "%s: integer data, so a mismatch is a bug and not rounding:\n  " % where + "\n  ".join(fails)


def _run_row(i, pl, xflags, full=True):
    K = _K()
    c = R.CASES[i]
    kind = "wide" if c.mix == "f32" else "rep"
    d, ref = R.draw(i, kind), R.reference(i, kind)
    in_dt, out_dt = _dt(c.mix)
    g, T, oshape, extras = _geom(c), c.transposed, R.out_shape(c), R.has_extras(c)
    w, b, gi, go = _dev(d["w"]), _dev(d["bias"]), _dev(d["gi"]), _dev(d["go"])
    fails = []
    mk = functools.partial(_slot, pl=pl, B=c.B)
    x = mk("x", C=c.cin, spatial=c.shape, dtype=in_dt, fill=R.SENT_IN, value=d["x"])
    dy = mk("dy", C=c.cout, spatial=oshape, dtype=out_dt, fill=R.SENT_IN, value=d["dy"])
    new_y = lambda base=None: mk("y", C=c.cout, spatial=oshape, dtype=out_dt, fill=R.SENT_OUT, value=base)
    new_dx = lambda base=None: mk("dx", C=c.cin, spatial=c.shape, dtype=in_dt, fill=R.SENT_OUT, value=base)
    # ---------------- forward
    y = new_y()
    K.conv_fwd(g, x.v, w, b, y.v, xflags, None, None, T)
    _check(fails, "y (bias)", y, ref["y"])
    y = new_y(d["base_y"])
    K.conv_fwd(g, x.v, w, b, y.v, xflags | K.ACCUMULATE, None, None, T)
    _check(fails, "y (accumulate)", y, ref["y_acc"])
    if extras:
        y = new_y()
        K.conv_fwd(g, x.v, w, None, y.v, xflags | K.RELU_IN, gi, None, False)
        _check(fails, "y (RELU_IN + in_gate)", y, ref["y_rg"])
    # ---------------- statistics rows (narrow set)
    if not c.depthwise:       # (the depthwise kernels take no statistics argument)
        dn, rn = R.draw(i, "narrow"), R.reference(i, "narrow")
        xn, y = mk("x", C=c.cin, spatial=c.shape, dtype=in_dt, fill=R.SENT_IN, value=dn["x"]), new_y()
        rows = K.conv_stats_rows(g, T, xflags, xn.v, y.v)
        # every row of the table has a shape whose forward kernel emits statistics, on the MFMA and on the generic path, in every
        # storage mix: a form that stopped emitting them would otherwise make this check vacuous
        if rows <= 0:
            fails.append("statistics: n3d_conv_stats_rows = %d, this row is expected to emit statistics rows" % rows)
        else:
            stats = torch.full((c.B, rows, c.cout, 2), float("nan"), dtype=torch.float64, device=DEV)
            K.conv_fwd(g, xn.v, _dev(dn["w"]), _dev(dn["bias"]), y.v, xflags, None, stats, T)
            _check(fails, "y (narrow set, statistics)", y, rn["y"])
            if bool(torch.isnan(stats).any()):
                fails.append("statistics: %d of %d rows left unwritten" % (int(torch.isnan(stats).any(dim=3).any(dim=2).sum()), c.B * rows))
            elif not torch.equal(stats.sum(dim=1).cpu(), rn["stats"]):
                fails.append("statistics: row sums %s" % _mismatch(stats.sum(dim=1).cpu(), rn["stats"]))
    # ---------------- data gradient
    dx = new_dx()
    K.conv_bwd_data(g, dy.v, w, dx.v, xflags, None, None, T)
    _check(fails, "dx", dx, ref["dx"])
    dx = new_dx(d["base_dx"])
    K.conv_bwd_data(g, dy.v, w, dx.v, xflags | K.ACCUMULATE, None, None, T)
    _check(fails, "dx (accumulate)", dx, ref["dx_acc"])
    rs = None
    if extras:
        rs = mk("rs", C=c.cin, spatial=c.shape, dtype=in_dt, fill=R.SENT_IN, value=d["rs"])
        dx = new_dx()
        K.conv_bwd_data(g, dy.v, w, dx.v, xflags, rs.v, None, False)
        _check(fails, "dx (relu_src)", dx, ref["dx_relu"])
        dx = new_dx()
        K.conv_bwd_data(g, dy.v, w, dx.v, xflags, None, go, False)
        _check(fails, "dx (out_gate)", dx, ref["dx_gate"])
        dx = new_dx(d["base_dx"])
        K.conv_bwd_data(g, dy.v, w, dx.v, xflags | K.ACCUMULATE, rs.v, go, False)
        _check(fails, "dx (accumulate + relu_src + out_gate)", dx, ref["dx_all"])
    # ---------------- weight / bias gradient
    want_db = True

    def wgrads(**kw):
        out = []
        dw, db = _sent(w), _sent(b)
        K.conv_bwd_weight(g, x.v, dy.v, dw, db if want_db else None, xflags, None, T, **kw)
        out += [("dw", dw, ref["dw"])] + ([("db", db, ref["db"])] if want_db else [])
        dw = _sent(w)
        K.conv_bwd_weight(g, x.v, dy.v, dw, None, xflags, None, T, **kw)
        out.append(("dw (no dbias)", dw, ref["dw"]))
        if extras:
            dw = _sent(w)
            K.conv_bwd_weight(g, x.v, dy.v, dw, None, xflags | K.RELU_IN, gi, False, **kw)
            out.append(("dw (RELU_IN + in_gate)", dw, ref["dw_rg"]))
        return out

    res = [("standalone", wgrads())]
    if full:
        ctx = K.StepContext(torch.device(DEV))
        with K.step_context(ctx):
            res.append(("defer=False", wgrads(defer=False)))
            res.append(("StepContext", wgrads()))
        ctx.flush_final()
    for tag, items in res:
        for what, got, want in items:
            _eq(fails, "%s, %s" % (what, tag), got, want)
    # ---------------- combined backward (an fp32 call; the depthwise family has no combined form)
    if c.mix == "f32" and not c.depthwise:
        dx, dw, db = new_dx(), _sent(w), _sent(b)
        K.conv_bwd_both(g, x.v, dy.v, w, dx.v, dw, None if T else db, xflags, None, None, xflags, None, T)
        _check(fails, "dx (both)", dx, ref["dx"])
        _eq(fails, "dw (both)", dw, ref["dw"])
        if not T:
            _eq(fails, "db (both)", db, ref["db"])
        if extras:
            dx, dw = new_dx(d["base_dx"]), _sent(w)
            K.conv_bwd_both(g, x.v, dy.v, w, dx.v, dw, None, xflags | K.ACCUMULATE, rs.v, go, xflags | K.RELU_IN, gi)
            _check(fails, "dx (both: accumulate + relu_src + out_gate)", dx, ref["dx_all"])
            _eq(fails, "dw (both: RELU_IN + in_gate)", dw, ref["dw_rg"])
    _finish(fails, "%s [%s] %s" % (IDS[i], c.form, pl))


@pytest.mark.parametrize("i,pl", ROWS, ids=["%s-%s" % (IDS[i], pl) for i, pl in ROWS])
def test_conv_row_is_exact(i, pl):
    """pl: a placement; "generic": the same row with N3D_NO_MFMA at node 1 (the gather / generic weight-gradient kernels, otherwise only
    tested where no MFMA kernel exists); "mm_bf16": see _run_mm_bf16"""
    from nas_3d_unet_amd import _lib
    c = R.CASES[i]
    if pl == "generic":
        _run_row(i, "n1", _lib.NO_MFMA, full=False)
    elif pl == "mm_bf16":
        _run_mm_bf16(i)
    else:
        assert _layouts(c) == c.lay, "%s: the kernel selection moved (n3d_conv_pack_info)" % IDS[i]
        _run_row(i, pl, 0)


def _run_mm_bf16(i):
    """N3D_MM_BF16 (fp32 storage, operands of the matrix products rounded to bf16 in registers).  Run 1, representable operands: the exact
    result, with and without the flag.  Run 2, the +-515 set: the fp64 conv of the RNE-rounded operands, exactly."""
    K = _K()
    c = R.CASES[i]
    g, T, oshape = _geom(c), c.transposed, R.out_shape(c)
    fails = []
    mk = functools.partial(_slot, pl="n1", B=c.B, dtype=torch.float32)
    for kind, ref, runs in (("rep", R.reference(i, "rep"), (False, True)), ("wide", R.reference_rounded(i), (True,))):
        d = R.draw(i, kind)
        w, b = _dev(d["w"]), _dev(d["bias"])
        x = mk("x", C=c.cin, spatial=c.shape, fill=R.SENT_IN, value=d["x"])
        dy = mk("dy", C=c.cout, spatial=oshape, fill=R.SENT_IN, value=d["dy"])
        for mm in runs:
            tag = "%s set, %s" % (kind, "N3D_MM_BF16" if mm else "no flag")
            y = mk("y", C=c.cout, spatial=oshape, fill=R.SENT_OUT)
            dx = mk("dx", C=c.cin, spatial=c.shape, fill=R.SENT_OUT)
            dw = _sent(w)
            with K.storage(torch.float32, mm):
                K.conv_fwd(g, x.v, w, b, y.v, 0, None, None, T)
                K.conv_bwd_data(g, dy.v, w, dx.v, 0, None, None, T)
                K.conv_bwd_weight(g, x.v, dy.v, dw, None, 0, None, T)
            _check(fails, "y (%s)" % tag, y, ref["y"])
            _check(fails, "dx (%s)" % tag, dx, ref["dx"])
            _eq(fails, "dw (%s)" % tag, dw, ref["dw"])
    _finish(fails, "%s [%s]" % (IDS[i], c.form))


# ================================================================================================ folded launches on shared buffers
def _job(name, j, **slots):
    """device operands of job j of a folded case: own pitched x / dy slots unless the caller hands shared ones"""
    c, d = R.FOLDED[name][j], R.folded_draw(name, j)
    mk = functools.partial(_slot, pl="n1", B=c.B, dtype=torch.float32)
    x = slots.get("x") or mk("x", C=c.cin, spatial=c.shape, fill=R.SENT_IN, value=d["x"])
    dy = mk("dy", C=c.cout, spatial=R.out_shape(c), fill=R.SENT_IN, value=d["dy"])
    return dict(c=c, d=d, ref=R.folded_reference(name, j), g=_geom(c), x=x, dy=dy, w=_dev(d["w"]), b=_dev(d["bias"]))


def _check_nodes(fails, what, buf, C, wants):
    """buf holds len(wants) node slices of C channels from channel 0 on, then untouched sentinel nodes"""
    exp = torch.full_like(buf, R.SENT_OUT)
    for k, wnt in enumerate(wants):
        exp[:, k * C:(k + 1) * C] = wnt.float().to(DEV)
    if not torch.equal(buf, exp):
        for k in range(buf.shape[1] // C):
            sl = slice(k * C, (k + 1) * C)
            if not torch.equal(buf[:, sl], exp[:, sl]):
                fails.append("%s, node %d%s: %s" % (what, k, "" if k < len(wants) else " (SENTINEL node)", _mismatch(buf[:, sl], exp[:, sl])))


def _folded(call):
    """run call(); -> the folded-kernel launches it made, by kind (kernels.conv_fold_counts), zero counts left out"""
    K = _K()
    before = K.conv_fold_counts()
    call()
    after = K.conv_fold_counts()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


@pytest.mark.parametrize("C", [4, 8])
def test_fwdN_four_convs_reading_node_slices_of_one_buffer(C):
    """n3d_conv_fwdN, the supernet node's form: four one-wave-tile 3x3x3 convs (stride 1 / 2, dilation 1 / 2), each reading a DIFFERENT node
    slice of the same 4-node buffer (pitch 4 C) and writing its own pitched output; the second accumulates"""
    K = _K()
    name = "fwdN C=%d" % C
    cs = R.FOLDED[name]
    xbuf = _buffer(2, 4 * C, cs[0].shape, torch.float32, R.SENT_IN)
    jobs, outs, calls, fails = [], [], [], []
    for j in range(4):
        job = _job(name, j, x=Slot(xbuf, j * C, C, R.SENT_IN, R.folded_draw(name, j)["x"]))
        acc = j == 1
        y = _slot("y", "n1" if j % 2 else "n2", 2, C, R.out_shape(job["c"]), torch.float32, R.SENT_OUT, job["d"]["base_y"] if acc else None)
        calls.append((job["g"], job["x"].v, job["w"], job["b"], y.v, K.ACCUMULATE if acc else 0, None, None, False))
        jobs.append(job); outs.append((y, job["ref"]["y_acc" if acc else "y"]))
    assert _folded(lambda: K.conv_fwdN(calls)) == {"vox_multi": 1}, "the four convs did not share one conv_vox_multi_kernel launch"
    for j, (y, want) in enumerate(outs):
        _check(fails, "y of conv %d (stride %d, dilation %d)" % (j, cs[j].stride, cs[j].dil), y, want)
    # and pairwise through n3d_conv_fwd2 (two jobs of the same launch form)
    y0 = _slot("y", "n1", 2, C, R.out_shape(cs[0]), torch.float32, R.SENT_OUT)
    y3 = _slot("y", "n2", 2, C, R.out_shape(cs[3]), torch.float32, R.SENT_OUT)
    pair = [calls[0][:4] + (y0.v,) + calls[0][5:], calls[3][:4] + (y3.v,) + calls[3][5:]]
    assert _folded(lambda: K.conv_fwd2(pair)) == {"vox_multi": 1}, "the two convs did not share one conv_vox_multi_kernel launch"
    _check(fails, "y of conv 0 (fwd2)", y0, jobs[0]["ref"]["y"])
    _check(fails, "y of conv 3 (fwd2)", y3, jobs[3]["ref"]["y"])
    _finish(fails, name)


def test_two_pointwise_jobs_into_interleaved_slices_of_one_buffer():
    """n3d_conv_fwd2 / n3d_conv_bwd_data2 with two small pointwise convs: ONE two-job launch of conv_point_kernel (counted), the
    destinations nodes 0 and 1 of one 3-node buffer -- distinct pointers, shared voxel records; node 2 keeps its sentinel"""
    K = _K()
    fails = []
    # ---- forward: 12 -> 8 with bias; 24 -> 8 stride 2 with ReLU on load (the launch shares one "transform x" switch between its jobs)
    a, b2 = _job("fwd2 pointwise", 0), _job("fwd2 pointwise", 1)
    ybuf = _buffer(2, 24, (8, 8, 8), torch.float32, R.SENT_OUT)
    ya, yb = Slot(ybuf, 0, 8, R.SENT_OUT), Slot(ybuf, 8, 8, R.SENT_OUT)
    n0 = K.conv_pointwise_counts()
    K.conv_fwd2([(a["g"], a["x"].v, a["w"], a["b"], ya.v, 0, None, None, False),
                 (b2["g"], b2["x"].v, b2["w"], None, yb.v, K.RELU_IN, _dev(b2["d"]["gi"]), None, False)])
    n1 = K.conv_pointwise_counts()
    assert (n1[0] - n0[0], n1[1] - n0[1]) == (1, 2), "the two pointwise convs did not share one launch"
    _check_nodes(fails, "y (fwd2)", ybuf, 8, [a["ref"]["y"], b2["ref"]["y_rg"]])
    # ---- data gradients: 8 <- 12 accumulating behind a ReLU mask from its own slice; 8 <- 16 stride 2 (zero-upsampling form)
    a, b2 = _job("bwd_data2 pointwise", 0), _job("bwd_data2 pointwise", 1)
    dbuf = _buffer(2, 24, (8, 8, 8), torch.float32, R.SENT_OUT)
    da, db_ = Slot(dbuf, 0, 8, R.SENT_OUT, a["d"]["base_dx"]), Slot(dbuf, 8, 8, R.SENT_OUT)
    rs = _slot("rs", "n1", 2, 8, (8, 8, 8), torch.float32, R.SENT_IN, a["d"]["rs"])
    n0 = K.conv_pointwise_counts()
    K.conv_bwd_data2([(a["g"], a["dy"].v, a["w"], da.v, K.ACCUMULATE, rs.v, _dev(a["d"]["go"]), False),
                      (b2["g"], b2["dy"].v, b2["w"], db_.v, 0, None, None, False)])
    n1 = K.conv_pointwise_counts()
    assert (n1[0] - n0[0], n1[1] - n0[1]) == (1, 2), "the two pointwise data gradients did not share one launch"
    _check_nodes(fails, "dx (bwd_data2)", dbuf, 8, [a["ref"]["dx_all"], b2["ref"]["dx"]])
    _finish(fails, "pointwise pair")


def test_two_small_mfma_jobs_into_interleaved_slices_of_one_buffer():
    """n3d_conv_fwd2 / n3d_conv_bwd_data2 / n3d_conv_bwd_both2 with two K-split-16 gemm16 jobs (64 -> 64, dilation 1 and 2, 4^3): the
    destinations are nodes 0 and 1 of one 3-node buffer, node 2 keeps its sentinel"""
    K = _K()
    fails = []
    a, b2 = _job("mfma pair", 0), _job("mfma pair", 1)
    shp = (4, 4, 4)
    ybuf = _buffer(2, 192, shp, torch.float32, R.SENT_OUT)
    ya, yb = Slot(ybuf, 0, 64, R.SENT_OUT), Slot(ybuf, 64, 64, R.SENT_OUT, b2["d"]["base_y"])
    pair = [(a["g"], a["x"].v, a["w"], a["b"], ya.v, 0, None, None, False),
            (b2["g"], b2["x"].v, b2["w"], b2["b"], yb.v, K.ACCUMULATE, None, None, False)]
    assert _folded(lambda: K.conv_fwd2(pair)) == {"gemm16_pair": 1}, "the two forward convs did not share one conv_gemm16_pair_kernel launch"
    _check_nodes(fails, "y (fwd2)", ybuf, 64, [a["ref"]["y"], b2["ref"]["y_acc"]])
    # three K-split convs through n3d_conv_fwdN (conv_gemm16_multi_kernel): all three nodes of one buffer
    ybuf = _buffer(2, 192, shp, torch.float32, R.SENT_OUT)
    ys = [Slot(ybuf, 64 * k, 64, R.SENT_OUT) for k in range(3)]
    three = [(j["g"], j["x"].v, j["w"], j["b"], ys[k].v, 0, None, None, False) for k, j in enumerate((a, b2, a))]
    assert _folded(lambda: K.conv_fwdN(three)) == {"gemm16_multi": 1}, "the three convs did not share one conv_gemm16_multi_kernel launch"
    _check_nodes(fails, "y (fwdN)", ybuf, 64, [a["ref"]["y"], b2["ref"]["y"], a["ref"]["y"]])
    # data gradients only: the first accumulates behind a ReLU mask and an output gate
    dbuf = _buffer(2, 192, shp, torch.float32, R.SENT_OUT)
    da, db_ = Slot(dbuf, 0, 64, R.SENT_OUT, a["d"]["base_dx"]), Slot(dbuf, 64, 64, R.SENT_OUT)
    rs = _slot("rs", "n1", 2, 64, shp, torch.float32, R.SENT_IN, a["d"]["rs"])
    pair = [(a["g"], a["dy"].v, a["w"], da.v, K.ACCUMULATE, rs.v, _dev(a["d"]["go"]), False),
            (b2["g"], b2["dy"].v, b2["w"], db_.v, 0, None, None, False)]
    assert _folded(lambda: K.conv_bwd_data2(pair)) == {"gemm16_pair": 1}, "the two data gradients did not share one conv_gemm16_pair_kernel launch"
    _check_nodes(fails, "dx (bwd_data2)", dbuf, 64, [a["ref"]["dx_all"], b2["ref"]["dx"]])
    # combined backward of both convs, both dx in one buffer
    dbuf = _buffer(2, 192, shp, torch.float32, R.SENT_OUT)
    da, db_ = Slot(dbuf, 0, 64, R.SENT_OUT), Slot(dbuf, 64, 64, R.SENT_OUT)
    dws = [_sent(a["w"]), _sent(b2["w"])]
    dbs = [_sent(a["b"]), _sent(b2["b"])]
    pair = [(a["g"], a["x"].v, a["dy"].v, a["w"], da.v, dws[0], dbs[0], 0, None, None, 0, None, False),
            (b2["g"], b2["x"].v, b2["dy"].v, b2["w"], db_.v, dws[1], dbs[1], 0, None, None, 0, None, False)]
    assert _folded(lambda: K.conv_bwd_both2(pair)) == {"bwd_quad": 1}, "the two backward passes did not share one conv_bwd16_quad_kernel launch"
    _check_nodes(fails, "dx (bwd_both2)", dbuf, 64, [a["ref"]["dx"], b2["ref"]["dx"]])
    for k, job in enumerate((a, b2)):
        _eq(fails, "dw of conv %d (bwd_both2)" % k, dws[k], job["ref"]["dw"])
        _eq(fails, "db of conv %d (bwd_both2)" % k, dbs[k], job["ref"]["db"])
    # combined backward of ONE conv (n3d_conv_bwd_both): data + weight gradient in one conv_bwd16_dual_kernel launch
    dx, dw, db = _slot("dx", "n2", 2, 64, shp, torch.float32, R.SENT_OUT), _sent(a["w"]), _sent(a["b"])
    one = lambda: K.conv_bwd_both(a["g"], a["x"].v, a["dy"].v, a["w"], dx.v, dw, db, 0, None, None, 0, None)
    assert _folded(one) == {"bwd_dual": 1}, "data and weight gradient did not share one conv_bwd16_dual_kernel launch"
    _check(fails, "dx (bwd_both, dual)", dx, a["ref"]["dx"])
    _eq(fails, "dw (bwd_both, dual)", dw, a["ref"]["dw"])
    _eq(fails, "db (bwd_both, dual)", db, a["ref"]["db"])
    _finish(fails, "mfma pair")
