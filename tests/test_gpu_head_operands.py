"""GPU: the fused head kernels (csrc/head.hip: head_fwd_kernel, head_bwd_kernel, head_dice_finalize_kernel) on pitched, strided and
flat-walk operands, with the exact dyadic data and the fp64 references of tests/_head_ref.py.

Every logit of every case is an exactly representable fp32 number whatever the summation order (asserted on the CPU by
tests/test_head_ref_host.py), so logits are compared with `==`; a placement or stride variant runs the same arithmetic per voxel index
as the dense contiguous call, so it is compared with torch.equal; the dense call is held to the suite's existing bounds against fp64.

A  placements: x dense / a channel slice (ld = Ci + 8, channel 4) / the last slice of its allocation; dx dense / a slice (ld = Ci + 12,
   channel 8), plain and accumulating onto an integer base; the four (x, dx) storage mixes; p / logits contiguous, channels-last with
   a guard column and a channel slice (through ctypes: the wrappers fix p's strides); float targets contiguous, channels-last, a channel
   slice; byte targets dense (the quad path on 1024 voxels), one byte into their allocation, channels-last; dp contiguous,
   channels-last, expanded with all strides 0, batch stride 0 -- over every entry point and every _loss_ref.SPECS.
B  dloss None / 1 / 0.5 / -4: a power-of-two scale commutes with every rounding of the backward pass; through autograd too.
C  the finalize's walks (_head_ref.WALKS): flat with per = 1 / 2 / 3, M > 8, BC = 64; the wave walk at BC = 68, 100 and 65 rows.
D  the weight gradient deferred through a StepContext equals the eager one.
E  refusals (host-side argument checks).          F  the layout kernels n3d_ncdhw_to_ndhwc / n3d_ndhwc_to_ncdhw.

Bounds (the suite's, unchanged): p, logits, sums 2e-6; loss 1e-6 max(1, |ref|); dx, dw, db 2e-5 (relative to the largest reference
value, _util.assert_close); bf16-stored dx: the two-sided check of test_gpu_head.test_head_bf16_storage.  The loss coefficients
(coef: k2, k0 per pair, then kb) are the fp32 factors of the gradients and are held to the gradients' 2e-5.

Results on an MI355X: all 207 cases pass the unchanged kernels (10 s wall for the whole file; the slowest cases are the B = 16 / 17
walk rows at 1.3 s each, most of it their fp64 references on the host).  No kernel or dispatch bug was found.  The one library change
is the argument check of item E: head_bwd_run checked dx's pitch but not its alignment, although the kernel stores a channel quad
per st4.  On the walk rows dw and db, which sum up to four times as many voxels as any older case, are within 5.2e-7 of fp64 (dx 2.3e-7,
sums 1.7e-8): the 2e-5 bound stands unwidened.

Mutation evidence (each mistake built alone into a scratch copy of csrc/ and loaded with N3D_LIB; this file and the older
test_gpu_head.py, test_gpu_loss.py, test_gpu_eval.py -- 115 cases -- run against it; every mistake stays inside its allocations, so the
pitch mistakes are made in the pitched layout only, where the channel count is the smaller pitch):
  1 head_fwd_kernel: CI in place of a.xld in the x address                  here: 63 fail (every test_forward_placements case: "x slice",
                                                                             "x last", "all strided"; the three autograd cases)                older: all pass
  2 head_bwd_kernel: CI in place of a.dxld in the dx store address           here: 120 fail (every test_backward_placements case: result,
                                                                             prefill left in the slice, neighbours overwritten)                 older: all pass
  3 head_bwd_kernel, COEF form: kb not multiplied by *a.dloss                here: 2 fail (test_dloss_scales_the_gradients_exactly at Co = 3:
                                                                             the two cross-entropy specs; autograd, tversky_bce)               older: all pass
  4 finalize flat walk: left = 1 instead of left = per after the first pair  here: 2 fail (test_finalize_walks per = 2 and per = 3)            older: 1 fails
                                                                             (test_gpu_eval.test_padded_twin_and_bf16_storage: the target
                                                                             counts of its 128^3 bf16 net, per = 8; every other case passes)
  5 head_bwd_kernel: the accumulate read through a.xld instead of a.dxld     here: 120 fail (every test_backward_placements case: "dx slice,
                                                                             accumulate", "x slice, dx slice, accumulate")                     older: all pass
Mutations 1, 2, 3 and 5 pass every older head, loss and evaluation test; mutation 4 passes them at per = 2 and 3 and is seen only through
one whole-net case at per = 8.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _head_ref as hr
import _loss_ref as lr
from _util import assert_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPECS = list(lr.SPECS)


def _K():
    from nas_3d_unet_amd import kernels as K
    return K


def _dt(s):
    return torch.bfloat16 if s == "bf16" else torch.float32


def _cid(c):
    return "ci%d-co%d-%s" % (c.ci, c.co, "x".join(map(str, c.shape)))


def _specs(c):
    """(index, spec) of the loss forms built for the case: the cross-entropy term is built for three channels only"""
    return [(i, s) for i, s in enumerate(SPECS) if c.co == 3 or s.bce_weight == 0]


@functools.lru_cache(maxsize=2)
def _dev_operands(c):
    d = hr.draw(c)
    return {k: v.to(DEV) for k, v in d.items()}


def _view(v):
    """kernels.as_view hands a pitched channel slice on untouched.  The one form it repacks -- bf16, four channels, no 8 bytes of
    slack behind the last voxel (the 16-byte tile fills of the bf16 convs) -- the head reads 8 bytes at a time: it gets the slice itself."""
    K = _K()
    xv = K.as_view(v)
    if xv.t.data_ptr() != v.data_ptr():
        assert v.dtype == torch.bfloat16 and v.shape[1] == 4, "as_view repacked a pitched slice"
        xv = K.View(v, K._pitch_of(v))
    assert xv.ld == v.stride(4)
    return xv


def _x_forms(c, xdt):
    """{name: (View, buffer or None, (off, C))}"""
    K = _K()
    xs = _dev_operands(c)["x"].to(_dt(xdt))
    dense = K.empty_ndhwc(c.B, c.ci, *c.shape, DEV, _dt(xdt))
    dense.copy_(xs)
    out = {"dense": (K.as_view(dense), None, None)}
    for name, pl in (("slice", hr.X_SLICE), ("last", hr.X_LAST)):
        buf, v = hr.place_ndhwc(xs, pl["off"], pl["extra"])
        out[name] = (_view(v), buf, pl["off"])
    assert out["dense"][0].ld == c.ci and out["slice"][0].ld == c.ci + 8
    return out


def _t_forms(c):
    """{name: target tensor}: float contiguous / channels-last / channel slice, and for three channels the byte forms"""
    t = _dev_operands(c)["t"]
    out = {"dense": t, "cl": hr.place_ndhwc(t, 0, 1)[1], "slice": hr.place_ncdhw(t, 1, 1)[1]}
    if c.co == 3:
        tb = t.to(torch.uint8)
        off1 = hr.place_bytes_offset(tb)[1]
        assert tb.data_ptr() % 4 == 0 and off1.data_ptr() % 4 == 1
        out.update({"u8": tb, "u8+1": off1, "u8cl": hr.place_ndhwc(tb, 0, 1, fill=255)[1]})
    return out


class _POut:
    """an output tensor for p or logits in one of the strided forms, prefilled with the output sentinel"""

    def __init__(self, c, form):
        self.form, self.co = form, c.co
        if form == "cl":          # channels-last: psc = 1, psv = Co + 1, one guard column
            self.buf = hr.ndhwc_buffer(c.B, c.shape, c.co + 1, hr.SENT_OUT, device=DEV)
            self.t = hr.channel_slice(self.buf, 0, c.co)
        else:                     # channels 1 .. Co of a (B, Co + 2, ...) NCDHW tensor
            self.buf = torch.full((c.B, c.co + 2) + tuple(c.shape), hr.SENT_OUT, device=DEV)
            self.t = self.buf[:, 1:1 + c.co]

    def problems(self):
        out = []
        if not hr.no_prefill_left(self.t):
            out.append("prefill left in the slice")
        ok = hr.outside_unchanged(self.buf, 0, self.co, hr.SENT_OUT) if self.form == "cl" else \
            bool((self.buf[:, 0] == hr.SENT_OUT).all() and (self.buf[:, -1] == hr.SENT_OUT).all())
        if not ok:
            out.append("guard overwritten")
        return out


def _raw_fwd(kind, xv, w, b, gate, t, p, z=None, spec=None, acc=None):
    """n3d_head_fwd / _loss_fwd / _eval / _loss_eval through ctypes with p's (and the logits') own strides; returns (sums, coef, loss)"""
    K = _K()
    from nas_3d_unet_amd import _lib
    lib = _lib.load()
    h = K._head_desc(xv, w, b, gate, t=t)
    co = int(w.shape[0])
    ps = K._bcv_strides(p)
    ts = K._bcv_strides(t) if t is not None else (0, 0, 0)
    if z is not None:
        assert K._bcv_strides(z) == ps
    S = 4 if spec is not None and spec.bce_weight > 0 else 3
    rows = int(lib.n3d_head_rows(xv.N))
    f64 = dict(dtype=torch.float64, device=DEV)
    partial, hpartial = torch.empty((xv.B, co, rows, S), **f64), torch.empty((xv.B, co, rows, 2), **f64)
    sums = torch.empty((xv.B, co, S), **f64)
    coef = torch.empty(2 * xv.B * co + 1, dtype=torch.float32, device=DEV)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    P, st = K.ptr, K.stream_ptr()
    l = K.loss_record(spec) if spec is not None else None
    if kind == "fwd":
        e = lib.n3d_head_fwd(C.byref(h), P(p), ps[0], ps[1], ps[2], P(z), P(t), ts[0], ts[1], ts[2], hr.DICE_SMOOTH, P(partial), P(sums), P(loss), st)
    elif kind == "loss":
        e = lib.n3d_head_loss_fwd(C.byref(h), C.byref(l), P(p), ps[0], ps[1], ps[2], P(z), P(t), ts[0], ts[1], ts[2], P(partial), P(sums), P(coef),
                                  P(loss), st)
    elif kind == "eval":
        e = lib.n3d_head_eval(C.byref(h), P(p), ps[0], ps[1], ps[2], P(t), ts[0], ts[1], ts[2], hr.DICE_SMOOTH, 0.5, P(partial), P(hpartial), P(sums),
                              P(loss), P(acc), st)
    else:
        e = lib.n3d_head_loss_eval(C.byref(h), C.byref(l), P(p), ps[0], ps[1], ps[2], P(t), ts[0], ts[1], ts[2], 0.5, P(partial), P(hpartial), P(sums),
                                   P(loss), P(acc), st)
    _lib.check(e, "n3d_head_" + kind)
    return sums, coef, loss


def _forward_all(c, xv, t, gated=True, pform=None, fails=None, tag=""):
    """every forward entry point on one operand configuration: {name: tensor}.  pform: None (the wrappers' contiguous p) or a strided
    form of p / logits through ctypes.  The evaluation forms take no gate."""
    K = _K()
    d = _dev_operands(c)
    w, b = d["w"], d["bias"]
    gate = d["gate"] if gated else None
    out = {}

    def outs(n):
        ts = [_POut(c, pform) for _ in range(n)]
        return ts

    def note(name, ts):
        for o in ts:
            for pr in o.problems():
                fails.append("%s %s: %s" % (tag, name, pr))

    if t.dtype == torch.float32:      # (the plain mode reads no targets: run it once per x / p form)
        if pform is None:
            out["plain.p"], out["plain.z"], _, _ = K.head_fwd(xv, w, b, gate, None, want_logits=True)
        else:
            po = outs(2)
            _raw_fwd("fwd", xv, w, b, gate, None, po[0].t, po[1].t)
            out["plain.p"], out["plain.z"] = po[0].t, po[1].t
            note("plain", po)
    if pform is None:
        out["dice.p"], out["dice.z"], out["dice.sums"], out["dice.loss"] = K.head_fwd(xv, w, b, gate, t, hr.DICE_SMOOTH, want_logits=True)
    else:
        po = outs(2)
        out["dice.sums"], _, out["dice.loss"] = _raw_fwd("fwd", xv, w, b, gate, t, po[0].t, po[1].t)
        out["dice.p"], out["dice.z"] = po[0].t, po[1].t
        note("dice", po)
    for i, spec in _specs(c):
        n = "loss%d" % i
        if pform is None:
            out[n + ".p"], out[n + ".z"], out[n + ".sums"], out[n + ".coef"], out[n + ".loss"] = K.head_loss_fwd(xv, w, b, gate, t, spec, want_logits=True)
        else:
            po = outs(2)
            out[n + ".sums"], out[n + ".coef"], out[n + ".loss"] = _raw_fwd("loss", xv, w, b, gate, t, po[0].t, po[1].t, spec)
            out[n + ".p"], out[n + ".z"] = po[0].t, po[1].t
            note(n, po)
    for n, spec in [("eval", None)] + [("leval%d" % i, s) for i, s in _specs(c)]:
        acc = K.eval_acc(c.co, DEV)
        if pform is None:
            if spec is None:
                out[n + ".loss"], out[n + ".p"] = K.head_eval(xv, w, b, t, acc, hr.DICE_SMOOTH, want_p=True)
            else:
                out[n + ".loss"], out[n + ".p"] = K.head_loss_eval(xv, w, b, t, acc, spec, want_p=True)
        else:
            po = outs(1)
            _, _, out[n + ".loss"] = _raw_fwd("eval" if spec is None else "leval", xv, w, b, None, t, po[0].t, None, spec, acc)
            out[n + ".p"] = po[0].t
            note(n, po)
        out[n + ".acc"] = acc
    return out


def _same(fails, tag, got, want):
    for k, v in got.items():
        if not torch.equal(v, want[k]):
            fails.append("%s: %s differs from the dense contiguous call" % (tag, k))


def _loss_ok(got, ref):
    got, ref = float(got), float(ref)
    assert abs(got - ref) <= 1e-6 * max(1.0, abs(ref)), (got, ref)


def _coef_ref(cl):
    return torch.cat([torch.stack([cl.k2, cl.k0], dim=-1).reshape(-1), torch.tensor([cl.kb], dtype=torch.float64)])


def _acc_ok(acc, loss_values, refs, c):
    """the accumulator after the batches: counts exact, the loss sum the sum of the returned fp32 losses, the per-sample hard Dice sums
    the same fp64 operations in the same order (held to 1e-12: the division)"""
    z, _ = hr.logits(c, False)
    batches = []
    for lv, tt in zip(loss_values, refs):
        I, P = hr.hard_sums(z, tt)
        batches.append((lv, I.numpy(), P.numpy(), tt.double().sum((2, 3, 4)).numpy()))
    want = hr.eval_accumulator(batches, c.co)
    got = acc.cpu().numpy()
    per_g, per_w = got[4:].reshape(-1, 4), want[4:].reshape(-1, 4)
    assert np.array_equal(got[:4], want[:4]), (got[:4], want[:4])
    assert np.array_equal(per_g[:, :3], per_w[:, :3]), "hard sums / target sums are exact integers"
    assert np.abs(per_g[:, 3] - per_w[:, 3]).max() <= 1e-12 * len(batches) * c.B


def _forward_vs_fp64(c, out):
    """the dense contiguous call against fp64"""
    t = hr.draw(c)["t"]
    zg, _ = hr.logits(c, True)
    zu, _ = hr.logits(c, False)
    names = ["plain", "dice"] + ["loss%d" % i for i, _ in _specs(c)]
    for n in names:
        assert torch.equal(out[n + ".z"].double().cpu(), zg), n + ": logits are exact"
        assert_close(out[n + ".p"], torch.sigmoid(zg), 2e-6, n + ".p")
    for n, spec in [("dice", hr.DICE)] + [("loss%d" % i, s) for i, s in _specs(c)]:
        cl = hr.reference(c, spec, True, False, False).c
        S = out[n + ".sums"].shape[-1]
        assert S == (4 if spec.bce_weight > 0 else 3)
        assert_close(out[n + ".sums"], cl.sums[..., :S], 2e-6, n + ".sums")
        assert torch.equal(out[n + ".sums"][..., 2].cpu(), t.double().sum((2, 3, 4))), n + ": target sums are exact"
        _loss_ok(out[n + ".loss"], cl.loss)
        if n != "dice":
            assert_close(out[n + ".coef"], _coef_ref(cl), 2e-5, n + ".coef")
    for n, spec in [("eval", hr.DICE)] + [("leval%d" % i, s) for i, s in _specs(c)]:
        cl = hr.reference(c, spec, False, False, False).c
        assert_close(out[n + ".p"], torch.sigmoid(zu), 2e-6, n + ".p")
        _loss_ok(out[n + ".loss"], cl.loss)
        _acc_ok(out[n + ".acc"], [float(out[n + ".loss"])], [t], c)


# ---- A: placements, forward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdt", ["f32", "bf16"])
@pytest.mark.parametrize("c", hr.PLACE_CASES, ids=_cid)
def test_forward_placements(c, xdt):
    xf, tf = _x_forms(c, xdt), _t_forms(c)
    fails = []
    dense = _forward_all(c, xf["dense"][0], tf["dense"])
    _forward_vs_fp64(c, dense)
    for xn in ("slice", "last"):
        xv, buf, off = xf[xn]
        before = buf.clone()
        _same(fails, "x " + xn, _forward_all(c, xv, tf["dense"]), dense)
        assert torch.equal(buf, before)
    for tn, t in tf.items():
        if tn != "dense":
            got = _forward_all(c, xf["dense"][0], t)
            _same(fails, "t " + tn, got, dense)
    for pform in ("cl", "slice"):
        _same(fails, "p " + pform, _forward_all(c, xf["dense"][0], tf["dense"], pform=pform, fails=fails, tag="p " + pform), dense)
    # everything strided at once
    _same(fails, "all strided", _forward_all(c, xf["slice"][0], tf["cl"], pform="cl", fails=fails, tag="all strided"), dense)
    if c.co == 3:
        _same(fails, "all strided, bytes", _forward_all(c, xf["last"][0], tf["u8+1"], pform="slice", fails=fails, tag="all strided, bytes"), dense)
    assert not fails, "\n".join(fails)


# ---- A: placements, backward -----------------------------------------------------------------------------------------------
def _dx_make(c, ddt, form, base=None):
    """a dx tensor prefilled with the output sentinel (or holding the accumulate base): (View, problems())"""
    K = _K()
    dt = _dt(ddt)
    if form == "dense":
        t = K.empty_ndhwc(c.B, c.ci, *c.shape, DEV, dt)
        t.fill_(hr.SENT_OUT) if base is None else t.copy_(base)
        return K.as_view(t), (lambda: [] if base is not None or hr.no_prefill_left(t) else ["prefill left in dx"])
    pl = hr.DX_SLICE
    buf = hr.ndhwc_buffer(c.B, c.shape, c.ci + pl["extra"], hr.SENT_OUT, dt, DEV)
    v = hr.channel_slice(buf, pl["off"], c.ci)
    if base is not None:
        v.copy_(base)

    def problems():
        out = [] if hr.outside_unchanged(buf, pl["off"], c.ci, hr.SENT_OUT) else ["dx buffer changed outside its slice"]
        if base is None and not hr.no_prefill_left(v):
            out.append("prefill left in dx")
        return out

    xv = _view(v)
    assert xv.ld == c.ci + pl["extra"]
    return xv, problems


def _backward_all(c, xv, ddt, dxform, fwd, t=None, dp=None, accumulate=False, entries=None, dloss=None, fails=None, tag=""):
    """the backward entry points on one operand configuration: {entry.dx / .dw / .db: tensor}.  fwd: the dense forward's sums / coef."""
    K = _K()
    d = _dev_operands(c)
    w, b, gate = d["w"], d["bias"], d["gate"]
    base = hr.draw_dp(c)[1].to(DEV) if accumulate else None
    out = {}
    for e in entries:
        dx, problems = _dx_make(c, ddt, dxform, base)
        dw, db = torch.full_like(w, hr.SENT_OUT), torch.full_like(b, hr.SENT_OUT)
        if e == "dp":
            K.head_bwd(xv, w, b, gate, dx, dw, db, dp=dp, accumulate=accumulate)
        elif e == "dice":
            K.head_bwd(xv, w, b, gate, dx, dw, db, t=t, sums=fwd["dice.sums"], dloss=dloss, smooth=hr.DICE_SMOOTH, accumulate=accumulate)
        else:
            K.head_loss_bwd(xv, w, b, gate, dx, dw, db, t, fwd[e + ".coef"], dloss=dloss, accumulate=accumulate)
        for pr in problems():
            fails.append("%s %s: %s" % (tag, e, pr))
        if not (hr.no_prefill_left(dw) and hr.no_prefill_left(db)):
            fails.append("%s %s: prefill left in dw / db" % (tag, e))
        out[e + ".dx"], out[e + ".dw"], out[e + ".db"] = dx.t, dw, db
    return out


def _bf16_two_sided(got, ref, what):
    """test_gpu_head.test_head_bf16_storage's check of a bf16-stored gradient"""
    ref = ref.float()
    assert_close(got.float(), ref, 2.0 ** -8, what)
    assert torch.equal(got.cpu(), ref.bfloat16()) or float((got.float().cpu() - ref.bfloat16().float()).abs().max()) <= float(ref.abs().max()) * 2.0 ** -7, what


def _backward_ref(c, e):
    if e == "dp":
        return hr.reference_dp(c)
    r = hr.reference(c, hr.DICE if e == "dice" else SPECS[int(e[4:])])
    return r.dx, r.dw, r.db


@pytest.mark.parametrize("xdt,ddt", hr.STORAGE)
@pytest.mark.parametrize("c", hr.PLACE_CASES, ids=_cid)
def test_backward_placements(c, xdt, ddt):
    xf, tf = _x_forms(c, xdt), _t_forms(c)
    xd = xf["dense"][0]
    fwd = _forward_all(c, xd, tf["dense"])
    dp, base = (v.to(DEV) for v in hr.draw_dp(c))
    loss_entries = ["dice"] + ["loss%d" % i for i, _ in _specs(c)]
    entries = ["dp"] + loss_entries
    fails = []
    run = functools.partial(_backward_all, c, fails=fails)
    dense = run(xd, ddt, "dense", fwd, t=tf["dense"], dp=dp, entries=entries, tag="dense")
    # the dense call against fp64
    for e in entries:
        dxr, dwr, dbr = _backward_ref(c, e)
        if ddt == "bf16":
            _bf16_two_sided(dense[e + ".dx"], dxr, e + ".dx (bf16)")
        else:
            assert_close(dense[e + ".dx"], dxr, 2e-5, e + ".dx")
        assert_close(dense[e + ".dw"], dwr, 2e-5, e + ".dw")
        assert_close(dense[e + ".db"], dbr, 2e-5, e + ".db")
    dense_acc = run(xd, ddt, "dense", fwd, t=tf["dense"], dp=dp, accumulate=True, entries=entries, tag="dense accumulate")
    for e in entries:
        if ddt == "f32":      # one fp32 add of the integer base onto the plain result
            assert torch.equal(dense_acc[e + ".dx"], dense[e + ".dx"] + base), e + ": accumulate"
        else:
            _bf16_two_sided(dense_acc[e + ".dx"], base.double().cpu() + _backward_ref(c, e)[0], e + ".dx accumulate (bf16)")
        assert torch.equal(dense_acc[e + ".dw"], dense[e + ".dw"]) and torch.equal(dense_acc[e + ".db"], dense[e + ".db"])
    # placements of x and dx (the accumulate read runs where x's pitch is not above dx's)
    for xn in ("slice", "last"):
        _same(fails, "x " + xn, run(xf[xn][0], ddt, "dense", fwd, t=tf["dense"], dp=dp, entries=entries, tag="x " + xn), dense)
    _same(fails, "dx slice", run(xd, ddt, "slice", fwd, t=tf["dense"], dp=dp, entries=entries, tag="dx slice"), dense)
    _same(fails, "dx slice, accumulate", run(xd, ddt, "slice", fwd, t=tf["dense"], dp=dp, accumulate=True, entries=entries, tag="dx slice acc"), dense_acc)
    _same(fails, "x slice, dx slice", run(xf["slice"][0], ddt, "slice", fwd, t=tf["cl"], dp=dp, entries=entries, tag="x, dx slices"), dense)
    _same(fails, "x slice, dx slice, accumulate",
          run(xf["slice"][0], ddt, "slice", fwd, t=tf["slice"], dp=dp, accumulate=True, entries=entries, tag="x, dx slices acc"), dense_acc)
    # targets
    for tn, t in tf.items():
        if tn != "dense":
            got = run(xd, ddt, "dense", fwd, t=t, entries=loss_entries, tag="t " + tn)
            _same(fails, "t " + tn, got, dense)
    # dp: channels-last on the same values; expanded (what p.sum().backward() hands on) and batch-stride-0 against their dense copies
    _same(fails, "dp channels-last", run(xd, ddt, "dense", fwd, dp=hr.place_ndhwc(dp, 0, 1)[1], entries=["dp"], tag="dp cl"), dense)
    K = _K()
    for name, dpe in (("expanded", torch.full((), 0.375, device=DEV).expand(dp.shape)), ("batch stride 0", dp[:1].expand(dp.shape))):
        assert (K._bcv_strides(dpe) == (0, 0, 0)) == (name == "expanded") and K._bcv_strides(dpe)[0] == 0
        want = run(xd, ddt, "dense", fwd, dp=dpe.contiguous(), entries=["dp"], tag="dp dense copy")
        _same(fails, "dp " + name, run(xf["slice"][0], ddt, "slice", fwd, dp=dpe, entries=["dp"], tag="dp " + name), want)
    assert not fails, "\n".join(fails)


# ---- B: dloss ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [hr.DLOSS_CASE, hr.DLOSS_CASE4], ids=_cid)
def test_dloss_scales_the_gradients_exactly(c):
    xd, t = _x_forms(c, "f32")["dense"][0], _dev_operands(c)["t"]
    fwd = _forward_all(c, xd, t)
    entries = ["dice"] + ["loss%d" % i for i, _ in _specs(c)]
    fails = []
    res = {}
    for dl in hr.DLOSS:
        dlt = None if dl is None else torch.tensor(dl, dtype=torch.float32, device=DEV)
        res[dl] = _backward_all(c, xd, "f32", "dense", fwd, t=t, entries=entries, dloss=dlt, fails=fails, tag="dloss %s" % dl)
    for dl in hr.DLOSS[1:]:
        for k, v in res[dl].items():
            if not torch.equal(v, res[None][k] * dl):
                fails.append("dloss %s: %s is not %s times the dloss = NULL result" % (dl, k, dl))
    assert not fails, "\n".join(fails)
    for dl in hr.DLOSS:
        for e in entries:
            for k, ref in zip((".dx", ".dw", ".db"), hr.scaled(_backward_ref(c, e), dl)):
                assert_close(res[dl][e + k], ref, 2e-5, "dloss %s %s%s" % (dl, e, k))


def _head_module(c):
    from nas_3d_unet_amd import prim_ops
    head = torch.nn.Sequential(prim_ops.ConvOps(c.ci, c.co, kernel_size=1, dropout_rate=0.1, ops_order="weight"), torch.nn.Sigmoid()).cuda().eval()
    d = _dev_operands(c)
    with torch.no_grad():
        head[0].conv.weight.copy_(d["w"])
        head[0].conv.bias.copy_(d["bias"])
    return head


@pytest.mark.parametrize("what", ["dice", "tversky_bce", "sum"])
def test_scaled_loss_and_expanded_dp_through_autograd(what):
    """(0.5 * loss).backward() as in gradient accumulation, and run(...).sum().backward() with its expanded dp, on a pitched x slice
    whose gradient lands in the slice of the buffer's gradient (eval mode: no gate)"""
    from nas_3d_unet_amd import head as H
    from nas_3d_unet_amd.loss import TverskyBCELoss
    K = _K()
    c = hr.DLOSS_CASE
    head = _head_module(c)
    d = _dev_operands(c)
    pl = hr.X_SLICE
    buf, v = hr.place_ndhwc(d["x"], pl["off"], pl["extra"])
    assert K.as_view(v).t.data_ptr() == v.data_ptr() and H.fusable(head, v)
    buf.requires_grad_(True)
    xs = hr.channel_slice(buf, pl["off"], c.ci)
    if what == "sum":
        p = H.run(head, xs)
        assert_close(p.detach(), torch.sigmoid(hr.logits(c, False)[0]), 2e-6, "p")
        p.sum().backward()
        ref = hr.reference_dp(c, False, True)
    else:
        spec = hr.DICE if what == "dice" else lr.Spec(0.3, 0.7, 0.75, 0.5)
        loss, _ = H.run_loss(head, xs, d["t"], hr.DICE_SMOOTH) if what == "dice" else H.run_loss(head, xs, d["t"], loss=TverskyBCELoss(*spec))
        _loss_ok(loss.detach(), hr.reference(c, spec, False).c.loss)
        (0.5 * loss).backward()
        r = hr.reference(c, spec, False)
        ref = hr.scaled((r.dx, r.dw, r.db), 0.5)
    g = buf.grad
    assert hr.outside_unchanged(g, pl["off"], c.ci, 0.0), "gradient outside the slice"
    assert_close(hr.channel_slice(g, pl["off"], c.ci), ref[0], 2e-5, "dx")
    assert_close(head[0].conv.weight.grad, ref[1], 2e-5, "dw")
    assert_close(head[0].conv.bias.grad, ref[2], 2e-5, "db")


# ---- C: the finalize's walks -------------------------------------------------------------------------------------------------
def _err(got, ref):
    ref = ref.to(DEV)
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp(min=1e-30))


@pytest.mark.parametrize("wk", hr.WALKS, ids=lambda wk: "%s-B%d-co%d" % ("x".join(map(str, wk.shape)), wk.B, wk.co))
def test_finalize_walks(wk):
    K = _K()
    from nas_3d_unet_amd import _lib
    c = hr.walk_case(wk)
    N = int(np.prod(c.shape))
    assert int(_lib.load().n3d_head_rows(N)) == wk.rows and hr.walk_reach(N, c.B, c.co) == (wk.rows, wk.per, wk.BC, wk.M)
    d = hr.draw(c)
    x = K.empty_ndhwc(c.B, c.ci, *c.shape, DEV, torch.float32)
    x.copy_(d["x"].to(DEV))
    xv = K.as_view(x)
    w, b, t = d["w"].to(DEV), d["bias"].to(DEV), d["t"].to(DEV)
    z, _ = hr.logits(c, False)
    forms = [("dice", hr.DICE), ("tversky", hr.TVERSKY)] + ([("bce", hr.BCE)] if c.co == 3 else [])
    for name, spec in forms:
        r = hr.reference(c, spec, False)
        S = 4 if spec.bce_weight > 0 else 3
        dx = K.as_view(K.empty_ndhwc(c.B, c.ci, *c.shape, DEV, torch.float32))
        dw, db = torch.empty_like(w), torch.empty_like(b)
        if name == "dice":
            p, logits, sums, loss = K.head_fwd(xv, w, b, None, t, hr.DICE_SMOOTH, want_logits=True)
            assert bool((logits.double() == z.to(DEV)).all()), "logits are exact"
            K.head_bwd(xv, w, b, None, dx, dw, db, t=t, sums=sums, smooth=hr.DICE_SMOOTH)
        else:
            p, _, sums, coef, loss = K.head_loss_fwd(xv, w, b, None, t, spec)
            assert _err(coef, _coef_ref(r.c)) <= 2e-5, name + ".coef"
            K.head_loss_bwd(xv, w, b, None, dx, dw, db, t, coef)
        errs = dict(sums=_err(sums, r.c.sums[..., :S]), dx=_err(dx.t, r.dx), dw=_err(dw, r.dw), db=_err(db, r.db))
        print("%s %s: loss %.9g ref %.9g  " % (wk.what, name, float(loss), float(r.c.loss)) + "  ".join("%s %.3e" % kv for kv in errs.items()))
        assert sums.shape[-1] == S and errs["sums"] <= 2e-6, (name, errs)
        assert torch.equal(sums[..., 2].cpu(), d["t"].double().sum((2, 3, 4))), name + ": target sums are exact"
        _loss_ok(loss, r.c.loss)
        assert errs["dx"] <= 2e-5 and errs["dw"] <= 2e-5 and errs["db"] <= 2e-5, (name, errs)
    if c.co != 3:
        return
    # the evaluation forms, two batches (t, then 1 - t on the same x) into one accumulator: the hard sums take the same walk
    t2h = hr.second_targets(c)
    t2 = t2h.to(DEV)
    for name, spec in forms:
        acc = K.eval_acc(c.co, DEV)
        got = []
        for k, tt in enumerate((t, t2)):
            if name == "dice":
                loss = K.head_eval(xv, w, b, tt, acc, hr.DICE_SMOOTH)[0]
            else:
                loss = K.head_loss_eval(xv, w, b, tt, acc, spec)[0]
            _loss_ok(loss, hr.reference(c, spec, False, k == 1, False).c.loss)
            got.append(float(loss))
        _acc_ok(acc, got, [d["t"], t2h], c)


# ---- D: the deferred weight gradient -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [hr.DLOSS_CASE, hr.PLACE_CASES[-1]], ids=_cid)
def test_deferred_weight_gradient_equals_the_eager_one(c):
    """under a StepContext head_bwd / head_loss_bwd return an n3d_final_job instead of finalizing (the trainers' form): flush_final must
    leave the eager call's bits"""
    K = _K()
    xd, t = _x_forms(c, "f32")["dense"][0], _dev_operands(c)["t"]
    fwd = _forward_all(c, xd, t)
    dp = hr.draw_dp(c)[0].to(DEV)
    entries = ["dp", "dice"] + ["loss%d" % i for i, _ in _specs(c)]
    fails = []
    eager = _backward_all(c, xd, "f32", "dense", fwd, t=t, dp=dp, entries=entries, fails=fails, tag="eager")
    ctx = K.StepContext(torch.device(DEV))
    K_fails = []
    with K.step_context(ctx):
        deferred = _backward_all(c, xd, "f32", "dense", fwd, t=t, dp=dp, entries=entries, fails=K_fails, tag="deferred")
        assert len(ctx.final) == len(entries), "every call must hand back a final job"
    torch.cuda.synchronize()
    assert all("dw / db" in f for f in K_fails) and len(K_fails) == len(entries), "dw / db must stay unwritten until flush_final: %s" % K_fails
    ctx.flush_final()
    _same(fails, "deferred", deferred, eager)
    assert not fails, "\n".join(fails)


# ---- E: refusals -----------------------------------------------------------------------------------------------------------
def test_refusals():
    """host-side argument checks: nothing is launched"""
    K = _K()
    ci, co, shape = 4, 4, (1, 2, 4)
    f32 = dict(dtype=torch.float32, device=DEV)
    w, b = torch.zeros((co, ci, 1, 1, 1), **f32), torch.zeros(co, **f32)
    # B * Co > 256 in the evaluation forms
    x = K.as_view(K.zeros_ndhwc(65, ci, *shape, DEV, torch.float32))
    t = torch.zeros((65, co) + shape, **f32)
    with pytest.raises(K.N3DError, match=r"head_eval: B \* Co <= 256"):
        K.head_eval(x, w, b, t, K.eval_acc(co, DEV))
    with pytest.raises(K.N3DError, match=r"head_loss_eval: B \* Co <= 256"):
        K.head_loss_eval(x, w, b, t, K.eval_acc(co, DEV), hr.TVERSKY)
    # a pitch that is no multiple of 4, a misaligned x
    B = 2
    t = torch.zeros((B, co) + shape, **f32)
    flat = torch.zeros(B * 8 * (ci + 2) + 8, **f32)
    odd = K.View(flat[:B * 8 * (ci + 2)].view(B, *shape, ci + 2).permute(0, 4, 1, 2, 3)[:, :ci], ci + 2)
    off = K.View(flat[1:1 + B * 8 * ci].view(B, *shape, ci).permute(0, 4, 1, 2, 3), ci)
    assert off.t.data_ptr() % 16 == 4
    good = K.as_view(K.zeros_ndhwc(B, ci, *shape, DEV, torch.float32))
    for bad in (odd, off):
        with pytest.raises(K.N3DError, match=r"x needs ld % 4 == 0 and quad alignment"):
            K.head_fwd(bad, w, b, None, t)
        with pytest.raises(K.N3DError, match=r"x needs ld % 4 == 0 and quad alignment"):
            K.head_bwd(bad, w, b, None, good, None, None, dp=t)
    # a misaligned dx: the kernel stores a channel quad per st4 (fp32: 16 bytes; bf16: 8)
    _, _, sums, _ = K.head_fwd(good, w, b, None, t)
    _, _, _, coef, _ = K.head_loss_fwd(good, w, b, None, t, hr.TVERSKY)
    flat16 = torch.zeros(B * 8 * ci + 8, dtype=torch.bfloat16, device=DEV)
    off16 = K.View(flat16[2:2 + B * 8 * ci].view(B, *shape, ci).permute(0, 4, 1, 2, 3), ci)
    assert off16.t.data_ptr() % 8 == 4
    for bad in (off, off16):
        with pytest.raises(K.N3DError, match=r"head_bwd: dx needs ld % 4 == 0 and quad alignment"):
            K.head_bwd(good, w, b, None, bad, None, None, t=t, sums=sums)
        with pytest.raises(K.N3DError, match=r"head_loss_bwd: dx needs ld % 4 == 0 and quad alignment"):
            K.head_loss_bwd(good, w, b, None, bad, None, None, t, coef)
    # ... and in the node-planar form
    nn, cn = 2, 4
    w2 = torch.zeros((co, nn * cn, 1, 1, 1), **f32)
    xp = K.empty_planar(nn, B, cn, *shape, DEV, torch.float32)
    xp.t.zero_()
    n = nn * B * 8 * cn
    dxp = K.Planar(torch.zeros(n + 8, **f32)[1:1 + n].view(nn, B, *shape, cn).permute(0, 1, 5, 2, 3, 4))
    assert dxp.nodes[0].t.data_ptr() % 16 == 4
    _, _, sums2, _ = K.head_fwd(xp, w2, b, None, t)
    with pytest.raises(K.N3DError, match=r"head_bwd: node-planar dx needs .*quad-aligned"):
        K.head_bwd(xp, w2, b, None, dxp, None, None, t=t, sums=sums2)
    torch.cuda.synchronize()


# ---- F: the layout kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [255, 256, 1200])
@pytest.mark.parametrize("Cc", [1, 3, 4, 12])
def test_layout_kernels(Cc, N):
    """n3d_ncdhw_to_ndhwc / n3d_ndhwc_to_ncdhw, the C ABI's way into and out of the head's input layout, dense and pitched (ld = C + 3):
    bit-exact against a permute, the pitch gap untouched, the round trip the identity"""
    K = _K()
    from nas_3d_unet_amd import _lib
    lib = _lib.load()
    B = 2
    rng = np.random.default_rng(100 * Cc + N)
    src = torch.from_numpy(rng.standard_normal((B, Cc, N)).astype(np.float32)).to(DEV)
    for ld in (Cc, Cc + 3):
        dst = torch.full((B, N, ld), hr.SENT_OUT, device=DEV)
        _lib.check(lib.n3d_ncdhw_to_ndhwc(K.ptr(src), K.ptr(dst), ld, B, Cc, N, K.stream_ptr()), "n3d_ncdhw_to_ndhwc")
        assert torch.equal(dst[..., :Cc], src.permute(0, 2, 1)), ld
        assert bool((dst[..., Cc:] == hr.SENT_OUT).all()), "the pitch gap"
        dst[..., Cc:] = hr.SENT_IN
        back = torch.full((B, Cc, N), hr.SENT_OUT, device=DEV)
        _lib.check(lib.n3d_ndhwc_to_ncdhw(K.ptr(dst), ld, K.ptr(back), B, Cc, N, K.stream_ptr()), "n3d_ndhwc_to_ncdhw")
        assert torch.equal(back, src), ld
    if N == 1200:
        assert torch.equal(K.ncdhw_to_ndhwc(src.view(B, Cc, 5, 6, 40)), src.view(B, Cc, 5, 6, 40))
