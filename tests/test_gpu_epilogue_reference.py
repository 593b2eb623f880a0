"""GPU: the epilogue, SE-gate, pooling and depthwise-batch kernels, called straight through their kernels.py wrappers, against the plain
fp64 torch-CPU restatements of tests/_epilogue_ref.py, element by element (max|err| / max|ref| through _util.assert_close).

  A  test_single_term_epilogue        channel_stats, gn_coeffs + affine_act / affine_act_gn, affine_act_bwd_reduce, gn_bwd_coeffs +
                                      affine_act_bwd_apply / affine_act_bwd_apply_gn (both forms wherever the fused one takes the shape)
     test_single_term_bf16_storage    the same launches with bf16 storage against fp32 storage on the bf16-rounded operands
  B  test_nterm_node                  channel_statsN, gn_coeffsN, affine_actN, GnGroupBwd.reduce / coeffs / apply, affine_act_bwd_reduceN,
                                      plain_bwd_coeffs + affine_act_bwd_apply for the un-normalised terms
     test_reduceN_16_terms_and_plain_dalphaN   affine_act_bwd_reduceN with 16 terms, plain_dalphaN
  C  test_se_gates                    se_gate_fwd / se_gate_bwd, se_gate_fwdN / se_gate_bwdN (1, 3, 8 gates), the input gradient A * dout + Bc
  D  test_pool_forward / test_pool_backward / test_pool_bf16_storage / test_pool_rejects_odd_dimensions
                                      pool2_fwd, pool2_bwd, pool2_fwd_both, pool2_bwd_both; random and tie inputs
  E  test_dwconv_batch                dwconv_batch with 1, 3, 8 jobs

Tolerances are the suite's own: forward outputs and coefficients 2e-5 (test_gpu_prims.TOL_FWD), d(raw) and other input gradients 1e-4
and dgamma / dbeta / dbias_conv 1e-4 (test_gpu_pair), the depthwise data gradient 5e-5 (test_gpu_conv), dalpha and the SE fc gradients
2e-4 (test_gpu_nets), fp64 statistics rows 1e-5 (test_gpu_conv).  ReLU masks agree by construction (_epilogue_ref.margin_inputs), no
element is excluded anywhere.

Padded channels (case A7, G = -6: 6 real channels stored in 8): forward tensors, coefficients, dgamma and dbeta are exactly 0 on the
padded channels and everything on the real ones is GroupNorm(1, 6)'s.  d(raw) of a padded channel is NOT zero in the kernels: the twin's
group statistics depend on that channel, so it receives the group's coupling term (train.py masks it: "GroupNorm couples a padded channel
to its group"); it is compared with the fp64 gradient of that twin formula instead of with zero.

Each of these mistakes, built into a scratch copy of elementwise.hip, fails the tests named (run on an MI355X, all other tests passing):
  0.125f -> 0.124f in pool2_bwd_kernel                  test_pool_backward, all 15 cases
  > -> >= in the arg-max of pool2_bwd_kernel            test_pool_backward[*-tie], [*-tie_relu] (10 cases; the random inputs cannot see it)
  S1 and S2 swapped in gn_bwd_coeffs_body               test_single_term_epilogue[A1..A10], test_nterm_node[B1..B5]
  `* cg` dropped from n in gn_bwd_coeffs_body           test_single_term_epilogue[A1..A10], test_nterm_node[B1..B5]
  hidden[0] for hidden[b] in se_gate_bwd_body2          test_se_gates[C2], [C4] (the B = 2 cases)
  last term skipped in affine_actN_kernel               test_nterm_node[B1..B5]
  fmaxf for pool_max in the pooling forward kernels       test_pool_forward on the tie inputs (fmaxf makes +0.0 of a window -0.0, +0.0)"""
import ctypes

import numpy as np
import pytest
import torch

import _epilogue_ref as R
from _util import assert_close

pytestmark = pytest.mark.gpu

TOL_FWD, TOL_DX, TOL_DW_DX, TOL_PARAM, TOL_ALPHA, TOL_ROWS = 2e-5, 1e-4, 5e-5, 1e-4, 2e-4, 1e-5
ULP_BF16 = 2.0 ** -8          # test_gpu_bf16: a tensor stored in bf16 against the fp32 kernel on the same bf16-rounded operands
SENTINEL = 7.0


def _K():
    from nas_3d_unet_amd import kernels as K
    assert K._stats_cache is None      # no `with K.stats_cache()` is open: channel_stats / channel_statsN launch on every call
    return K


class Bufs:
    """device tensors of a test; a View with a pitch larger than its channel count is a channel slice of a wider buffer whose other
    channels hold a sentinel that must still be there at the end (a kernel that ignores the pitch writes over it)"""

    def __init__(self, K, dtype=torch.float32):
        self.K, self.dtype, self.guards = K, dtype, []

    def view(self, arr, ld=None, c0=0):
        """View of the numpy (B, C, D, H, W) array stored as channels [c0, c0 + C) of a (B, D, H, W, ld) buffer"""
        B, C, D, H, W = arr.shape
        ld = C if ld is None else ld
        n = B * D * H * W * ld
        buf = torch.full((n + 8,), SENTINEL, dtype=self.dtype, device="cuda")      # (+ 8: the readable slack bf16 tensors need)
        box = buf[:n].view(B, D, H, W, ld)
        t = box[..., c0:c0 + C].permute(0, 4, 1, 2, 3)
        t.copy_(torch.from_numpy(np.ascontiguousarray(arr)).to(self.dtype))
        v = self.K.as_view(t)
        assert v.ld == ld and v.t.data_ptr() == t.data_ptr(), "as_view repacked a tensor the test wants in place"
        if ld > C:
            self.guards.append((box, c0, C))
        return v

    def empty(self, shape, ld=None, c0=0):
        return self.view(np.full(shape, np.nan, np.float32), ld, c0)

    def check_guards(self):
        for box, c0, C in self.guards:
            assert bool((box[..., :c0] == SENTINEL).all()) and bool((box[..., c0 + C:] == SENTINEL).all()), "a kernel wrote outside its channel slice"


def _scalar(w):
    return None if w is None else torch.tensor([w], dtype=torch.float32, device="cuda")


def _param(a):
    return torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(a)).cuda())


def _vp(t, i=0):
    """ctypes pointer to element i of a float32 device tensor (None: NULL)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * i)


def _np(t):
    return t.detach().float().cpu().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().numpy()


def _regime(K, N, C):
    """(rows, fused, ragged) of the row mapping: fused = the one-launch forms take the shape; ragged = the last block of a sample is
    partial (the rows do not cut the sample into equal whole block-iterations)"""
    rows = K.stats_rows(N, C)
    vpb = 256 // (C // 4)
    return rows, rows <= K.fused_max_rows(), (N % rows != 0) or ((N // rows) % vpb != 0)


# ================================================================================================= A. single-term epilogue
def _run_single(K, c, inp, fused_fwd, fused_bwd, dtype=torch.float32):
    """forward and backward of one GroupNorm -> [ReLU] -> weight epilogue with the case's options; fused_*: the one-launch forms"""
    bufs = Bufs(K, dtype)
    C, shape5 = c.C, (c.B, c.C) + c.shape
    N = int(np.prod(c.shape))
    raw = bufs.view(inp["raw"], 3 * C, C) if c.slice else bufs.view(inp["raw"])
    dout = bufs.view(inp["dout"])
    pitch = C + 4 if c.pitch else None
    out = bufs.view(inp["prev_out"], pitch) if c.acc else bufs.empty(shape5, pitch)
    draw = bufs.view(inp["prev_draw"], pitch) if c.acc else bufs.empty(shape5, pitch)
    gamma, beta = _param(inp["gamma"]), _param(inp["beta"])
    wt = _scalar(R.W_SCALAR if c.w else None)
    cb = torch.nn.Parameter(torch.zeros(C, device="cuda")) if c.bias else None
    da = torch.full((1,), float("nan"), device="cuda") if c.dalpha else None
    fl = (K.RELU if c.relu else 0) | (K.ACCUMULATE if c.acc else 0)
    res = {}
    st, rows = K.channel_stats(raw)
    res["stats"] = st.sum(1)
    if fused_fwd:
        a, b, mr, sr = K.affine_act_gn(raw, st, rows, gamma, beta, c.G, R.EPS, _vp(wt), out, fl)
    else:
        a, b, mr, sr = K.gn_coeffs(st, rows, gamma, beta, c.B, C, c.G, N, R.EPS)
        K.affine_act(raw, a, b, _vp(wt), out, fl)
    sums, rows2 = K.affine_act_bwd_reduce(dout, raw, a, b, K.RELU if c.relu else 0)
    assert rows2 == rows and tuple(sums.shape) == (c.B, rows, C, 3)
    if fused_bwd:
        dg, db, dcb = K.affine_act_bwd_apply_gn(dout, raw, a, b, sums, rows, gamma, beta, mr, _vp(wt), sr if c.bias else None, cb, draw, c.G, fl, _vp(da))
    else:
        dg, db, cA, cB, cC, dcb = K.gn_bwd_coeffs(sums, rows, gamma, mr, _vp(wt), c.B, C, c.G, N, _vp(da), beta, sr if c.bias else None, cb)
        K.affine_act_bwd_apply(dout, raw, a, b, cA, cB, cC, draw, fl)
    torch.cuda.synchronize()
    bufs.check_guards()
    res.update(a=a, b=b, mean_rstd=mr, sumraw=sr, out=out.t, sums=sums.sum(1), draw=draw.t, dgamma=dg, dbeta=db, dalpha=da, dbias_conv=dcb)
    return {k: (_np(v) if v is not None else None) for k, v in res.items()}


@pytest.mark.parametrize("cid", list(R.SINGLE_CASES))
def test_single_term_epilogue(cid):
    K = _K()
    c, inp = R.SINGLE_CASES[cid], R.single_inputs(cid)
    N = int(np.prod(c.shape))
    rows, fused, ragged = _regime(K, N, c.C)
    assert (fused, ragged) == (c.fused, c.ragged), "%s no longer reaches its regime (rows = %d): pick new shapes" % (cid, rows)
    real = R.real_channels(c.C, c.G)
    w = R.W_SCALAR if c.w else None
    ref = R.term_reference(inp["raw"], inp["gamma"], inp["beta"], c.G, c.relu, w, inp["dout"])
    want_out = ref["y"] + (inp["prev_out"].astype(np.float64) if c.acc else 0.0)
    want_draw = R.twin_draw(inp["raw"], inp["gamma"], inp["beta"], c.G, c.relu, w, inp["dout"]) if c.G < 0 else ref["draw"]
    if c.G < 0:
        assert_close(want_draw[:, :real], ref["draw"][:, :real], 1e-9, "the twin formula against GroupNorm(1, real)")
    if c.acc:
        want_draw = want_draw + inp["prev_draw"].astype(np.float64)
    # the one-launch backward takes at most 4 samples (programs.seg_backward picks the forms the same way)
    forms = [(False, False)] + ([(True, c.B <= 4)] if fused else [])
    for ffwd, fbwd in forms:
        tag = "%s fused=%d/%d " % (cid, ffwd, fbwd)
        got = _run_single(K, c, inp, ffwd, fbwd)
        assert_close(got["stats"], ref["stats"], TOL_ROWS, tag + "stats")
        assert_close(got["a"], ref["a"], TOL_FWD, tag + "a")
        assert_close(got["b"], ref["b"], TOL_FWD, tag + "b")
        assert_close(got["mean_rstd"], ref["mean_rstd"], TOL_FWD, tag + "mean_rstd")
        assert_close(got["sumraw"], ref["sumraw"], TOL_ROWS, tag + "sumraw")
        assert_close(got["out"], want_out, TOL_FWD, tag + "out")
        for k, name in enumerate(("S1", "S2", "Sz")):
            assert_close(got["sums"][..., k], ref["sums"][..., k], TOL_ROWS, tag + name)
        assert_close(got["draw"], want_draw, TOL_DX, tag + "d raw")
        assert_close(got["dgamma"], ref["dgamma"], TOL_PARAM, tag + "dgamma")
        assert_close(got["dbeta"], ref["dbeta"], TOL_PARAM, tag + "dbeta")
        if c.dalpha:
            assert_close(got["dalpha"], ref["dalpha"], TOL_ALPHA, tag + "dalpha")
        if c.bias:
            assert_close(got["dbias_conv"], ref["dbias_conv"], TOL_PARAM, tag + "dbias_conv")
        if c.G < 0:
            assert not c.acc
            assert_close(got["draw"][:, real:], want_draw[:, real:], TOL_DX, tag + "d raw of the padded channels (the group's coupling term)")
            for k in ("a", "b", "sumraw", "stats"):
                assert not got[k][:, real:].any(), tag + k + " of a padded channel"
            assert not got["out"][:, real:].any() and not got["dgamma"][real:].any() and not got["dbeta"][real:].any(), tag + "padded channels"


@pytest.mark.parametrize("cid", ["A1", "A3"])
def test_single_term_bf16_storage(cid):
    """every activation tensor in bf16 storage against the same launches in fp32 storage on the bf16-rounded operands (the way
    test_gpu_bf16.test_node_epilogues_bf16_storage does it, at its tolerances: one rounding of a stored tensor, 1e-5 where fp32)"""
    K = _K()
    c, inp = R.SINGLE_CASES[cid], R.single_inputs(cid)
    assert not c.acc
    rnd = lambda a: torch.from_numpy(a).bfloat16().float().numpy()
    inp16 = dict(inp, raw=rnd(inp["raw"]), dout=rnd(inp["dout"]))
    _, fused, _ = _regime(K, int(np.prod(c.shape)), c.C)
    for f in ([False, True] if fused and c.B <= 4 else [False]):
        r32 = _run_single(K, c, inp16, f, f, torch.float32)
        r16 = _run_single(K, c, inp16, f, f, torch.bfloat16)
        for k in ("stats", "sumraw", "a", "b", "mean_rstd"):      # the same fp32 arithmetic on the same values
            assert np.array_equal(r16[k], r32[k]), k
        assert_close(r16["out"], r32["out"], ULP_BF16, "out")
        assert_close(r16["draw"], r32["draw"], ULP_BF16, "d raw")
        assert_close(r16["sums"], r32["sums"], 1e-5, "reduction rows")
        assert_close(r16["dgamma"], r32["dgamma"], 1e-5, "dgamma")
        assert_close(r16["dbeta"], r32["dbeta"], 1e-5, "dbeta")
        assert_close(r16["dalpha"], r32["dalpha"], 1e-5, "dalpha")
        if c.bias:
            assert_close(r16["dbias_conv"], r32["dbias_conv"], 1e-5, "dbias_conv")


# ================================================================================================= B. N-term forms
def _nterm_views(c, inp, bufs):
    """term 0 reads a channel slice of a 3C-wide buffer, the last one a slice of a (C + 4)-wide one"""
    n = len(inp["terms"])
    views = []
    for k, t in enumerate(inp["terms"]):
        views.append(bufs.view(t["raw"], 3 * c.C, c.C) if k == 0 else (bufs.view(t["raw"], c.C + 4) if k == n - 1 else bufs.view(t["raw"])))
    return views


def _check_statsN(K, views, refs):
    sts = K.channel_statsN(views)
    assert len(sts) == len(views)
    for k, (v, (st, rows)) in enumerate(zip(views, sts)):
        assert_close(st.sum(1), refs[k]["stats"], TOL_ROWS, "channel_statsN %d" % k)
        one, rows1 = K.channel_stats(v)
        assert rows1 == rows and torch.equal(one, st), "channel_statsN differs from channel_stats (tensor %d)" % k
    return sts


@pytest.mark.parametrize("cid", ["B1", "B2", "B3", "B4", "B5"])
def test_nterm_node(cid):
    K = _K()
    c, inp = R.NTERM_CASES[cid], R.nterm_inputs(cid)
    N = int(np.prod(c.shape))
    node, refs = R.node_reference(inp, c.G, c.acc)
    bufs = Bufs(K)
    rv = _nterm_views(c, inp, bufs)
    n = len(rv)
    shape5 = (c.B, c.C) + c.shape
    sts = _check_statsN(K, rv, refs)
    gn = [k for k, t in enumerate(inp["terms"]) if t["kind"] == "gn"]
    plain = [k for k in range(n) if k not in gn]
    gam = {k: _param(inp["terms"][k]["gamma"]) for k in gn}
    bet = {k: _param(inp["terms"][k]["beta"]) for k in gn}
    wts = [_scalar(t["w"]) for t in inp["terms"]]
    # ---- forward: coefficients of every GroupNorm term in one launch, the node in one pass
    saved = dict(zip(gn, K.gn_coeffsN([(rv[k], sts[k][0], sts[k][1], gam[k], bet[k]) for k in gn], c.G, R.EPS)))
    for k in gn:
        a, b, mr, sr = saved[k]
        assert_close(a, refs[k]["a"], TOL_FWD, "a %d" % k)
        assert_close(b, refs[k]["b"], TOL_FWD, "b %d" % k)
        assert_close(mr, refs[k]["mean_rstd"], TOL_FWD, "mean_rstd %d" % k)
        assert_close(sr, refs[k]["sumraw"], TOL_ROWS, "sumraw %d" % k)
    out = bufs.view(inp["prev"], c.C + 4) if c.acc else bufs.empty(shape5, c.C + 4)
    K.affine_actN([(rv[k], saved[k][0] if k in saved else None, saved[k][1] if k in saved else None, wts[k], inp["terms"][k]["relu"]) for k in range(n)],
                  out, K.ACCUMULATE if c.acc else 0)
    assert_close(out.t, node, TOL_FWD, "node")
    # ---- backward of the GroupNorm terms: reductions, coefficients + parameter gradients, d(raw)
    dout = bufs.view(inp["dout"])
    da = torch.full((n,), float("nan"), device="cuda")
    cbs = {k: torch.nn.Parameter(torch.zeros(c.C, device="cuda")) for k in gn} if c.bias else {}
    draws = {k: (bufs.empty(shape5, c.C + 4) if k == gn[0] else bufs.empty(shape5)) for k in range(n)}
    tds = [dict(raw=rv[k], a=saved[k][0], b=saved[k][1], mr=saved[k][2], sumraw=saved[k][3] if c.bias else None, gamma=gam[k], beta=bet[k],
                wptr=wts[k].data_ptr() if wts[k] is not None else None, relu=inp["terms"][k]["relu"], conv_bias=cbs.get(k), draw=draws[k],
                dalpha_ptr=da.data_ptr() + 4 * k) for k in gn]
    grp = K.GnGroupBwd(dout, tds, c.G)
    grp.reduce()
    grp.coeffs()
    grp.apply()
    for i, k in enumerate(gn):
        for j, name in enumerate(("S1", "S2", "Sz")):
            assert_close(grp.sums[i].sum(1)[..., j], refs[k]["sums"][..., j], TOL_ROWS, "%s of term %d" % (name, k))
        assert_close(draws[k].t, refs[k]["draw"], TOL_DX, "d raw %d" % k)
        assert_close(grp.outs[i][0], refs[k]["dgamma"], TOL_PARAM, "dgamma %d" % k)
        assert_close(grp.outs[i][1], refs[k]["dbeta"], TOL_PARAM, "dbeta %d" % k)
        assert_close(da[k:k + 1], refs[k]["dalpha"], TOL_ALPHA, "dalpha %d" % k)
        if c.bias:
            assert_close(grp.outs[i][2], refs[k]["dbias_conv"], TOL_PARAM, "dbias_conv %d" % k)
    # ---- the un-normalised terms: reduction rows in one launch, A = w and dalpha, d(raw) = w * dout behind the ReLU mask
    if plain:
        red = K.affine_act_bwd_reduceN(dout, [(rv[k], None, None, inp["terms"][k]["relu"]) for k in plain])
        for (sums, rows), k in zip(red, plain):
            for j, name in enumerate(("S1", "S2", "Sz")):
                assert_close(sums.sum(1)[..., j], refs[k]["sums"][..., j], TOL_ROWS, "%s of plain term %d" % (name, k))
            cA = K.plain_bwd_coeffs(sums, rows, _vp(wts[k]), c.B, c.C, sums.device, _vp(da, k), want_A=True)
            assert_close(cA, np.full((c.B, c.C), R.w64(inp["terms"][k]["w"])), 0.0, "A of plain term %d" % k)
            K.affine_act_bwd_apply(dout, rv[k], None, None, cA, None, None, draws[k], K.RELU if inp["terms"][k]["relu"] else 0)
            assert_close(draws[k].t, refs[k]["draw"], TOL_DX, "d raw of plain term %d" % k)
            assert_close(da[k:k + 1], refs[k]["dalpha"], TOL_ALPHA, "dalpha of plain term %d" % k)
    torch.cuda.synchronize()
    bufs.check_guards()


def test_reduceN_16_terms_and_plain_dalphaN():
    """B6: the reduction rows of a whole node level (8 GroupNorm terms with their coefficients and 8 un-normalised ones) in ONE
    n3d_affine_act_bwd_reduceN launch, and dalpha of the 8 un-normalised ones in one n3d_plain_bwd_coeffsN launch"""
    K = _K()
    c, inp = R.NTERM_CASES["B6"], R.nterm_inputs("B6")
    assert len(inp["terms"]) == K.MAX_REDUCE_TERMS
    _, refs = R.node_reference(inp, c.G, False)
    bufs = Bufs(K)
    rv = _nterm_views(c, inp, bufs)
    gn = [k for k, t in enumerate(inp["terms"]) if t["kind"] == "gn"]
    plain = [k for k in range(len(rv)) if k not in gn]
    sts = _check_statsN(K, rv[:8], refs[:8])
    saved = dict(zip(gn, K.gn_coeffsN([(rv[k], sts[k][0], sts[k][1], _param(inp["terms"][k]["gamma"]), _param(inp["terms"][k]["beta"])) for k in gn],
                                      c.G, R.EPS)))
    dout = bufs.view(inp["dout"], c.C + 4)
    red = K.affine_act_bwd_reduceN(dout, [(rv[k], saved[k][0] if k in saved else None, saved[k][1] if k in saved else None, inp["terms"][k]["relu"])
                                          for k in range(len(rv))])
    for k, (sums, rows) in enumerate(red):
        for j, name in enumerate(("S1", "S2", "Sz")):
            assert_close(sums.sum(1)[..., j], refs[k]["sums"][..., j], TOL_ROWS, "%s of term %d" % (name, k))
    da = torch.full((len(rv),), float("nan"), device="cuda")
    K.plain_dalphaN([(red[k][0], red[k][1], da.data_ptr() + 4 * k) for k in plain], c.B, c.C)
    for k in plain:
        assert_close(da[k:k + 1], refs[k]["dalpha"], TOL_ALPHA, "dalpha of plain term %d" % k)
    assert bool(torch.isnan(da[gn]).all())
    bufs.check_guards()


# ================================================================================================= C. SE gates
def _fc(g):
    fc = torch.nn.Sequential(torch.nn.Linear(g["w1"].shape[1], 1), torch.nn.ReLU(), torch.nn.Linear(1, g["w1"].shape[1])).cuda()
    with torch.no_grad():
        for p, k in zip(fc.parameters(), ("w1", "b1", "w2", "b2")):
            p.copy_(torch.from_numpy(g[k]))
    return fc


def _check_se(tag, ref, fwd, bwd, da, dx):
    mean, hidden, gate = fwd
    dw1, db1, dw2, db2, _, _ = bwd
    assert_close(mean, ref["mean"], TOL_FWD, tag + "mean")
    assert_close(hidden, ref["hidden"], TOL_FWD, tag + "hidden")
    assert np.array_equal(_np(hidden) == 0, ref["hidden"] == 0), tag + "live / dead samples"
    assert_close(gate, ref["gate"], TOL_FWD, tag + "gate")
    assert_close(dw1, ref["dw1"], TOL_ALPHA, tag + "dw1")
    assert_close(db1, ref["db1"], TOL_ALPHA, tag + "db1")
    assert_close(dw2, ref["dw2"], TOL_ALPHA, tag + "dw2")
    assert_close(db2, ref["db2"], TOL_ALPHA, tag + "db2")
    assert_close(da, ref["dalpha"], TOL_ALPHA, tag + "dalpha")
    assert_close(dx.t, ref["dx"], TOL_DX, tag + "dx")


@pytest.mark.parametrize("cid", list(R.SE_CASES))
def test_se_gates(cid):
    K = _K()
    c, inp = R.SE_CASES[cid], R.se_inputs(cid)
    N = int(np.prod(c.shape))
    B, C = c.B, c.C
    refs = [R.se_reference(g, c.w, inp["dout"]) for g in inp["gates"]]
    bufs = Bufs(K)
    xs = [bufs.view(g["x"], C + 4) if k == 0 else bufs.view(g["x"]) for k, g in enumerate(inp["gates"])]
    fcs = [_fc(g) for g in inp["gates"]]
    dout = bufs.view(inp["dout"])
    wt = _scalar(c.w)
    sts = [K.channel_stats(x) for x in xs]
    shape5 = (B, C) + c.shape
    # ---- one gate at a time: n3d_se_gate_fwd / n3d_se_gate_bwd; reduction rows with a = gate and no ReLU, as programs.py forms them
    for k, (x, fc, (st, rows)) in enumerate(zip(xs, fcs, sts)):
        fwd = K.se_gate_fwd(st, rows, N, fc[0].weight, fc[0].bias, fc[2].weight, fc[2].bias, B, C)
        y = bufs.empty(shape5)
        K.affine_act(x, fwd[2], None, _vp(wt), y, 0)
        assert_close(y.t, refs[k]["y"], TOL_FWD, "gate %d: w * x * gate" % k)
        sums, rows2 = K.affine_act_bwd_reduce(dout, x, fwd[2], None, 0)
        da = torch.full((1,), float("nan"), device="cuda")
        bwd = K.se_gate_bwd(sums, rows2, _vp(wt), fwd[0], fwd[1], fwd[2], fc[0].weight, fc[2].weight, B, C, N, _vp(da), fc)
        dx = bufs.empty(shape5, C + 4)
        K.affine_act_bwd_apply(dout, x, None, None, bwd[4], bwd[5], None, dx, 0)
        _check_se("single gate %d: " % k, refs[k], fwd, bwd, da, dx)
    # ---- all gates of the case in one launch each way
    fwds = K.se_gate_fwdN([(st, rows, fc) for (st, rows), fc in zip(sts, fcs)], N, B, C)
    red = K.affine_act_bwd_reduceN(dout, [(x, f[2], None, False) for x, f in zip(xs, fwds)])
    da = torch.full((c.gates,), float("nan"), device="cuda")
    bwds = K.se_gate_bwdN([dict(sums=s, rows=r, wptr=wt.data_ptr() if wt is not None else None, mean=f[0], hidden=f[1], gate=f[2], fc=fc,
                                dalpha_ptr=da.data_ptr() + 4 * k) for k, ((s, r), f, fc) in enumerate(zip(red, fwds, fcs))], N, B, C)
    for k in range(c.gates):
        dx = bufs.empty(shape5)
        K.affine_act_bwd_apply(dout, xs[k], None, None, bwds[k][4], bwds[k][5], None, dx, 0)
        _check_se("gate %d of %d: " % (k, c.gates), refs[k], fwds[k], bwds[k], da[k:k + 1], dx)
    torch.cuda.synchronize()
    bufs.check_guards()


# ================================================================================================= D. pooling
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _pool_views(c, inp, bufs):
    oshape = inp["dy"].shape
    x = bufs.view(inp["x"], c.C + 4) if c.pitched else bufs.view(inp["x"])
    ld_o = 2 * c.C if c.pitched else None
    return x, oshape, ld_o


@pytest.mark.parametrize("family", R.POOL_FAMILIES)
@pytest.mark.parametrize("cid", list(R.POOL_CASES))
def test_pool_forward(cid, family):
    K = _K()
    c, inp = R.POOL_CASES[cid], R.pool_inputs(cid, family)
    bufs = Bufs(K)
    x, oshape, ld_o = _pool_views(c, inp, bufs)
    ya, ym, yba, ybm = (bufs.empty(oshape, ld_o, c.C if ld_o else 0) for _ in range(4))
    K.pool2_fwd(x, ya, False)
    K.pool2_fwd(x, ym, True)
    K.pool2_fwd_both(x, yba, ybm)
    torch.cuda.synchronize()
    ref_avg, _ = R.pool_reference(inp["x"], inp["dy"], False)
    ref_max32, _ = R.pool_reference(inp["x"], inp["dy"], True, torch.float32)
    assert_close(ya.t, ref_avg, TOL_FWD, "avg")
    assert torch.equal(_bits(ym.t), _bits(ref_max32)), "max pooling forward is not bit-equal to F.max_pool3d (fp32, CPU)"
    assert torch.equal(_bits(yba.t), _bits(ya.t)) and torch.equal(_bits(ybm.t), _bits(ym.t)), "pool2_fwd_both differs from the single kernels"
    bufs.check_guards()


@pytest.mark.parametrize("family", R.POOL_FAMILIES)
@pytest.mark.parametrize("cid", list(R.POOL_CASES))
def test_pool_backward(cid, family):
    K = _K()
    c, inp = R.POOL_CASES[cid], R.pool_inputs(cid, family)
    bufs = Bufs(K)
    x, oshape, ld_o = _pool_views(c, inp, bufs)
    dy = bufs.view(inp["dy"], ld_o, c.C if ld_o else 0)
    wt, wt2 = _scalar(R.W_SCALAR), _scalar(0.81)
    grads = {m: R.pool_reference(inp["x"], inp["dy"], m)[1].numpy() for m in (False, True)}
    prev = inp["prev"].astype(np.float64)
    ld_x = c.C + 4 if c.pitched else None
    for is_max in (False, True):
        for acc in (False, True):
            for w in (None, wt):
                dx = bufs.view(inp["prev"], ld_x) if acc else bufs.empty(inp["x"].shape, ld_x)
                K.pool2_bwd(dy, x, dx, is_max, acc, _vp(w))
                want = (R.w64(R.W_SCALAR) if w is not None else 1.0) * grads[is_max] + (prev if acc else 0.0)
                assert_close(dx.t, want, TOL_DX, "dx max=%d acc=%d w=%d" % (is_max, acc, w is not None))
                if is_max and not acc and w is None:
                    ref32 = R.pool_reference(inp["x"], inp["dy"], True, torch.float32)[1]
                    assert torch.equal(_bits(dx.t), _bits(ref32)), "max pooling backward is not torch's: the first arg-max in (d, h, w) order takes the gradient"
    for acc in (False, True):
        dx = bufs.view(inp["prev"], ld_x) if acc else bufs.empty(inp["x"].shape, ld_x)
        K.pool2_bwd_both(dy, x, dx, acc, _vp(wt), _vp(wt2))
        want = R.w64(R.W_SCALAR) * grads[False] + R.w64(0.81) * grads[True] + (prev if acc else 0.0)
        assert_close(dx.t, want, TOL_DX, "pool2_bwd_both acc=%d" % acc)
    dx = bufs.empty(inp["x"].shape, ld_x)
    K.pool2_bwd_both(dy, x, dx, False, None, None)
    assert_close(dx.t, grads[False] + grads[True], TOL_DX, "pool2_bwd_both without weights")
    torch.cuda.synchronize()
    bufs.check_guards()


@pytest.mark.parametrize("family", ["normal", "tie"])
@pytest.mark.parametrize("cid", list(R.POOL_CASES))
def test_pool_bf16_storage(cid, family):
    """the single kernels with bf16 storage against fp32 storage on the bf16-rounded operands: max pooling moves values, so it is
    exact; the average and the accumulating backward round their stored result once"""
    K = _K()
    c, inp = R.POOL_CASES[cid], R.pool_inputs(cid, family)
    rnd = lambda a: torch.from_numpy(a).bfloat16().float().numpy()
    inp = {k: rnd(v) for k, v in inp.items()}
    res = {}
    for dt in (torch.float32, torch.bfloat16):
        bufs = Bufs(K, dt)
        x, oshape, ld_o = _pool_views(c, inp, bufs)
        dy = bufs.view(inp["dy"], ld_o, c.C if ld_o else 0)
        ld_x = c.C + 4 if c.pitched else None
        r = {}
        for is_max in (False, True):
            y = bufs.empty(oshape, ld_o, c.C if ld_o else 0)
            K.pool2_fwd(x, y, is_max)
            dx = bufs.empty(inp["x"].shape, ld_x)
            K.pool2_bwd(dy, x, dx, is_max)
            dxa = bufs.view(inp["prev"], ld_x)
            K.pool2_bwd(dy, x, dxa, is_max, True, _vp(_scalar(R.W_SCALAR)))
            r[is_max] = (_np(y.t), _np(dx.t), _np(dxa.t))
        torch.cuda.synchronize()
        bufs.check_guards()
        res[dt] = r
    f32, b16 = res[torch.float32], res[torch.bfloat16]
    assert np.array_equal(b16[True][0], f32[True][0]) and np.array_equal(b16[True][1], f32[True][1]), "max pooling in bf16 storage"
    assert_close(b16[False][0], f32[False][0], ULP_BF16, "avg")
    assert_close(b16[False][1], f32[False][1], ULP_BF16, "avg dx")
    for m in (False, True):
        assert_close(b16[m][2], f32[m][2], ULP_BF16, "accumulated weighted dx max=%d" % m)


def test_pool_rejects_odd_dimensions():
    """all four pooling entries refuse an odd spatial dimension on the host (2x2x2 windows with stride 2 would leave voxels of dx
    unwritten); nothing is launched"""
    K = _K()
    bufs = Bufs(K)
    for shape in ((3, 4, 4), (4, 5, 4), (4, 4, 7)):
        x = bufs.view(np.zeros((1, 4) + shape, np.float32))
        o = tuple(s // 2 for s in shape)
        y, y2, dy = (bufs.view(np.zeros((1, 4) + o, np.float32)) for _ in range(3))
        dx = bufs.view(np.full((1, 4) + shape, SENTINEL, np.float32))
        with pytest.raises(K.N3DError):
            K.pool2_fwd(x, y, True)
        with pytest.raises(K.N3DError):
            K.pool2_fwd_both(x, y, y2)
        for is_max in (False, True):
            with pytest.raises(K.N3DError):
                K.pool2_bwd(dy, x, dx, is_max)
        with pytest.raises(K.N3DError):
            K.pool2_bwd_both(dy, x, dx, False)
        torch.cuda.synchronize()
        assert bool((dx.t == SENTINEL).all())


# ================================================================================================= E. depthwise batch
@pytest.mark.parametrize("njobs", R.DW_JOBS)
@pytest.mark.parametrize("cid", list(R.DW_CASES))
def test_dwconv_batch(cid, njobs):
    K = _K()
    c = R.DW_CASES[cid]
    jobs = R.dw_inputs(cid, njobs)
    bufs = Bufs(K)
    calls, dsts = [], []
    for j in jobs:
        src = bufs.view(j["src"], c.C + 4) if j["pitched"] else bufs.view(j["src"])
        dst = bufs.view(j["prev"], 2 * c.C, c.C) if j["acc"] else bufs.empty((c.B, c.C) + c.shape)
        stride = 2 if j["kind"] in ("fwd2", "convT") else 1
        # the geometry's i side is what the window slides over: the source of a forward job, the destination of a gather-transposed one
        iside = j["src"].shape[2:] if j["kind"] in ("fwd1", "fwd2") else c.shape
        g = K.conv_geom(c.B, *iside, c.C, c.C, 3, stride, 1, 1, True)
        w = torch.from_numpy(j["w"]).cuda()
        b = torch.from_numpy(j["bias"]).cuda() if j["bias"] is not None else None
        calls.append((g, j["kind"] in ("dgrad1", "convT"), src, w, b, dst, K.ACCUMULATE if j["acc"] else 0))
        dsts.append(dst)
    K.dwconv_batch(calls)
    torch.cuda.synchronize()
    for i, (j, dst) in enumerate(zip(jobs, dsts)):
        assert_close(dst.t, R.dw_reference(j), TOL_DW_DX if j["kind"] == "dgrad1" else TOL_FWD, "job %d (%s)" % (i, j["kind"]))
    bufs.check_guards()
