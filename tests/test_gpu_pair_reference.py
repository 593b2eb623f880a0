"""GPU: the two-term GroupNorm epilogues -- what programs.pair_forward / pair_backward / pair_backward_epilogue run for every node of
a searched cell -- against the fp64 torch-CPU pair reference of tests/_pair_ref.py, element by element (_util.assert_close), on the
operands production hands them: every activation tensor a channel slice of a wider buffer, each with its own pitch and front offset
(eight pitches in one call), neighbour channels holding a sentinel that must survive, output slices starting as NaN.

Every case of _pair_ref.PAIR_CASES names the route it is meant to reach; the route is asserted first (K.stats_rows, K.fused_max_rows,
K.pair_ok, n3d_bwd_small_mode, iters from the Python restatement of ew_map) and then again on the calls themselves: the library entry
points a wrapper call went through are recorded and compared.  A retuning therefore fails with "route moved, pick a new shape".

Kernel instantiations reached (fp32 storage; P1, P2, P6, P8 again in bf16):
  affine_act_gn2_kernel<ACC, PRE>            <0|1, 0> P1-P5, <0|1, 1> P6-P11; out1 in both; iters 1, 2, 4 and, in the beyond-four loop, 5 (P9:
                                             one live slot of its second group of four) and 6 (P11: two live slots, ragged last block)
  gn_coeffs_kernel (grid (B, 2))             P6-P11, with G < 0 in P10
  affine_bwd_reduce2_kernel<TWO>             <0>, <1> on every case; cpb 1, 2, 4, 8, 16
  affine_bwd_apply_gn2_kernel<PRE, TWO>      <0, 0|1> P1-P5 (leader <2, 2, 4> at B = 2, <2, GNF_MAXB, 2> at B = 3 and 4), <1, 0|1> P6-P11
  gn_bwd_coeffs_kernel<2> / <GNB_BP>         P6, P8, P9, P11 / P7, P10
  gn_bwd_small2_kernel<QPT, TWO, SPLIT, 2>   <2, 0|1, 0> P1, P3, <1, 0|1, 0> P12 (mode 1); <2, 0|1, 1> P4, <1, 0|1, 1> P13 (mode 2); P1 also
                                             through n3d_affine_act_bwd_small2, which no Python path calls
Options, each with asserted results on both forward routes and on the three backward routes it can reach (the one-launch route takes no
dalpha: the wrapper must send such a call to the two-launch forms, asserted): w0 != w1 and w1 alone, the four ReLU pairs, node mode and
two-output mode with and without N3D_ACCUMULATE (out is accumulated into, out1 overwritten), dout1 at a pitch of its own, dalpha and
dbias_conv of both terms, padded channels (G = -6: exact zeros forward, d(raw) of the padded channels against the padded twin).

Tolerances are the suite's own (test_gpu_epilogue_reference.py): 2e-5 forward and coefficients, 1e-4 d(raw) and parameter gradients,
2e-4 dalpha, 1e-5 fp64 rows; bf16 storage 2^-8 against fp32 storage on the bf16-rounded operands.

Each of these value mutations, built alone into a scratch copy of elementwise.hip, fails the tests named (MI355X; every other test of
this file and of test_gpu_pair.py passing unless listed); "old" = whether test_gpu_pair.py notices.  The bf16 runs compare the library
with itself and see none of them.
  1 w1 taken from t0.wptr in affine_act_gn2_kernel             test_pair_case: every variant, dense and single_launches run of every case (84).
                                                                old: no (it never passes a weight)
  2 term 1's ReLU threshold taken from term 0 in               node, node_acc, node_w1 and dense of every case (42: the (T, F) and (F, T) pairs).
    affine_bwd_apply_gn2_kernel                                 old: yes, 5 cases ([8-shape6-5-False] and the two-term one-launch cases' two-launch leg)
  3 dq for dq1 under TWO in affine_bwd_reduce2_kernel          two, two_acc, two_tt of every case (29).  old: one case ([32-shape2-2-2-True])
  4 the accumulate add also applied to the out1 value          two_acc and two_tt of every case but P9 and P11 (16).  old: no (no out1 in any forward)
  5 q1[0] for q1[j] in the beyond-four loop of the forward     P11, all four runs.  P9 cannot see it: at iters == 5 slot 0 is the only live one of
                                                                that group, which is why P11 (iters == 6) is in the table.  old: no
  6 cC[1] = cC[0] in the PRE apply                             every variant and dense of P6-P11 (26).  old: yes, [8-shape6-5-False], [4-shape7-2-True]
  7 the leader leaves its own sample out of dgamma             every variant and dense of P1-P5, P12, P13 (45).  old: yes, 5 cases
  8 Sz of term 1 taken from term 0 for dalpha                  node_acc and two_acc of P1-P5, P12, P13 (14).  old: no (dalpha is never requested)
  - the parent commit's n3d_affine_act_bwd_apply_gn2 (no      test_apply_gn2_refuses_more_than_four_samples: N3D_OK instead of
    B <= GNF_MAXB refusal)                                      N3D_ERR_UNSUPPORTED.  old: no"""
import ctypes

import numpy as np
import pytest
import torch

import _epilogue_ref as R
import _pair_ref as P
from _util import assert_close
from test_gpu_epilogue_reference import SENTINEL, Bufs

pytestmark = pytest.mark.gpu

TOL_FWD, TOL_DX, TOL_PARAM, TOL_ALPHA, TOL_ROWS = 2e-5, 1e-4, 1e-4, 2e-4, 1e-5
ULP_BF16 = 2.0 ** -8
N3D_OK, N3D_ERR_INVALID, N3D_ERR_UNSUPPORTED = 0, -1, -2
MOVED = "%s: route moved, pick a new shape (%s)"

# pitch = C + 4 * k, front offset = 4 * j channels: every operand of a call its own (in bf16 storage 4 channels are 8 bytes, so the
# odd j give slices that are only 8-byte aligned)
PITCH = {"raw0": (2, 2), "raw1": (1, 1), "out": (5, 3), "out1": (3, 0), "dout": (4, 4), "dout1": (7, 5), "draw0": (6, 6), "draw1": (8, 7)}
PAIR_ENTRIES = ("n3d_affine_act_gn2", "n3d_gn_coeffs2", "n3d_affine_act2", "n3d_affine_act_bwd_reduce2", "n3d_affine_act_bwd_apply_gn2",
                "n3d_gn_bwd_coeffs2", "n3d_affine_act_bwd_apply2", "n3d_affine_act_bwd_small", "n3d_affine_act_bwd_small2")
FWD_CALLS = {True: ["n3d_affine_act_gn2"], False: ["n3d_gn_coeffs2", "n3d_affine_act2"]}
BWD_CALLS = {"small": ["n3d_affine_act_bwd_small"], "apply_gn2": ["n3d_affine_act_bwd_reduce2", "n3d_affine_act_bwd_apply_gn2"],
             "apply2": ["n3d_affine_act_bwd_reduce2", "n3d_gn_bwd_coeffs2", "n3d_affine_act_bwd_apply2"]}


def _K():
    from nas_3d_unet_amd import kernels as K
    assert K._stats_cache is None
    return K


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """a device fault ends the session: nothing more is started on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU fault, no further test is started: %s" % e, returncode=3)


class Calls:
    """records which of the pair entry points of the library a block of wrapper calls goes through"""

    def __init__(self, K):
        self.lib, self.names, self.orig = K._lib.load(), [], {}

    def __enter__(self):
        for n in PAIR_ENTRIES:
            fn = getattr(self.lib, n)
            self.orig[n] = fn
            setattr(self.lib, n, self._recorder(n, fn))
        return self

    def _recorder(self, n, fn):
        def call(*a):
            self.names.append(n)
            return fn(*a)
        return call

    def __exit__(self, *exc):
        for n, fn in self.orig.items():
            setattr(self.lib, n, fn)
        return False


def _scalar(w):
    return None if w is None else torch.tensor([w], dtype=torch.float32, device="cuda")


def _param(a, nan_grad=True):
    """a parameter whose gradient target starts as NaN (kernels.grad_target writes into `_n3d_grad` in place)"""
    p = torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    if nan_grad:
        p._n3d_grad = torch.full_like(p.data, float("nan"))
    return p


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _assert_route(K, cid):
    """the route the case table names, from the library's and the wrappers' own predicates"""
    c = P.PAIR_CASES[cid]
    N = int(np.prod(c.shape))
    msg = MOVED % (cid, c.note)
    m = P.ew_map(N, c.C)
    assert K.fused_max_rows() == P.FUSED_MAX_ROWS, msg
    assert K.stats_rows(N, c.C) == m.rows == c.rows and m.iters == c.iters, msg
    assert K.pair_shape_ok(c.C), msg
    assert K.pair_ok(c.C, c.G, c.rows, c.rows, c.B) == c.fused, msg
    assert int(K._lib.load().n3d_bwd_small_mode(c.B, N, c.C, c.G)) == c.small, msg
    K._small_modes.pop((c.B, N, c.C, c.G), None)          # (test_gpu_pair.py forces mode 2 on for the shape of P4 and leaves it on)
    assert K.small_backward_mode(c.B, N, c.C, c.G) == (1 if c.small == 1 else 0), msg
    assert P.routes(c, K.fused_max_rows()) == (c.rows, c.iters, c.ragged, c.fused, c.small), msg


def _bwd_plans(c, v):
    """[(how the backward is called, the route it must take)]: auto = K.affine_act_bwd_gn2 as the trainers call it, two_launch = the same
    with SMALL_NODE_BACKWARD off, small = K.affine_act_bwd_small with mode 2 switched on (as test_one_launch_epilogue_backward does)"""
    two = "apply_gn2" if c.fused else "apply2"
    if v.dalpha or c.small == 0:
        return [("auto", two)]
    if c.small == 1:
        return [("auto", "small"), ("two_launch", two)]
    return [("small", "small"), ("auto", two)]


class Run:
    """one variant of one case on the device: operands (pitched: each a channel slice with its own pitch and offset), the forward, and
    any number of backward calls on fresh NaN d(raw) slices"""

    def __init__(self, K, cid, v, pitched, dtype=torch.float32, inp=None):
        self.K, self.cid, self.c, self.v, self.pitched = K, cid, P.PAIR_CASES[cid], v, pitched
        self.inp = P.pair_inputs(cid) if inp is None else inp
        self.bufs = Bufs(K, dtype)
        c, inp = self.c, self.inp
        self.shape5 = (c.B, c.C) + c.shape
        self.N = int(np.prod(c.shape))
        self.raw = [self.view("raw%d" % k, inp["terms"][k]["raw"]) for k in range(2)]
        self.dout = self.view("dout", inp["dout"])
        self.dout1 = self.view("dout1", inp["dout1"]) if v.two else None
        self.gamma = [_param(inp["terms"][k]["gamma"]) for k in range(2)]
        self.beta = [_param(inp["terms"][k]["beta"]) for k in range(2)]
        self.wt = [_scalar(w) for w in P.variant_weights(v)]
        self.bias = v.bias and c.G > 0          # include/n3d.h: dbias_conv must not be requested with padded channels

    def view(self, name, arr):
        if not self.pitched:
            return self.bufs.view(arr)
        k, j = PITCH[name]
        return self.bufs.view(arr, arr.shape[1] + 4 * k, 4 * j)

    def forward(self):
        K, c, v, inp = self.K, self.c, self.v, self.inp
        nan = np.full(self.shape5, np.nan, np.float32)
        self.out = self.view("out", inp["prev"] if v.acc else nan)
        # two-output mode under N3D_ACCUMULATE: out1 starts with real numbers, which the kernel must overwrite, not add to
        self.out1 = self.view("out1", inp["prev1"] if v.acc else nan) if v.two else None
        self.stats = [K.channel_stats(r) for r in self.raw]
        assert all(rows == c.rows for _, rows in self.stats)
        with Calls(K) as calls:
            self.saved = K.affine_act_gn2([(self.raw[k], self.stats[k][0], self.stats[k][1], self.gamma[k], self.beta[k], self.wt[k], v.relu[k])
                                           for k in range(2)], c.G, R.EPS, self.out, K.ACCUMULATE if v.acc else 0, self.out1)
        assert calls.names == FWD_CALLS[c.fused], MOVED % (self.cid, c.note) + ": forward went through %s" % calls.names
        res = dict(out=_np(self.out.t), out1=_np(self.out1.t) if v.two else None)
        for k in range(2):
            a, b, mr, sr = self.saved[k]
            res[k] = dict(stats=_np(self.stats[k][0].sum(1)), a=_np(a), b=_np(b), mean_rstd=_np(mr), sumraw=_np(sr))
        return res

    def _bwd_term(self, k, draw, sums=None, rows=0, dalpha=None, coef=(None, None, None), grads=(None, None, None)):
        """n3d_gn_bwd_term of term k for the direct C ABI calls"""
        L = self.K._lib
        a, b, mr, sr = self.saved[k]
        p = lambda t: None if t is None else t.data_ptr()
        return L.GnBwdTerm(self.raw[k].p.value, self.raw[k].ld, a.data_ptr(), b.data_ptr(), p(sums), rows, 1 if self.v.relu[k] else 0,
                           self.gamma[k].data_ptr(), mr.data_ptr(), p(self.wt[k]), sr.data_ptr(), draw.p.value if draw is not None else None,
                           draw.ld if draw is not None else 0, p(grads[0]), p(grads[1]), dalpha, p(grads[2]), p(coef[0]), p(coef[1]), p(coef[2]),
                           self.raw[k].dt, 0)

    def _dout1(self):
        return (self.dout1.p, self.dout1.ld) if self.dout1 is not None else (None, 0)

    def reduce_rows(self):
        """n3d_affine_act_bwd_reduce2 called directly (the wrappers keep its rows to themselves): [B][C][3] sums over the rows, per term"""
        K, c = self.K, self.c
        sums = torch.full((2, c.B, c.rows, c.C, 3), float("nan"), dtype=torch.float64, device="cuda")
        ts = [self._bwd_term(k, None, sums[k], c.rows) for k in range(2)]
        d1p, d1ld = self._dout1()
        K._lib.check(K._lib.load().n3d_affine_act_bwd_reduce2(self.dout.p, self.dout.ld, d1p, d1ld, ctypes.byref(ts[0]), ctypes.byref(ts[1]),
                                                             c.B, self.N, c.C, K.stream_ptr()), "n3d_affine_act_bwd_reduce2")
        return [_np(sums[k].sum(1)) for k in range(2)]

    def backward(self, how, route):
        K, c, v = self.K, self.c, self.v
        draws = [self.view("draw%d" % k, np.full(self.shape5, np.nan, np.float32)) for k in range(2)]
        da = torch.full((2,), float("nan"), device="cuda") if v.dalpha else None
        cbs = [_param(np.zeros(c.C, np.float32)) if self.bias else None for _ in range(2)]
        for p in self.gamma + self.beta:
            p._n3d_grad = torch.full_like(p.data, float("nan"))
        tl = [dict(raw=self.raw[k], a=self.saved[k][0], b=self.saved[k][1], mr=self.saved[k][2], sumraw=self.saved[k][3], gamma=self.gamma[k],
                   beta=self.beta[k], wptr=self.wt[k], relu=v.relu[k], conv_bias=cbs[k], draw=draws[k],
                   dalpha_ptr=(da.data_ptr() + 4 * k) if v.dalpha else None) for k in range(2)]
        key = (c.B, self.N, c.C, c.G)
        prev_small = K.SMALL_NODE_BACKWARD
        K._small_modes.pop(key, None)
        try:
            with Calls(K) as calls:
                if how == "small":
                    assert not v.dalpha
                    K._small_modes[key] = c.small            # (the trainers leave mode 2 off; this runs the kernel)
                    outs = K.affine_act_bwd_small(self.dout, tl, c.G, self.dout1)
                else:
                    K.SMALL_NODE_BACKWARD = how != "two_launch"
                    outs = K.affine_act_bwd_gn2(self.dout, tl, c.G, self.dout1)
        finally:
            K.SMALL_NODE_BACKWARD = prev_small
            K._small_modes.pop(key, None)
        assert calls.names == BWD_CALLS[route], MOVED % (self.cid, c.note) + ": backward (%s) went through %s" % (how, calls.names)
        res = {}
        for k in range(2):
            dg, db, dcb = outs[k]
            assert (dcb is not None) == self.bias
            res[k] = dict(draw=_np(draws[k].t), dgamma=_np(dg), dbeta=_np(db), dbias_conv=_np(dcb), dalpha=_np(da[k:k + 1]) if v.dalpha else None)
        return res

    def finish(self):
        torch.cuda.synchronize()
        self.bufs.check_guards()


def _check_forward(tag, c, v, got, ref):
    out, out1, terms = ref
    real = R.real_channels(c.C, c.G)
    for k in range(2):
        g, t = got[k], terms[k]
        assert_close(g["stats"], t["stats"], TOL_ROWS, tag + "stats %d" % k)
        assert_close(g["a"], t["a"], TOL_FWD, tag + "a %d" % k)
        assert_close(g["b"], t["b"], TOL_FWD, tag + "b %d" % k)
        assert_close(g["mean_rstd"], t["mean_rstd"], TOL_FWD, tag + "mean_rstd %d" % k)
        assert_close(g["sumraw"], t["sumraw"], TOL_ROWS, tag + "sumraw %d" % k)
        if c.G < 0:
            for n in ("a", "b", "sumraw", "stats"):
                assert not g[n][:, real:].any(), tag + "%s %d of a padded channel" % (n, k)
    assert_close(got["out"], out, TOL_FWD, tag + "out")
    if v.two:
        # (under N3D_ACCUMULATE out1 held prev1 before the launch: an accumulating kernel would be off by it)
        assert_close(got["out1"], out1, TOL_FWD, tag + "out1 (overwritten, never accumulated into)")
    if c.G < 0:
        assert not got["out"][:, real:].any() and (not v.two or not got["out1"][:, real:].any()), tag + "forward of a padded channel"


def _check_rows(tag, got, terms):
    for k in range(2):
        for j, name in enumerate(("S1", "S2", "Sz")):
            assert_close(got[k][..., j], terms[k]["sums"][..., j], TOL_ROWS, tag + "%s of term %d" % (name, k))


def _check_backward(tag, c, v, bias, got, terms):
    real = R.real_channels(c.C, c.G)
    for k in range(2):
        g, t = got[k], terms[k]
        assert_close(g["draw"], t["draw"], TOL_DX, tag + "d raw %d" % k)
        assert_close(g["dgamma"], t["dgamma"], TOL_PARAM, tag + "dgamma %d" % k)
        assert_close(g["dbeta"], t["dbeta"], TOL_PARAM, tag + "dbeta %d" % k)
        if v.dalpha:
            assert_close(g["dalpha"], t["dalpha"], TOL_ALPHA, tag + "dalpha %d = <dout_%d, z_%d>" % (k, k if v.two else 0, k))
        if bias:
            assert_close(g["dbias_conv"], t["dbias_conv"], TOL_PARAM, tag + "dbias_conv %d" % k)
        if c.G < 0:
            assert_close(g["draw"][:, real:], t["draw"][:, real:], TOL_DX, tag + "d raw %d of the padded channels (the group's coupling term)" % k)
            assert not g["dgamma"][real:].any() and not g["dbeta"][real:].any(), tag + "parameter gradients of a padded channel"


def _run_variant(cid, name, pitched):
    K = _K()
    c, v = P.PAIR_CASES[cid], P.VARIANTS[name]
    _assert_route(K, cid)
    ref = P.pair_reference(cid, v)
    run = Run(K, cid, v, pitched)
    tag = "%s %s %s: " % (cid, name, "pitched" if pitched else "dense")
    _check_forward(tag, c, v, run.forward(), ref)
    _check_rows(tag, run.reduce_rows(), ref[2])
    plans = _bwd_plans(c, v)
    if v.dalpha:
        assert [r for _, r in plans] == ["apply_gn2" if c.fused else "apply2"]       # never the one-launch route
    for how, route in plans:
        _check_backward(tag + route + ": ", c, v, run.bias, run.backward(how, route), ref[2])
    run.finish()
    return [r for _, r in plans]


CASE_VARIANTS = [(cid, name) for cid, c in P.PAIR_CASES.items() for name in c.variants]
# everything a case runs, case by case (a case's inputs and fp64 references are built once and dropped when the next case starts)
CASE_RUNS = [(cid, kind) for cid, c in P.PAIR_CASES.items()
             for kind in c.variants + ("dense", "single_launches") + (("bf16",) if cid in P.BF16_CASES else ())]


@pytest.mark.parametrize("cid,kind", CASE_RUNS, ids=["%s-%s" % ck for ck in CASE_RUNS])
def test_pair_case(cid, kind):
    """kind = a variant of _pair_ref.VARIANTS: forward and backward against the fp64 reference with every activation operand a channel
    slice of its own wider buffer (PITCH), sentinels around the slices, outputs starting as NaN;
    dense: the control, the case's first variant on dense tensors (ld == C);
    single_launches: the pair forward bit-equal to the two single-term launches; bf16: bf16 storage against fp32 storage"""
    if kind == "dense":
        _run_variant(cid, P.PAIR_CASES[cid].variants[0], False)
    elif kind == "single_launches":
        _forward_equals_single_launches(cid)
    elif kind == "bf16":
        _bf16_storage(cid)
    else:
        _run_variant(cid, kind, True)


def test_every_option_on_every_route():
    """the case table and the plans above put every option on both forward routes and on each backward route it can reach (no device
    work: this is the table's own bookkeeping, kept beside the plans it depends on)"""
    fwd, bwd = {True: set(), False: set()}, {"small": set(), "apply_gn2": set(), "apply2": set()}
    for cid, name in CASE_VARIANTS:
        c, v = P.PAIR_CASES[cid], P.VARIANTS[name]
        opts = {("relu",) + v.relu, ("w",) + v.w, ("two", v.two), ("acc", v.acc)}
        fwd[c.fused] |= opts | ({"padded"} if c.G < 0 else set())
        for _, route in _bwd_plans(c, v):
            bwd[route] |= {("relu",) + v.relu, ("w",) + v.w, ("dout1", v.two), ("dalpha", v.dalpha), ("bias", v.bias and c.G > 0)}
            bwd[route] |= {"padded"} if c.G < 0 else set()
    relus = {("relu", a, b) for a in (True, False) for b in (True, False)}
    for fused in (True, False):
        assert relus <= fwd[fused] and {("w", True, True), ("w", False, True), "padded"} <= fwd[fused]
        assert {("two", t) for t in (True, False)} | {("acc", t) for t in (True, False)} <= fwd[fused]
    for route in ("apply_gn2", "apply2"):
        assert relus | {("w", True, True), ("w", False, True), ("dout1", True), ("dout1", False), ("dalpha", True), ("bias", True), "padded"} <= bwd[route]
    # the one-launch route takes neither dalpha nor padded channels
    assert relus | {("w", True, True), ("w", False, True), ("dout1", True), ("dout1", False), ("bias", True)} <= bwd["small"]
    assert ("dalpha", True) not in bwd["small"] and "padded" not in bwd["small"]


def _forward_equals_single_launches(cid):
    """the cross-route identity of test_gpu_pair.py on pitched operands, with both weights: the pair forward (node mode) is bit-equal to
    the two single-term launches it replaces (term 0 written, term 1 accumulated), whichever coefficient route either side takes"""
    K = _K()
    c = P.PAIR_CASES[cid]
    _assert_route(K, cid)
    v = P.Variant(((True, False), (False, True), (True, True), (False, False))[list(P.PAIR_CASES).index(cid) % 4], (True, True), False, False, False, False)
    run = Run(K, cid, v, True)
    run.forward()
    single = run.view("out1", np.full(run.shape5, np.nan, np.float32))       # (another pitch than the pair's output)
    for k in range(2):
        fl = (K.RELU if v.relu[k] else 0) | (K.ACCUMULATE if k else 0)
        st, rows = run.stats[k]
        if rows <= K.fused_max_rows():
            a, b, _, _ = K.affine_act_gn(run.raw[k], st, rows, run.gamma[k], run.beta[k], c.G, R.EPS, run.wt[k].data_ptr(), single, fl)
        else:
            a, b, _, _ = K.gn_coeffs(st, rows, run.gamma[k], run.beta[k], c.B, c.C, c.G, run.N, R.EPS)
            K.affine_act(run.raw[k], a, b, run.wt[k].data_ptr(), single, fl)
        assert torch.equal(a, run.saved[k][0]) and torch.equal(b, run.saved[k][1]), "saved coefficients of term %d differ from the single form's" % k
    assert torch.equal(single.t, run.out.t), "pair forward differs from the two single launches"
    run.finish()


# ================================================================================================= bf16 storage
def _bf16_storage(cid):
    """every activation tensor in bf16 storage (pitched; 8-byte aligned slices at C = 4) against the same launches in fp32 storage on the
    bf16-rounded operands, as test_gpu_bf16.test_node_epilogues_bf16_storage does: one rounding of a stored tensor, 1e-5 where fp32"""
    K = _K()
    c = P.PAIR_CASES[cid]
    _assert_route(K, cid)
    rnd = lambda a: torch.from_numpy(a).bfloat16().float().numpy()
    src = P.pair_inputs(cid)
    inp16 = {k: rnd(src[k]) for k in ("dout", "dout1", "prev", "prev1")}
    inp16["terms"] = [dict(t, raw=rnd(t["raw"])) for t in src["terms"]]
    for name in c.variants:
        v = P.VARIANTS[name]
        res = {}
        for dt in (torch.float32, torch.bfloat16):
            run = Run(K, cid, v, True, dt, inp16)
            fwd = run.forward()
            rows = run.reduce_rows()
            bwd = [run.backward(how, route) for how, route in _bwd_plans(c, v)]
            run.finish()
            res[dt] = (fwd, rows, bwd)
        (f32, r32, b32), (f16, r16, b16) = res[torch.float32], res[torch.bfloat16]
        tag = "%s %s bf16: " % (cid, name)
        for k in range(2):
            for n in ("stats", "sumraw", "a", "b", "mean_rstd"):          # the same fp32 arithmetic on the same values
                assert np.array_equal(f16[k][n], f32[k][n]), tag + "%s %d" % (n, k)
            assert_close(r16[k], r32[k], 1e-5, tag + "reduction rows %d" % k)
        assert_close(f16["out"], f32["out"], ULP_BF16, tag + "out")
        if v.two:
            assert_close(f16["out1"], f32["out1"], ULP_BF16, tag + "out1")
        for g16, g32, (how, route) in zip(b16, b32, _bwd_plans(c, v)):
            for k in range(2):
                assert_close(g16[k]["draw"], g32[k]["draw"], ULP_BF16, tag + route + " d raw %d" % k)
                for n in ("dgamma", "dbeta", "dalpha", "dbias_conv"):
                    if g32[k][n] is not None:
                        assert_close(g16[k][n], g32[k][n], 1e-5, tag + route + " %s %d" % (n, k))


# ================================================================================================= the C ABI, called directly
def _direct_small(run, entry, reps=3, scratch=None, tickets=None):
    """`reps` launches of one of the one-launch entry points on fresh outputs; [(draw0, draw1, dgamma0, dbeta0, dcb0, dgamma1, ...)]"""
    K, c = run.K, run.c
    lib = K._lib.load()
    d1p, d1ld = run._dout1()
    results = []
    for _ in range(reps):
        draws = [run.view("draw%d" % k, np.full(run.shape5, np.nan, np.float32)) for k in range(2)]
        grads = [[torch.full((c.C,), float("nan"), device="cuda") for _ in range(3)] for _ in range(2)]
        ts = [run._bwd_term(k, draws[k], grads=grads[k]) for k in range(2)]
        args = (run.dout.p, run.dout.ld, d1p, d1ld, ctypes.byref(ts[0]), ctypes.byref(ts[1]), c.B, run.N, c.C, c.G)
        if entry == "n3d_affine_act_bwd_small2":
            st = lib.n3d_affine_act_bwd_small2(*args, K.stream_ptr())
        else:
            st = lib.n3d_affine_act_bwd_small(*args, scratch.data_ptr() if scratch is not None else None, scratch.numel() * 8 if scratch is not None else 0,
                                              tickets.data_ptr() if tickets is not None else None, K.stream_ptr())
        K._lib.check(st, entry)
        torch.cuda.synchronize()
        if tickets is not None:
            assert not bool(tickets.any()), "the ticket words are not back at zero after the launch"
        results.append([d.t.clone() for d in draws] + grads[0] + grads[1])
    return results


@pytest.mark.parametrize("name", ["node", "two"])
def test_small2_entry_point_is_the_small_one(name):
    """n3d_affine_act_bwd_small2 (no Python path calls it) on P1: bit-equal to n3d_affine_act_bwd_small on the same pitched operands,
    each launched three times with repeating results, and right against the fp64 reference"""
    K = _K()
    cid, v = "P1", P.VARIANTS[name]
    c = P.PAIR_CASES[cid]
    _assert_route(K, cid)
    assert c.small == 1 and not v.dalpha and int(K._lib.load().n3d_bwd_small2_ok(c.B, int(np.prod(c.shape)), c.C, c.G)) == 1
    run = Run(K, cid, v, True)
    run.forward()
    tick = torch.zeros(c.G, dtype=torch.int32, device="cuda")
    a = _direct_small(run, "n3d_affine_act_bwd_small2")
    b = _direct_small(run, "n3d_affine_act_bwd_small", tickets=tick)
    for r in a[1:] + b:
        assert all(torch.equal(x, y) for x, y in zip(r, a[0])), "a repeated launch, or the other entry point, gives other bits"
    terms = P.pair_reference(cid, v)[2]
    for k in range(2):
        assert_close(a[0][k], terms[k]["draw"], TOL_DX, "d raw %d" % k)
        assert_close(a[0][2 + 3 * k], terms[k]["dgamma"], TOL_PARAM, "dgamma %d" % k)
        assert_close(a[0][3 + 3 * k], terms[k]["dbeta"], TOL_PARAM, "dbeta %d" % k)
        assert_close(a[0][4 + 3 * k], terms[k]["dbias_conv"], TOL_PARAM, "dbias_conv %d" % k)
    run.finish()


def test_small_mode2_tickets_repeat():
    """mode 2 (P4: one workgroup per group and sample, parameter gradients by ticket) three times on the same ticket words: they are
    zero again after every launch and the results repeat bit for bit"""
    K = _K()
    cid, v = "P4", P.VARIANTS["two"]
    c = P.PAIR_CASES[cid]
    _assert_route(K, cid)
    assert c.small == 2
    run = Run(K, cid, v, True)
    run.forward()
    tick = torch.zeros(c.G, dtype=torch.int32, device="cuda")
    scratch = torch.full((int(K._lib.load().n3d_bwd_small_scratch_bytes(c.B, c.G)) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    r = _direct_small(run, "n3d_affine_act_bwd_small", scratch=scratch, tickets=tick)
    for x in r[1:]:
        assert all(torch.equal(p, q) for p, q in zip(x, r[0])), "a repeated launch differs (ticket words not reset?)"
    terms = P.pair_reference(cid, v)[2]
    for k in range(2):
        assert_close(r[0][k], terms[k]["draw"], TOL_DX, "d raw %d" % k)
        assert_close(r[0][2 + 3 * k], terms[k]["dgamma"], TOL_PARAM, "dgamma %d" % k)
        assert_close(r[0][4 + 3 * k], terms[k]["dbias_conv"], TOL_PARAM, "dbias_conv %d" % k)
    run.finish()


# ================================================================================================= refusals: nothing is launched
class Abi:
    """fully sized, valid dense operands of the pair entry points for (B, C, shape, G); every tensor an entry point may write holds a
    sentinel, so a refused call can be shown to have touched nothing"""

    def __init__(self, K, B, C, shape, G=1, rows=None):
        self.K, self.B, self.C, self.G, self.N = K, B, C, G, int(np.prod(shape))
        self.rows = K.stats_rows(self.N, C) if rows is None else rows
        ng, N, rows = R.n_groups(G), self.N, self.rows
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
        self.outs = []

        def o(*s, dt=torch.float32):
            t = torch.full(s, SENTINEL, dtype=dt, device="cuda")
            self.outs.append(t)
            return t
        f64 = torch.float64
        self.dout, self.dout1, self.out, self.out1 = z(B * N * C), z(B * N * C), o(B * N * C), o(B * N * C)
        self.t = []
        for _ in range(2):
            mr = z(B, ng, 2)
            mr[..., 1] = 1.0
            self.t.append(dict(raw=z(B * N * C), stats=z(B, rows, C, 2, dt=f64), gamma=torch.ones(C, device="cuda"), beta=z(C), a=torch.ones(B, C, device="cuda"),
                               b=z(B, C), mr=mr, sumraw=z(B, C, dt=f64), a_out=o(B, C), b_out=o(B, C), mr_out=o(B, ng, 2), sr_out=o(B, C, dt=f64),
                               sums=o(B, rows, C, 3, dt=f64), draw=o(B * N * C), dgamma=o(C), dbeta=o(C), dalpha=o(1), dbias=o(C), cA=o(B, C), cB=o(B, C),
                               cC=o(B, C)))

    def fwd(self, k, rows=None, dtype=0):
        L, t = self.K._lib, self.t[k]
        return L.GnFwdTerm(t["raw"].data_ptr(), self.C, t["stats"].data_ptr(), self.rows if rows is None else rows, 1, t["gamma"].data_ptr(),
                           t["beta"].data_ptr(), None, t["a_out"].data_ptr(), t["b_out"].data_ptr(), t["mr_out"].data_ptr(), t["sr_out"].data_ptr(), dtype, 0)

    def bwd(self, k, rows=None, dalpha=False, dbias=False, sumraw=True, dtype=0):
        L, t = self.K._lib, self.t[k]
        return L.GnBwdTerm(t["raw"].data_ptr(), self.C, t["a"].data_ptr(), t["b"].data_ptr(), t["sums"].data_ptr(), self.rows if rows is None else rows, 1,
                           t["gamma"].data_ptr(), t["mr"].data_ptr(), None, t["sumraw"].data_ptr() if sumraw else None, t["draw"].data_ptr(), self.C,
                           t["dgamma"].data_ptr(), t["dbeta"].data_ptr(), t["dalpha"].data_ptr() if dalpha else None,
                           t["dbias"].data_ptr() if dbias else None, t["cA"].data_ptr(), t["cB"].data_ptr(), t["cC"].data_ptr(), dtype, 0)

    # ---- the entry points on these operands; t0 / t1: structures from fwd() / bwd()
    def gn2(self, t0, t1, G=None):
        return self.K._lib.load().n3d_affine_act_gn2(ctypes.byref(t0), ctypes.byref(t1), self.G if G is None else G, R.EPS, self.out.data_ptr(), self.C,
                                                      None, 0, self.B, self.N, self.C, 0, self.K.stream_ptr())

    def _b(self, name, t0, t1, *tail):
        fn = getattr(self.K._lib.load(), name)
        return fn(self.dout.data_ptr(), self.C, None, 0, ctypes.byref(t0), ctypes.byref(t1), self.B, self.N, self.C, *tail, self.K.stream_ptr())

    def reduce2(self, t0, t1):
        return self._b("n3d_affine_act_bwd_reduce2", t0, t1)

    def apply_gn2(self, t0, t1, G=None):
        return self._b("n3d_affine_act_bwd_apply_gn2", t0, t1, self.G if G is None else G)

    def apply2(self, t0, t1):
        return self._b("n3d_affine_act_bwd_apply2", t0, t1)

    def small2(self, t0, t1, G=None):
        return self._b("n3d_affine_act_bwd_small2", t0, t1, self.G if G is None else G)

    def small(self, t0, t1, G=None):
        return self._b("n3d_affine_act_bwd_small", t0, t1, self.G if G is None else G, None, 0, None)

    def coeffs2(self, t0, t1):
        return self.K._lib.load().n3d_gn_bwd_coeffs2(ctypes.byref(t0), ctypes.byref(t1), self.B, self.C, self.G, self.N, self.K.stream_ptr())

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.outs)


def test_apply_gn2_refuses_more_than_four_samples():
    """include/n3d.h: "B <= 4 for the backward apply; otherwise N3D_ERR_UNSUPPORTED".  On P7 (2 rows, B = 5), with valid buffers for all
    five samples: the parameter-gradient wave of n3d_affine_act_bwd_apply_gn2 holds GNF_MAXB = 4 samples, so an accepted call would sum
    dgamma / dbeta / dalpha / dbias_conv over four of the five and say N3D_OK"""
    K = _K()
    c = P.PAIR_CASES["P7"]
    _assert_route(K, "P7")
    assert c.B == 5 and c.rows <= K.fused_max_rows()
    ab = Abi(K, c.B, c.C, c.shape, c.G)
    st = ab.apply_gn2(ab.bwd(0, dalpha=True, dbias=True), ab.bwd(1, dalpha=True, dbias=True))
    assert st == N3D_ERR_UNSUPPORTED, "n3d_affine_act_bwd_apply_gn2 took B = 5 (status %d)" % st
    assert ab.untouched()
    # four samples of the same buffers are taken
    ab.B = 4
    assert ab.apply_gn2(ab.bwd(0), ab.bwd(1)) == N3D_OK
    assert not ab.untouched()


def test_pair_refuses_a_channel_count_that_is_no_power_of_two():
    K = _K()
    ab = Abi(K, 2, 12, (4, 4, 4))
    assert ab.gn2(ab.fwd(0), ab.fwd(1)) == N3D_ERR_UNSUPPORTED
    assert ab.reduce2(ab.bwd(0), ab.bwd(1)) == N3D_ERR_UNSUPPORTED
    assert ab.apply_gn2(ab.bwd(0), ab.bwd(1)) == N3D_ERR_UNSUPPORTED
    assert ab.small(ab.bwd(0), ab.bwd(1)) == N3D_ERR_UNSUPPORTED
    assert ab.small2(ab.bwd(0), ab.bwd(1)) == N3D_ERR_UNSUPPORTED
    assert not K.pair_ok(12, 1, ab.rows, ab.rows, 2) and not K.pair_shape_ok(12) and K.small_backward_mode(2, 64, 12, 1) == 0
    assert ab.untouched()


def test_pair_refuses_more_than_16_channels_per_group():
    K = _K()
    ab = Abi(K, 2, 32, (4, 4, 4), 2)        # (buffers for two groups; asked for as ONE group of 32 channels)
    assert ab.gn2(ab.fwd(0), ab.fwd(1), G=1) == N3D_ERR_UNSUPPORTED
    assert ab.apply_gn2(ab.bwd(0), ab.bwd(1), G=1) == N3D_ERR_UNSUPPORTED
    assert ab.small(ab.bwd(0), ab.bwd(1), G=1) == N3D_ERR_UNSUPPORTED
    assert ab.small2(ab.bwd(0), ab.bwd(1), G=1) == N3D_ERR_UNSUPPORTED
    assert not K.pair_ok(32, 1, ab.rows, ab.rows, 2) and K.pair_ok(32, 2, ab.rows, ab.rows, 2)
    assert ab.untouched()
    assert ab.gn2(ab.fwd(0), ab.fwd(1)) == N3D_OK            # the same operands in two groups are taken
    assert not ab.untouched()


def test_fused_pair_refuses_more_rows_than_the_fused_limit():
    """P6's shape (66 rows of real size): either term over the limit refuses the fused forward and the fused backward apply"""
    K = _K()
    c = P.PAIR_CASES["P6"]
    ab = Abi(K, c.B, c.C, c.shape, c.G)
    fmax = K.fused_max_rows()
    assert ab.rows == c.rows == fmax + 2
    for r0, r1 in ((ab.rows, ab.rows), (fmax, fmax + 1), (fmax + 1, fmax), (0, fmax)):
        assert ab.gn2(ab.fwd(0, r0), ab.fwd(1, r1)) == N3D_ERR_UNSUPPORTED, (r0, r1)
        assert ab.apply_gn2(ab.bwd(0, r0), ab.bwd(1, r1)) == N3D_ERR_UNSUPPORTED, (r0, r1)
    assert not K.pair_ok(c.C, c.G, ab.rows, ab.rows, c.B) and not K.pair_ok(c.C, c.G, fmax, fmax + 1, c.B) and K.pair_ok(c.C, c.G, fmax, fmax, c.B)
    assert ab.untouched()


def test_small_entry_points_refuse_dalpha():
    K = _K()
    c = P.PAIR_CASES["P1"]
    ab = Abi(K, c.B, c.C, c.shape, c.G)
    for d0, d1 in ((True, False), (False, True)):
        assert ab.small(ab.bwd(0, dalpha=d0), ab.bwd(1, dalpha=d1)) == N3D_ERR_INVALID
        assert ab.small2(ab.bwd(0, dalpha=d0), ab.bwd(1, dalpha=d1)) == N3D_ERR_INVALID
    assert ab.untouched()


def test_pair_refuses_dbias_conv_without_sumraw():
    K = _K()
    c = P.PAIR_CASES["P1"]
    ab = Abi(K, c.B, c.C, c.shape, c.G)
    for k in (0, 1):
        ts = [ab.bwd(j, dbias=True, sumraw=(j != k)) for j in (0, 1)]
        assert ab.apply_gn2(*ts) == N3D_ERR_INVALID
        assert ab.small(*ts) == N3D_ERR_INVALID
        assert ab.small2(*ts) == N3D_ERR_INVALID
        assert ab.coeffs2(*ts) == N3D_ERR_INVALID
    assert ab.untouched()


def test_pair_refuses_terms_of_different_storage_types():
    K = _K()
    c = P.PAIR_CASES["P1"]
    ab = Abi(K, c.B, c.C, c.shape, c.G)
    for d0, d1 in ((K._lib.F32, K._lib.BF16), (K._lib.BF16, K._lib.F32)):
        ts = [ab.bwd(0, dtype=d0), ab.bwd(1, dtype=d1)]
        assert ab.reduce2(*ts) == N3D_ERR_INVALID
        assert ab.apply_gn2(*ts) == N3D_ERR_INVALID
        assert ab.apply2(*ts) == N3D_ERR_INVALID
        assert ab.small(*ts) == N3D_ERR_INVALID
        assert ab.small2(*ts) == N3D_ERR_INVALID
    assert ab.untouched()
    v32, v16 = K.as_view(torch.zeros(1, 4, 2, 2, 2, device="cuda")), K.as_view(torch.zeros(1, 4, 2, 2, 2, device="cuda", dtype=torch.bfloat16))
    with pytest.raises(K.N3DError):
        K._same_dt("pair", v32, v16)
