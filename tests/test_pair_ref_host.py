"""CPU: the pair reference and the case table of tests/_pair_ref.py, which test_gpu_pair_reference.py compares the two-term GroupNorm
epilogue kernels with -- ReLU margins of every term of every case, the weight-scaled closed forms against torch autograd with the weight
as a leaf, exact zeros on padded channels, and the route table against the library's own host functions."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _epilogue_ref as R
import _pair_ref as P

SMALL_CASES = [c for c in P.PAIR_CASES if c not in P.LARGE_CASES]       # (4.2 and 5.3 M elements per tensor belong to the GPU run)


@pytest.mark.parametrize("cid", SMALL_CASES)
def test_margin_of_pair_cases(cid):
    """either term may carry the ReLU, so both keep min|z| at or above the margin_inputs floor; distinct operands everywhere"""
    c, inp = P.PAIR_CASES[cid], P.pair_inputs(cid)
    real = R.real_channels(c.C, c.G)
    for t in inp["terms"]:
        assert t["zmin"] >= 5e-4 and t["passes"] <= 4
        assert float(np.abs(R.gn_z(t["raw"], c.G, t["gamma"], t["beta"])).min()) >= 5e-4
        assert (t["gamma"][:real] < 0).any() and np.abs(t["gamma"][:real]).min() >= 0.5
    tensors = [inp["terms"][0]["raw"], inp["terms"][1]["raw"], inp["dout"], inp["dout1"], inp["prev"], inp["prev1"]]
    assert len({a.tobytes() for a in tensors}) == 6
    assert all(a.shape == (c.B, c.C) + c.shape and a.dtype == np.float32 for a in tensors)


def test_margin_of_the_large_case_shapes():
    """the builder of P9 and P11 is the one of the others; their margin is asserted where their inputs are built (margin_inputs raises
    otherwise)"""
    for cid in P.LARGE_CASES:
        c = P.PAIR_CASES[cid]
        assert c.B == 1 and int(np.prod(c.shape)) > 65536 and set(c.variants) == {"node_acc", "two"}


@pytest.mark.parametrize("cid", ["P5", "P10"])
def test_padded_inputs_are_exactly_zero(cid):
    c, inp = P.PAIR_CASES[cid], P.pair_inputs(cid)
    real = R.real_channels(c.C, c.G)
    assert c.G < 0 and real == 6 and c.C == 8
    for t in inp["terms"]:
        assert not t["raw"][:, real:].any() and not t["gamma"][real:].any() and not t["beta"][real:].any()
        assert t["raw"][:, :real].all() and t["gamma"][:real].all()
    for k in ("dout", "dout1", "prev", "prev1"):
        assert not inp[k][:, real:].any() and inp[k][:, :real].any()
    for name, v in P.VARIANTS.items():
        out, out1, terms = P.pair_reference(cid, v)
        assert not out[:, real:].any() and (out1 is None or not out1[:, real:].any()), name
        for t in terms:
            for k in ("a", "b", "sumraw", "dgamma", "dbeta"):
                assert not np.moveaxis(t[k], -1, 0)[real:].any(), (name, k)
            assert t["draw"][:, real:].any(), "the twin's coupling term on the padded channels is not zero"


@pytest.mark.parametrize("cid,name", [("P1", "node"), ("P3", "node_acc"), ("P7", "two"), ("P2", "two_acc"), ("P5", "two_acc")])
def test_pair_reference_against_autograd(cid, name):
    """the pair reference (weight-1 terms, scaled) against ONE autograd graph of the whole pair with both weights as leaves"""
    c, inp, v = P.PAIR_CASES[cid], P.pair_inputs(cid), P.VARIANTS[name]
    real, g = R.real_channels(c.C, c.G), R.n_groups(c.G)
    out, out1, terms = P.pair_reference(cid, v)
    w = P.variant_weights(v)
    xs, ws, gs, bs, ys = [], [], [], [], []
    for k, t in enumerate(inp["terms"]):
        x = torch.from_numpy(np.ascontiguousarray(t["raw"][:, :real])).double().requires_grad_(True)
        wt = torch.tensor(R.w64(w[k]), dtype=torch.float64, requires_grad=True)
        gm = torch.from_numpy(t["gamma"][:real]).double().requires_grad_(True)
        bt = torch.from_numpy(t["beta"][:real]).double().requires_grad_(True)
        z = F.group_norm(x, g, gm, bt, R.EPS)
        ys.append(wt * (F.relu(z) if v.relu[k] else z))
        xs.append(x), ws.append(wt), gs.append(gm), bs.append(bt)
    d = [torch.from_numpy(inp[n][:, :real]).double() for n in ("dout", "dout1", "prev")]
    if v.two:
        y0 = ys[0] + d[2] if v.acc else ys[0]
        ((y0 * d[0]).sum() + (ys[1] * d[1]).sum()).backward()
        np.testing.assert_allclose(out[:, :real], y0.detach().numpy(), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(out1[:, :real], ys[1].detach().numpy(), rtol=1e-12, atol=1e-13)
    else:
        y = ys[0] + ys[1] + (d[2] if v.acc else 0.0)
        (y * d[0]).sum().backward()
        np.testing.assert_allclose(out[:, :real], y.detach().numpy(), rtol=1e-12, atol=1e-13)
    for k, t in enumerate(terms):
        np.testing.assert_allclose(t["draw"][:, :real], xs[k].grad.numpy(), rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(t["dgamma"][:real], gs[k].grad.numpy(), rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(t["dbeta"][:real], bs[k].grad.numpy(), rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(t["dalpha"], ws[k].grad.numpy().reshape(1), rtol=1e-9, atol=1e-10)
        dk = inp["dout1"] if (v.two and k) else inp["dout"]
        assert abs(R.dalpha_closed(dk, t["z"]) - float(t["dalpha"][0])) <= 1e-11 * abs(float(t["dalpha"][0])) + 1e-11
        if c.G > 0:
            np.testing.assert_allclose(R.dbias_conv_closed(t["draw"]), t["dbias_conv"], rtol=1e-10, atol=1e-10)


def test_scaled_term_is_the_weighted_term():
    """term_reference with the weight inside against the weight-1 reference scaled afterwards, field by field"""
    cid = "P2"
    c, inp = P.PAIR_CASES[cid], P.pair_inputs(cid)
    t = inp["terms"][1]
    for relu in (True, False):
        direct = R.term_reference(t["raw"], t["gamma"], t["beta"], c.G, relu, P.W1, inp["dout"])
        scaled = P.pair_term(cid, 1, relu, P.W1)
        assert set(direct) == set(scaled)
        for k in direct:
            np.testing.assert_allclose(scaled[k], direct[k], rtol=1e-12, atol=1e-13, err_msg=k)


def test_variants_cover_the_options():
    vs = list(P.VARIANTS.values())
    assert {v.relu for v in vs} == {(True, False), (False, True), (False, False), (True, True)}
    assert {(v.two, v.acc) for v in vs} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(v.w == (False, True) for v in vs) and any(v.w == (True, True) for v in vs) and P.W0 != P.W1
    assert any(v.dalpha and v.two for v in vs) and any(v.dalpha and not v.two for v in vs)
    assert any(v.bias and v.two for v in vs) and any(v.bias and not v.two for v in vs)
    assert any(not v.dalpha and v.two for v in vs) and any(not v.dalpha and not v.two for v in vs)      # what the one-launch route can take
    for cid in P.BF16_CASES:
        assert set(P.ALL) <= set(P.PAIR_CASES[cid].variants)
    # the cases the one-launch backward takes also run the ReLU pairs and the lone w1 that the dalpha variants would keep from it
    for cid, c in P.PAIR_CASES.items():
        assert (c.variants == P.SMALL) == (c.small != 0), cid
    small = [P.VARIANTS[n] for n in P.SMALL if not P.VARIANTS[n].dalpha]
    assert {v.relu for v in small} == {v.relu for v in vs} and any(v.w == (False, True) for v in small)


@pytest.mark.parametrize("cid", list(P.PAIR_CASES))
def test_route_table_against_the_library(cid):
    """rows, iters, the fused limit and the one-launch mode of every case from the library's host functions (no device needed)"""
    from nas_3d_unet_amd import _lib
    lib = _lib.load()
    c = P.PAIR_CASES[cid]
    N = int(np.prod(c.shape))
    fmax = int(lib.n3d_fused_max_rows())
    assert fmax == P.FUSED_MAX_ROWS, "n3d_fused_max_rows moved: revisit the routes of _pair_ref.PAIR_CASES"
    msg = "%s: route moved, pick a new shape (%s)" % (cid, c.note)
    assert int(lib.n3d_stats_rows(N, c.C)) == P.ew_map(N, c.C).rows == c.rows, msg
    assert int(lib.n3d_bwd_small_mode(c.B, N, c.C, c.G)) == P.small_mode(c.B, N, c.C, c.G) == c.small, msg
    assert int(lib.n3d_bwd_small2_ok(c.B, N, c.C, c.G)) == (1 if c.small == 1 else 0), msg
    assert P.routes(c, fmax) == (c.rows, c.iters, c.ragged, c.fused, c.small), msg


def test_row_mapping_restatement_against_the_library():
    """the Python ew_map against n3d_stats_rows over the sizes of both regimes and every channel count the pair kernels take"""
    from nas_3d_unet_amd import _lib
    lib = _lib.load()
    for C in (4, 8, 16, 32, 64):
        for N in list(range(1, 70)) + [96, 255, 256, 257, 512, 840, 1024, 2047, 2048, 2049, 4096, 5544, 16383, 16384, 16385, 32768, 33792,
                                       65535, 65536, 65537, 65600, 262144, 2097152]:
            assert P.ew_map(N, C).rows == int(lib.n3d_stats_rows(N, C)), (N, C)
    for B in (1, 2, 3, 4, 5):
        for C, G in ((4, 1), (8, 1), (16, 1), (32, 2), (64, 4), (8, -6), (64, 1)):
            for N in (8, 64, 96, 128, 256, 512, 840, 1024, 2048, 4096, 4097):
                assert P.small_mode(B, N, C, G) == int(lib.n3d_bwd_small_mode(B, N, C, G)), (B, N, C, G)


def test_table_reaches_what_the_issue_names():
    """the regimes the table exists for, stated on the table itself"""
    T = P.PAIR_CASES
    assert [c.iters for c in T.values()].count(4) >= 1 and T["P9"].iters > 4 and T["P9"].iters % 4 != 0       # a partial last group of four
    assert T["P11"].iters % 4 >= 2 and T["P11"].ragged                                                          # ... with two live slots
    assert {c.small for c in T.values()} == {0, 1, 2}
    assert T["P6"].rows > P.FUSED_MAX_ROWS and T["P8"].rows > P.FUSED_MAX_ROWS and T["P8"].ragged
    assert T["P7"].rows <= P.FUSED_MAX_ROWS and T["P7"].B > P.GNF_MAXB and not T["P7"].fused
    assert T["P2"].B == 3 and T["P3"].B == 4 and T["P3"].G == 4
    assert T["P5"].fused and T["P5"].G < 0 and not T["P10"].fused and T["P10"].G < 0
    # mode 1 at exactly two quads per thread: 2048 quads of the group in one 1024-thread workgroup
    assert T["P1"].B * (int(np.prod(T["P1"].shape)) * (T["P1"].C // T["P1"].G // 4)) == 2048
