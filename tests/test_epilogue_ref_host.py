"""CPU: the fp64 restatements and input builders of tests/_epilogue_ref.py, which test_gpu_epilogue_reference.py compares the HIP
kernels with -- the closed forms against torch autograd, the ReLU margins of every GPU case, the ties of every pooling tie input."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _epilogue_ref as R


@pytest.mark.parametrize("C,shape,B,G,relu,w", [(8, (2, 3, 4), 2, 1, True, 0.37), (32, (2, 2, 2), 3, 2, False, None)])
def test_closed_forms_against_autograd(C, shape, B, G, relu, w):
    """dalpha = <dout, z>, dbias_conv = channel sum of d(raw), sumraw, mean_rstd and the affine (a, b) against plain autograd /
    F.group_norm on a graph that has the weight and the conv bias as leaves"""
    rng = np.random.default_rng(C)
    gamma, beta = R.draw_gamma_beta(rng, C)
    raw, _, _ = R.margin_inputs(R.draw_tensor(rng, B, C, shape, None, 1.5, 0.3), G, gamma, beta)
    dout = R.draw_tensor(rng, B, C, shape)
    ref = R.term_reference(raw, gamma, beta, G, relu, w, dout)
    assert abs(R.dalpha_closed(dout, ref["z"]) - float(ref["dalpha"][0])) <= 1e-12 * abs(float(ref["dalpha"][0])) + 1e-12
    np.testing.assert_allclose(R.dbias_conv_closed(ref["draw"]), ref["dbias_conv"], rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(ref["sumraw"], raw.astype(np.float64).sum(axis=(2, 3, 4)), rtol=1e-12)
    # z = a * raw + b with the saved coefficients is GroupNorm itself; mean_rstd normalises every group to (0, 1)
    z = ref["a"][:, :, None, None, None] * raw + ref["b"][:, :, None, None, None]
    np.testing.assert_allclose(np.maximum(z, 0) if relu else z, ref["z"], rtol=1e-10, atol=1e-10)
    xg = raw.astype(np.float64).reshape(B, G, -1)
    xn = (xg - ref["mean_rstd"][..., :1]) * ref["mean_rstd"][..., 1:]
    np.testing.assert_allclose(xn.mean(-1), 0.0, atol=1e-12)
    np.testing.assert_allclose((xn * xn).mean(-1), 1.0, rtol=1e-4)        # (eps = 1e-5 inside the root)
    # the three reduction sums give back dgamma / dbeta: dbeta = w sum_b S1, dgamma = w sum_b rstd (S2 - mean S1)
    S1, S2 = ref["sums"][..., 0], ref["sums"][..., 1]
    cg = C // G
    mean_c, rstd_c = (np.repeat(ref["mean_rstd"][..., k], cg, axis=1) for k in (0, 1))
    np.testing.assert_allclose(R.w64(w) * S1.sum(0), ref["dbeta"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(R.w64(w) * (rstd_c * (S2 - mean_c * S1)).sum(0), ref["dgamma"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("relu", [True, False])
def test_padded_channel_count(relu):
    """6 real channels stored in 8: the padded twin (sums over all stored channels divided by N * 6) is GroupNorm(1, 6) on the real
    channels, forward and backward, and exactly 0 forward on the padded ones"""
    C, real, B, shape = 8, 6, 2, (2, 3, 4)
    rng = np.random.default_rng(7)
    gamma, beta = R.draw_gamma_beta(rng, C, real)
    raw, _, _ = R.margin_inputs(R.draw_tensor(rng, B, C, shape, real, 1.5, 0.3), -real, gamma, beta)
    dout = R.draw_tensor(rng, B, C, shape, real)
    assert not raw[:, real:].any() and not gamma[real:].any() and not beta[real:].any()
    ref = R.term_reference(raw, gamma, beta, -real, relu, 0.37, dout)
    z = R.twin_forward(torch.from_numpy(raw).double(), torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), real, relu).numpy()
    np.testing.assert_allclose(z[:, :real], ref["z"][:, :real], rtol=1e-10, atol=1e-10)
    assert not z[:, real:].any() and not ref["z"][:, real:].any() and not ref["dgamma"][real:].any() and not ref["dbeta"][real:].any()
    d = R.twin_draw(raw, gamma, beta, -real, relu, 0.37, dout)
    np.testing.assert_allclose(d[:, :real], ref["draw"][:, :real], rtol=1e-9, atol=1e-10)
    # plain torch on the 6 channels, nothing of ours in between
    x6 = torch.from_numpy(raw[:, :real]).double()
    z6 = F.group_norm(x6, 1, torch.from_numpy(gamma[:real]).double(), torch.from_numpy(beta[:real]).double(), 1e-5)
    np.testing.assert_allclose((F.relu(z6) if relu else z6).numpy(), ref["z"][:, :real], rtol=0, atol=0)


@pytest.mark.parametrize("C,shape,B", [(4, (2, 2, 2), 1), (8, (2, 3, 4), 3)])
def test_se_chain_against_the_module(C, shape, B):
    """se_chain / se_reference against the reference's module stack (AdaptiveAvgPool3d, Linear, ReLU, Linear, Sigmoid) in fp64"""
    rng = np.random.default_rng(C + B)
    g = R.draw_se_gate(rng, B, C, shape)
    dout = R.draw_tensor(rng, B, C, shape)
    ref = R.se_reference(g, 0.37, dout)
    fc = torch.nn.Sequential(torch.nn.Linear(C, 1), torch.nn.ReLU(), torch.nn.Linear(1, C), torch.nn.Sigmoid()).double()
    with torch.no_grad():
        for p, k in zip(fc.parameters(), ("w1", "b1", "w2", "b2")):
            p.copy_(torch.from_numpy(g[k]).double())
    x = torch.from_numpy(g["x"]).double().requires_grad_(True)
    y = fc(torch.nn.AdaptiveAvgPool3d(1)(x).view(B, C)).view(B, C, 1, 1, 1)
    out = np.float32(0.37).astype(np.float64) * x * y
    (out * torch.from_numpy(dout).double()).sum().backward()
    np.testing.assert_allclose(ref["gate"], y.detach().numpy()[:, :, 0, 0, 0], rtol=1e-12)
    np.testing.assert_allclose(ref["y"], out.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(ref["dx"], x.grad.numpy(), rtol=1e-10, atol=1e-13)
    for p, k in zip(fc.parameters(), ("dw1", "db1", "dw2", "db2")):
        np.testing.assert_allclose(ref[k], p.grad.numpy(), rtol=1e-10, atol=1e-13)
    # a dead sample (hidden = 0) contributes nothing to dw1 / db1 and has a constant-free input gradient dx = w * gate * dout
    if B >= 2:
        dead = ref["hidden"] == 0
        assert dead.any() and (~dead).any()
        b = int(np.argmax(dead))
        np.testing.assert_allclose(ref["dx"][b], R.w64(0.37) * ref["gate"][b][:, None, None, None] * dout[b], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("cid", list(R.SE_CASES))
def test_se_cases_have_live_and_dead_samples(cid):
    c = R.SE_CASES[cid]
    inp = R.se_inputs(cid)
    assert len(inp["gates"]) == c.gates
    for g in inp["gates"]:
        ref = R.se_reference(g, c.w, inp["dout"])        # asserts |pre| >= 0.1 itself
        assert np.abs(ref["pre"]).min() >= R.SE_MARGIN
        live = ref["hidden"] > 0
        assert live.any() and (c.B == 1 or (~live).any())
    assert len({g["w1"].tobytes() for g in inp["gates"]}) == c.gates        # distinct weights


@pytest.mark.parametrize("cid", list(R.SINGLE_CASES))
def test_margin_of_single_cases(cid):
    inp = R.single_inputs(cid)           # margin_inputs asserts min|z| >= 5e-4 itself
    assert inp["zmin"] >= 5e-4 and inp["passes"] <= 4
    c = R.SINGLE_CASES[cid]
    real = R.real_channels(c.C, c.G)
    assert (inp["gamma"][:real] < 0).any() and 0.5 <= np.abs(inp["gamma"][:real]).min() and np.abs(inp["gamma"]).max() <= 1.5


@pytest.mark.parametrize("cid", list(R.NTERM_CASES))
def test_margin_of_nterm_cases(cid):
    c = R.NTERM_CASES[cid]
    inp = R.nterm_inputs(cid)
    assert len(inp["terms"]) == len(c.terms)
    for t in inp["terms"]:
        if t["kind"] == "gn":
            assert t["zmin"] >= 5e-4 and t["passes"] <= 4
            assert float(np.abs(R.gn_z(t["raw"], c.G, t["gamma"], t["beta"])).min()) >= 5e-4


def test_margin_inputs_moves_what_is_close():
    """an input built to sit ON the threshold (beta = 0 and one element per channel equal to the group mean) ends up at least 5e-4 away"""
    rng = np.random.default_rng(3)
    gamma, beta = R.draw_gamma_beta(rng, 4)
    beta[:] = 0.0
    raw = R.draw_tensor(rng, 1, 4, (2, 2, 4))
    raw[0, :, 0, 0, 0] = 0.0
    raw[0, :, 0, 0, 0] = raw.astype(np.float64).sum() / (raw.size - 4)      # = the mean of the others, hence of all: z ~ 1e-8 there
    assert np.abs(R.gn_z(raw, 1, gamma, beta)).min() < 1e-3
    out, zmin, passes = R.margin_inputs(raw, 1, gamma, beta)
    assert zmin >= 5e-4 and 1 <= passes <= 4
    assert (out != raw).sum() <= 8


@pytest.mark.parametrize("cid", list(R.POOL_CASES))
def test_tie_inputs_contain_ties(cid):
    x = R.pool_inputs(cid, "tie")["x"]
    xr = R.pool_inputs(cid, "tie_relu")["x"]
    for a in (x, xr):
        assert np.array_equal(a, np.round(a * 4) / 4) and np.abs(a).max() <= 1.0
        zeros = a[a == 0]
        assert np.signbit(zeros).any() and (~np.signbit(zeros)).any(), "needs both +0.0 and -0.0"
        several, all_equal = R.tie_fractions(a)
        assert all_equal >= 1 and several > 0
    assert R.tie_fractions(xr)[0] >= 0.5, "at least half of the ReLU'd windows hold several equal maxima"
    assert R.tie_fractions(R.pool_inputs(cid, "normal")["x"]) == (0.0, 0)


def test_pool_reference_takes_the_first_arg_max():
    """torch's CPU max_pool3d backward sends the gradient to the FIRST maximum in (d, h, w) scan order: the rule pool2_bwd_kernel states"""
    x = np.zeros((1, 1, 2, 2, 2), np.float32)
    x[0, 0, 0, 1, 1] = x[0, 0, 1, 0, 0] = 1.0
    for dt in (torch.float32, torch.float64):
        y, dx = R.pool_reference(x, np.full((1, 1, 1, 1, 1), 2.0, np.float32), True, dt)
        assert float(y) == 1.0 and float(dx[0, 0, 0, 1, 1]) == 2.0 and float(dx.sum()) == 2.0
    w = R.pool_windows(np.arange(8, dtype=np.float32).reshape(1, 1, 2, 2, 2))
    assert w.reshape(-1).tolist() == list(range(8))


@pytest.mark.parametrize("cid", list(R.DW_CASES))
def test_depthwise_job_references(cid):
    """the data-gradient job's reference IS autograd's gradient of conv3d; every job of a batch has the case's destination shape"""
    c = R.DW_CASES[cid]
    for n in R.DW_JOBS:
        jobs = R.dw_inputs(cid, n)
        assert len(jobs) == n and sum(j["acc"] for j in jobs) == 1 and sum(j["pitched"] for j in jobs) == 1
        for j in jobs:
            assert R.dw_reference(j).shape == (c.B, c.C) + c.shape
    assert {j["kind"] for j in R.dw_inputs(cid, 8)} == set(R.DW_KINDS)
    j = next(j for j in R.dw_inputs(cid, 8) if j["kind"] == "dgrad1")
    x = torch.zeros((c.B, c.C) + c.shape, dtype=torch.float64, requires_grad=True)
    (F.conv3d(x, torch.from_numpy(j["w"]).double(), None, stride=1, padding=1, groups=c.C) * torch.from_numpy(j["src"]).double()).sum().backward()
    want = x.grad.numpy() + (j["prev"] if j["acc"] else 0.0)
    np.testing.assert_allclose(R.dw_reference(j), want, rtol=1e-12, atol=1e-13)
