"""CPU checks of tests/_step_form_ref.py: the references and input constructions the GPU tests of the step-form kernels rely on."""
import numpy as np
import pytest
import torch

import _step_form_ref as R


# ------------------------------------------------------------------------------------------ A. slab reduction
@pytest.mark.parametrize("spec", [R.fspec("a", 3, 27, (2, 4), 3, 6), R.fspec("b", 5, 2, (4, 2), 6, 3, has_pb=True)], ids=["taps27", "taps2"])
def test_final_reference_matches_index_formulas(spec):
    """the vectorised fp64 reference against one element at a time from p = tile * T + ci_l * co_t + co_l (ragged tiles on both sides)"""
    assert spec.tci * spec.ci_t > spec.Ci and spec.tco * spec.co_t > spec.Co
    rng = np.random.default_rng(5)
    ns, nb = R.final_slab_floats(spec)
    part = rng.standard_normal((spec.nchunks, ns)).astype(np.float32)
    pb = rng.standard_normal((spec.nchunks, nb)).astype(np.float32)
    dw, dwa, db, dba = R.final_reference(spec, part, pb)
    dw2, db2 = R.final_reference_loops(spec, part, pb)
    assert dw.shape == (spec.Co, spec.Ci, spec.taps)
    np.testing.assert_allclose(dw, dw2, rtol=0, atol=1e-12)
    np.testing.assert_allclose(db, db2, rtol=0, atol=1e-12)
    assert (dwa >= np.abs(dw)).all() and (dba >= np.abs(db)).all()
    # every position of a ragged tile's padding is outside the reference: the number of slab positions used is Co * Ci * taps
    assert dw.size == spec.Co * spec.Ci * spec.taps < ns


def _all_final_batches():
    return {"main": R.final_main_jobs(), "small": R.final_many_small_jobs(200), "overflow": R.final_map_overflow_jobs(), "giant": R.final_giant_jobs()}


def test_final_jobs_pass_the_argument_checks():
    for name, jobs in _all_final_batches().items():
        for s in jobs:
            assert R.final_args_ok(s), (name, s)
            # the tile path transposes a tile through co_t * (ci_t * taps | 1) floats of LDS; the kernel holds 7168
            if R.final_path(s) == "tile":
                assert s.co_t * ((s.ci_t * s.taps) | 1) <= 7168, (name, s)


def test_final_job_tables_reach_what_they_claim():
    main = R.final_main_jobs()
    by = {}
    for s in main:
        by.setdefault(R.final_path(s), []).append(s)
    assert set(by) == {"none", "tile", "direct4", "direct16", "many64", "many16", "many8", "many4"}
    assert {s.nchunks for s in by["tile"]} >= {1, 3, 4}
    assert any(s.ci_t == 1 and s.taps == 27 for s in by["tile"]) and any(s.taps == 1 for s in by["tile"])
    assert any(s.Ci % s.ci_t for s in by["tile"]) and any(s.Co % s.co_t for s in by["tile"])
    assert all(s.ci_t * s.co_t > 256 for s in by["direct4"] + by["direct16"])
    assert {s.nchunks for s in by["direct4"]} >= {2} and {s.nchunks for s in by["direct16"]} >= {5, 16}
    many = {s.nchunks for p in ("many64", "many16", "many8", "many4") for s in by[p]}
    assert many >= {17, 64, 65, 200, 256, 257, 1000, 1024, 1025, 2050}
    for path in ("tile", "direct", "many"):
        fam = [s for p, v in by.items() if p.startswith(path) for s in v]
        assert any(not s.has_pb for s in fam) and any(not s.has_dw for s in fam), path
    # the empty jobs are in the middle of the batch
    empties = [i for i, s in enumerate(main) if s.nchunks == 0]
    assert len(empties) == 3 and all(0 < i < len(main) - 1 for i in empties)
    assert R.final_launch_plan(main) == [(0, len(main))]
    assert [m for _, m in R.final_launch_plan(R.final_many_small_jobs(200))] == [80, 80, 40]
    ov = R.final_map_overflow_jobs()
    assert len(ov) < R.N_FINAL_JOBS and len(R.final_launch_plan(ov)) >= 3
    giant = R.final_giant_jobs()
    assert [R.final_blocks(s) > 8192 for s in giant] == [False, True, False, True, False]
    assert R.final_path(giant[1]) == "tile" and giant[1].tci * giant[1].tco == 9216
    assert R.final_path(giant[3]) == "many8" and giant[3].nchunks == 257


# ------------------------------------------------------------------------------------------ C. stem recompute kernels
def _k1_cases_and_mixes():
    return [(cid, mix) for cid in R.K1_CASES for mix in (R.K1_MIXES if cid in R.K1_BF16_CASES else R.K1_MIXES[:1])]


@pytest.mark.parametrize("cid,mix", _k1_cases_and_mixes())
def test_k1_inputs_keep_their_relu_margin(cid, mix):
    """no voxel within the margin of a ReLU threshold, with and without the conv bias, on the values the device will hold"""
    inp = R.k1_inputs(cid, mix)
    c = inp["case"]
    assert len(inp["redrawn"]) <= R.K1_MAX_PASSES + 1 and inp["redrawn"][-1] == 0 and inp["redrawn"][0] > 0
    for bias in (inp["bias"], None):
        assert not R.k1_near_zero(inp["x"], inp["w"], bias, inp["a"], inp["b"]).any()
    if mix.startswith("bf16"):
        assert np.array_equal(R.bf16_round(inp["x"]), inp["x"])
    if mix.endswith("bf16"):
        assert np.array_equal(R.bf16_round(inp["dout"]), inp["dout"])
    assert inp["x"].shape == (c.B, c.Ci, inp["N"]) and inp["dout"].shape == (c.B, c.Co, inp["N"])
    assert (inp["a"] >= 0.5).all() and (inp["a"] <= 1.5).all()


def test_k1_margin_finds_a_planted_voxel():
    """a voxel whose z is exactly zero in one channel is reported, and only that voxel"""
    w = np.array([[1.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0], [0.0, 1.0, 0.0, -1.0]], np.float32)
    x = np.full((1, 4, 6), 2.0, np.float32)
    x[0, :, 3] = (3.0, 1.0, 1.0, 1.0)          # channel 3: raw = 1 - 1 = 0, z = b = 0
    a, b = np.ones((1, 4), np.float32), np.array([[0.5, 0.5, 0.5, 0.0]], np.float32)
    x[0, 3, :] = 1.0
    x[0, 1, :] = 1.5
    x[0, 1, 3] = 1.0
    bad = R.k1_near_zero(x, w, None, a, b)
    assert bad.tolist() == [[False, False, False, True, False, False]]


def test_k1_chunks_of_the_cases():
    chunks = {cid: R.k1_chunk(int(np.prod(c.shape))) for cid, c in R.K1_CASES.items()}
    assert chunks == {"K1": 512, "K2": 512, "K3": 512, "K4": 512, "K5": 512, "K6": 1024, "K7": 2048}
    N2, N3 = 32 * 33 * 33, 32 * 35 * 37
    assert N2 % 512 == 32 and N2 % 1024 == 32 and N3 % 512 == 480


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_k1_formulas_match_autograd(with_bias, relu):
    """the closed forms of k1_reference on a 4^3 volume against torch fp64 autograd of y = act(a (W x + bias) + b): the sums columns,
    and dW for the coefficients (A, Bc, Cc) = (a, 0, 0), with which d(raw) = A g + Cc raw + Bc is the gradient of sum(dout y)"""
    rng = np.random.default_rng(11)
    B, Ci, Co, N = 2, 4, 12, 64
    inp = dict(x=rng.standard_normal((B, Ci, N)).astype(np.float32), dout=rng.standard_normal((B, Co, N)).astype(np.float32),
               w=(rng.standard_normal((Co, Ci)) * 0.3).astype(np.float32), bias=rng.standard_normal(Co).astype(np.float32),
               a=rng.uniform(0.5, 1.5, (B, Co)).astype(np.float32), b=rng.standard_normal((B, Co)).astype(np.float32))
    inp["A"], inp["Bc"], inp["Cc"] = inp["a"], np.zeros((B, Co), np.float32), np.zeros((B, Co), np.float32)
    ref = R.k1_reference(inp, with_bias)
    x = torch.from_numpy(inp["x"]).double()
    w = torch.from_numpy(inp["w"]).double().requires_grad_(True)
    cb = (torch.from_numpy(inp["bias"]).double() if with_bias else torch.zeros(Co, dtype=torch.float64)).requires_grad_(True)
    a = torch.from_numpy(inp["a"]).double().requires_grad_(True)
    b = torch.from_numpy(inp["b"]).double().requires_grad_(True)
    raw = torch.einsum("oc,bcn->bon", w, x) + cb[None, :, None]
    raw.retain_grad()
    zn = a[:, :, None] * raw + b[:, :, None]
    y = torch.relu(zn) if relu else zn
    d = torch.from_numpy(inp["dout"]).double()
    (y * d).sum().backward()
    np.testing.assert_allclose(ref["y"], zn.detach().numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref["stats"][..., 0], raw.detach().sum(-1).numpy(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(ref["stats"][..., 1], (raw.detach() ** 2).sum(-1).numpy(), rtol=0, atol=1e-10)
    # sum g = dL/db, sum g raw = dL/da, sum dout z = <dout, y>
    np.testing.assert_allclose(ref["sums", relu][..., 0], b.grad.numpy(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(ref["sums", relu][..., 1], a.grad.numpy(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(ref["sums", relu][..., 2], (d * y.detach()).sum(-1).numpy(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(ref["dw", relu], w.grad.numpy(), rtol=0, atol=1e-10)


def test_k1_general_coefficients_enter_dw_linearly():
    """dW for random (A, Bc, Cc) = A-part + Cc-part + Bc-part, each against its own einsum"""
    inp = dict(R.k1_inputs("K2"))
    ref = R.k1_reference(inp, True)
    x, d = inp["x"].astype(np.float64), inp["dout"].astype(np.float64)
    raw = R.k1_raw(inp["x"], inp["w"], inp["bias"])
    z = inp["a"].astype(np.float64)[:, :, None] * raw + inp["b"].astype(np.float64)[:, :, None]
    g = d * (z > 0)
    want = (np.einsum("bo,bon,bcn->oc", inp["A"].astype(np.float64), g, x) + np.einsum("bo,bon,bcn->oc", inp["Cc"].astype(np.float64), raw, x)
            + np.einsum("bo,bcn->oc", inp["Bc"].astype(np.float64), x))
    np.testing.assert_allclose(ref["dw", True], want, rtol=1e-12, atol=1e-9)


def test_k1_chain_reference_is_group_norm_of_the_conv():
    """the chain reference against _epilogue_ref.term_reference on the fp64 raw (the reference the epilogue tests use)"""
    import _epilogue_ref as E
    inp = R.k1_inputs("K2")
    c = inp["case"]
    ref = R.k1_chain_reference(inp, True, 1)
    raw5 = ref["raw"].reshape(c.B, c.Co, *c.shape)
    t = E.term_reference(raw5, inp["gamma"], inp["beta"], 1, False, None, inp["dout"].reshape(c.B, c.Co, *c.shape))
    # (term_reference takes raw in the dtype it is given: fp64 here)
    np.testing.assert_allclose(ref["y"].reshape(raw5.shape), t["y"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(ref["dgamma"], t["dgamma"], rtol=1e-9, atol=1e-7)
    np.testing.assert_allclose(ref["dbeta"], t["dbeta"], rtol=1e-9, atol=1e-7)
    np.testing.assert_allclose(ref["dbias"], t["dbias_conv"], rtol=1e-9, atol=1e-7)
    np.testing.assert_allclose(ref["dw"], np.einsum("bon,bcn->oc", t["draw"].reshape(c.B, c.Co, -1), inp["x"].astype(np.float64)), rtol=1e-9, atol=1e-7)


# ------------------------------------------------------------------------------------------ B. conv table
def test_conv_table_shapes_and_padding():
    from nas_3d_unet_amd.prim_ops import _padding
    ids = [R.conv_case_id(c) for c in R.CONV_CASES]
    assert len(set(ids)) == len(ids) == 22
    for i, c in enumerate(R.CONV_CASES):
        assert R.conv_padding(c.k, c.stride, c.dil) == _padding(c.k, c.stride, c.dil)
    for i in (0, 2, 17, 20):          # plain, transposed, depthwise transposed, bf16 transposed
        ref = R.conv_reference(i)
        assert tuple(ref["y"].shape[2:]) == R.conv_out_shape(R.CONV_CASES[i])
        if R.CONV_CASES[i].bf16:
            for k in ("x", "dy", "w"):
                assert np.array_equal(R.bf16_round(ref[k]), ref[k])


def test_pack_launch_plan():
    assert R.pack_launch_plan([1] * 161) == [(160, "table"), (1, "end")]
    assert R.pack_launch_plan([2048, 1, 4096, 1]) == [(1, "map"), (1, "map"), (1, "map"), (1, "end")]
    assert R.pack_blocks(64, 64, 27, 0, 1, 64) == 16 and R.pack_blocks(64, 192, 1, 1, 1, 192) == 48 and R.pack_blocks(12, 4, 27, 0, 0, 12) == 1


def test_conv_table_reach_record_is_complete():
    assert set(R.CONV_REACHES) == {R.conv_case_id(c) for c in R.CONV_CASES}
    assert {l for v in R.CONV_REACHES.values() for l in v[:2]} == {-1, 0, 1, 2, 3, 4, 5}
