"""CPU checks of the exact integer conv data (_conv_exact_ref.py): for EVERY case and value set of tests/test_gpu_conv_exact.py the
worst-case absolute sums stay below 2^24 (so no fp32 partial sum of any summation order can round), every reference value is an
integer -- with ReLU-on-load, the gates and the accumulate bases too -- and torch's own fp32 kernels reproduce the fp64 reference
bit for bit.  A case whose data could round is rejected here, without a GPU."""
import pytest
import torch

import _conv_exact_ref as R

IDS = [R.case_id(i) for i in range(len(R.CASES))]


def _pairs():
    return [(i, kind) for i, c in enumerate(R.CASES) for kind in dict.fromkeys(R.value_kinds(c))]


def test_case_table_is_well_formed():
    assert len(set(IDS)) == len(IDS)
    for c in R.CASES:
        assert c.mix in ("f32", "bf16->bf16", "bf16->f32", "f32->bf16") and len(c.lay) == 2
        assert c.cin % 4 == 0 and c.cout % 4 == 0
        assert not (c.mm and c.mix != "f32"), "N3D_MM_BF16 belongs to fp32 storage"
        assert not c.depthwise or c.cin == c.cout
    # 515 is what the wide set needs it to be: not representable in bf16 and not a rounding tie
    v = torch.tensor([R.SPRINKLE, -R.SPRINKLE, 2 * R.SPRINKLE], dtype=torch.float64)
    assert R.round_bf16(v).tolist() == [516.0, -516.0, 1032.0]
    assert R.round_bf16(torch.tensor([R.SENT_IN, R.SENT_OUT], dtype=torch.float64)).tolist() == [R.SENT_IN, R.SENT_OUT]


@pytest.mark.parametrize("i,kind", _pairs(), ids=["%s-%s" % (IDS[i], k) for i, k in _pairs()])
def test_budgets_integrality_and_fp32_reproduction(i, kind):
    c, d = R.CASES[i], R.draw(i, kind)
    # ---- the draw is what the docstring says
    for k, v in d.items():
        if k not in ("gi", "go"):
            assert bool((v == v.round()).all()), k
    assert set(d["gi"].unique().tolist()) <= {0.5, 1.0, 2.0} and set(d["go"].unique().tolist()) <= {0.5, 1.0, 2.0}
    if c.mix != "f32" or kind != "wide":
        for k in ("x", "w", "bias", "dy", "base_y", "base_dx", "rs"):
            assert float(d[k].abs().max()) <= 256 and torch.equal(R.round_bf16(d[k]), d[k]), "%s is not bf16-representable" % k
    else:
        assert int((d["x"].abs() >= R.SPRINKLE).sum()) > 0 and int((d["dy"].abs() >= R.SPRINKLE).sum()) > 0
    assert float(d["w"].abs().sum()) > 0
    # ---- budgets: conditions, not measurements
    b = R.budgets(i, kind)
    for k, v in b.items():
        assert v < R.LIMIT, "%s: worst-case |%s| sum %.0f is not below 2^24: lower the density or the range" % (IDS[i], k, v)
    # ---- the reference is integer-valued and torch fp32 reproduces it exactly
    ref, f32 = R.reference(i, kind), R.fp32_results(i, kind)
    assert set(f32) <= set(ref)
    if kind != "narrow" and R.has_extras(c):
        assert {"y_rg", "dw_rg", "dx_relu", "dx_gate", "dx_all"} <= set(ref)
    for k, v in ref.items():
        assert bool((v == v.round()).all()), "%s: reference %s is not integer-valued" % (IDS[i], k)
        assert float(v.abs().max()) < R.LIMIT
        if k in f32:
            assert torch.equal(f32[k].double(), v), "%s: torch fp32 does not reproduce the fp64 %s" % (IDS[i], k)
    assert float(ref["y"].abs().sum()) > 0 and float(ref["dx"].abs().sum()) > 0 and float(ref["dw"].abs().sum()) > 0
    if kind == "narrow":
        assert bool((ref["stats"][..., 1].sum(dim=1) > 0).all())


@pytest.mark.parametrize("i", [i for i, c in enumerate(R.CASES) if c.mm], ids=[IDS[i] for i, c in enumerate(R.CASES) if c.mm])
def test_rounded_operand_reference_is_exact_and_differs(i):
    """N3D_MM_BF16 run 2: the conv of the bf16-rounded wide set is integer-valued, inside the budget (|516| against |515|: the budgets
    scale by less than 1.002) and NOT the exact result -- so the run tells the two arithmetics apart"""
    ref, rr = R.reference(i, "wide"), R.reference_rounded(i)
    b = R.budgets(i, "wide")
    assert max(b.values()) * 1.002 < R.LIMIT
    for k in ("y", "dx", "dw"):
        assert bool((rr[k] == rr[k].round()).all())
        assert not torch.equal(rr[k], ref[k]), k


@pytest.mark.parametrize("name", sorted(R.FOLDED))
def test_folded_launch_cases(name):
    """the jobs of the folded-launch tests: same budgets, integrality and fp32 reproduction"""
    for j, c in enumerate(R.FOLDED[name]):
        d, ref = R.folded_draw(name, j), R.folded_reference(name, j)
        for k, v in R.budgets_of(c, d).items():
            assert v < R.LIMIT, (name, j, k, v)
        f32 = R.compute(c, d, torch.float32)
        for k, v in ref.items():
            assert bool((v == v.round()).all()) and torch.equal(f32[k].double(), v), (name, j, k)
