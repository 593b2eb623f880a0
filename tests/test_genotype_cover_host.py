"""CPU: the genotype list of the searched-net sweep (_genotype_cover.SWEEP) is what its builder makes, covers every goal, is what the
parser can emit, and its reference is well conditioned at the sweep's inputs (no GPU)."""
import pytest
import torch

import _genotype_cover as gcv
from nas_3d_unet_amd import prim_ops
from nas_3d_unet_amd.genotype import GenoParser
from oracle import ref_path as orc


def test_sweep_is_the_builders_and_meets_every_goal():
    assert (prim_ops.DownOps, prim_ops.UpOps, prim_ops.NormOps) == (orc.DOWN_NAMES, orc.UP_NAMES, orc.NORM_NAMES)
    assert set(gcv.KIND) == set(orc.PRIMS)
    built = gcv.build_sweep()
    assert [(e.genotype, e.n_nodes) for e in gcv.SWEEP] == [(e.genotype, e.n_nodes) for e in built], "SWEEP is not build_sweep()'s list"
    assert len(gcv.build_cover()) <= gcv.CAP and len(gcv.SWEEP) <= gcv.CAP + 2
    assert all(e.n_nodes == 3 for e in gcv.SWEEP)
    for i, e in enumerate(gcv.SWEEP):
        assert gcv.is_legal(e), (i, e)
    goals = gcv.all_goals()
    assert len(goals) == 215
    missing = sorted(goals - gcv.goals_met(gcv.SWEEP), key=repr)
    for g in missing:
        print("goal not met:", g)
    assert not missing, "%d goals not met" % len(missing)
    # the two hand-written shapes
    pre_only = [e for e in gcv.SWEEP if all(i < 2 for cell in e.genotype for _, i in cell)]
    last_first = [e for e in gcv.SWEEP if all((cell[4][1], cell[5][1]) == (3, 2) for cell in e.genotype)]
    assert pre_only and last_first
    for name, g in gcv.REGRESSIONS.items():
        assert gcv.cell_is_legal(g.down, True) and gcv.cell_is_legal(g.up, False), name


def test_legality_rule_rejects_what_the_parser_cannot_emit():
    ok = gcv.SWEEP[0].genotype.down
    assert gcv.cell_is_legal(ok, True)
    assert not gcv.cell_is_legal(ok, False)                                   # DownOps names in an up cell
    assert not gcv.cell_is_legal([("avg_pool", 0), ("avg_pool", 0)] + list(ok[2:]), True)      # one input twice
    assert not gcv.cell_is_legal(list(ok[:2]) + [("conv", 3), ("avg_pool", 0)] + list(ok[4:]), True)   # node 1 reads itself
    assert not gcv.cell_is_legal(list(ok[:4]) + [("conv", 1), ("conv", 2)], True)                # a stride-1 name on a strided edge
    assert not gcv.cell_is_legal(ok[:4], True)


@pytest.mark.parametrize("index", range(len(gcv.SWEEP)))
def test_parser_emits_every_entry(index):
    """alphas from which GenoParser(3).parse returns exactly the entry's cells: the list is tied to what the parser can emit"""
    e = gcv.SWEEP[index]
    for downward, cell in ((True, e.genotype.down), (False, e.genotype.up)):
        a1, a2 = gcv.alphas_for(cell, downward)
        assert abs(a1.sum(1) - 1).max() < 1e-12 and abs(a2.sum(1) - 1).max() < 1e-12 and a1.min() > 0 and a2.min() > 0
        assert GenoParser(e.n_nodes).parse(a1, a2, downward=downward) == list(cell)
        assert orc.parse_genotype(a1, a2, e.n_nodes, downward) == list(cell)
        assert GenoParser(e.n_nodes).parse(a1.astype("float32"), a2.astype("float32"), downward=downward) == list(cell)


WORST = {}


@pytest.mark.parametrize("index,batch,shape", gcv.CASES + gcv.FOLD_CASES)
def test_reference_is_well_conditioned_at_the_sweeps_inputs(index, batch, shape):
    """the oracle in fp32 against itself in fp64 at the sweep's configuration and inputs: within 0.1 x each bound of the GPU sweep.
    An input with a pre-activation within rounding of zero flips a ReLU mask between two correct evaluations (the seed-17 note in
    test_gpu_nets.py) and would show here, without a GPU; such an entry gets the next seed, recorded in SWEEP (FOLD_SEEDS at FOLD_SHAPE)."""
    l32, p32, g32 = gcv.oracle_run(index, batch, torch.float32, shape)
    l64, p64, g64 = gcv.oracle_run(index, batch, torch.float64, shape)
    rl = abs(float(l32) - float(l64)) / gcv.TOL_LOSS
    rp = float((p32.double() - p64).abs().max()) / gcv.TOL_P
    bounds = gcv.grad_bounds(g64)
    assert g32.keys() == g64.keys()
    rg = 0.0
    for n, ref in g64.items():
        assert (ref is None) == (g32[n] is None), n
        if ref is not None:
            rg = max(rg, float((g32[n].double() - ref).abs().max()) / bounds[n])
    worst = WORST.setdefault(tuple(shape), {})
    for k, v in (("loss", rl), ("probabilities", rp), ("gradients", rg)):
        worst[k] = max(worst.get(k, 0.0), v)
    print("entry %d batch %d shape %s: fp32 oracle / bound: loss %.4f probabilities %.4f gradients %.4f   (worst so far at this shape %s)"
          % (index, batch, tuple(shape), rl, rp, rg, {k: round(v, 4) for k, v in worst.items()}))
    assert rl <= 0.1 and rp <= 0.1 and rg <= 0.1, (index, batch, rl, rp, rg)
