"""GPU: searched nets over every genotype shape the parser can emit (_genotype_cover.SWEEP: 215 coverage goals, see that file).

How a searched cell is launched depends on its genotype -- which kinds of primitive sit on a node's two edges and which states they
read: fused._run_forward_impl (folded pair / early conv on the side stream / SIDE_PAIRS_BOTH fork / plain pair_forward),
fused._run_backward_nodes (side_idx, the dropped side stream, pair_backward_epilogue + split _weight_backward against pair_backward)
and programs._weight_backward (conv_bwd_both2 / conv_bwd_data2 / folded data pair, the se_gate_bwdN run, the dwconv_batch run).
Every entry of the sweep runs
  (a) through autograd against the fp64 oracle (loss, probabilities, every parameter gradient; _check_net_vs_oracle's bounds),
  (b) through the trainers' eager side-stream schedule, fused.FOLD_SMALL_PAIRS on and off: against the one-stream trainer, against the
      oracle, and pass 2 against pass 3 bit for bit (all writers of a buffer stay on one stream: a race would show as run-to-run noise),
  (c) through the captured three-stream step against the captured plain step (first-step gradients, losses and weights of four steps),
  (d) and one census test shows that the sweep reaches the branches it is there for.
At the sweep's 8 x 8 x 16 patch only the last up cell (C = 4) has the 16-voxel rows the one-launch conv pairs need, so four picked
entries (most two-conv nodes, most early convs, first S+S, first E2+E2) also run (a), (b) and the folded-against-forked bit comparison
at 16 x 16 x 64, where the C = 8 cells fold too.
What the sweep found (a main-stream write into a buffer the side stream was still accumulating into, DESIGN.md "Genotype sweep") is kept
as a named genotype (_genotype_cover.REGRESSIONS) and as a check of the launch order that needs no unlucky timing.
The reference is computed once per (entry, batch) and shared (never modified).  The bounds are the project's own; the worst
error / bound seen so far is printed by every case (pytest -s) -- DESIGN.md "Genotype sweep" records them next to the fp32 oracle's.
"""
import functools
import sys

import numpy as np
import pytest
import torch

import _genotype_cover as gcv
from _util import dev, fill_module
from oracle import ref_path as orc

pytestmark = pytest.mark.gpu

CASES = gcv.CASES + gcv.FOLD_CASES      # (entry, batch, shape)
WORST = {}


@functools.lru_cache(maxsize=None)
def _ref(index, batch, shape=gcv.SHAPE):
    """the fp64 oracle's (loss, probabilities, gradients, per-parameter bounds) of one case"""
    l, p, g = gcv.oracle_run(index, batch, None, shape)
    return float(l), p, g, gcv.grad_bounds(g)


def _net(index):
    """the sweep's net for entry `index` of SWEEP (or for a Genotype), closed-form parameters, head dropout off"""
    from nas_3d_unet_amd import searched
    cfg = orc.NetCfg(*gcv.CFG)
    g = gcv.SWEEP[index].genotype if isinstance(index, int) else index
    net = searched.SearchedNet(cfg.in_channels, cfg.init_n_kernels, cfg.out_channels, cfg.depth, cfg.n_nodes, cfg.channel_change,
                               searched.Genotype(list(g.down), list(g.up)))
    fill_module(net)
    net.last_conv[0].dropout = None         # head dropout off, the way test_gpu_nets.build_net does
    net.last_conv[0]._segments = None
    return net.cuda()


def _batch(index, batch, shape=gcv.SHAPE):
    x, t = gcv.sweep_batch(index, batch, shape)
    return dev(x), dev(t)


def _note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    return ratio


def _check_grads(what, named_grads, index, batch, shape):
    """every (name, gradient) against the oracle's within 3e-4 max|ref| + 2e-5 ||g_total||; no reference gradient: exactly zero"""
    _, _, ref, bounds = _ref(index, batch, shape)
    bad, worst = [], 0.0
    seen = set()
    for n, g in named_grads:
        seen.add(n)
        assert g is not None, "%s: no gradient" % n
        if ref[n] is None:
            assert float(g.abs().max()) == 0.0, "%s has no reference gradient and is not zero" % n
            continue
        d = float((g.detach().cpu().double().reshape(ref[n].shape) - ref[n]).abs().max())
        worst = max(worst, d / bounds[n])
        if not d <= bounds[n]:
            bad.append((n, d, bounds[n]))
    assert seen == set(ref), "parameters differ from the oracle's"
    print("%s entry %d batch %d: gradients error / bound %.4f" % (what, index, batch, _note(what + " gradients", worst)))
    assert not bad, bad


# ---- (a) autograd path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,batch,shape", CASES)
def test_autograd_path_vs_fp64_oracle(index, batch, shape):
    from nas_3d_unet_amd import loss
    lr, pr, _, _ = _ref(index, batch, shape)
    net = _net(index)
    x, t = _batch(index, batch, shape)
    p = net(x)
    l = loss.WeightedDiceLoss()(p, t)
    l.backward()
    rl = _note("(a) loss", abs(float(l.detach()) - lr) / gcv.TOL_LOSS)
    rp = _note("(a) probabilities", float((p.detach().cpu().double() - pr).abs().max()) / gcv.TOL_P)
    print("(a) entry %d batch %d: loss error / bound %.4f, probabilities %.4f" % (index, batch, rl, rp))
    assert rl < 1.0
    assert rp < 1.0
    _check_grads("(a)", [(n, q.grad) for n, q in net.named_parameters()], index, batch, shape)
    print("worst error / bound so far:", {k: float("%.3g" % v) for k, v in sorted(WORST.items())})


# ---- (b) eager side-stream schedule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("index,batch,shape", CASES)
def test_side_schedule_eager(index, batch, shape, fold):
    from nas_3d_unet_amd import fused
    from nas_3d_unet_amd.train import Trainer
    lr = _ref(index, batch, shape)[0]
    x, t = _batch(index, batch, shape)
    with fused.switched(FOLD_SMALL_PAIRS=fold):
        plain = Trainer(_net(index), graph=False, side_wgrad=False)
        plain._fwd_bwd(x, t)
        ref = plain.fp.grad.clone()
        tot = float(ref.double().norm())
        net2 = _net(index)
        tr = Trainer(net2, graph=False, side_wgrad=True)
        assert tr.side is not None and tr._side_ok(), "the side stream was not accepted on this box"
        passes = []
        for _ in range(3):        # first pass records the pack jobs; later ones run pre-packed
            tr.fp.grad.zero_()
            l = tr._side_step_eager(x, t)
            torch.cuda.synchronize()
            tr.check_sync()         # a timed-out hand-off raises here
            passes.append((l.detach().clone(), tr.fp.grad.clone()))
    names = [n for n, _ in net2.named_parameters()]
    what = "(b) fold %s" % ("on" if fold else "off")
    for k, (l, g) in enumerate(passes):
        r = float((g - ref).double().norm()) / (1e-5 * tot)
        print("%s entry %d batch %d pass %d: |grad - plain| / bound %.3g" % (what, index, batch, k, _note(what + " vs plain", r)))
        assert r <= 1.0
        assert abs(float(l) - lr) < gcv.TOL_LOSS
        _check_grads(what, [(n, g[off:off + q.numel()]) for n, q, off in zip(names, tr.fp.params, tr.fp.offsets)], index, batch, shape)
    assert torch.equal(passes[1][0], passes[2][0]) and torch.equal(passes[1][1], passes[2][1]), "passes 2 and 3 differ: a race"
    print("worst error / bound so far:", {k: float("%.3g" % v) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("index,batch,shape", gcv.FOLD_CASES)
def test_folded_schedule_computes_the_forked_schedule_bits(index, batch, shape):
    """the picked entries at the extents where the C = 8 cells' pairs fold: the folded launch runs the single kernels' bodies and every
    buffer keeps its writers in program order on one stream, so the eager side schedule with fused.FOLD_SMALL_PAIRS on and off gives
    the same loss and gradients bit for bit (test_gpu_vox_pair.py shows it for G_CONV) -- whichever kinds the genotype puts into one
    launch (stride 1 / stride 2 / transposed, either dilation)"""
    from nas_3d_unet_amd import fused, kernels as K
    from nas_3d_unet_amd.train import Trainer
    x, t = _batch(index, batch, shape)
    res = []
    for fold in (True, False):
        with fused.switched(FOLD_SMALL_PAIRS=fold):
            tr = Trainer(_net(index), graph=False, side_wgrad=True)
            assert tr.side is not None and tr._side_ok()
            n0 = K.conv_fold_counts()["vox_multi"]
            for _ in range(2):
                tr.fp.grad.zero_()
                l = tr._side_step_eager(x, t)
                torch.cuda.synchronize()
                tr.check_sync()
            res.append((l.detach().clone(), tr.fp.grad.clone(), K.conv_fold_counts()["vox_multi"] - n0))
    (l1, g1, n1), (l0, g0, n0) = res
    candidates = sum(dd for dd, _ in gcv.forms_of(index))
    print("entry %d: folded launches in two passes: FOLD_SMALL_PAIRS on %d, off %d (%d nodes with two plain convs)" % (index, n1, n0, candidates))
    if index == gcv.picked_entries_by_role()["folds"]:
        assert n1 > n0, "the switch folded nothing at this size"
    assert torch.equal(l1, l0)
    assert torch.equal(g1, g0)


# ---- (c) captured step ---------------------------------------------------------------------------------------------------------------
def _captured_runs(index, x, t, sides):
    """four captured steps per trainer -> [(losses, weights after them, gradients of the first step)]"""
    from nas_3d_unet_amd.train import Trainer
    out = []
    for side in sides:
        tr = Trainer(_net(index), graph=True, side_wgrad=side)
        losses = [float(tr.step(x, t))]
        torch.cuda.synchronize()
        g1 = tr.fp.grad.clone()
        losses += [float(tr.step(x, t)) for _ in range(3)]
        torch.cuda.synchronize()
        tr.check_sync()
        if side:
            assert tr._use_side and tr._side_graphs is not None
        out.append((losses, tr.fp.flat.clone(), g1))
    return out


@pytest.mark.parametrize("index", range(len(gcv.SWEEP)))
def test_captured_side_step_matches_captured_plain_step(index):
    """four steps of Trainer(graph=True, side_wgrad='force') against the captured one-stream trainer
    (test_side_schedule_graph_replay_matches_plain_trainer's bounds: Adam turns fp32 noise into lr-sized moves, a missing weight gradient
    moves a layer by 1e-2 of the norm).  Every entry, not only the picked ones: replayed graphs overlap the streams far more than eager
    launches do, and the one race the sweep found showed only here."""
    x, t = _batch(index, 2)
    out = _captured_runs(index, x, t, (False, "force"))
    assert abs(out[0][0][0] - _ref(index, 2)[0]) < gcv.TOL_LOSS      # (the first step's loss is the untrained net's)
    # the first step's gradients belong to the same weights on both sides: (b)'s bound.  (The weight bound below did not see the race
    # of REGRESSIONS['pools_behind_paired_nodes'] on entry 0 -- 1.5e-3 of the norm -- this one does: 1.1e-2 against 1e-5)
    r = float((out[0][2] - out[1][2]).double().norm()) / (1e-5 * float(out[0][2].double().norm()))
    print("(c) entry %s: first step |grad - plain| / bound %.3g" % (index, r))
    assert r <= 1.0
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=2e-5)
    d = float((out[0][1] - out[1][1]).double().norm()) / float(out[0][1].double().norm())
    print("(c) entry %d: weight difference / norm %.3e (bound 2e-3)" % (index, d))
    assert d <= 2e-3


@pytest.mark.parametrize("name", sorted(gcv.REGRESSIONS))
def test_regression_genotypes_captured(name):
    """the named regression genotypes through the captured side step: first-step gradients against the captured plain step ((b)'s
    bound) and two side trainers against each other, bit for bit (test_side_schedule_is_reproducible_run_to_run's condition)"""
    g = gcv.REGRESSIONS[name]
    assert gcv.cell_is_legal(g.down, True) and gcv.cell_is_legal(g.up, False)
    x, t = _batch(0, 2)
    plain, side, again = _captured_runs(g, x, t, (False, "force", "force"))
    r = float((plain[2] - side[2]).double().norm()) / (1e-5 * float(plain[2].double().norm()))
    print("%s: first step |grad - plain| / bound %.3g" % (name, r))
    assert r <= 1.0
    assert torch.equal(side[2], again[2]) and torch.equal(side[1], again[1]) and side[0] == again[0]
    np.testing.assert_allclose(plain[0], side[0], rtol=0, atol=2e-5)
    assert float((plain[1] - side[1]).double().norm()) <= 2e-3 * float(plain[1].double().norm())


def test_main_stream_never_touches_a_buffer_the_side_stream_is_writing(monkeypatch):
    """the rule of fused._run_backward_nodes, checked on the launch ORDER (no timing involved): a data gradient the side stream writes
    (programs._weight_backward under kernels.on_side) is neither written nor read by a main-stream backward call before the main stream
    has joined a flag the side stream stored behind that write.  One eager side pass per entry and regression genotype."""
    from nas_3d_unet_amd import fused, kernels as K, programs as P
    from nas_3d_unet_amd.train import SideSchedule, Trainer
    state = {"seq": 0, "pending": [], "flag_seq": {}, "bad": [], "side_writes": 0, "who": None}
    on_side = lambda: K._redirect is not None
    from_fused = lambda: sys._getframe(2).f_globals.get("__name__") == fused.__name__

    def touch(what, views):
        busy = {p for _, p in state["pending"]}
        for v in views:
            if getattr(v, "p", None) is not None and v.p.value in busy:
                state["bad"].append((state["who"], what))

    real_wb, real_pb, real_sb = P._weight_backward, P.pair_backward, P.seg_backward

    def weight_backward(order, *a, **kw):
        if from_fused():
            if on_side():
                for o in order:
                    if o[4][0] and o[4][1] is not None:
                        state["seq"] += 1
                        state["pending"].append((state["seq"], o[4][1].p.value))
                        state["side_writes"] += 1
            else:
                touch("_weight_backward writes", [o[4][1] for o in order])
        return real_wb(order, *a, **kw)

    def pair_backward(segA, sA, segB, sB, dout, argsA, argsB, doutB=None, *a, **kw):
        if from_fused() and not on_side():
            touch("pair_backward", [dout, doutB, argsA[1], argsB[1]])
        return real_pb(segA, sA, segB, sB, dout, argsA, argsB, doutB, *a, **kw)

    def seg_backward(seg, s, dout, need_dx=True, dx_out=None, *a, **kw):
        if from_fused() and not on_side():
            touch("seg_backward", [dout, dx_out])
        return real_sb(seg, s, dout, need_dx, dx_out, *a, **kw)

    real_signal, real_join, real_join_many = SideSchedule.side_signal, SideSchedule.join, SideSchedule.join_many

    def side_signal(self):
        i = real_signal(self)
        state["flag_seq"][i] = state["seq"]
        return i

    def joined(i):
        upto = state["flag_seq"].get(i, 0)      # the side stream runs in order: its flag covers everything it was given before
        state["pending"] = [(q, p) for q, p in state["pending"] if q > upto]

    def join(self, i):
        joined(i)
        return real_join(self, i)

    def join_many(self, ids):
        ids = list(ids)
        for i in ids:
            joined(i)
        return real_join_many(self, ids)

    monkeypatch.setattr(P, "_weight_backward", weight_backward)
    monkeypatch.setattr(P, "pair_backward", pair_backward)
    monkeypatch.setattr(P, "seg_backward", seg_backward)
    monkeypatch.setattr(SideSchedule, "side_signal", side_signal)
    monkeypatch.setattr(SideSchedule, "join", join)
    monkeypatch.setattr(SideSchedule, "join_many", join_many)
    cases = [(i, gcv.SWEEP[i].genotype) for i in range(len(gcv.SWEEP))] + sorted(gcv.REGRESSIONS.items())
    x, t = _batch(0, 2)
    for who, g in cases:
        state.update(seq=0, pending=[], flag_seq={}, who=who)
        tr = Trainer(_net(g), graph=False, side_wgrad=True)
        assert tr.side is not None and tr._side_ok()
        tr._side_step_eager(x, t)
        torch.cuda.synchronize()
        tr.check_sync()
    print("data gradients written on the side stream over the walk: %d; main-stream calls that touched one too early: %d"
          % (state["side_writes"], len(state["bad"])))
    assert state["side_writes"] > 0, "the side stream wrote no data gradient: nothing was checked"
    assert not state["bad"], state["bad"]


# ---- (d) branch census ---------------------------------------------------------------------------------------------------------------
def test_branch_census(monkeypatch):
    """one eager side pass per entry, FOLD_SMALL_PAIRS on and off, with counters around the launches the genotype decides between:
    every one of them is reached, and the forward forms are the ones the genotype asks for"""
    from nas_3d_unet_amd import fused, kernels as K, programs as P
    from nas_3d_unet_amd.train import Trainer
    count = {}

    def counted(mod, name, key=None, size=False, caller=None):
        fn = getattr(mod, name)
        key = key or name

        def wrapper(*a, **kw):
            r = fn(*a, **kw)
            if caller is not None and sys._getframe(1).f_globals.get("__name__") != caller.__name__:
                return r
            count[key] = count.get(key, 0) + 1
            if size:
                count[key + " terms"] = count.get(key + " terms", 0) + len(a[0])
            if name == "pair_backward_epilogue" and r is None:
                count[key + " -> None"] = count.get(key + " -> None", 0) + 1
            if name in ("_fold_pair_nodes", "_fold_pair_nodes_bwd"):
                count[key] += len(r) - 1
            if name == "_fold_pair_nodes_bwd":
                # fused._run_backward_nodes' rule, restated: the side stream is left out of a cell's backward where every node that writes
                # the busier preprocess gradient folds
                edges = a[0].edges
                side_idx = 0 if sum(e[1] == 0 for e in edges) > sum(e[1] == 1 for e in edges) else 1
                if all(n in r for n in range(a[0].n_nodes) if side_idx in (edges[2 * n][1], edges[2 * n + 1][1])):
                    count["side stream left out of a cell's backward"] = count.get("side stream left out of a cell's backward", 0) + 1
            return r
        monkeypatch.setattr(mod, name, wrapper)

    for name in ("conv_fwd2", "conv_bwd_both2", "conv_bwd_data2", "affine_act_gn2", "affine_act_bwd_gn2"):
        counted(K, name)
    counted(K, "dwconv_batch", size=True)
    counted(K, "se_gate_bwdN", size=True)
    # (only fused's own calls, the forked forms: programs.pair_forward runs the same two halves back to back)
    counted(P, "pair_weight_phase", "fork: pair_weight_phase", caller=fused)
    counted(P, "pair_epilogue_phase", "fork: pair_epilogue_phase", caller=fused)
    counted(P, "pair_backward_epilogue")
    counted(fused, "_fold_pair_nodes", "folded nodes, forward")
    counted(fused, "_fold_pair_nodes_bwd", "folded nodes, backward")
    totals = {}
    unread = 0
    walk = [(i, 2, gcv.SHAPE) for i in range(len(gcv.SWEEP))] + gcv.FOLD_CASES
    for fold in (True, False):
        for index, batch, shape in walk:
            g = gcv.SWEEP[index].genotype
            # a preprocess output that no edge reads (its gradient buffer is zeroed at the end of fused._run_backward_nodes)
            unread += sum(all(i != k for _, i in cell) for cell in g for k in (0, 1))
            x, t = _batch(index, batch, shape)
            count.clear()
            f0 = K.conv_fold_counts()
            with fused.switched(FOLD_SMALL_PAIRS=fold):
                tr = Trainer(_net(index), graph=False, side_wgrad=True)
                assert tr.side is not None and tr._side_ok()
                tr._side_step_eager(x, t)
                torch.cuda.synchronize()
                tr.check_sync()
            f1 = K.conv_fold_counts()
            for kind in K.FOLD_KINDS:
                count["fold kind " + kind] = f1[kind] - f0[kind]
            # the forward form of every C <= 8 node: forks + folds are exactly the nodes the genotype makes fork candidates
            forms = gcv.forms_of(index)
            forked = sum(fork is not None for _, fork in forms)
            got = count.get("fork: pair_epilogue_phase", 0) + count.get("folded nodes, forward", 0)
            assert got == forked, (index, fold, got, forked, forms)
            if not fold:
                assert count.get("folded nodes, forward", 0) == 0 and count.get("folded nodes, backward", 0) == 0
            for k, v in count.items():
                key = (k, fold)
                totals[key] = totals.get(key, 0) + v
    keys = sorted({k for k, _ in totals})
    print("branch census over %d genotypes + %d of them at %s (one eager side pass each): launches / nodes with FOLD_SMALL_PAIRS on, off"
          % (len(gcv.SWEEP), len(gcv.FOLD_CASES), gcv.FOLD_SHAPE))
    for k in keys:
        print("  %-44s %6d %6d" % (k, totals.get((k, True), 0), totals.get((k, False), 0)))
    both = sum(fork == "both" for i, _, _ in walk for _, fork in gcv.forms_of(i))
    early = sum(fork == "early" for i, _, _ in walk for _, fork in gcv.forms_of(i))
    print("  fork candidates per walk: %d early, %d both-on-nodes; preprocess outputs nothing reads: %d" % (early, both, unread))
    assert both > 0 and early > 0
    total = lambda k: totals.get((k, True), 0) + totals.get((k, False), 0)
    for k in ("conv_fwd2", "conv_bwd_both2", "conv_bwd_data2", "dwconv_batch", "se_gate_bwdN", "affine_act_gn2", "affine_act_bwd_gn2",
              "fork: pair_weight_phase", "fork: pair_epilogue_phase", "pair_backward_epilogue", "pair_backward_epilogue -> None",
              "folded nodes, forward", "folded nodes, backward", "side stream left out of a cell's backward", "fold kind vox_multi"):
        assert total(k) > 0, "never reached: " + k
    assert totals.get(("fold kind vox_multi", True), 0) > totals.get(("fold kind vox_multi", False), 0)
    # node 0 of a cell reads two distinct states out of two: BOTH preprocess outputs are read in every genotype the parser can emit, so
    # the zeroing of an unread preprocess gradient (the last lines of the node walk) cannot be reached from a legal genotype
    assert unread == 0
