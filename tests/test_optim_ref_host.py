"""CPU: the fp64 numpy restatement of AdaBound / AdaBoundW and of clip_grad_norm_ (tests/_optim_ref.py) reproduces what the
reference's own classes computed (tests/golden/optim.npz, make_golden_optim.py); the fixture's inputs exercise all three clamp regimes;
and the checkpoint layout the trainers write for these optimisers has the reference state_dict()'s key names."""
import numpy as np
import pytest

import _optim_ref as orf
import make_golden_optim as mo


@pytest.fixture(scope="module")
def inputs():
    return mo.optim_inputs()


def test_inputs_are_what_the_issue_asks_for(inputs):
    p0, g = inputs
    assert p0.shape == (mo.N,) and g.shape == (mo.STEPS, mo.N)
    assert np.array_equal(g, g.astype(np.float32).astype(np.float64)) and np.array_equal(p0, p0.astype(np.float32).astype(np.float64))
    assert not g[:, ::17].any() and (g[:, 1] != 0).all()
    assert mo.lr_of_step(mo.HALVE_AFTER) == mo.LR and mo.lr_of_step(mo.HALVE_AFTER + 1) == mo.LR / 2


@pytest.mark.parametrize("name", list(mo.CASES))
def test_helper_reproduces_the_reference_classes(golden, inputs, name):
    """1e-12 relative to max|x|: fp64 round-off over 24 steps is ~1e-14; the slack covers FMA contraction inside torch's CPU loops"""
    g = golden("optim")
    assert list(g["cases"]) == list(mo.CASES)
    p0, grads = inputs
    case = mo.CASES[name]
    last, kept, norms = orf.run_case(case, p0, grads, mo.lr_of_step, mo.LR, record=(1,))
    for a, x, x1 in zip(mo.ARRAYS, last, kept[1]):
        if a == "vmax" and not case["amsbound"]:
            assert not g["%s/vmax" % name].any()
            continue
        for got, ref in ((x, g["%s/%s" % (name, a)]), (x1, g["%s/%s1" % (name, a)])):
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (name, a)
    if case["max_norm"] is not None:
        ref = g["%s/norms" % name]
        assert ref.shape == (mo.STEPS,) and np.abs(norms - ref).max() <= 1e-12 * ref.max()
        assert (ref > case["max_norm"]).any(), "the clip never engages"
    # the parameters really moved, and fp32 arithmetic costs what the GPU tests' tolerance assumes (a few 1e-7 of max|x|)
    assert np.abs(last[0] - p0).max() > 5e-3
    for a in mo.ARRAYS[:3]:
        rel = float(g["%s/d32/%s" % (name, a)]) / np.abs(g["%s/%s" % (name, a)]).max()
        assert 2e-8 < rel < 2e-6, (name, a, rel)


def test_every_clamp_regime_is_covered(golden, inputs):
    """below the lower bound, above the upper bound, unclamped: each holds >= 5 % of the entries with m != 0 at the last step of
    some case (the zero-gradient entries reach the upper bound only where coupled weight decay gives them a gradient)"""
    g = golden("optim")
    best = [0.0, 0.0, 0.0]
    for name, case in mo.CASES.items():
        v_hat = g["%s/%s" % (name, "vmax" if case["amsbound"] else "v")]
        fr = orf.regimes(g["%s/m" % name], v_hat, mo.STEPS, mo.lr_of_step(mo.STEPS), mo.LR, case["final_lr"], case["gamma"])
        assert abs(sum(fr) - 1.0) < 1e-12
        best = [max(b, f) for b, f in zip(best, fr)]
    assert min(best) >= 0.05, best


def test_clip_coefficient_both_sides_of_one():
    g = np.array([3.0, 4.0])
    assert orf.clip_coef(g, 10.0) == (5.0, 1.0)
    norm, c = orf.clip_coef(g, 1.0, grad_scale=0.5)
    assert norm == 2.5 and c == 1.0 / (2.5 + 1e-6)
    assert orf.clip_coef(np.zeros(3), 0.05) == (0.0, 1.0)


@pytest.mark.parametrize("optimizer,amsbound", [("adabound", False), ("adaboundw", True)])
def test_checkpoint_layout_has_the_reference_key_names(golden, optimizer, amsbound):
    """a CPU FlatParams (construction only: no kernel runs) round-trips through the `optim` layout, whose key names are the ones
    the reference class's state_dict() had when the fixture was made"""
    import torch
    from nas_3d_unet_amd import checkpoint as ck
    from nas_3d_unet_amd.train import FlatParams, OptimSpec
    g = golden("optim")
    name = "w_wd1_ams1" if amsbound else "b_wd1_ams0"
    gen = torch.Generator().manual_seed(3)
    mk = lambda: [torch.nn.Parameter(torch.zeros(s)) for s in ((3, 5), (7,), (2, 2, 2))]
    fp = FlatParams(mk(), "cpu")
    spec = OptimSpec(optimizer, 1e-3, optim_args=dict(weight_decay=1e-2, amsbound=amsbound, gamma=1e-2, final_lr=0.2))
    if amsbound:
        fp.ensure_amsbound()
    else:
        assert fp.max_exp_avg_sq is None
    bufs = [fp.exp_avg, fp.exp_avg_sq] + ([fp.max_exp_avg_sq] if amsbound else [])
    for b in bufs:
        b.copy_(torch.rand(fp.numel, generator=gen))
    fp.step.fill_(9)
    sd = ck.adabound_state_dict(fp, spec, 2.5e-4)
    assert sorted(sd["state"][0]) == list(g["%s/state_keys" % name])
    assert sorted(sd["param_groups"][0]) == list(g["%s/group_keys" % name])
    assert sd["state"][1]["step"] == 9 and sd["state"][2]["exp_avg"].shape == (2, 2, 2)
    grp = sd["param_groups"][0]
    assert (grp["lr"], grp["final_lr"], grp["gamma"], grp["weight_decay"], grp["amsbound"]) == (2.5e-4, 0.2, 1e-2, 1e-2, amsbound)
    fp2 = FlatParams(mk(), "cpu")
    assert ck.load_adabound_state_dict(fp2, spec, sd) == 2.5e-4 and int(fp2.step) == 9
    bufs2 = [fp2.exp_avg, fp2.exp_avg_sq] + ([fp2.max_exp_avg_sq] if amsbound else [])
    for p, o in zip(fp.params, fp.offsets):     # (the flat buffers pad every tensor to a multiple of 4 elements)
        for b, b2 in zip(bufs, bufs2):
            assert torch.equal(b[o:o + p.numel()], b2[o:o + p.numel()])
    # state of the other variant, or of Adam, is refused
    other = OptimSpec(optimizer, 1e-3, optim_args=dict(amsbound=not amsbound))
    with pytest.raises(ValueError, match="amsbound"):
        ck.load_adabound_state_dict(FlatParams(mk(), "cpu"), other, sd)
    with pytest.raises(ValueError, match="not AdaBound"):
        ck.load_adabound_state_dict(FlatParams(mk(), "cpu"), spec, ck.adam_state_dict(fp, 1e-3))


def test_trainer_checkpoint_records_its_optimizer():
    """train_state_dicts of an AdaBoundW trainer names the optimiser; an Adam trainer refuses the file, and an Adam file (which
    carries no record, key for key the reference's) is refused by the AdaBoundW trainer"""
    from nas_3d_unet_amd import checkpoint as ck, searched
    from nas_3d_unet_amd.train import Trainer
    gene = searched.Genotype(down=[("down_conv", 0), ("down_dil_conv", 1), ("down_conv", 1), ("conv", 2), ("dil_conv", 2), ("conv", 3)],
                             up=[("conv", 0), ("up_conv", 1), ("up_conv", 1), ("dil_conv", 2), ("conv", 3), ("up_dil_conv", 1)])
    mk = lambda **kw: Trainer(searched.SearchedNet(4, 4, 3, 2, 3, True, gene), graph=False, **kw)     # construction only
    trw = mk(optimizer="adaboundw", optim_args=dict(amsbound=True, weight_decay=1e-2), grad_clip=5)
    assert trw.fp.max_exp_avg_sq is not None and trw.grad_norm is not None and trw.grad_norm.shape == ()
    tra = mk()
    assert tra.fp.max_exp_avg_sq is None and tra.grad_norm is None
    trw.fp.step.fill_(2)
    trw.fp.max_exp_avg_sq.fill_(0.25)
    sdw = ck.train_state_dicts(trw, 1, {}, 0.5)
    assert sdw["optimizer"] == "adaboundw" and "max_exp_avg_sq" in sdw["optim"]["state"][0]
    sda = ck.train_state_dicts(tra, 1, {}, 0.5)
    assert "optimizer" not in sda
    with pytest.raises(ValueError, match="adaboundw"):
        ck.load_train_state_dicts(tra, sdw)
    with pytest.raises(ValueError, match="adam"):
        ck.load_train_state_dicts(trw, sda)
    with pytest.raises(ValueError, match="adabound"):
        ck.load_train_state_dicts(mk(optimizer="adabound", optim_args=dict(amsbound=True)), sdw)
    tr2 = mk(optimizer="adaboundw", optim_args=dict(amsbound=True, weight_decay=1e-2))
    ck.load_train_state_dicts(tr2, sdw)
    assert int(tr2.fp.step) == 2
    import torch
    for p, o in zip(tr2.fp.params, tr2.fp.offsets):
        assert torch.equal(tr2.fp.max_exp_avg_sq[o:o + p.numel()], trw.fp.max_exp_avg_sq[o:o + p.numel()])


@pytest.mark.parametrize("kw", [dict(optimizer="sgd"), dict(optimizer="adabound", optim_args=dict(gamma=1.0)),
                                dict(optimizer="adabound", optim_args=dict(final_lr=-0.1)), dict(optimizer="adaboundw", betas=(0.9, 1.0)),
                                dict(optimizer="adabound", eps=-1e-8), dict(optimizer="adabound", lr=-1e-3),
                                dict(optimizer="adabound", optim_args=dict(momentum=0.9)), dict(optimizer="adam", optim_args=dict(gamma=1e-3))])
def test_argument_validation_raises_value_error(kw):
    """adabound.py:27-38"""
    from nas_3d_unet_amd.train import OptimSpec
    args = dict(name=kw.get("optimizer", "adam"), lr=kw.get("lr", 1e-3), betas=kw.get("betas", (0.9, 0.999)), eps=kw.get("eps", 1e-8),
                optim_args=kw.get("optim_args"))
    with pytest.raises(ValueError):
        OptimSpec(**args)
