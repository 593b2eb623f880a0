"""CPU: the fp64 restatement of the training recipe (tests/_recipe_ref.py: SGD, AdamW, the device learning-rate schedule, the
moving average of the weights) against torch's own classes; the validation of the spec objects; and the checkpoints of trainers
built on the CPU (construction only: no kernel runs) with an SGD / AdamW optimiser, a schedule and averaged weights."""
import numpy as np
import pytest
import torch

import _recipe_ref as rr
import make_golden_optim as mo


@pytest.fixture(scope="module")
def inputs():
    return mo.optim_inputs(257)


@pytest.mark.parametrize("name", list(rr.CASES))
def test_helper_reproduces_torch_sgd_and_adamw(inputs, name):
    """24 steps in fp64, the rate halved after 12, on inputs with zero-gradient lanes.  1e-12 relative to max|x|: the slack
    test_helper_reproduces_the_reference_classes argues for (fp64 round-off over 24 steps ~1e-14, FMA contraction in torch's loops)"""
    p0, grads = inputs
    assert not grads[:, ::17].any()
    case = rr.CASES[name]
    got = rr.run_case(case, p0, grads)
    want, _ = rr.torch_run(case, p0, grads, torch.float64)
    for a, x, ref in zip(rr.ARRAYS[case["kind"]], got, want):
        assert np.abs(x - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), (name, a)
    assert np.abs(got[0] - p0).max() > 1e-3          # the parameters really moved
    if case["max_norm"] is not None:
        assert any(rr.clip_coef(g, case["max_norm"])[1] < 1.0 for g in grads), "the clip never engages"


def test_first_momentum_step_clones_the_gradient(inputs):
    """dampening 0.5: buf after step one is g, not 0.5 g"""
    p0, grads = inputs
    case = rr.CASES["sgd_mom_damp"]
    got = rr.run_case(case, p0, grads[:1])
    want, _ = rr.torch_run(case, p0, grads[:1], torch.float64)
    assert np.array_equal(got[1], grads[0]) and np.array_equal(want[1], grads[0])


@pytest.mark.parametrize("decay", rr.EMA_DECAYS)
def test_helper_reproduces_averaged_model(inputs, decay):
    params = rr.ema_inputs(*inputs)
    want, n = rr.torch_ema_run(params, decay, torch.float64)
    got = rr.run_ema(params, decay)
    assert n == rr.STEPS and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(got - params[-1]).max() > 1e-3         # the average lags the drifting parameter
    first, n1 = rr.ema_step(np.zeros_like(params[0]), params[0], 0, decay)
    assert n1 == 1 and np.array_equal(first, params[0])  # the first call copies


# ------------------------------------------------------------------------------------------------ schedule
BASE, T, A, POWER, MIN_LR = 1e-2, 1000, 0.1, 0.9, 1e-5


def _torch_rates(kind, W):
    """the rates torch's recursive schedulers give for s = 0 .. T"""
    import warnings
    from torch.optim import lr_scheduler as ls
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=BASE)
    decay = (lambda: ls.PolynomialLR(opt, total_iters=T - W, power=POWER)) if kind == "poly" else \
            (lambda: ls.CosineAnnealingLR(opt, T_max=T - W, eta_min=MIN_LR))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = decay() if W == 0 else ls.SequentialLR(opt, [ls.LinearLR(opt, start_factor=A, total_iters=W), decay()], milestones=[W])
        out = []
        for _ in range(T + 1):
            out.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
    return np.array(out)


@pytest.mark.parametrize("kind", ["poly", "cosine"])
@pytest.mark.parametrize("W", [0, 20])
def test_schedule_statement_matches_torch_schedulers(kind, W):
    """4 T 2^-52 relative: the multiplicative round-off of torch's recursions over T steps (worst gap measured 2.3e-15).  torch's
    PolynomialLR has no floor; the statement's floor at min_lr changes the last entry only (s = T, where torch reaches 0), so torch's
    rates are floored the same way before the comparison.  Past T torch's cosine turns back up: compared up to T only."""
    want = _torch_rates(kind, W)
    if kind == "poly":
        assert (want[:-1] > MIN_LR).all() and want[-1] == 0.0
        want = np.maximum(want, MIN_LR)
    got = np.array([rr.schedule_lr(kind, s, BASE, T, POWER, W, A, MIN_LR) for s in range(T + 1)])
    gap = np.abs(got - want) / want
    print("%s W=%d: worst relative gap %.2e" % (kind, W, gap.max()))
    assert gap.max() <= 4 * T * 2.0 ** -52


@pytest.mark.parametrize("kind", ["poly", "cosine"])
def test_schedule_statement_edges(kind):
    """warm-up starts at a * base and ends exactly at base; at and past T the rate is min_lr (cosine) or max(0, min_lr) (poly)"""
    f = lambda s, **kw: rr.schedule_lr(kind, s, BASE, T, POWER, **dict(dict(warmup_steps=20, warmup_start=A, min_lr=MIN_LR), **kw))
    assert f(0) == BASE * A and f(20) == BASE and f(0, warmup_steps=0) == BASE
    assert f(19) < BASE and f(21) < BASE
    for s in (T, T + 1, T + 7):
        assert f(s) == MIN_LR and f(s, min_lr=0.0) == 0.0


# ------------------------------------------------------------------------------------------------ specs
@pytest.mark.parametrize("make", [
    lambda tr: tr.SGD(momentum=-0.1), lambda tr: tr.SGD(weight_decay=-1e-5), lambda tr: tr.SGD(nesterov=True),
    lambda tr: tr.SGD(momentum=0.9, nesterov=True, dampening=0.1), lambda tr: tr.SGD().bound(-1e-3),
    lambda tr: tr.AdamW(weight_decay=-1e-2), lambda tr: tr.AdamW(betas=(1.0, 0.999)), lambda tr: tr.AdamW(betas=(0.9, -0.1)),
    lambda tr: tr.AdamW(eps=-1e-8), lambda tr: tr.AdamW().bound(-1.0), lambda tr: tr.EMA(0.5), lambda tr: tr.EMA(1.0),
    lambda tr: tr.PolyLR(total_steps=10, warmup_steps=10), lambda tr: tr.CosineLR(total_steps=10, warmup_start=1.5),
    lambda tr: tr.PolyLR(total_steps=10, min_lr=-1.0), lambda tr: tr.OptimSpec("sgd"), lambda tr: tr.OptimSpec("adamw"),
    lambda tr: tr._optim_spec(tr.SGD(), 1e-3, (0.9, 0.999), 1e-8, dict(weight_decay=1e-2))])
def test_spec_validation_raises_value_error(make):
    from nas_3d_unet_amd import train
    with pytest.raises(ValueError):
        make(train)


def test_specs_carry_their_names_and_constants():
    from nas_3d_unet_amd import train
    s = train.SGD(momentum=0.99, nesterov=True, dampening=0.0, weight_decay=3e-5)
    a = train.AdamW(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    assert (s.name, s.momentum, s.nesterov, s.dampening, s.weight_decay) == ("sgd", 0.99, True, 0.0, 3e-5)
    assert (a.name, a.betas, a.eps, a.weight_decay) == ("adamw", (0.9, 0.999), 1e-8, 1e-2)
    assert train.PolyLR(total_steps=5).state_dict() == dict(kind="poly", total_steps=5, power=0.9, warmup_steps=0, warmup_start=0.1, min_lr=0.0)
    assert train.CosineLR(total_steps=5, warmup_steps=2, min_lr=1e-6).state_dict()["kind"] == "cosine"
    assert train.EMA().decay == 0.999


# ------------------------------------------------------------------------------------------------ CPU-built trainers
def _net():
    from nas_3d_unet_amd import searched
    gene = searched.Genotype(down=[("down_conv", 0), ("down_dil_conv", 1), ("down_conv", 1), ("conv", 2), ("dil_conv", 2), ("conv", 3)],
                             up=[("conv", 0), ("up_conv", 1), ("up_conv", 1), ("dil_conv", 2), ("conv", 3), ("up_dil_conv", 1)])
    return searched.SearchedNet(4, 4, 3, 2, 3, True, gene)


def _trainer(**kw):
    from nas_3d_unet_amd.train import Trainer
    return Trainer(_net(), graph=False, **kw)     # construction only


def _fill(tr, seed, step):
    gen = torch.Generator().manual_seed(seed)
    for b in (tr.fp.exp_avg, tr.fp.exp_avg_sq) + ((tr.fp.ema,) if tr.fp.ema is not None else ()):
        b.copy_(torch.rand(tr.fp.numel, generator=gen))
    tr.fp.step.fill_(step)


def _same_per_parameter(a, b, fp):
    return all(torch.equal(a[o:o + p.numel()], b[o:o + p.numel()]) for p, o in zip(fp.params, fp.offsets))


def test_default_trainer_checkpoint_keeps_todays_keys():
    from nas_3d_unet_amd import checkpoint as ck
    tr = _trainer()
    assert tr.schedule is None and tr.ema is None and tr.fp.ema is None and tr.scheduler is not None
    tr.fp.step.fill_(3)
    sd = ck.train_state_dicts(tr, 1, {}, 0.5)
    assert sorted(sd) == ["best_loss", "epoch", "history", "model_param", "optim", "scheduler"]
    ref = torch.optim.Adam(_net().parameters(), lr=1e-3).state_dict()
    assert sorted(sd["optim"]["param_groups"][0]) == sorted(ref["param_groups"][0])
    assert sorted(sd["optim"]["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    assert "kind" not in sd["scheduler"] and sd["scheduler"]["mode"] == "min"
    with pytest.raises(Exception, match="ema"):
        tr.averaged_weights()


def test_sgd_checkpoint_is_torchs_layout_and_round_trips():
    from nas_3d_unet_amd import checkpoint as ck, train
    spec = dict(momentum=0.99, nesterov=True, weight_decay=3e-5)
    tr = _trainer(lr=1e-2, optimizer=train.SGD(**spec), schedule=train.PolyLR(total_steps=100, warmup_steps=5), ema=train.EMA(0.9))
    assert tr.scheduler is None and tr.optim.name == "sgd"
    _fill(tr, 5, 7)
    tr.fp.ema_state[0] = 7
    sd = ck.train_state_dicts(tr, 1, {}, 0.5)
    assert sd["optimizer"] == "sgd" and sd["optimizer_step"] == 7
    assert sd["scheduler"] == dict(kind="poly", total_steps=100, power=0.9, warmup_steps=5, warmup_start=0.1, min_lr=0.0)
    assert sd["ema"]["n_averaged"] == 7 and sorted(sd["ema"]["params"]) == sorted(sd["model_param"])
    # torch's own class takes what the trainer wrote ...
    net = _net()
    opt = torch.optim.SGD(net.parameters(), lr=0.5, **spec)
    ref_sd = opt.state_dict()
    assert sorted(sd["optim"]["param_groups"][0]) == sorted(ref_sd["param_groups"][0])
    assert {k: v for k, v in sd["optim"]["param_groups"][0].items() if k != "params"} == \
           dict({k: v for k, v in ref_sd["param_groups"][0].items() if k != "params"}, lr=1e-2)
    opt.load_state_dict(sd["optim"])
    assert sorted(sd["optim"]["state"][0]) == ["momentum_buffer"]
    for i, (p, q, o) in enumerate(zip(net.parameters(), tr.fp.params, tr.fp.offsets)):
        assert torch.equal(opt.state[p]["momentum_buffer"].reshape(-1), tr.fp.exp_avg[o:o + q.numel()])
    # ... and the trainer what torch wrote (no step record: 1, a first step was taken), and its own file
    tr2 = _trainer(lr=1e-3, optimizer=train.SGD(**spec))
    assert ck.load_sgd_state_dict(tr2.fp, tr2.optim, opt.state_dict()) == 1e-2 and int(tr2.fp.step) == 1
    assert _same_per_parameter(tr2.fp.exp_avg, tr.fp.exp_avg, tr.fp)
    tr3 = _trainer(lr=1e-3, optimizer=train.SGD(**spec), schedule=train.PolyLR(total_steps=100, warmup_steps=5), ema=train.EMA(0.9))
    ck.load_train_state_dicts(tr3, sd)
    assert int(tr3.fp.step) == 7 and tr3.lr == 1e-2 and float(tr3._sched_rec[1]) == 1e-2
    assert tr3.fp.ema_state.tolist() == [7, 7, 0]
    assert _same_per_parameter(tr3.fp.exp_avg, tr.fp.exp_avg, tr.fp) and _same_per_parameter(tr3.fp.ema, tr.fp.ema, tr.fp)
    # the averaged parameters load into a module of the same net
    net.load_state_dict(sd["ema"]["params"])
    p0, q0, o0 = next(net.parameters()), tr.fp.params[0], tr.fp.offsets[0]
    assert torch.equal(p0.detach().reshape(-1), tr.fp.ema[o0:o0 + q0.numel()])
    # a file without averaged weights: averaging starts over
    del sd["ema"]
    ck.load_train_state_dicts(tr3, sd)
    assert tr3.fp.ema_state.tolist() == [0, 7, 0] and float(tr3.fp.ema.abs().max()) == 0.0


def test_adamw_checkpoint_is_torchs_layout_and_round_trips():
    from nas_3d_unet_amd import checkpoint as ck, train
    spec = dict(betas=(0.8, 0.99), eps=1e-7, weight_decay=5e-2)
    tr = _trainer(lr=2e-3, optimizer=train.AdamW(**spec), schedule=train.CosineLR(total_steps=50, warmup_steps=3, min_lr=1e-6))
    _fill(tr, 6, 4)
    sd = ck.train_state_dicts(tr, 1, {}, 0.5)
    assert sd["optimizer"] == "adamw" and "optimizer_step" not in sd and "ema" not in sd and sd["scheduler"]["kind"] == "cosine"
    net = _net()
    opt = torch.optim.AdamW(net.parameters(), lr=0.5, **spec)
    ref_sd = opt.state_dict()
    assert {k: v for k, v in sd["optim"]["param_groups"][0].items() if k != "params"} == \
           dict({k: v for k, v in ref_sd["param_groups"][0].items() if k != "params"}, lr=2e-3)
    assert sorted(sd["optim"]["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    opt.load_state_dict(sd["optim"])
    p0, q0, o0 = next(net.parameters()), tr.fp.params[0], tr.fp.offsets[0]
    assert float(opt.state[p0]["step"]) == 4 and torch.equal(opt.state[p0]["exp_avg_sq"].reshape(-1), tr.fp.exp_avg_sq[o0:o0 + q0.numel()])
    tr2 = _trainer(optimizer=train.AdamW(**spec), schedule=train.CosineLR(total_steps=50))
    ck.load_train_state_dicts(tr2, dict(sd, optim=opt.state_dict()))
    assert int(tr2.fp.step) == 4 and tr2.lr == 2e-3
    assert _same_per_parameter(tr2.fp.exp_avg, tr.fp.exp_avg, tr.fp) and _same_per_parameter(tr2.fp.exp_avg_sq, tr.fp.exp_avg_sq, tr.fp)


def test_mismatched_optimizer_or_schedule_raises():
    from nas_3d_unet_amd import checkpoint as ck, train
    sgd = _trainer(optimizer=train.SGD(momentum=0.9))
    adamw = _trainer(optimizer=train.AdamW())
    adam = _trainer()
    poly = _trainer(schedule=train.PolyLR(total_steps=10))
    cosine = _trainer(schedule=train.CosineLR(total_steps=10))
    files = {k: ck.train_state_dicts(t, 1, {}, 0.5) for k, t in dict(sgd=sgd, adamw=adamw, adam=adam, poly=poly, cosine=cosine).items()}
    for tr, key, match in ((adam, "sgd", "sgd"), (adam, "adamw", "adamw"), (sgd, "adamw", "adamw"), (adamw, "sgd", "sgd"), (sgd, "adam", "adam"),
                           (adamw, "adam", "adam"), (adam, "poly", "poly"), (poly, "adam", "plateau"), (poly, "cosine", "cosine"),
                           (cosine, "poly", "poly")):
        with pytest.raises(ValueError, match=match):
            ck.load_train_state_dicts(tr, files[key])
    # the layouts refuse each other also without the record
    with pytest.raises(ValueError, match="not SGD"):
        ck.load_sgd_state_dict(sgd.fp, sgd.optim, files["adamw"]["optim"])
    with pytest.raises(ValueError, match="not AdamW"):
        ck.load_adamw_state_dict(adamw.fp, adamw.optim, files["sgd"]["optim"])
    # new_lr=True takes the weights only
    assert ck.load_train_state_dicts(poly, files["cosine"], new_lr=True)[0] == 2
    assert ck.load_train_state_dicts(adam, files["sgd"], new_lr=True)[0] == 2


def test_search_trainer_takes_a_spec_object_and_no_schedule_or_ema():
    import inspect
    from nas_3d_unet_amd import train
    sig = inspect.signature(train.SearchTrainer.__init__).parameters
    assert "optimizer" in sig and "schedule" not in sig and "ema" not in sig
