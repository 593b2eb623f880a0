"""GPU: the flat SGD and AdamW updates (n3d_sgd_step*, n3d_adamw_step*), the device learning-rate schedule (n3d_lr_schedule), the
moving average of the weights (n3d_ema_step) and the buffer exchange (n3d_swap_f32), and their way through Trainer, against the fp64
helper tests/_recipe_ref.py (itself held to torch's classes by tests/test_recipe_ref_host.py).

Tolerance of every comparison of p / buf / exp_avg / exp_avg_sq / ema with the helper, the AdaBound test's rule:
    max|dev - ref64| <= 4 * d32 + 2^-23 * max|ref64|
d32 is max|torch fp32 run - torch fp64 run| of the same case, size and array on the CPU, computed here: what torch's own fp32
arithmetic costs on that trajectory.  The factor 4 covers contraction (fma) and another association than torch's CPU loops; the
floor is one rounding of the largest entry.  The helper is given the rate the kernel is given (the fp32 value of the device word).
The kernel tests print max|dev - ref64| / d32 per array at n = 257.  Measured on MI355X: SGD p 1.000, momentum buffer 0.82-1.12; AdamW
p 1.000-1.001, exp_avg 3.32, exp_avg_sq 1.64; EMA 1.000 ("Training recipe").
"""
import numpy as np
import pytest
import torch

import _recipe_ref as rr
import make_golden_optim as mo
from _util import dev

pytestmark = pytest.mark.gpu

SIZES = (1, 5, 257, 16421)        # 16421 = 2 * 8192 + 37: three workgroups, a ragged float4 tail
F32 = lambda x: float(np.float32(x))
lr32_of_step = lambda t: F32(rr.lr_of_step(t))
_REF = {}


def _reference(name, n):
    """(p0, grads, helper's fp64 final state, d32 per array) of a case at size n, computed once"""
    if (name, n) not in _REF:
        p0, grads = mo.optim_inputs(n)
        case = rr.CASES[name]
        t64, t32 = rr.torch_run(case, p0, grads, torch.float64)[0], rr.torch_run(case, p0, grads, torch.float32)[0]
        _REF[name, n] = (p0, grads, rr.run_case(case, p0, grads, lr32_of_step), tuple(float(np.abs(a - b).max()) for a, b in zip(t32, t64)))
    return _REF[name, n]


def _ema_reference(decay, n):
    if ("ema", decay, n) not in _REF:
        params = rr.ema_inputs(*mo.optim_inputs(n))
        d32 = float(np.abs(rr.torch_ema_run(params, decay, torch.float32)[0] - rr.torch_ema_run(params, decay, torch.float64)[0]).max())
        _REF["ema", decay, n] = (params, rr.run_ema(params, decay), d32)
    return _REF["ema", decay, n]


def _tol(d32, ref):
    return 4.0 * d32 + 2.0 ** -23 * float(np.abs(ref).max())


def _buf(n, offset, fill=None):
    """n floats, `offset` floats off a 16-byte boundary"""
    t = torch.zeros(n + offset, device="cuda")[offset:]
    if fill is not None:
        t.copy_(torch.from_numpy(np.asarray(fill, np.float32)))
    return t


def _step_word(ticketed):
    from nas_3d_unet_amd import kernels as K
    return K.step_counter("cuda") if ticketed else torch.zeros(1, dtype=torch.int32, device="cuda")


class _Run:
    """24 launches of one case on the device: eagerly, or one captured {norm, update} pair replayed 24 times"""

    def __init__(self, name, n, offset=0, ticketed=True, graph=False):
        from nas_3d_unet_amd import kernels as K
        case = rr.CASES[name]
        p0, grads = _reference(name, n)[:2]
        self.p, self.m, self.v = _buf(n, offset, p0), _buf(n, offset), _buf(n, offset)
        self.step = _step_word(ticketed)
        gs = [_buf(n, offset, g) for g in grads]
        gbuf = _buf(n, offset)
        lr_dev = torch.full((1,), rr.LR, dtype=torch.float32, device="cuda")
        out = torch.zeros(2, device="cuda")
        scratch = K.grad_clip_scratch("cuda")

        def launch(g):
            coef = None
            if case["max_norm"] is not None:
                K.grad_clip_coef(g, case["max_norm"], scratch, out)
                coef = out[1:]
            if case["kind"] == "sgd":
                K.sgd_step(self.p, g, self.m if case["momentum"] != 0 else None, self.step, rr.LR, case["momentum"], case["dampening"],
                           case["weight_decay"], case["nesterov"], lr_dev=lr_dev, coef=coef)
            else:
                K.adamw_step(self.p, g, self.m, self.v, self.step, rr.LR, case["betas"][0], case["betas"][1], case["eps"],
                             case["weight_decay"], lr_dev=lr_dev, coef=coef)

        graph_obj = None
        if graph:
            graph_obj = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph_obj, capture_error_mode="thread_local"):
                launch(gbuf)
        for t in range(1, rr.STEPS + 1):
            if graph:
                gbuf.copy_(gs[t - 1])
                graph_obj.replay()
            else:
                launch(gs[t - 1])
            if t == rr.HALVE_AFTER:
                lr_dev.fill_(rr.LR * 0.5)
        torch.cuda.synchronize()
        self.tensors = (self.p, self.m) if case["kind"] == "sgd" else (self.p, self.m, self.v)

    def arrays(self):
        return [x.double().cpu().numpy() for x in self.tensors]


class _EmaRun:
    """24 averaged updates of a drifting parameter; the step word moves by one in front of every launch (the optimiser's part)"""

    def __init__(self, decay, n, offset=0, graph=False):
        from nas_3d_unet_amd import kernels as K
        params = _ema_reference(decay, n)[0]
        self.ema, p = _buf(n, offset), _buf(n, offset)
        self.state = K.ema_state("cuda")
        step = _step_word(True)
        ps = [_buf(n, offset, q) for q in params]

        def launch():
            step.add_(1)
            K.ema_step(self.ema, p, decay, step, self.state)

        graph_obj = None
        if graph:
            graph_obj = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph_obj, capture_error_mode="thread_local"):
                launch()
        for q in ps:
            p.copy_(q)
            graph_obj.replay() if graph else launch()
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ kernels against the helper
@pytest.mark.parametrize("name", list(rr.CASES))
def test_update_kernels_match_the_fp64_helper(name):
    """every case at n in {1, 5, 257, 16421}, 24 launches with lr_dev halved after 12.  Prints max|dev - ref64| / d32 per array at
    n = 257 (allowed: 4 + the floor)"""
    kind = rr.CASES[name]["kind"]
    for n in SIZES:
        run = _Run(name, n)
        assert int(run.step) == rr.STEPS and int(run.step._base[1]) == 0
        _, _, ref, d32 = _reference(name, n)
        for a, got, want, d in zip(rr.ARRAYS[kind], run.arrays(), ref, d32):
            err, tol = float(np.abs(got - want).max()), _tol(d, want)
            if n == 257:
                print("%s %s: max|dev - ref64| / d32 = %s" % (name, a, "%.3f" % (err / d) if d > 0 else "d32 = 0, err %.1e" % err))
            assert err <= tol, (name, n, a, err, tol)
        if kind == "sgd" and rr.CASES[name]["momentum"] == 0:
            assert float(run.m.abs().max()) == 0.0          # no buffer was passed: nothing but p is written


@pytest.mark.parametrize("decay", rr.EMA_DECAYS)
def test_ema_kernel_matches_the_fp64_helper(decay):
    for n in SIZES:
        run = _EmaRun(decay, n)
        _, ref, d32 = _ema_reference(decay, n)
        err = float(np.abs(run.ema.double().cpu().numpy() - ref).max())
        if n == 257:
            print("ema %g: max|dev - ref64| / d32 = %.3f" % (decay, err / d32))
        assert err <= _tol(d32, ref), (decay, n, err, d32)
        assert run.state.tolist() == [rr.STEPS, rr.STEPS, 0]


# ------------------------------------------------------------------------------------------------ same bits across launch forms
@pytest.mark.parametrize("name", list(rr.CASES))
def test_unaligned_views_unticketed_counter_and_graph_replay_give_the_same_bits(name):
    """a view one float off the 16-byte boundary takes the element-wise path, a plain int32 step word the second tiny launch, a
    captured launch 24 replays: all bit-identical to the aligned, ticketed, eager run, and the counters end at 24"""
    for n in (257, 16421):
        base = _Run(name, n)
        for kw in (dict(offset=1), dict(ticketed=False), dict(graph=True), dict(graph=True, offset=1, ticketed=False)):
            other = _Run(name, n, **kw)
            assert int(other.step) == rr.STEPS, kw
            for x, y in zip(base.tensors, other.tensors):
                assert torch.equal(x, y), (name, n, kw)


@pytest.mark.parametrize("decay", rr.EMA_DECAYS)
def test_ema_launch_forms_give_the_same_bits(decay):
    for n in (257, 16421):
        base = _EmaRun(decay, n)
        for kw in (dict(offset=1), dict(graph=True), dict(graph=True, offset=1)):
            other = _EmaRun(decay, n, **kw)
            assert torch.equal(base.ema, other.ema) and other.state.tolist() == [rr.STEPS, rr.STEPS, 0], (n, kw)


def test_swap_twice_restores_both_buffers():
    from nas_3d_unet_amd import kernels as K
    for n in SIZES:
        for oa, ob in ((0, 0), (1, 1), (1, 0)):
            rng = np.random.default_rng(n + oa)
            an, bn = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
            a, b = _buf(n, oa, an), _buf(n, ob, bn)
            a0, b0 = a.clone(), b.clone()
            K.swap_f32(a, b)
            assert torch.equal(a, b0) and torch.equal(b, a0), (n, oa, ob)
            K.swap_f32(a, b)
            assert torch.equal(a, a0) and torch.equal(b, b0), (n, oa, ob)
    with pytest.raises(K.N3DError):
        K.swap_f32(a, a)


# ------------------------------------------------------------------------------------------------ guards
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_guarded_update_withholds_the_update_and_the_average(kind):
    """time-outs != acknowledged (or a peer's flag) -> parameters, buffers and the step counter are bit-unchanged, the loss reads NaN,
    the host word is set, and the EMA launch behind it leaves ema and n_averaged as they are; equal counters -> the ordinary update,
    bit-identical to the unguarded launch, and the average moves"""
    from nas_3d_unet_amd import kernels as K
    n = 10000
    g = torch.randn(n, device="cuda")
    mk = lambda: (torch.ones(n, device="cuda"), torch.full((n,), 0.125, device="cuda"), torch.full((n,), 0.5, device="cuda"), K.step_counter("cuda"))

    def update(p, m, v, st, guard=None):
        if kind == "sgd":
            K.sgd_step(p, g, m, st, 1e-2, 0.9, 0.0, 1e-2, True, guard=guard)
        else:
            K.adamw_step(p, g, m, v, st, 1e-2, guard=guard)

    words = torch.zeros(4, dtype=torch.int32, device="cuda")     # [0] time-outs, [1] acknowledged
    flag = torch.zeros(1, device="cuda")
    hw = K.HostWord()
    p0, m0, v0, st0 = mk()
    for _ in range(2):                                           # (two steps: the second takes the momentum rule, not the clone)
        update(p0, m0, v0, st0)
    assert not torch.equal(p0, torch.ones_like(p0)) and int(st0) == 2
    for bad_words, bad_flag in ((False, False), (True, False), (False, True)):
        p, m, v, st = mk()
        update(p, m, v, st)
        ema, state = torch.zeros(n, device="cuda"), K.ema_state("cuda")
        K.ema_step(ema, p, 0.9, st, state)
        p1, m1, v1, ema1 = p.clone(), m.clone(), v.clone(), ema.clone()
        assert state.tolist() == [1, 1, 0] and torch.equal(ema, p)
        loss = torch.full((), 0.5, device="cuda")
        words[0], words[1] = (3 if bad_words else 2), 2
        flag[0] = 1.0 if bad_flag else 0.0
        hw.clear()
        update(p, m, v, st, K.UpdateGuard(words.data_ptr(), words.data_ptr() + 4, flag.data_ptr(), loss.data_ptr(), hw.ptr))
        K.ema_step(ema, p, 0.9, st, state)
        torch.cuda.synchronize()
        if bad_words or bad_flag:
            assert torch.equal(p, p1) and torch.equal(m, m1) and torch.equal(v, v1)
            assert int(st) == 1 and int(st._base[1]) == 0
            assert torch.isnan(loss) and hw.value == 1
            assert torch.equal(ema, ema1) and state.tolist() == [1, 1, 0]
        else:
            assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0) and int(st) == 2
            assert float(loss) == 0.5 and hw.value == 0
            assert state.tolist() == [2, 2, 0] and not torch.equal(ema, ema1)
            want = ema1.double() + float(np.float32(1.0 - 0.9)) * (p.double() - ema1.double())
            assert float((ema.double() - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------ schedule
BASE, T, W, A, POWER, MIN_LR = 1e-2, 1000, 20, 0.1, 0.9, 1e-5


@pytest.mark.parametrize("kind,min_lr", [("poly", MIN_LR), ("poly", 0.0), ("cosine", MIN_LR)])
def test_lr_schedule_kernel_follows_the_statement(kind, min_lr):
    """for a step word set to each s, lr_out is within one fp32 step of the fp32 rounding of the statement (the allowance is for the
    device's fp64 pow / cos against libm's); exactly fl32(base) at s = W, where the warm-up ends"""
    from nas_3d_unet_amd import kernels as K
    rec = K.lr_schedule_record(K.LR_POLY if kind == "poly" else K.LR_COSINE, BASE, min_lr, W, A, T, POWER, "cuda")
    assert rec.numel() == K.LR_REC_LEN
    step, out = _step_word(True), torch.full((1,), -1.0, device="cuda")
    for s in (0, 1, W - 1, W, W + 1, T // 2, T - 1, T, T + 7):
        step.fill_(s)
        K.lr_schedule(step, rec, out)
        got, want = float(out), np.float32(rr.schedule_lr(kind, s, BASE, T, POWER, W, A, min_lr))
        assert abs(got - float(want)) <= float(np.spacing(want)), (kind, s, got, float(want))
        if s == W:
            assert got == F32(BASE)
        if s >= T:
            assert got == F32(min_lr)
    rec[1:2].fill_(BASE / 4)             # a new base rate is one device fill
    step.fill_(W)
    K.lr_schedule(step, rec, out)
    assert float(out) == F32(BASE / 4) and int(step) == W


# ------------------------------------------------------------------------------------------------ through Trainer
def _small_net():
    import golden_common as gc
    from test_gpu_nets import build_net
    key, kind, gname, depth, size, batch, adam = [c for c in gc.net_cases() if c[6] and c[1] == "searched"][0]
    xn, tn = gc.net_batch(key, batch, size)
    return (lambda: build_net(kind, gname, depth)[0]), dev(xn), dev(tn)


N_STEPS = 6


def _recipes():
    from nas_3d_unet_amd import train
    return {
        "sgd_poly": (dict(lr=1e-2, optimizer=train.SGD(momentum=0.99, nesterov=True, weight_decay=3e-5),
                          schedule=train.PolyLR(total_steps=N_STEPS, warmup_steps=2)),
                     rr._sgd(momentum=0.99, nesterov=True, weight_decay=3e-5), ("flat", "exp_avg"), "poly", dict(power=0.9, warmup_steps=2)),
        "adamw_cosine": (dict(lr=1e-3, optimizer=train.AdamW(weight_decay=1e-2), schedule=train.CosineLR(total_steps=N_STEPS, warmup_steps=1, min_lr=1e-6)),
                         rr._adamw(weight_decay=1e-2), ("flat", "exp_avg", "exp_avg_sq"), "cosine", dict(warmup_steps=1, min_lr=1e-6)),
    }


@pytest.mark.parametrize("recipe", ["sgd_poly", "adamw_cosine"])
def test_trainer_steps_follow_the_helper_and_the_schedule(recipe):
    """graph=True, six steps: after every step the weights (and the optimiser's buffers) equal the helper applied to the state before
    it, the step's own fp.grad and the rate lr_dev holds; lr_dev is within one fp32 step of the schedule statement at the updates
    applied before the step.  d32: torch's class run from the initial weights over the recorded gradients, fp32 against fp64,
    through that step"""
    from nas_3d_unet_amd.train import Trainer
    kw, case, keys, kind, skw = _recipes()[recipe]
    mk, x, t = _small_net()
    tr = Trainer(mk(), graph=True, **kw)
    assert tr.scheduler is None
    snap = lambda: {k: getattr(tr.fp, k).double().cpu().numpy() for k in keys}
    start = prev = snap()
    grads, rates = [], []
    for k in range(N_STEPS):
        tr.step(x, t)
        cur, grad, lr = snap(), tr.fp.grad.double().cpu().numpy(), float(tr.lr_dev)
        want_lr = np.float32(rr.schedule_lr(kind, k, kw["lr"], N_STEPS, **skw))
        assert abs(lr - float(want_lr)) <= float(np.spacing(want_lr)), (k, lr, float(want_lr))
        grads.append(grad)
        rates.append(lr)
        t64, t32 = [], []
        rr.torch_run(case, start["flat"], grads, torch.float64, lambda s: rates[s - 1], t64)
        rr.torch_run(case, start["flat"], grads, torch.float32, lambda s: rates[s - 1], t32)
        want = rr.apply_case(case, tuple(prev[key] for key in keys), grad, k + 1, lr)
        for i, key in enumerate(keys):
            d32 = float(np.abs(t32[-1][i] - t64[-1][i]).max())
            err = float(np.abs(cur[key] - want[i]).max())
            assert err <= _tol(d32, want[i]), (recipe, k, key, err, d32)
        assert float(np.abs(cur["flat"] - prev["flat"]).max()) > 0 or lr == 0.0
        prev = cur
    assert int(tr.fp.step) == N_STEPS
    tr.set_lr(kw["lr"] / 2)              # the base rate, between replays: the next issued step reads it
    tr.step(x, t)
    want_lr = np.float32(rr.schedule_lr(kind, N_STEPS, kw["lr"] / 2, N_STEPS, **skw))
    assert abs(float(tr.lr_dev) - float(want_lr)) <= float(np.spacing(want_lr))
    tr.check_sync()


@pytest.fixture(scope="module")
def ema_runs():
    """two trainers with ema=EMA(0.9) on default Adam, four steps each: `a` enters averaged_weights() after step three (evaluates there,
    and tries a step), `b` never does"""
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd.train import EMA, Trainer
    mk, x, t = _small_net()
    out = {}
    for tag in ("a", "b"):
        tr = Trainer(mk(), graph=True, ema=EMA(0.9))
        rec = dict(flat=[], ema=[], loss=[])
        for k in range(4):
            if k == 3 and tag == "a":
                before = tr.fp.flat.clone()
                with tr.averaged_weights() as same:
                    assert same is tr and torch.equal(tr.fp.flat, rec["ema"][-1]) and torch.equal(tr.fp.ema, before)
                    rec["eval_inside"] = tr.evaluate(x, t).clone()
                    rec["state_dict_inside"] = {n: v.clone() for n, v in tr.model.state_dict().items()}
                    with pytest.raises(K.N3DError, match="averaged_weights"):
                        tr.step(x, t)
                assert torch.equal(tr.fp.flat, before) and torch.equal(tr.fp.ema, rec["ema"][-1])
            loss = tr.step(x, t)
            rec["loss"].append(loss.clone())
            rec["flat"].append(tr.fp.flat.clone())
            rec["ema"].append(tr.fp.ema.clone())
        tr.check_sync()
        assert tr.fp.ema_state.tolist() == [4, 4, 0]
        out[tag] = (tr, rec)
    return out, (mk, x, t)


def test_trainer_ema_follows_the_helper(ema_runs):
    tr, rec = ema_runs[0]["b"]
    flats = np.stack([f.double().cpu().numpy() for f in rec["flat"]])
    for k in range(4):
        ref = rr.run_ema(flats[:k + 1], 0.9)
        d32 = float(np.abs(rr.torch_ema_run(flats[:k + 1], 0.9, torch.float32)[0] - rr.torch_ema_run(flats[:k + 1], 0.9, torch.float64)[0]).max())
        err = float(np.abs(rec["ema"][k].double().cpu().numpy() - ref).max())
        assert err <= _tol(d32, ref), (k, err, d32)
    assert torch.equal(rec["ema"][0], rec["flat"][0]) and not torch.equal(rec["ema"][3], rec["flat"][3])


def test_averaged_weights_block_evaluates_the_average_and_restores_the_bits(ema_runs):
    """inside the block evaluate() returns the loss of a second trainer loaded with the averaged weights, and model.state_dict() holds
    them; after it the weights and the next step's loss are bit-identical to the run that never entered it"""
    from nas_3d_unet_amd.train import Trainer
    runs, (mk, x, t) = ema_runs
    (tra, a), (trb, b) = runs["a"], runs["b"]
    for k in range(4):
        assert torch.equal(a["loss"][k], b["loss"][k]) and torch.equal(a["flat"][k], b["flat"][k]) and torch.equal(a["ema"][k], b["ema"][k]), k
    other = Trainer(mk(), graph=True)
    other.fp.flat.copy_(b["ema"][2])
    want = other.evaluate(x, t).clone()
    assert torch.equal(a["eval_inside"], want)
    other.fp.flat.copy_(b["flat"][2])
    assert not torch.equal(other.evaluate(x, t), want)
    other.fp.flat.copy_(b["ema"][2])
    assert sorted(a["state_dict_inside"]) == sorted(other.model.state_dict())
    for n, v in other.model.state_dict().items():
        assert torch.equal(a["state_dict_inside"][n], v), n


def test_averaged_weights_needs_an_average():
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd.train import EMA, Trainer
    mk, x, t = _small_net()
    with pytest.raises(K.N3DError, match="ema"):
        Trainer(mk(), graph=False, side_wgrad=False).averaged_weights()
    tr = Trainer(mk(), graph=False, side_wgrad=False, ema=EMA(0.9))
    with pytest.raises(K.N3DError, match="averaged yet"):
        with tr.averaged_weights():
            pass
    assert not tr._averaged


@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_padded_twin_entries_stay_zero(which):
    """init_n_kernels = 6: the net trains as its zero-padded twin; under SGD with momentum and weight decay and under AdamW the padded
    entries of the weights, of the optimiser's buffers and of the averaged weights are still exactly 0 after two steps"""
    from nas_3d_unet_amd import searched, train
    from oracle import ref_path as orc
    from test_gpu_nets import _genotype_for
    from _util import fill_module
    cfg = orc.NetCfg(4, 6, 3, 2, 3, True)
    gene = _genotype_for(cfg.n_nodes)
    net = searched.SearchedNet(cfg.in_channels, cfg.init_n_kernels, cfg.out_channels, cfg.depth, cfg.n_nodes, cfg.channel_change,
                               searched.Genotype(list(gene.down), list(gene.up)))
    fill_module(net)
    net.last_conv[0].dropout = None
    rng = np.random.default_rng(23)
    x = dev(rng.standard_normal((2, 4, 16, 16, 32)).astype(np.float32))
    t = dev((rng.uniform(0, 1, (2, 3, 16, 16, 32)) < 0.3).astype(np.float32))
    opt = train.SGD(momentum=0.9, nesterov=True, weight_decay=1e-2) if which == "sgd" else train.AdamW(weight_decay=1e-2)
    tr = train.Trainer(net.cuda(), lr=1e-2, graph=True, optimizer=opt, ema=train.EMA(0.9), schedule=train.PolyLR(total_steps=10))
    assert tr._twin is not None and tr._pad_mask is not None
    before = tr.fp.flat.clone()
    for _ in range(2):
        tr.step(x, t)
    tr.check_sync()
    pad = tr._pad_mask == 0
    assert int(pad.sum()) > 0
    for buf in (tr.fp.flat, tr.fp.exp_avg, tr.fp.exp_avg_sq, tr.fp.ema):
        assert float(buf[pad].abs().max()) == 0.0
    assert float((tr.fp.flat - before)[~pad].abs().max()) > 0 and float(tr.fp.ema[~pad].abs().max()) > 0


def test_search_trainer_weight_pass_takes_a_spec_object():
    """one search step with optimizer=SGD(momentum, weight decay): the kernel weights and the momentum buffer match the helper (step
    1 from the initial weights and the weight pass' fp.grad); the alphas are bit-identical to a default SearchTrainer's"""
    from nas_3d_unet_amd import nas, train
    from oracle import ref_path as orc
    from _util import fill_module
    cfg = orc.DEFAULT_CFG._replace(depth=2)
    rng = np.random.default_rng(23)
    mk = lambda: (rng.standard_normal((2, 4, 16, 16, 16)).astype(np.float32), (rng.uniform(0, 1, (2, 3, 16, 16, 16)) < 0.3).astype(np.float32))
    (xn, tn), (vxn, vtn) = mk(), mk()
    batches = [dev(a) for a in (xn, tn, vxn, vtn)]
    case = rr._sgd(momentum=0.9, weight_decay=1e-2)
    res = {}
    for tag, kw in (("adam", {}), ("sgd", dict(optimizer=train.SGD(momentum=0.9, weight_decay=1e-2)))):
        net = nas.ShellNet(cfg.in_channels, cfg.init_n_kernels, cfg.out_channels, cfg.depth, cfg.n_nodes, False, cfg.channel_change)
        fill_module(net)
        net.kernel.last_conv[0].dropout = None
        tr = train.SearchTrainer(net.cuda(), graph=False, side_wgrad=False, **kw)
        before = tr.fp.flat.double().cpu().numpy()
        tr.step(*batches)
        assert int(tr.fp.step) == 1 and int(tr.a_step) == 1
        res[tag] = (tr, before)
    tr, before = res["sgd"]
    assert torch.equal(tr.aflat, res["adam"][0].aflat) and torch.equal(tr.a_m, res["adam"][0].a_m)
    assert not torch.equal(tr.fp.flat, res["adam"][0].fp.flat) and float(tr.fp.exp_avg_sq.abs().max()) == 0.0
    grad = tr.fp.grad.double().cpu().numpy()
    want = rr.sgd_step(before, grad, np.zeros_like(before), 1, F32(1e-3), 0.9, 0.0, 1e-2)
    t64, t32 = (rr.torch_run(case, before, [grad], dt, lambda s: 1e-3)[0] for dt in (torch.float64, torch.float32))
    for i, got in enumerate((tr.fp.flat, tr.fp.exp_avg)):
        err = float(np.abs(got.double().cpu().numpy() - want[i]).max())
        assert err <= _tol(float(np.abs(t32[i] - t64[i]).max()), want[i]), (i, err)


class _Calls:
    """the libn3d entry points called while the block runs, in order"""

    def __init__(self):
        self.names = []

    def __enter__(self):
        from nas_3d_unet_amd import _lib
        self._lib, self._real = _lib, _lib.load()
        outer = self

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(outer._real, name)
                if not name.startswith("n3d_"):
                    return fn

                def counted(*a):
                    outer.names.append(name)
                    return fn(*a)
                return counted

        _lib._lib = Proxy()
        return self

    def __exit__(self, *exc):
        self._lib._lib = self._real


def test_default_trainer_issues_the_launches_it_always_did():
    """the library calls of one eager single-stream step: a trainer built with today's arguments makes none of the new ones and ONE
    optimiser call, n3d_adam_step; and the full recipe's step is that very list with the optimiser call exchanged and exactly one
    schedule call in front of it and one averaging call behind it -- the new launches sit beside the old ones, nothing else moved"""
    from nas_3d_unet_amd import train
    mk, x, t = _small_net()
    lists = {}
    for tag, kw in (("default", {}), ("recipe", dict(optimizer=train.SGD(momentum=0.99, nesterov=True), ema=train.EMA(0.9),
                                                       schedule=train.PolyLR(total_steps=10)))):
        tr = train.Trainer(mk(), graph=False, side_wgrad=False, **kw)
        tr.step(x, t)
        with _Calls() as c:
            tr.step(x, t)
        torch.cuda.synchronize()
        lists[tag] = [n for n in c.names if n != "n3d_last_error"]
    new = {"n3d_sgd_step", "n3d_sgd_step_guarded", "n3d_adamw_step", "n3d_adamw_step_guarded", "n3d_lr_schedule", "n3d_ema_step", "n3d_swap_f32"}
    d, r = lists["default"], lists["recipe"]
    assert len(d) > 20 and not new & set(d)
    assert d[-1] == "n3d_adam_step" and d.count("n3d_adam_step") == 1 and not [n for n in d if "adabound" in n or "grad_clip" in n]
    assert r == d[:-1] + ["n3d_lr_schedule", "n3d_sgd_step", "n3d_ema_step"]
