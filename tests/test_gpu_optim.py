"""GPU: the flat AdaBound / AdaBoundW update (n3d_adabound_step*), the one-launch gradient norm + clip coefficient
(n3d_grad_clip_coef), the coefficient read of the Adam kernel (n3d_adam_step_coef) and their way through Trainer / SearchTrainer
and the checkpoints, against the fp64 helper tests/_optim_ref.py (itself pinned to the reference's classes by tests/golden/optim.npz).

Tolerance of every comparison of p / exp_avg / exp_avg_sq / max_exp_avg_sq with the helper:
    max|dev - ref64| <= 4 * d32 * max|ref64| / max|fixture ref64| + 2^-23 * max|ref64|
where d32 is the fixture's max|ref32 - ref64| of the same case and array after the 24 steps: what the reference's own fp32 run
differs from its fp64 run by.  The factor 4 is there because the kernel contracts (fma) and associates differently from torch's CPU
loops.  Measured max|dev - ref64| / d32 on MI355X (n = 257, all eleven cases, 24 launches): p 0.93-1.04, exp_avg 0.66-1.09,
exp_avg_sq 0.30-1.64, max_exp_avg_sq 0.74-1.64 -- none above 2 ("AdaBound and gradient clipping").
"""
import numpy as np
import pytest
import torch

import _optim_ref as orf
import make_golden_optim as mo
from _util import dev

pytestmark = pytest.mark.gpu

SIZES = (1, 5, 257, 16421)        # 16421 = 2 * 8192 + 37: three workgroups, a ragged float4 tail
F32 = lambda x: float(np.float32(x))
_REF = {}


def _reference(name, n):
    """(inputs, fp64 trajectory of the helper) of a fixture case at size n, computed once"""
    if (name, n) not in _REF:
        p0, grads = mo.optim_inputs(n)
        _REF[name, n] = (p0, grads) + orf.run_case(mo.CASES[name], p0, grads, mo.lr_of_step, mo.LR)
    return _REF[name, n]


def _tol(g, name, a, ref):
    scale = float(np.abs(ref).max())
    fix = float(np.abs(g["%s/%s" % (name, a)]).max())
    return 4.0 * float(g["%s/d32/%s" % (name, a)]) * (scale / fix if fix > 0 else 0.0) + 2.0 ** -23 * scale


def _buf(n, offset, fill=None):
    """n floats, `offset` floats off a 16-byte boundary"""
    t = torch.zeros(n + offset, device="cuda")[offset:]
    if fill is not None:
        t.copy_(torch.from_numpy(np.asarray(fill, np.float32)))
    return t


class _Run:
    """24 launches of one case on the device: eagerly, or one captured {norm, update} pair replayed 24 times"""

    def __init__(self, name, n, offset=0, ticketed=True, graph=False):
        from nas_3d_unet_amd import kernels as K
        case = mo.CASES[name]
        p0, grads = _reference(name, n)[:2]
        self.p, self.m, self.v = _buf(n, offset, p0), _buf(n, offset), _buf(n, offset)
        self.vmax = _buf(n, offset) if case["amsbound"] else None
        self.step = K.step_counter("cuda") if ticketed else torch.zeros(1, dtype=torch.int32, device="cuda")
        gs = [_buf(n, offset, g) for g in grads]
        gbuf = _buf(n, offset)
        lr_dev = torch.full((1,), mo.LR, dtype=torch.float32, device="cuda")
        out = torch.zeros(2, device="cuda")
        scratch = K.grad_clip_scratch("cuda")
        self.norms = []

        def launch(g):
            coef = None
            if case["max_norm"] is not None:
                K.grad_clip_coef(g, case["max_norm"], scratch, out)
                coef = out[1:]
            K.adabound_step(self.p, g, self.m, self.v, self.step, mo.LR, weight_decay=case["weight_decay"], lr_dev=lr_dev, coef=coef,
                            final_lr=case["final_lr"], gamma=case["gamma"], base_lr=F32(mo.LR), max_exp_avg_sq=self.vmax,
                            decoupled=case["decoupled"])

        graph_obj = None
        if graph:
            graph_obj = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph_obj, capture_error_mode="thread_local"):
                launch(gbuf)
        for t in range(1, mo.STEPS + 1):
            if graph:
                gbuf.copy_(gs[t - 1])
                graph_obj.replay()
            else:
                launch(gs[t - 1])
            if case["max_norm"] is not None:
                self.norms.append(out[0].clone())
            if t == mo.HALVE_AFTER:
                lr_dev.fill_(mo.LR * 0.5)
        torch.cuda.synchronize()

    def arrays(self):
        return [x if x is None else x.double().cpu().numpy() for x in (self.p, self.m, self.v, self.vmax)]


@pytest.mark.parametrize("name", list(mo.CASES))
def test_adabound_kernel_matches_the_fp64_helper(golden, name):
    """every fixture case at n in {1, 5, 257, 16421}, 24 launches with lr_dev halved after 12; at n = 257 the reference is the
    fixture itself (the reference class's fp64 run).  Prints max|dev - ref64| / d32 per array (allowed: 4 + the floor)."""
    g = golden("optim")
    for n in SIZES:
        run = _Run(name, n)
        assert int(run.step) == mo.STEPS and int(run.step._base[1]) == 0
        ref = _reference(name, n)[2] if n != mo.N else tuple(g["%s/%s" % (name, a)] for a in mo.ARRAYS)
        for a, got, want in zip(mo.ARRAYS, run.arrays(), ref):
            if got is None:
                continue
            err, tol = float(np.abs(got - want).max()), _tol(g, name, a, want)
            if n == mo.N:
                print("%s %s: max|dev - ref64| / d32 = %.3f" % (name, a, err / float(g["%s/d32/%s" % (name, a)])))
            assert err <= tol, (name, n, a, err, tol)
        if mo.CASES[name]["max_norm"] is not None and n == mo.N:
            got = np.array([float(x) for x in run.norms])
            want = g["%s/norms" % name]
            assert np.all(np.abs(got - want) <= np.spacing(want.astype(np.float32)))


@pytest.mark.parametrize("name", ["b_wd1_ams0", "w_wd1_ams1_clip"])
def test_unaligned_views_unticketed_counter_and_graph_replay_give_the_same_bits(name):
    """a view one float off the 16-byte boundary takes the element-wise path, a plain int32 step word the second tiny launch, a
    captured {norm, update} pair 24 replays: all bit-identical to the aligned, ticketed, eager run, and the counters end at 24"""
    for n in (257, 16421):
        base = _Run(name, n)
        for kw in (dict(offset=1), dict(ticketed=False), dict(graph=True), dict(graph=True, offset=1, ticketed=False)):
            other = _Run(name, n, **kw)
            assert int(other.step) == mo.STEPS, kw
            for a, x, y in zip(mo.ARRAYS, (base.p, base.m, base.v, base.vmax), (other.p, other.m, other.v, other.vmax)):
                assert (x is None and y is None) or torch.equal(x, y), (name, n, kw, a)
            assert all(torch.equal(x, y) for x, y in zip(base.norms, other.norms)), kw


def test_guarded_adabound_withholds_the_update():
    """the contract of the guarded Adam launch (test_gpu_side.py): time-outs != acknowledged (or a peer's flag) -> parameters, all
    three moments and the step counter are bit-unchanged, the loss reads NaN, the host word is set; equal counters -> the ordinary
    update, bit-identical to the unguarded launch"""
    from nas_3d_unet_amd import kernels as K
    n = 10000
    g = torch.randn(n, device="cuda")
    kw = dict(weight_decay=1e-2, decoupled=True)
    mk = lambda: (torch.ones(n, device="cuda"), torch.zeros(n, device="cuda"), torch.full((n,), 0.5, device="cuda"),
                  torch.full((n,), 0.25, device="cuda"), K.step_counter("cuda"))
    words = torch.zeros(4, dtype=torch.int32, device="cuda")     # [0] time-outs, [1] acknowledged
    flag = torch.zeros(1, device="cuda")
    hw = K.HostWord()
    p0, m0, v0, x0, st0 = mk()
    K.adabound_step(p0, g, m0, v0, st0, max_exp_avg_sq=x0, **kw)                    # reference: the unguarded update
    assert not torch.equal(p0, torch.ones_like(p0)) and int(st0) == 1
    for bad_words, bad_flag in ((False, False), (True, False), (False, True)):
        p, m, v, x, st = mk()
        loss = torch.full((), 0.5, device="cuda")
        words[0], words[1] = (3 if bad_words else 2), 2
        flag[0] = 1.0 if bad_flag else 0.0
        hw.clear()
        guard = K.UpdateGuard(words.data_ptr(), words.data_ptr() + 4, flag.data_ptr(), loss.data_ptr(), hw.ptr)
        K.adabound_step(p, g, m, v, st, max_exp_avg_sq=x, guard=guard, **kw)
        torch.cuda.synchronize()
        if bad_words or bad_flag:
            assert torch.equal(p, torch.ones_like(p)) and float(m.abs().max()) == 0.0
            assert torch.equal(v, torch.full_like(v, 0.5)) and torch.equal(x, torch.full_like(x, 0.25))
            assert int(st) == 0 and int(st._base[1]) == 0
            assert torch.isnan(loss) and hw.value == 1
        else:
            assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0) and torch.equal(x, x0) and int(st) == 1
            assert float(loss) == 0.5 and hw.value == 0


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_grad_norm_and_clip_coefficient(grad_scale):
    """out[0] within one fp32 ulp of the fp64 numpy norm (the products are exact in fp64, the sum carries ~n * 2^-53); out[1]
    exactly min(1, max_norm / (float64(out[0]) + 1e-6)) rounded to fp32, on both sides of 1; two launches and a graph replay give
    equal bits; an all-zero gradient gives norm 0 and coefficient 1"""
    from nas_3d_unet_amd import kernels as K
    for n in SIZES + (256 * 8192 + 4099,):       # (the last: more elements than the fixed grid's 256 workgroups take in one round)
        rng = np.random.default_rng(900 + n)
        gn = (rng.standard_normal(n) * np.exp(rng.uniform(-6.0, 0.0, n))).astype(np.float32)
        norm64 = float(np.sqrt(np.sum((gn.astype(np.float64) * grad_scale) ** 2)))
        for offset in (0, 1):
            g = _buf(n, offset, gn)
            scratch = K.grad_clip_scratch("cuda")
            for max_norm in (0.5 * norm64, 2.0 * norm64 + 1.0):
                out, out2, out3 = (torch.full((2,), -1.0, device="cuda") for _ in range(3))
                K.grad_clip_coef(g, max_norm, scratch, out, grad_scale)
                K.grad_clip_coef(g, max_norm, scratch, out2, grad_scale)
                graph = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    K.grad_clip_coef(g, max_norm, scratch, out3, grad_scale)
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, out2), (n, offset)
                first = out3.clone()
                out3.fill_(-1.0)
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, first) and torch.equal(out, out3), (n, offset)
                got = out.cpu().numpy()
                assert abs(float(got[0]) - norm64) <= float(np.spacing(np.float32(norm64))), (n, offset, got[0], norm64)
                want = np.float32(min(1.0, max_norm / (float(got[0]) + 1e-6)))
                assert got[1] == want and (got[1] < 1.0) == (max_norm < norm64), (n, offset, got[1], want)
                assert int(scratch.view(torch.int32)[0]) == 0          # the ticket word is ready for the next launch
    z = torch.zeros(257, device="cuda")
    out = torch.full((2,), -1.0, device="cuda")
    K.grad_clip_coef(z, 0.05, K.grad_clip_scratch("cuda"), out, grad_scale)
    assert out.tolist() == [0.0, 1.0]
    bad = z.clone()
    bad[5] = float("nan")
    K.grad_clip_coef(bad, 0.05, K.grad_clip_scratch("cuda"), out, grad_scale)
    assert torch.isnan(out).all()           # (error_if_nonfinite=False: the NaN reaches the coefficient, as in torch)


def test_adam_coefficient_path():
    """coef == NULL: n3d_adam_step_coef is K.adam_step bit for bit (three steps); with a coefficient it equals K.adam_step on a
    pre-scaled gradient within 2 ulp"""
    from nas_3d_unet_amd import kernels as K
    for n in (5, 16421):
        rng = np.random.default_rng(n)
        gs = [dev(rng.standard_normal(n).astype(np.float32)) for _ in range(3)]
        p0 = dev(rng.standard_normal(n).astype(np.float32))
        coef = torch.full((1,), 0.3125, device="cuda")          # (a power-of-two multiple: the pre-scaled gradient is exact)
        coef2 = torch.full((1,), 0.3, device="cuda")
        res = {}
        for tag in ("plain", "null", "coef", "prescaled", "coef2", "prescaled2"):
            p, m, v, st = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), K.step_counter("cuda")
            for g in gs:
                if tag == "plain":
                    K.adam_step(p, g, m, v, st, weight_decay=1e-2, grad_scale=0.5)
                elif tag == "null":
                    K.adam_step_coef(p, g, m, v, st, weight_decay=1e-2, grad_scale=0.5)
                elif tag in ("coef", "coef2"):
                    K.adam_step_coef(p, g, m, v, st, weight_decay=1e-2, coef=coef if tag == "coef" else coef2)
                else:
                    K.adam_step(p, g * (coef if tag == "prescaled" else coef2), m, v, st, weight_decay=1e-2)
            assert int(st) == 3
            res[tag] = (p, m, v)
        for x, y in zip(res["plain"], res["null"]):
            assert torch.equal(x, y)
        for a, b in (("coef", "prescaled"), ("coef2", "prescaled2")):
            for x, y in zip(res[a], res[b]):
                x, y = x.double().cpu().numpy(), y.double().cpu().numpy()
                assert np.all(np.abs(x - y) <= 2 * np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)), (n, a)


# ------------------------------------------------------------------------------------------------ trainers
CLIP_CASE = "w_wd1_ams1_clip"
OPT = dict(optimizer="adaboundw", optim_args=dict(amsbound=True, weight_decay=1e-2), grad_clip=1e-2)


def _small_net():
    import golden_common as gc
    from test_gpu_nets import build_net
    key, kind, gname, depth, size, batch, adam = [c for c in gc.net_cases() if c[6] and c[1] == "searched"][0]
    xn, tn = gc.net_batch(key, batch, size)
    return (lambda: build_net(kind, gname, depth)[0]), dev(xn), dev(tn)


def _snap(tr, loss):
    fp = tr.fp
    return dict(loss=loss.clone(), norm=tr.grad_norm.clone(), **{k: getattr(fp, k).clone() for k in ("flat", "grad", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")})


@pytest.fixture(scope="module")
def trajectories(tmp_path_factory):
    """four AdaBoundW + amsbound + clip steps of the smallest net, lr halved after two, once from the captured graph and once
    eagerly (single-stream schedule on both sides, as test_lr_schedule_follows_through_graph_replay); the graph run writes a
    checkpoint after step two"""
    from nas_3d_unet_amd import checkpoint as ck
    from nas_3d_unet_amd.train import Trainer
    mk, x, t = _small_net()
    path = tmp_path_factory.mktemp("optim") / "last.pth"
    out = {}
    for graph in (True, False):
        tr = Trainer(mk(), graph=graph, side_wgrad=False, **OPT)
        start = {k: getattr(tr.fp, k).clone() for k in ("flat", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")}
        steps = []
        for k in range(4):
            if k == 2:
                if graph:
                    torch.save(ck.train_state_dicts(tr, 1, {}, 0.5), path)
                tr.set_lr(tr.lr / 2)
            steps.append(_snap(tr, tr.step(x, t)))
        assert int(tr.fp.step) == 4
        out[graph] = (start, steps, tr.optim.base_lr)
    return out, path, (mk, x, t)


def test_trainer_steps_match_the_helper(golden, trajectories):
    """after each step fp.flat (and every moment) equals the helper applied to the previous state, the step's fp.grad and the
    coefficient tr.grad_norm gives; the norm is the fp64 norm of fp.grad within one fp32 ulp and the clip engages"""
    g = golden("optim")
    start, steps, base_lr = trajectories[0][True]
    prev = {k: v.double().cpu().numpy() for k, v in start.items()}
    lr = 1e-3
    for k, s in enumerate(steps):
        if k == 2:
            lr = lr / 2
        grad = s["grad"].double().cpu().numpy()
        norm = float(s["norm"])
        norm64 = float(np.sqrt(np.sum(grad * grad)))
        assert abs(norm - norm64) <= float(np.spacing(np.float32(norm64))) and norm > OPT["grad_clip"]
        coef = F32(min(1.0, OPT["grad_clip"] / (norm + 1e-6)))
        want = orf.adabound_step(prev["flat"], grad, prev["exp_avg"], prev["exp_avg_sq"], prev["max_exp_avg_sq"], k + 1, F32(lr), base_lr,
                                 weight_decay=1e-2, amsbound=True, decoupled=True, coef=coef)
        cur = {key: s[key].double().cpu().numpy() for key in prev}
        for a, key, w in zip(mo.ARRAYS, ("flat", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"), want):
            err, tol = float(np.abs(cur[key] - w).max()), _tol(g, CLIP_CASE, a, w)
            assert err <= tol, (k, key, err, tol)
        assert float(np.abs(cur["flat"] - prev["flat"]).max()) > 0
        prev = cur


def test_trainer_graph_and_eager_give_the_same_bits(trajectories):
    (_, a, _), (_, b, _) = trajectories[0][True], trajectories[0][False]
    for k, (sa, sb) in enumerate(zip(a, b)):
        for key in sa:
            assert torch.equal(sa[key], sb[key]), (k, key)


def test_trainer_resumes_bit_identically_and_adam_refuses_the_file(trajectories):
    """save after step two, load into a fresh trainer, halve the rate as the uninterrupted run did: step three has the same bits.
    The same file loaded into an optimizer="adam" trainer raises"""
    from nas_3d_unet_amd import checkpoint as ck
    from nas_3d_unet_amd.train import Trainer
    out, path, (mk, x, t) = trajectories
    sd = torch.load(path, weights_only=False)
    assert sd["optimizer"] == "adaboundw" and sd["optim"]["state"][0]["step"] == 2
    tr = Trainer(mk(), graph=True, side_wgrad=False, **OPT)
    ck.load_train_state_dicts(tr, sd)
    assert int(tr.fp.step) == 2 and tr.lr == 1e-3
    tr.set_lr(tr.lr / 2)
    got = _snap(tr, tr.step(x, t))
    want = out[True][1][2]
    for key in want:
        assert torch.equal(got[key], want[key]), key
    with pytest.raises(ValueError, match="adaboundw"):
        ck.load_train_state_dicts(Trainer(mk(), graph=False, side_wgrad=False), sd)


def test_padded_twin_entries_stay_zero_under_adaboundw_with_weight_decay():
    """init_n_kernels = 6: the net trains as its zero-padded twin; with weight_decay = 1e-2, amsbound and clipping the padded
    entries of the weights and of all three moments are still exactly 0 after two steps, while the real ones moved"""
    from nas_3d_unet_amd import searched
    from nas_3d_unet_amd.train import Trainer
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
    tr = Trainer(net.cuda(), graph=True, **OPT)
    assert tr._twin is not None and tr._pad_mask is not None
    before = tr.fp.flat.clone()
    for _ in range(2):
        tr.step(x, t)
    tr.check_sync()
    pad = tr._pad_mask == 0
    assert int(pad.sum()) > 0 and float(tr.grad_norm) > 0
    for buf in (tr.fp.flat, tr.fp.exp_avg, tr.fp.exp_avg_sq, tr.fp.max_exp_avg_sq):
        assert float(buf[pad].abs().max()) == 0.0
    assert float((tr.fp.flat - before)[~pad].abs().max()) > 1e-3


def test_search_trainer_weight_pass_on_adabound_with_clip(golden):
    """one search step with optimizer="adabound", grad_clip=5: the kernel weights match the helper (step 1 from the initial
    weights, the weight pass' fp.grad and grad_norm); the alphas are bit-identical to a default SearchTrainer's"""
    from nas_3d_unet_amd import nas
    from nas_3d_unet_amd.train import SearchTrainer
    from oracle import ref_path as orc
    from _util import fill_module
    g = golden("optim")
    cfg = orc.DEFAULT_CFG._replace(depth=2)
    rng = np.random.default_rng(23)
    mk = lambda: (rng.standard_normal((2, 4, 16, 16, 16)).astype(np.float32), (rng.uniform(0, 1, (2, 3, 16, 16, 16)) < 0.3).astype(np.float32))
    (xn, tn), (vxn, vtn) = mk(), mk()
    batches = [dev(a) for a in (xn, tn, vxn, vtn)]
    res = {}
    for tag, kw in (("adam", {}), ("adabound", dict(optimizer="adabound", grad_clip=5))):
        net = nas.ShellNet(cfg.in_channels, cfg.init_n_kernels, cfg.out_channels, cfg.depth, cfg.n_nodes, False, cfg.channel_change)
        fill_module(net)
        net.kernel.last_conv[0].dropout = None
        tr = SearchTrainer(net.cuda(), graph=False, side_wgrad=False, **kw)
        before = tr.fp.flat.double().cpu().numpy()
        tr.step(*batches)
        assert int(tr.fp.step) == 1 and int(tr.a_step) == 1
        res[tag] = (tr, before)
    tr, before = res["adabound"]
    assert torch.equal(tr.aflat, res["adam"][0].aflat) and torch.equal(tr.a_m, res["adam"][0].a_m)
    assert not torch.equal(tr.fp.flat, res["adam"][0].fp.flat) and tr.fp.max_exp_avg_sq is None
    grad = tr.fp.grad.double().cpu().numpy()
    norm = float(tr.grad_norm)
    assert abs(norm - float(np.sqrt(np.sum(grad * grad)))) <= float(np.spacing(np.float32(norm)))
    coef = F32(min(1.0, 5.0 / (norm + 1e-6)))
    zero = np.zeros_like(before)
    want = orf.adabound_step(before, grad, zero, zero, zero, 1, F32(1e-3), F32(1e-3), coef=coef)
    for a, got, w in zip(mo.ARRAYS[:3], (tr.fp.flat, tr.fp.exp_avg, tr.fp.exp_avg_sq), want):
        err, tol = float(np.abs(got.double().cpu().numpy() - w).max()), _tol(g, "b_wd0_ams0", a, w)
        assert err <= tol, (a, err, tol)
