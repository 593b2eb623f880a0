"""GPU: loss.TverskyBCELoss -- the Tversky / focal / cross-entropy loss formed inside the fused head's passes (n3d_head_loss_fwd /
_bwd / _eval), its form on probabilities (n3d_tversky_fwd / _bwd) and the trainers that train with it -- against the fp64 reference
of tests/_loss_ref.py.  Shapes sit where the kernels branch: a partial 1024-voxel chunk, 1.5 chunks, 32 partial rows (the
one-wave-per-pair finalize), 256 rows (the flat finalize walk), node-planar input, byte targets on quad-eligible and other shapes."""
import functools

import numpy as np
import pytest
import torch

import _loss_ref as lr
from _util import assert_close, dev, fill_module
from oracle import ref_path as orc

pytestmark = pytest.mark.gpu

BCE_SPEC = lr.Spec(0.3, 0.7, 0.75, 0.5)     # the trainers' tests: TverskyBCELoss(0.3, 0.7, 0.75, 0.5)


def _module(spec):
    from nas_3d_unet_amd.loss import TverskyBCELoss
    return TverskyBCELoss(*spec)


@functools.lru_cache(maxsize=None)
def _data(ci, co, shape, batch, use_gate):
    """head operands as numpy arrays; one class of one sample has an empty target"""
    rng = np.random.default_rng(ci * 100 + co * 10 + batch)
    xn = rng.standard_normal((batch, ci) + shape).astype(np.float32)
    wn = (rng.standard_normal((co, ci, 1, 1, 1)) * 0.4).astype(np.float32)
    bn = rng.standard_normal(co).astype(np.float32) * 0.2
    tn = (rng.uniform(0, 1, (batch, co) + shape) < 0.3).astype(np.float32)
    tn[0, co - 1] = 0
    gn = ((rng.uniform(0, 1, (batch, ci)) >= 0.5) / 0.5).astype(np.float32) if use_gate else None
    return xn, wn, bn, tn, gn


@functools.lru_cache(maxsize=None)
def _reference(ci, co, shape, batch, use_gate, spec):
    xn, wn, bn, tn, gn = _data(ci, co, shape, batch, use_gate)
    T = torch.from_numpy
    return lr.head_reference(T(xn), T(wn), T(bn), T(gn) if use_gate else None, T(tn), spec)


def _loss_ok(got, ref):
    got, ref = float(got), float(ref)
    assert abs(got - ref) <= 1e-6 * max(1.0, abs(ref)), (got, ref)


def _sums_ok(sums, c, spec):
    S = 4 if spec.bce_weight > 0 else 3
    assert sums.shape[-1] == S
    # (fp32 voxel terms summed in fp64 against fp64 ones: the bound of the loss, relative to the largest sum)
    assert_close(sums, c.sums[..., :S], 2e-6, "sums")


HEAD_CASES = [(8, 3, (5, 3, 7), 2, True), (12, 3, (8, 12, 16), 2, True), (12, 3, (32, 32, 32), 2, False), (4, 3, (64, 64, 64), 1, False),
              (24, 2, (6, 6, 6), 1, False), (32, 4, (4, 8, 8), 5, False)]


@pytest.mark.parametrize("spec", lr.SPECS)
@pytest.mark.parametrize("ci,co,shape,batch,use_gate", HEAD_CASES)
def test_head_loss_matches_the_reference(ci, co, shape, batch, use_gate, spec):
    from nas_3d_unet_amd import kernels as K
    xn, wn, bn, tn, gn = _data(ci, co, shape, batch, use_gate)
    xv = K.as_view(dev(xn))
    w, b, t = dev(wn), dev(bn), dev(tn)
    gate = dev(gn) if use_gate else None
    if co != 3 and spec.bce_weight > 0:
        with pytest.raises(K.N3DError, match="Co = 3"):
            K.head_loss_fwd(xv, w, b, gate, t, spec)
        return
    c, dxr, dwr, dbr = _reference(ci, co, shape, batch, use_gate, spec)
    p, _, sums, coef, loss = K.head_loss_fwd(xv, w, b, gate, t, spec)
    print("loss %.9g ref %.9g" % (float(loss), float(c.loss)))
    _loss_ok(loss, c.loss)
    _sums_ok(sums, c, spec)
    assert coef.numel() == 2 * batch * co + 1
    dx = K.as_view(K.empty_ndhwc(batch, ci, *shape, xv.t.device))
    dw, db = torch.empty_like(w), torch.empty_like(b)
    K.head_loss_bwd(xv, w, b, gate, dx, dw, db, t, coef)
    assert_close(dx.t, dxr, 2e-5, "dx")
    assert_close(dw, dwr, 2e-5, "dw")
    assert_close(db, dbr, 2e-5, "db")
    K.head_loss_bwd(xv, w, b, gate, dx, None, None, t, coef, accumulate=True)
    assert_close(dx.t, 2 * dxr, 2e-5, "dx accumulate")


@pytest.mark.parametrize("spec", lr.SPECS)
def test_head_loss_on_node_planar_input(spec):
    """3 x 4 channels as three dense node tensors, with a node-planar dx (include/n3d.h, n3d_head.node_c)"""
    from nas_3d_unet_amd import kernels as K
    cn, nn, shape, batch = 4, 3, (8, 8, 16), 2
    xn, wn, bn, tn, _ = _data(cn * nn, 3, shape, batch, False)
    c, dxr, dwr, dbr = _reference(cn * nn, 3, shape, batch, False, spec)
    d = torch.device("cuda")
    pl = K.empty_planar(nn, batch, cn, *shape, d)
    for k in range(nn):
        pl.nodes[k].t.copy_(dev(xn[:, k * cn:(k + 1) * cn]))
    w, b, t = dev(wn), dev(bn), dev(tn)
    _, _, sums, coef, loss = K.head_loss_fwd(pl, w, b, None, t, spec)
    _loss_ok(loss, c.loss)
    _sums_ok(sums, c, spec)
    dx = K.empty_planar(nn, batch, cn, *shape, d)
    dw, db = torch.empty_like(w), torch.empty_like(b)
    K.head_loss_bwd(pl, w, b, None, dx, dw, db, t, coef)
    assert_close(torch.cat([n.t for n in dx.nodes], dim=1), dxr, 2e-5, "dx")
    assert_close(dw, dwr, 2e-5, "dw")
    assert_close(db, dbr, 2e-5, "db")
    K.head_loss_bwd(pl, w, b, None, dx, None, None, t, coef, accumulate=True)
    assert_close(torch.cat([n.t for n in dx.nodes], dim=1), 2 * dxr, 2e-5, "dx accumulate")


def test_head_loss_bf16_storage():
    """bf16 storage of the head input / its gradient: method and bounds of test_gpu_head.test_head_bf16_storage -- the reference on the
    bf16-rounded input; dx compared after rounding to bf16 (one ulp = 2^-8 relative)"""
    from nas_3d_unet_amd import kernels as K
    spec = lr.SPECS[3]
    rng = np.random.default_rng(5)
    batch, ci, co, shape = 2, 12, 3, (8, 16, 16)
    xb = torch.from_numpy(rng.standard_normal((batch, ci) + shape).astype(np.float32)).bfloat16()
    wn = (rng.standard_normal((co, ci, 1, 1, 1)) * 0.4).astype(np.float32)
    bn = rng.standard_normal(co).astype(np.float32) * 0.2
    tn = (rng.uniform(0, 1, (batch, co) + shape) < 0.3).astype(np.float32)
    c, dxr, dwr, dbr = lr.head_reference(xb.float(), torch.from_numpy(wn), torch.from_numpy(bn), None, torch.from_numpy(tn), spec)
    xd = K.empty_ndhwc(batch, ci, *shape, torch.device("cuda"), torch.bfloat16)
    xd.copy_(xb.cuda())
    xv = K.as_view(xd, bf16_ok=True)
    w, b, t = dev(wn), dev(bn), dev(tn)
    _, _, sums, coef, loss = K.head_loss_fwd(xv, w, b, None, t, spec)
    _loss_ok(loss, c.loss)
    dx = K.as_view(K.empty_ndhwc(batch, ci, *shape, xv.t.device, torch.bfloat16), bf16_ok=True)
    dw, db = torch.empty_like(w), torch.empty_like(b)
    K.head_loss_bwd(xv, w, b, None, dx, dw, db, t, coef)
    assert_close(dw, dwr, 2e-5, "dw")
    assert_close(db, dbr, 2e-5, "db")
    dxr = dxr.float()
    assert_close(dx.t.float(), dxr, 2.0 ** -8, "dx (bf16)")
    assert torch.equal(dx.t.cpu(), dxr.bfloat16()) or float((dx.t.float().cpu() - dxr.bfloat16().float()).abs().max()) <= float(dxr.abs().max()) * 2.0 ** -7


def test_head_loss_saturated_logits_stay_finite():
    """zero weights and biases (-200, +200, 0), empty targets in classes 0 and 1, gamma = 0.75: class 0 has p == 0 exactly, u == 0 and a
    zero gradient (not the infinite derivative of pow); class 1 has a per-voxel cross-entropy of 200 and d z = kb"""
    from nas_3d_unet_amd import kernels as K
    spec = BCE_SPEC
    ci, shape = 8, (8, 8, 16)
    N = int(np.prod(shape))
    rng = np.random.default_rng(17)
    xn = rng.standard_normal((1, ci) + shape).astype(np.float32)
    wn = np.zeros((3, ci, 1, 1, 1), np.float32)
    bn = np.array([-200.0, 200.0, 0.0], np.float32)
    tn = (rng.uniform(0, 1, (1, 3) + shape) < 0.3).astype(np.float32)
    tn[0, :2] = 0
    T = torch.from_numpy
    c, dxr, dwr, dbr = lr.head_reference(T(xn), T(wn), T(bn), None, T(tn), spec)
    xv = K.as_view(dev(xn))
    w, b, t = dev(wn), dev(bn), dev(tn)
    p, _, sums, coef, loss = K.head_loss_fwd(xv, w, b, None, t, spec)
    assert torch.isfinite(loss) and torch.isfinite(sums).all() and torch.isfinite(coef).all()
    _loss_ok(loss, c.loss)
    _sums_ok(sums, c, spec)
    assert float(p[0, 0].abs().max()) == 0.0 and float(sums[0, 0, :3].abs().sum()) == 0.0
    assert float(sums[0, 1, 3]) == 200.0 * N
    cf = coef.cpu()
    assert float(cf[0]) == 0.0 and float(cf[1]) == 0.0          # class 0: u == 0, zero coefficients
    assert abs(float(cf[6]) - c.kb) <= 1e-6 * c.kb
    dx = K.as_view(K.empty_ndhwc(1, ci, *shape, xv.t.device))
    dw, db = torch.empty_like(w), torch.empty_like(b)
    K.head_loss_bwd(xv, w, b, None, dx, dw, db, t, coef)
    assert torch.isfinite(dx.t).all() and torch.isfinite(dw).all() and torch.isfinite(db).all()
    assert float(dx.t.abs().max()) == 0.0                        # zero weights
    assert float(db[0]) == 0.0 and float(dw[0].abs().max()) == 0.0
    assert abs(float(db[1]) - N * c.kb) <= 2e-5 * N * c.kb       # d z = kb at every voxel of class 1
    assert_close(dw, dwr, 2e-5, "dw")
    assert_close(db, dbr, 2e-5, "db")


@pytest.mark.parametrize("spec", [lr.SPECS[2], lr.SPECS[3]])
@pytest.mark.parametrize("shape", [(8, 8, 16), (5, 3, 7)])
def test_head_loss_byte_targets_are_bit_identical_to_float_targets(shape, spec):
    """quad-eligible (whole 1024-voxel chunks: a lane fetches four voxels' bytes) and not"""
    from nas_3d_unet_amd import kernels as K
    ci, batch = 12, 2
    xn, wn, bn, tn, gn = _data(ci, 3, shape, batch, True)
    xv = K.as_view(dev(xn))
    w, b, gate = dev(wn), dev(bn), dev(gn)
    res = {}
    for name, t in (("float", dev(tn)), ("bytes", dev(tn.astype(np.uint8)))):
        _, _, sums, coef, loss = K.head_loss_fwd(xv, w, b, gate, t, spec)
        dx = K.as_view(K.empty_ndhwc(batch, ci, *shape, xv.t.device))
        dw, db = torch.empty_like(w), torch.empty_like(b)
        K.head_loss_bwd(xv, w, b, gate, dx, dw, db, t, coef)
        res[name] = [v.clone() for v in (loss, sums, coef, dx.t, dw, db)]
    for a, c, what in zip(res["float"], res["bytes"], ("loss", "sums", "coef", "dx", "dw", "db")):
        assert torch.equal(a, c), what


def test_tversky_half_half_equals_the_dice_entry_points():
    """TverskyBCELoss(0.5, 0.5, 1, 0, smooth=5e-7) through the new entry points against n3d_head_fwd / n3d_head_bwd at smooth=1e-6"""
    from nas_3d_unet_amd import kernels as K
    ci, shape, batch = 12, (32, 32, 32), 2
    xn, wn, bn, tn, _ = _data(ci, 3, shape, batch, False)
    xv = K.as_view(dev(xn))
    w, b, t = dev(wn), dev(bn), dev(tn)
    out = []
    for dice in (True, False):
        dx = K.as_view(K.empty_ndhwc(batch, ci, *shape, xv.t.device))
        dw, db = torch.empty_like(w), torch.empty_like(b)
        if dice:
            _, _, sums, loss = K.head_fwd(xv, w, b, None, t, 1e-6)
            K.head_bwd(xv, w, b, None, dx, dw, db, t=t, sums=sums, smooth=1e-6)
        else:
            _, _, sums, coef, loss = K.head_loss_fwd(xv, w, b, None, t, lr.Spec(0.5, 0.5, 1.0, 0.0, 5e-7))
            K.head_loss_bwd(xv, w, b, None, dx, dw, db, t, coef)
        out.append((float(loss), sums.clone(), dx.t.clone(), dw, db))
    assert abs(out[0][0] - out[1][0]) <= 1e-6
    assert torch.equal(out[0][1], out[1][1])
    for k, what in ((2, "dx"), (3, "dw"), (4, "db")):
        assert_close(out[1][k], out[0][k], 2e-5, what)


def _head_module(ci):
    from nas_3d_unet_amd import prim_ops
    head = torch.nn.Sequential(prim_ops.ConvOps(ci, 3, kernel_size=1, dropout_rate=0.1, ops_order="weight"), torch.nn.Sigmoid())
    return fill_module(head, "last_conv.").cuda().eval()


@pytest.mark.parametrize("spec", [lr.SPECS[2], lr.SPECS[3]])
@pytest.mark.parametrize("ci,shape,batch", [(12, (8, 12, 16), 2), (4, (64, 64, 64), 1)])
def test_run_eval_with_a_loss(ci, shape, batch, spec):
    """the evaluation form returns run_loss's eval-mode loss bit for bit, the region counts of the Dice evaluation, and accumulates the
    configured loss in acc[0]"""
    from nas_3d_unet_amd import head as H, kernels as K
    head = _head_module(ci)
    fn = _module(spec)
    rng = np.random.default_rng(ci)
    batches = []
    for _ in range(2):
        x = K.empty_ndhwc(batch, ci, *shape, torch.device("cuda")).copy_(dev(rng.standard_normal((batch, ci) + shape).astype(np.float32)))
        batches.append((x, dev((rng.uniform(0, 1, (batch, 3) + shape) < 0.3).astype(np.float32))))
    acc, acc_dice = K.eval_acc(3, x.device), K.eval_acc(3, x.device)
    losses = []
    with torch.no_grad():
        for x, t in batches:
            l = H.run_eval(head, x, t, acc, loss=fn).clone()
            assert torch.equal(l, H.run_loss(head, x, t, loss=fn)[0])
            H.run_eval(head, x, t, acc_dice)
            losses.append(float(l))
    torch.cuda.synchronize()
    assert torch.equal(acc[4:], acc_dice[4:]) and torch.equal(acc[1:3], acc_dice[1:3])
    assert float(acc[0]) == losses[0] + losses[1]
    op = head[0]
    c = lr.head_reference(batches[1][0].cpu(), op.conv.weight.detach().cpu(), op.conv.bias.detach().cpu(), None, batches[1][1].cpu(), spec)[0]
    _loss_ok(losses[1], c.loss)


@pytest.mark.parametrize("shape", [(2, 3, 5, 3, 7), (2, 3, 32, 32, 32)])
def test_module_on_probabilities(shape):
    from nas_3d_unet_amd._lib import N3DError
    spec = lr.Spec(0.3, 0.7, 0.75)
    rng = np.random.default_rng(shape[-1])
    pn = rng.uniform(0.01, 0.99, shape).astype(np.float32)
    tn = (rng.uniform(0, 1, shape) < 0.3).astype(np.float32)
    tn[1, 0] = 0
    lref, dpr = lr.closed_form_probs(torch.from_numpy(pn), torch.from_numpy(tn), spec)
    p, t = dev(pn, True), dev(tn)
    l = _module(spec)(p, t)
    l.backward()
    _loss_ok(l.detach(), lref)
    assert_close(p.grad, dpr, 2e-5, "dp")
    # NDHWC-strided probabilities (what the op-by-op head emits)
    p2 = dev(pn).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    l2 = _module(spec)(p2, t)
    l2.backward()
    _loss_ok(l2.detach(), lref)
    assert_close(p2.grad, dpr, 2e-5, "dp (NDHWC)")
    with pytest.raises(N3DError, match="logits"):
        _module(spec._replace(bce_weight=0.5))(dev(pn), t)


# ---- trainers ------------------------------------------------------------------------------------------------------------------
def _trainer_cfg(init):
    from test_gpu_nets import _genotype_for
    cfg = orc.NetCfg(4, init, 3, 2, 3, True)
    return cfg, _genotype_for(cfg.n_nodes)


@functools.lru_cache(maxsize=None)
def _trainer_reference(init):
    """three Adam steps of the fp64 oracle with the loss of _loss_ref, then the eval-mode losses of two batches"""
    cfg, gene = _trainer_cfg(init)
    rng = np.random.default_rng(23)
    mk = lambda: (rng.standard_normal((2, 4, 16, 16, 32)).astype(np.float32), (rng.uniform(0, 1, (2, 3, 16, 16, 32)) < 0.3).astype(np.float32))
    (xn, tn), (x2, t2) = mk(), mk()
    D = lambda a: torch.from_numpy(a).double()
    P = orc.make_params(orc.searched_param_specs(cfg, gene), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam(list(P.values()))
    fwd = lambda x, t: lr.torch_loss(orc.searched_forward(P, D(x), gene, cfg, return_logits=True)[1], D(t), BCE_SPEC)
    ref = []
    for _ in range(3):
        opt.zero_grad()
        l = fwd(xn, tn)
        l.backward(); opt.step()
        ref.append(float(l.detach()))
    with torch.no_grad():
        ev = [float(fwd(xn, tn)), float(fwd(x2, t2))]
    return (xn, tn, x2, t2), ref, {n: float(q.detach().norm()) for n, q in P.items()}, ev


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("init", [4, 6])
def test_trainer_with_tversky_bce_matches_torch_adam(init, graph):
    """pattern of test_gpu_train.test_trainer_on_a_net_with_odd_channel_counts_matches_torch_adam: init_n_kernels = 4 runs the direct
    pipeline, 6 the zero-padded twin"""
    from nas_3d_unet_amd import searched
    from nas_3d_unet_amd.train import Trainer
    cfg, gene = _trainer_cfg(init)
    (xn, tn, x2, t2), ref, norms, ev = _trainer_reference(init)
    net = searched.SearchedNet(cfg.in_channels, cfg.init_n_kernels, cfg.out_channels, cfg.depth, cfg.n_nodes, cfg.channel_change,
                               searched.Genotype(list(gene.down), list(gene.up)))
    fill_module(net)
    net.last_conv[0].dropout = None
    net = net.cuda()
    tr = Trainer(net, graph=graph, loss=_module(BCE_SPEC))
    assert (tr._twin is not None) == (init == 6) and tr._direct_ok()
    losses = [float(tr.step(dev(xn), dev(tn))) for _ in range(3)]
    print("losses", losses, "ref", ref)
    np.testing.assert_allclose(losses, ref, rtol=0, atol=2e-4)
    tr.check_sync()
    for n, q in net.named_parameters():
        assert abs(float(q.detach().double().norm()) - norms[n]) <= 5e-4 * norms[n] + 3e-3, n
    tr.evaluate(dev(xn), dev(tn))
    tr.evaluate(dev(x2), dev(t2))
    res = tr.eval_result()
    print("eval", res.loss, "ref", ev)
    assert res.n_batches == 2 and abs(res.loss - (ev[0] + ev[1]) / 2) <= 2e-4


@functools.lru_cache(maxsize=None)
def _search_reference():
    cfg = orc.DEFAULT_CFG._replace(depth=2)
    rng = np.random.default_rng(11)
    mk = lambda: (rng.standard_normal((2, 4, 16, 16, 16)).astype(np.float32), (rng.uniform(0, 1, (2, 3, 16, 16, 16)) < 0.3).astype(np.float32))
    (xn, tn), (vxn, vtn) = mk(), mk()
    D = lambda a: torch.from_numpy(a).double()
    P = orc.make_params(orc.supernet_param_specs(cfg), dtype=torch.float64, requires_grad=True)
    alphas = [P[n] for n in ("alpha2_down", "alpha2_up", "alpha1_down", "alpha1_up")]
    kern = [v for n, v in P.items() if n.startswith("kernel.")]
    oa, ok = torch.optim.Adam(alphas), torch.optim.Adam(kern)
    fwd = lambda x, t: lr.torch_loss(orc.supernet_forward(P, D(x), cfg, return_logits=True)[1], D(t), BCE_SPEC)
    ref = []
    for _ in range(2):
        oa.zero_grad()
        la = fwd(vxn, vtn)
        la.backward(); oa.step()
        ok.zero_grad()
        lw = fwd(xn, tn)
        lw.backward(); ok.step()
        ref.append((float(la.detach()), float(lw.detach())))
    return cfg, (xn, tn, vxn, vtn), ref, {n: P[n].detach().numpy() for n in ("alpha2_down", "alpha2_up", "alpha1_down", "alpha1_up")}


@pytest.mark.parametrize("graph", [False, True])
def test_search_trainer_with_tversky_bce_matches_oracle(graph):
    """the smallest configuration of test_gpu_search.test_search_step_matches_oracle, its tolerances; the loss applies to both passes"""
    from nas_3d_unet_amd import nas
    from nas_3d_unet_amd.train import SearchTrainer
    cfg, arrays, ref, alphas = _search_reference()
    net = nas.ShellNet(cfg.in_channels, cfg.init_n_kernels, cfg.out_channels, cfg.depth, cfg.n_nodes, False, cfg.channel_change)
    fill_module(net)
    net.kernel.last_conv[0].dropout = None
    net = net.cuda()
    tr = SearchTrainer(net, graph=graph, loss=_module(BCE_SPEC))
    x, t, vx, vt = (torch.from_numpy(a).cuda() for a in arrays)
    got = []
    for _ in range(2):
        la, lw = tr.step(x, t, vx, vt)
        got.append((float(la), float(lw)))
    print("got", got, "ref", ref)
    np.testing.assert_allclose(np.array(got), np.array(ref), rtol=0, atol=3e-4)
    for n, a in alphas.items():
        assert np.abs(getattr(net, n).detach().cpu().numpy() - a).max() <= 2.5e-3, n


def test_the_default_loss_is_unchanged():
    """Trainer(net) and Trainer(net, loss=WeightedDiceLoss()), captured: the same launches, so the losses and the flat parameter buffer are
    bit-identical.  (Both on the single-stream schedule: a captured trainer otherwise TIMES its two schedules and keeps the faster, and
    the side-stream schedule differs from the plain one by an fp32 rounding -- test_gpu_train.test_lr_schedule_follows_through_graph_replay.)"""
    from nas_3d_unet_amd.loss import WeightedDiceLoss
    from nas_3d_unet_amd.train import Trainer
    from test_gpu_nets import build_net
    rng = np.random.default_rng(31)
    x = dev(rng.standard_normal((2, 4, 32, 32, 32)).astype(np.float32))
    t = dev((rng.uniform(0, 1, (2, 3, 32, 32, 32)) < 0.3).astype(np.float32))
    out = []
    for kw in ({}, {"loss": WeightedDiceLoss()}):
        net, _ = build_net("searched", "G_CONV", 2)
        tr = Trainer(net, graph=True, side_wgrad=False, **kw)
        losses = torch.stack([tr.step(x, t).clone() for _ in range(3)])
        torch.cuda.synchronize()
        out.append((losses, tr.fp.flat.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
