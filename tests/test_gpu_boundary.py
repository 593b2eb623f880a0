"""GPU: loss.BoundaryLoss -- the signed distance maps of a target batch (n3d_target_sdt) against scipy's recorded answers
(tests/golden/boundary.npz) bit for bit, the boundary term inside the fused head's two passes (n3d_head_bnd_fwd / _bwd) against the
fp64 statement of tests/_boundary_ref.py, its identities with the loss entry points, the device weight, and the trainers.

Bounds.  The base loss and the gradients are held to tests/test_gpu_loss.py's bounds.  The boundary part of the loss, w * mean(p phi),
is a sum of fp32 products -- four fp32 adds per lane, fp64 from there on: about 4 * 2^-24 relative to sum |p phi| (phi is signed and
cancels, so the error scales with the absolute sum, not with the result); the bound is 4x that, 2^-20 * w * mean |p phi|, on top of the
base loss's 1e-6 * max(1, |ref|)."""
import functools
import os

import numpy as np
import pytest
import torch

import _boundary_ref as br
import _loss_ref as lr
from _util import assert_close, dev, fill_module
from oracle import ref_path as orc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boundary.npz")
TV, TV_BCE = lr.SPECS[2], lr.SPECS[3]          # a base without and with the cross-entropy term (records of 4 and 5 doubles)
TRAIN_SPEC = lr.Spec(0.5, 0.5, 1.0, 0.5)       # the trainers' tests: TverskyBCELoss(bce_weight=0.5)
W = 0.05


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


def _module(spec, weight):
    from nas_3d_unet_amd.loss import BoundaryLoss, TverskyBCELoss
    return BoundaryLoss(TverskyBCELoss(*spec), weight)


# ---- 1. the transform ------------------------------------------------------------------------------------------------------------
def _strided_targets(tn):
    """the targets through a channels-last view: (B, C, D0, D1, D2) of a (B, D0, D1, D2, C) tensor -- voxel stride C, channel stride 1"""
    t = dev(np.ascontiguousarray(np.moveaxis(tn, 1, -1))).permute(0, 4, 1, 2, 3)
    assert t.is_contiguous() == (tn.shape[1] == 1)      # (one channel: the view is the dense tensor)
    return t


def _pitched_out(shape):
    """an output whose voxels are C + 1 floats apart (channels-last with one float of padding), pre-filled so unwritten words show"""
    B, Cc = shape[:2]
    buf = torch.full((B,) + tuple(shape[2:]) + (Cc + 1,), -777.0, device="cuda")
    return buf, buf[..., :Cc].permute(0, 4, 1, 2, 3)


@pytest.mark.parametrize("pitched", [False, True], ids=["dense_out", "pitched_out"])
@pytest.mark.parametrize("strided", [False, True], ids=["dense_t", "strided_t"])
@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["float", "bytes"])
@pytest.mark.parametrize("name", list(br.SHAPES))
def test_target_sdt_equals_the_fixture(name, dtype, strided, pitched):
    """(2, 3, 16^3), (1, 3, 8, 12, 20), (1, 3, 4, 4, 130) -- a z line longer than two waves -- and (1, 1, 1, 1, 7)"""
    from nas_3d_unet_amd import kernels as K
    g = _golden()
    tn, want = g[name + ".t"].astype(dtype), g[name + ".phi"]
    t = _strided_targets(tn) if strided else dev(tn)
    if pitched:
        buf, out = _pitched_out(tn.shape)
        assert K.target_sdt(t, out=out) is out
        assert float(buf[..., -1].min()) == -777.0 and float(buf[..., -1].max()) == -777.0      # the padding is untouched
    else:
        out = K.target_sdt(t)
        assert out.is_contiguous() and out.dtype == torch.float32
    got = out.cpu().numpy()
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, "%d of %d voxels differ, worst |err| %.3g" % (bad, got.size, np.abs(got - want).max())
    again = K.target_sdt(t).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


def test_signed_distance_is_the_public_function():
    from nas_3d_unet_amd import loss
    from nas_3d_unet_amd._lib import N3DError
    g = _golden()
    t = dev(g["box.t"])
    want = g["box.phi"]
    for fn in (loss.signed_distance, loss.BoundaryLoss.signed_distance):
        assert np.array_equal(fn(t).cpu().numpy().view(np.uint32), want.view(np.uint32))
    with pytest.raises(N3DError, match="float32 or uint8"):
        loss.signed_distance(t.to(torch.int32))
    with pytest.raises(N3DError, match=r"\(B, C, D0, D1, D2\)"):
        loss.signed_distance(t[0])


# ---- 2. / 3. the head against the fp64 statement ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(shape, batch, use_gate, bf16=False):
    """head operands (12 -> 3) as numpy arrays: tumour-like targets, their phi by the numpy statement, x (bf16-rounded on request)"""
    ci, co = 12, 3
    rng = np.random.default_rng(shape[-1] * 10 + batch)
    xn = rng.standard_normal((batch, ci) + shape).astype(np.float32)
    if bf16:
        xn = torch.from_numpy(xn).bfloat16().float().numpy()
    wn = (rng.standard_normal((co, ci, 1, 1, 1)) * 0.4).astype(np.float32)
    bn = rng.standard_normal(co).astype(np.float32) * 0.2
    tn = br.tumour_targets(batch, shape, 7)
    gn = ((rng.uniform(0, 1, (batch, ci)) >= 0.5) / 0.5).astype(np.float32) if use_gate else None
    return xn, wn, bn, tn, gn, br.signed_distance(tn)


@functools.lru_cache(maxsize=None)
def _reference(shape, batch, use_gate, spec, weight, bf16=False):
    xn, wn, bn, tn, gn, fn = _data(shape, batch, use_gate, bf16)
    T = torch.from_numpy
    return br.head_reference(T(xn), T(wn), T(bn), T(gn) if use_gate else None, T(tn), T(fn), spec, weight)


def _wdev(w):
    return torch.full((1,), w, dtype=torch.float32, device="cuda")


def _loss_ok(got, c, what=""):
    """bound 2 of the module docstring"""
    got = float(got)
    tol = 1e-6 * max(1.0, abs(c.base)) + 2.0 ** -20 * c.w * c.mean_abs
    print("%s loss %.9g ref %.9g (base %.9g boundary %.9g) |err| %.3g bound %.3g" % (what, got, c.loss, c.base, c.bnd, abs(got - c.loss), tol))
    assert abs(got - c.loss) <= tol, (got, c.loss, tol)


def _check_forward(c, sums, coef, loss, spec, batch, N, weight, what):
    S = (4 if spec.bce_weight > 0 else 3) + 1
    _loss_ok(loss, c, what)
    assert sums.shape == (batch, 3, S) and coef.numel() == 2 * batch * 3 + 2
    ref = torch.cat([c.sums[..., :S - 1], c.sums[..., 4:]], dim=-1)
    assert_close(sums[..., :S - 1], ref[..., :S - 1], 2e-6, "sums")
    # sum p phi per pair: 4 * 2^-24 of the pair's sum |p phi| at most (with the margin of the loss: 2^-20); the mean over the pairs bounds it
    assert float((sums[..., S - 1].cpu() - ref[..., S - 1]).abs().max()) <= 2.0 ** -20 * c.mean_abs * batch * 3 * N
    assert float(coef[2 * batch * 3 + 1]) == float(np.float32(np.float64(np.float32(weight)) / (batch * 3 * N)))


HEAD_SHAPES = [((16, 16, 16), 2, True), ((8, 12, 20), 2, False)]      # 4 whole chunks of 1024 voxels; 1.875 chunks (N = 1920)


@pytest.mark.parametrize("tdtype", [np.float32, np.uint8], ids=["float_t", "byte_t"])
@pytest.mark.parametrize("spec", [TV, TV_BCE], ids=["tversky", "tversky_bce"])
@pytest.mark.parametrize("shape,batch,use_gate", HEAD_SHAPES)
def test_head_bnd_matches_the_reference(shape, batch, use_gate, spec, tdtype):
    from nas_3d_unet_amd import kernels as K
    ci = 12
    xn, wn, bn, tn, gn, fn = _data(shape, batch, use_gate)
    c, dxr, dwr, dbr = _reference(shape, batch, use_gate, spec, W)
    xv = K.as_view(dev(xn))
    w, b, t, phi = dev(wn), dev(bn), dev(tn.astype(tdtype)), dev(fn)
    gate = dev(gn) if use_gate else None
    p, _, sums, coef, loss = K.head_bnd_fwd(xv, w, b, gate, t, phi, spec, _wdev(W))
    _check_forward(c, sums, coef, loss, spec, batch, int(np.prod(shape)), W, "pitched")
    assert_close(p, torch.sigmoid(_logits(xn, wn, bn, gn)), 1e-5, "p")
    dx = K.as_view(K.empty_ndhwc(batch, ci, *shape, xv.t.device))
    dw, db = torch.empty_like(w), torch.empty_like(b)
    K.head_bnd_bwd(xv, w, b, gate, dx, dw, db, t, phi, coef)
    assert_close(dx.t, dxr, 2e-5, "dx")
    assert_close(dw, dwr, 2e-5, "dw")
    assert_close(db, dbr, 2e-5, "db")
    K.head_bnd_bwd(xv, w, b, gate, dx, None, None, t, phi, coef, accumulate=True)
    assert_close(dx.t, 2 * dxr, 2e-5, "dx accumulate")
    # the boundary term moves the gradient by far more than the bound: the check above sees it
    c0, dx0 = _reference(shape, batch, use_gate, spec, 0.0)[:2]
    assert float((dxr - dx0).abs().max()) > 100 * 2e-5 * float(dxr.abs().max())


def _logits(xn, wn, bn, gn):
    x, w = torch.from_numpy(xn).double(), torch.from_numpy(wn).double().reshape(wn.shape[0], -1)
    if gn is not None:
        x = x * torch.from_numpy(gn).double()[:, :, None, None, None]
    return torch.einsum("oc,bcdhw->bodhw", w, x) + torch.from_numpy(bn).double()[None, :, None, None, None]


@pytest.mark.parametrize("spec", [TV, TV_BCE], ids=["tversky", "tversky_bce"])
@pytest.mark.parametrize("shape,batch", [((16, 16, 16), 2), ((8, 12, 20), 2)])
def test_head_bnd_on_node_planar_input(shape, batch, spec):
    """3 x 4 channels as three dense node tensors, with a node-planar dx; phi through a pitched view"""
    from nas_3d_unet_amd import kernels as K
    cn, nn = 4, 3
    xn, wn, bn, tn, _, fn = _data(shape, batch, False)
    c, dxr, dwr, dbr = _reference(shape, batch, False, spec, W)
    d = torch.device("cuda")
    pl = K.empty_planar(nn, batch, cn, *shape, d)
    for k in range(nn):
        pl.nodes[k].t.copy_(dev(xn[:, k * cn:(k + 1) * cn]))
    w, b, t = dev(wn), dev(bn), dev(tn)
    _, phi = _pitched_out(tn.shape)
    phi.copy_(dev(fn))
    _, _, sums, coef, loss = K.head_bnd_fwd(pl, w, b, None, t, phi, spec, _wdev(W), want_p=False)
    _check_forward(c, sums, coef, loss, spec, batch, int(np.prod(shape)), W, "node-planar")
    dx = K.empty_planar(nn, batch, cn, *shape, d)
    dw, db = torch.empty_like(w), torch.empty_like(b)
    K.head_bnd_bwd(pl, w, b, None, dx, dw, db, t, phi, coef)
    assert_close(torch.cat([n.t for n in dx.nodes], dim=1), dxr, 2e-5, "dx")
    assert_close(dw, dwr, 2e-5, "dw")
    assert_close(db, dbr, 2e-5, "db")


@pytest.mark.parametrize("tdtype", [np.float32, np.uint8], ids=["float_t", "byte_t"])
@pytest.mark.parametrize("shape,batch", [((16, 16, 16), 2), ((8, 12, 20), 2)])
def test_head_bnd_bf16_storage(shape, batch, tdtype):
    """bf16 storage of the head input and its gradient: method and bounds of test_gpu_loss.test_head_loss_bf16_storage"""
    from nas_3d_unet_amd import kernels as K
    spec, ci = TV_BCE, 12
    xn, wn, bn, tn, _, fn = _data(shape, batch, False, True)
    c, dxr, dwr, dbr = _reference(shape, batch, False, spec, W, True)
    xd = K.empty_ndhwc(batch, ci, *shape, torch.device("cuda"), torch.bfloat16)
    xd.copy_(dev(xn).bfloat16())
    xv = K.as_view(xd, bf16_ok=True)
    w, b, t, phi = dev(wn), dev(bn), dev(tn.astype(tdtype)), dev(fn)
    _, _, sums, coef, loss = K.head_bnd_fwd(xv, w, b, None, t, phi, spec, _wdev(W))
    _check_forward(c, sums, coef, loss, spec, batch, int(np.prod(shape)), W, "bf16")
    dx = K.as_view(K.empty_ndhwc(batch, ci, *shape, xv.t.device, torch.bfloat16), bf16_ok=True)
    dw, db = torch.empty_like(w), torch.empty_like(b)
    K.head_bnd_bwd(xv, w, b, None, dx, dw, db, t, phi, coef)
    assert_close(dw, dwr, 2e-5, "dw")
    assert_close(db, dbr, 2e-5, "db")
    dxr = dxr.float()
    assert_close(dx.t.float(), dxr, 2.0 ** -8, "dx (bf16)")
    assert torch.equal(dx.t.cpu(), dxr.bfloat16()) or float((dx.t.float().cpu() - dxr.bfloat16().float()).abs().max()) <= float(dxr.abs().max()) * 2.0 ** -7


def test_head_bnd_takes_the_three_channel_head_only():
    from nas_3d_unet_amd import kernels as K
    rng = np.random.default_rng(2)
    shape = (4, 8, 8)
    for co in (2, 4):
        xv = K.as_view(dev(rng.standard_normal((1, 8) + shape).astype(np.float32)))
        w, b = dev(rng.standard_normal((co, 8, 1, 1, 1)).astype(np.float32)), dev(np.zeros(co, np.float32))
        t = dev((rng.uniform(0, 1, (1, co) + shape) < 0.3).astype(np.float32))
        phi = torch.zeros_like(t)
        with pytest.raises(K.N3DError, match="Co = 3"):
            K.head_bnd_fwd(xv, w, b, None, t, phi, TV, _wdev(W))
        dx = K.as_view(K.empty_ndhwc(1, 8, *shape, xv.t.device))
        with pytest.raises(K.N3DError, match="Co = 3"):
            K.head_bnd_bwd(xv, w, b, None, dx, None, None, t, phi, torch.zeros(2 * co + 2, device="cuda"))


# ---- 4. identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdtype", [np.float32, np.uint8], ids=["float_t", "byte_t"])
@pytest.mark.parametrize("spec", [TV, TV_BCE], ids=["tversky", "tversky_bce"])
@pytest.mark.parametrize("how", ["zero_weight", "empty_targets"])
@pytest.mark.parametrize("shape,batch,use_gate", HEAD_SHAPES)
def test_without_a_boundary_term_the_outputs_are_the_loss_entry_points(shape, batch, use_gate, how, spec, tdtype):
    """w = 0 with a live phi, and phi == 0 (empty targets: the zero-map rule, phi from the device) with a live weight: loss, sums,
    coefficients and gradients equal n3d_head_loss_fwd / _bwd bit for bit"""
    from nas_3d_unet_amd import kernels as K
    ci, BC = 12, batch * 3
    xn, wn, bn, tn, gn, fn = _data(shape, batch, use_gate)
    if how == "empty_targets":
        tn = np.zeros_like(tn)
    xv = K.as_view(dev(xn))
    w, b, t = dev(wn), dev(bn), dev(tn.astype(tdtype))
    gate = dev(gn) if use_gate else None
    phi = K.target_sdt(t)
    if how == "empty_targets":
        assert float(phi.abs().max()) == 0.0
    else:
        assert np.array_equal(phi.cpu().numpy().view(np.uint32), fn.view(np.uint32))
    S = 4 if spec.bce_weight > 0 else 3
    _, _, sums0, coef0, loss0 = K.head_loss_fwd(xv, w, b, gate, t, spec)
    _, _, sums1, coef1, loss1 = K.head_bnd_fwd(xv, w, b, gate, t, phi, spec, _wdev(0.0 if how == "zero_weight" else 0.5))
    assert torch.equal(loss0, loss1)
    assert torch.equal(sums0, sums1[..., :S]) and torch.equal(coef0, coef1[:2 * BC + 1])
    out = []
    for bnd in (False, True):
        dx = K.as_view(K.empty_ndhwc(batch, ci, *shape, xv.t.device))
        dw, db = torch.empty_like(w), torch.empty_like(b)
        if bnd:
            K.head_bnd_bwd(xv, w, b, gate, dx, dw, db, t, phi, coef1)
        else:
            K.head_loss_bwd(xv, w, b, gate, dx, dw, db, t, coef0)
        out.append((dx.t.clone(), dw, db))
    for a, c, what in zip(out[0], out[1], ("dx", "dw", "db")):
        assert torch.equal(a, c), what


# ---- 5. / 6. trainers ------------------------------------------------------------------------------------------------------------
def _trainer_cfg():
    from test_gpu_nets import _genotype_for
    cfg = orc.NetCfg(4, 4, 3, 2, 3, True)
    return cfg, _genotype_for(cfg.n_nodes)


@functools.lru_cache(maxsize=None)
def _batch():
    rng = np.random.default_rng(29)
    xn = rng.standard_normal((2, 4, 16, 16, 16)).astype(np.float32)
    tn = br.tumour_targets(2, (16, 16, 16), 12)
    return xn, tn, br.signed_distance(tn)


def _net():
    from nas_3d_unet_amd import searched
    cfg, gene = _trainer_cfg()
    net = searched.SearchedNet(cfg.in_channels, cfg.init_n_kernels, cfg.out_channels, cfg.depth, cfg.n_nodes, cfg.channel_change,
                               searched.Genotype(list(gene.down), list(gene.up)))
    fill_module(net)
    net.last_conv[0].dropout = None
    return net.cuda()


@functools.lru_cache(maxsize=None)
def _trainer_reference(weight):
    """three Adam steps of the fp64 oracle with the loss of _boundary_ref"""
    cfg, gene = _trainer_cfg()
    xn, tn, fn = _batch()
    D = lambda a: torch.from_numpy(a).double()
    P = orc.make_params(orc.searched_param_specs(cfg, gene), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam(list(P.values()))
    ref = []
    for _ in range(3):
        opt.zero_grad()
        l = br.torch_loss(orc.searched_forward(P, D(xn), gene, cfg, return_logits=True)[1], D(tn), D(fn), TRAIN_SPEC, weight)
        l.backward(); opt.step()
        ref.append(float(l.detach()))
    return ref, {n: float(q.detach().norm()) for n, q in P.items()}


@pytest.mark.parametrize("graph", [False, True])
def test_trainer_with_the_boundary_loss_matches_torch_adam(graph):
    """Trainer(loss=BoundaryLoss(TverskyBCELoss(bce_weight=0.5), 0.01)) at 2 x 4 x 16^3: three steps against the fp64 trajectory, with
    test_gpu_loss.py's trajectory tolerances"""
    from nas_3d_unet_amd.train import Trainer
    xn, tn, _ = _batch()
    ref, norms = _trainer_reference(0.01)
    net = _net()
    tr = Trainer(net, graph=graph, loss=_module(TRAIN_SPEC, 0.01))
    assert tr._direct_ok()
    losses = [float(tr.step(dev(xn), dev(tn))) for _ in range(3)]
    print("losses", losses, "ref", ref)
    np.testing.assert_allclose(losses, ref, rtol=0, atol=2e-4)
    tr.check_sync()
    for n, q in net.named_parameters():
        assert abs(float(q.detach().double().norm()) - norms[n]) <= 5e-4 * norms[n] + 3e-3, n


def _three_steps(graph, loss, steps=3, tdtype=np.float32):
    from nas_3d_unet_amd.train import Trainer
    xn, tn, _ = _batch()
    tr = Trainer(_net(), graph=graph, side_wgrad=False, loss=loss)
    x, t = dev(xn), dev(tn.astype(tdtype))
    losses = torch.stack([tr.step(x, t).clone() for _ in range(steps)])
    torch.cuda.synchronize()
    return tr, losses, tr.fp.flat.clone()


@pytest.mark.parametrize("tdtype", [np.float32, np.uint8], ids=["float_t", "byte_t"])
def test_eager_and_captured_steps_are_bit_identical(tdtype):
    """the single-stream schedule: the captured step launches what the eager step launches, phi included"""
    _, le, fe = _three_steps(False, _module(TRAIN_SPEC, 0.01), tdtype=tdtype)
    _, lg, fg = _three_steps(True, _module(TRAIN_SPEC, 0.01), tdtype=tdtype)
    assert torch.equal(le, lg) and torch.equal(fe, fg)


def test_weight_zero_trains_what_the_base_loss_trains():
    from nas_3d_unet_amd.loss import TverskyBCELoss
    _, l0, f0 = _three_steps(True, TverskyBCELoss(*TRAIN_SPEC), steps=2)
    _, l1, f1 = _three_steps(True, _module(TRAIN_SPEC, 0.0), steps=2)
    assert torch.equal(l0, l1) and torch.equal(f0, f1)
    # and a live weight does train something else
    _, l2, f2 = _three_steps(True, _module(TRAIN_SPEC, 0.01), steps=2)
    assert not torch.equal(l0, l2) and not torch.equal(f0, f2)


@pytest.mark.parametrize("graph", [False, True])
def test_evaluate_reports_the_base_loss(graph):
    """the boundary weight moves during training; evaluate() reports the loss whose definition does not"""
    from nas_3d_unet_amd.loss import TverskyBCELoss
    from nas_3d_unet_amd.train import Trainer
    xn, tn, _ = _batch()
    x, t = dev(xn), dev(tn)
    got = []
    for loss in (TverskyBCELoss(*TRAIN_SPEC), _module(TRAIN_SPEC, 0.3)):
        tr = Trainer(_net(), graph=graph, side_wgrad=False, loss=loss)
        got.append((tr.evaluate(x, t).clone(), tr.eval_result()))
    assert torch.equal(got[0][0], got[1][0]) and got[0][1].loss == got[1][1].loss
    assert np.array_equal(got[0][1].dice, got[1][1].dice)


def test_the_device_weight_moves_without_a_recapture():
    """one captured step at w1, the state put back, set_boundary_weight(w2), a replay on the same batch and weights: the same graph
    object, and loss2 - loss1 = (w2 - w1) mean(p phi) of the fp64 statement (p from the fp64 oracle on the restored weights)"""
    import copy
    from nas_3d_unet_amd import checkpoint as ck
    from nas_3d_unet_amd.train import Trainer
    cfg, gene = _trainer_cfg()
    xn, tn, fn = _batch()
    w1, w2 = 0.01, 0.4
    net = _net()
    bl = _module(TRAIN_SPEC, w1)
    tr = Trainer(net, graph=True, side_wgrad=False, loss=bl)
    x, t = dev(xn), dev(tn)
    tr.step(x, t)                                  # captures (and trains one step)
    graph, wdev = tr._graph, bl._wdev
    assert graph is not None and wdev is not None
    sd = copy.deepcopy(ck.train_state_dicts(tr, 0, {}, 1.0))
    P = {n: q.detach().double().cpu() for n, q in net.named_parameters()}
    loss1 = float(tr.step(x, t))
    ck.load_train_state_dicts(tr, sd)
    for n, q in net.named_parameters():
        assert torch.equal(q.detach().double().cpu(), P[n]), n
    tr.set_boundary_weight(w2)
    loss2 = float(tr.step(x, t))
    assert tr._graph is graph and bl._wdev is wdev and float(wdev) == float(np.float32(w2)) and bl.weight == w2
    D = lambda a: torch.from_numpy(a).double()
    with torch.no_grad():
        z = orc.searched_forward(P, D(xn), gene, cfg, return_logits=True)[1]
    c1, c2 = (br.closed_form(z, D(tn), D(fn), TRAIN_SPEC, w) for w in (w1, w2))
    want = c2.bnd - c1.bnd
    tol = 2 * 1e-6 * max(1.0, abs(c1.base)) + 2.0 ** -20 * (c1.w + c2.w) * c1.mean_abs
    print("loss1 %.9g loss2 %.9g difference %.9g, (w2 - w1) mean(p phi) %.9g, bound %.3g" % (loss1, loss2, loss2 - loss1, want, tol))
    assert abs(want) > 100 * tol          # the move is far above the bound: an unread weight would show
    assert abs((loss2 - loss1) - want) <= tol
    with pytest.raises(ValueError, match="weight >= 0"):
        tr.set_boundary_weight(-1.0)


def test_set_boundary_weight_needs_a_boundary_loss():
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd.train import Trainer
    tr = Trainer(_net(), graph=False)
    with pytest.raises(K.N3DError, match="not a BoundaryLoss"):
        tr.set_boundary_weight(0.1)


def test_search_trainer_forms_phi_for_both_passes(monkeypatch):
    from nas_3d_unet_amd import kernels as K, nas
    from nas_3d_unet_amd.train import SearchTrainer
    cfg = orc.DEFAULT_CFG._replace(depth=2)
    net = nas.ShellNet(cfg.in_channels, cfg.init_n_kernels, cfg.out_channels, cfg.depth, cfg.n_nodes, False, cfg.channel_change)
    fill_module(net)
    net.kernel.last_conv[0].dropout = None
    net = net.cuda()
    tr = SearchTrainer(net, graph=False, loss=_module(TRAIN_SPEC, 0.01))
    xn, tn, _ = _batch()
    rng = np.random.default_rng(5)
    vxn, vtn = rng.standard_normal(xn.shape).astype(np.float32), br.tumour_targets(2, (16, 16, 16), 13)
    seen = []
    real = K.target_sdt

    def counting(t, out=None):
        phi = real(t, out)
        seen.append((t, phi))
        return phi

    monkeypatch.setattr(K, "target_sdt", counting)
    la, lw = tr.step(dev(xn), dev(tn), dev(vxn), dev(vtn))
    assert np.isfinite(float(la)) and np.isfinite(float(lw))
    assert len(seen) == 2      # the architecture pass on the validation batch, then the weight pass on the training batch
    for (t, phi), want in zip(seen, (vtn, tn)):
        assert np.array_equal(t.cpu().numpy(), want)
        assert np.array_equal(phi.cpu().numpy().view(np.uint32), br.signed_distance(want).view(np.uint32))
    tr.set_boundary_weight(0.02)
    assert tr.loss_fn.weight == 0.02


def test_other_heads_are_refused_at_construction():
    from nas_3d_unet_amd import kernels as K, prim_ops, searched
    from nas_3d_unet_amd.train import Trainer
    cfg, gene = _trainer_cfg()
    mk = lambda co: searched.SearchedNet(cfg.in_channels, cfg.init_n_kernels, co, cfg.depth, cfg.n_nodes, cfg.channel_change,
                                         searched.Genotype(list(gene.down), list(gene.up))).cuda()
    with pytest.raises(K.N3DError, match="three-channel head"):
        Trainer(mk(5), graph=False, loss=_module(TRAIN_SPEC, 0.01))
    net = mk(3)
    ci = net.last_conv[0].conv.weight.shape[1]
    net.last_conv = torch.nn.Sequential(prim_ops.ConvOps(ci, 3, kernel_size=3, ops_order="weight"), torch.nn.Sigmoid()).cuda()
    with pytest.raises(K.N3DError, match="not one it takes"):
        Trainer(net, graph=False, loss=_module(TRAIN_SPEC, 0.01))
