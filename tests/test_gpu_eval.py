"""GPU: the trainers' evaluation pass (evaluate / eval_result; the reference's validate(), train.py:138-157, search.py:251-271) --
eval-mode forward of the trained module, Dice loss and the region counts of the prediction p >= 0.5 (prediction.py:157-164) added into
a device accumulator by n3d_head_eval -- against the eager eval path, the CPU oracle, the training it must not disturb, and data
parallel ranks."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_gpu_nets import build_net
from _util import dev, fill_module
from oracle import ref_path as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def one_rank_group():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["N3D_FORCE_DP"] = "1"
    dist.init_process_group("nccl", rank=0, world_size=1)
    yield
    dist.destroy_process_group()
    os.environ.pop("N3D_FORCE_DP", None)


def _batch(seed, b, size, u8=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((b, 4, size, size, size)).astype(np.float32)
    t = rng.uniform(0, 1, (b, 3, size, size, size)) < 0.3
    return dev(x), dev(t.astype(np.uint8 if u8 else np.float32))


def _eager_eval(net, x, t):
    """the reference's pattern: net.eval(); forward under no_grad"""
    was = net.training
    net.eval()
    try:
        with torch.no_grad():
            loss, p = net.forward_loss(x, t)
    finally:
        net.train(was)
    return loss, p


def _counts(p, t, thr=0.5):
    """(I, P, T) per (sample, class) of the thresholded probabilities, float64 on the host"""
    h = (p >= thr).double()
    tt = t.double()
    return [a.cpu().numpy() for a in ((h * tt).sum((2, 3, 4)), h.sum((2, 3, 4)), tt.sum((2, 3, 4)))]


def _acc_counts(acc):
    a = acc.detach().cpu().numpy()
    per = a[4:].reshape(-1, 4)
    return per[:, 0], per[:, 1], per[:, 2], per[:, 3]


def _one_eval(tr, x, t):
    """evaluate one batch into a fresh accumulator: (loss, accumulator copy)"""
    tr.eval_accumulator().zero_()
    loss = tr.evaluate(x, t)
    torch.cuda.synchronize()
    return loss.clone(), tr.eval_accumulator().clone()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("u8", [False, True])
def test_evaluate_equals_the_eager_eval_path(graph, u8):
    from nas_3d_unet_amd.train import Trainer
    net, _ = build_net("searched", "G_CONV", 4, keep_dropout=True)      # eval mode must switch the head's Dropout3d off
    tr = Trainer(net, graph=graph)
    x, t = _batch(5, 2, 64, u8)
    tx, tt = _batch(6, 2, 64, u8)
    for rnd in range(2):
        loss, acc = _one_eval(tr, x, t)
        ref, p = _eager_eval(net, x, t)
        assert torch.equal(loss, ref), (rnd, float(loss), float(ref))
        I, P, T = _counts(p, t)
        aI, aP, aT, _ = _acc_counts(acc)
        np.testing.assert_array_equal(aI, I.sum(0))
        np.testing.assert_array_equal(aP, P.sum(0))
        np.testing.assert_array_equal(aT, T.sum(0))
        assert float(acc[1]) == 1.0 and float(acc[2]) == 2.0 and float(acc[0]) == float(ref)
        assert net.training
        for _ in range(3):
            tr.step(tx, tt)      # the evaluation graph must read the weights the steps moved
        torch.cuda.synchronize()


def test_evaluate_against_the_cpu_oracle():
    from nas_3d_unet_amd import searched
    from nas_3d_unet_amd.head import eval_figures
    from nas_3d_unet_amd.train import Trainer
    cfg = orc.DEFAULT_CFG._replace(depth=2)
    gene = orc.G_CONV
    P = orc.make_params(orc.searched_param_specs(cfg, gene))
    P["last_conv.0.conv.bias"][2] = -30.0        # class 2: nothing predicted
    net = searched.SearchedNet(cfg.in_channels, cfg.init_n_kernels, cfg.out_channels, cfg.depth, cfg.n_nodes, cfg.channel_change,
                               searched.Genotype(*gene))
    with torch.no_grad():
        for n, q in net.named_parameters():
            q.copy_(P[n])
    net = net.cuda()
    rng = np.random.default_rng(9)
    xn = rng.standard_normal((2, 4, 32, 32, 32)).astype(np.float32)
    tn = (rng.uniform(0, 1, (2, 3, 32, 32, 32)) < 0.3).astype(np.float32)
    tn[0, 2] = 0.0                                # sample 0, class 2: prediction and target both empty -> Dice 1
    tr = Trainer(net, graph=True)
    loss = tr.evaluate(dev(xn), dev(tn))
    acc = tr.eval_accumulator().detach().cpu().numpy().copy()
    res = tr.eval_result(reset=True)
    with torch.no_grad():
        po = orc.searched_forward(P, torch.from_numpy(xn), gene, cfg)
        lo = orc.dice_loss(po, torch.from_numpy(tn))
    assert abs(float(loss) - float(lo)) < 1e-5
    po = po.double().numpy()
    band = np.abs(po - 0.5) < 1e-5
    h = po >= 0.5
    aI, aP, aT, _ = _acc_counts(torch.from_numpy(acc))
    assert np.all(np.abs(aI - (h * tn).sum((0, 2, 3, 4))) <= (band * tn).sum((0, 2, 3, 4)))
    assert np.all(np.abs(aP - h.sum((0, 2, 3, 4))) <= band.sum((0, 2, 3, 4)))
    np.testing.assert_array_equal(aT, tn.sum((0, 2, 3, 4)))
    # the figures against a numpy restatement of the accumulator
    per = acc[4:].reshape(3, 4)
    assert per[2, 1] == 0.0 and per[2, 2] == tn[1, 2].sum()
    I, Pp, T = per[:, 0], per[:, 1], per[:, 2]
    np.testing.assert_array_equal(res.dice_global, 2 * I / (Pp + T))
    np.testing.assert_array_equal(res.dice, per[:, 3] / 2)
    assert res.dice[2] == 0.5                     # sample 0 empty-and-empty (1), sample 1 nothing predicted (0)
    assert res.loss == float(loss) and res.n_batches == 1 and res.n_samples == 2
    again = eval_figures(acc)
    assert again.loss == res.loss and np.array_equal(again.dice, res.dice) and np.array_equal(again.dice_global, res.dice_global)
    with pytest.raises(ValueError):
        tr.eval_result()                          # reset: no batch in the accumulator


@pytest.mark.parametrize("side", [False, "force"])
def test_evaluate_does_not_perturb_training(side):
    from nas_3d_unet_amd import programs
    from nas_3d_unet_amd.train import Trainer, _dropout_states
    x, t = _batch(11, 2, 32)
    vx, vt = _batch(12, 2, 32)
    runs = []
    for with_eval in (False, True):
        net, _ = build_net("searched", "G_CONV", 4, keep_dropout=True)
        drops = [m for m in net.modules() if isinstance(m, torch.nn.Dropout3d)]
        assert drops
        for i, m in enumerate(drops):
            programs.dropout_state(m, x.device, seed=1234 + i)    # the two nets draw the same masks (seeds are per module otherwise)
        tr = Trainer(net, graph=True, side_wgrad=side)
        losses = []
        for _ in range(5):
            losses.append(tr.step(x, t).clone())
            if with_eval:
                tr.evaluate(vx, vt)
        torch.cuda.synchronize()
        assert tr._n_steps == 5
        runs.append((torch.stack(losses).cpu(), tr.fp.flat.cpu(), tr.fp.exp_avg.cpu(), tr.fp.exp_avg_sq.cpu(),
                     [s.cpu() for s in _dropout_states(tr.net)]))
    (l0, w0, m0, v0, d0), (l1, w1, m1, v1, d1) = runs
    assert torch.equal(l0, l1) and torch.equal(w0, w1) and torch.equal(m0, m1) and torch.equal(v0, v1)
    assert len(d0) == len(d1) > 0 and all(torch.equal(a, b) for a, b in zip(d0, d1))


def test_accumulation_remainder_and_reset():
    from nas_3d_unet_amd.train import Trainer
    net, _ = build_net("searched", "G_CONV", 4)
    tr = Trainer(net, graph=True)
    batches = [_batch(21, 2, 32), _batch(22, 1, 32), _batch(23, 2, 32)]     # the middle one runs eagerly
    sep = [_one_eval(tr, x, t) for x, t in batches]
    tr.eval_result(reset=True)
    for x, t in batches:
        tr.evaluate(x, t)
    acc = tr.eval_accumulator().detach().cpu().numpy().copy()
    res = tr.eval_result(reset=True)
    assert res.n_batches == 3 and res.n_samples == 5
    tot = sum(a.cpu().numpy() for _, a in sep)
    np.testing.assert_array_equal(acc[1:3], tot[1:3])
    for c in range(3):
        np.testing.assert_array_equal(acc[4 + 4 * c:7 + 4 * c], tot[4 + 4 * c:7 + 4 * c])
    np.testing.assert_allclose(acc[7::4], tot[7::4], rtol=1e-14)
    np.testing.assert_allclose(res.loss, np.mean([float(l) for l, _ in sep]), rtol=1e-14)
    # replays are counted, and reset starts a fresh epoch
    for _ in range(4):
        tr.evaluate(*batches[0])
    res = tr.eval_result(reset=True)
    assert res.n_batches == 4 and res.n_samples == 8
    np.testing.assert_allclose(res.loss, float(sep[0][0]), rtol=1e-14)


def test_padded_twin_and_bf16_storage():
    from nas_3d_unet_amd import searched
    from nas_3d_unet_amd.train import Trainer
    from test_gpu_nets import _genotype_for
    cfg = orc.NetCfg(4, 6, 3, 2, 3, True)
    gene = _genotype_for(cfg.n_nodes)
    net = searched.SearchedNet(cfg.in_channels, cfg.init_n_kernels, cfg.out_channels, cfg.depth, cfg.n_nodes, cfg.channel_change,
                               searched.Genotype(list(gene.down), list(gene.up)))
    fill_module(net)
    net = net.cuda()
    tr = Trainer(net, graph=True)
    assert tr._twin is not None
    x, t = _batch(31, 2, 32)
    tr.step(x, t)
    loss, acc = _one_eval(tr, x, t)
    tr.check_sync()
    ref, p = _eager_eval(net, x, t)
    assert abs(float(loss) - float(ref)) <= 1e-6
    band = ((p - 0.5).abs() < 1e-5).double()
    I, P, _ = _counts(p, t)
    aI, aP, aT, _ = _acc_counts(acc)
    assert np.all(np.abs(aI - I.sum(0)) <= (band * t.double()).sum((0, 2, 3, 4)).cpu().numpy())
    assert np.all(np.abs(aP - P.sum(0)) <= band.sum((0, 2, 3, 4)).cpu().numpy())
    np.testing.assert_array_equal(aT, t.double().sum((0, 2, 3, 4)).cpu().numpy())
    # bf16 activation storage at 4 x 128^3, batch 1
    net, _ = build_net("searched", "G_CONV", 4)
    tr = Trainer(net, graph=True, storage="bf16")
    x, t = _batch(32, 1, 128)
    loss, acc = _one_eval(tr, x, t)
    ref, p = _eager_eval(net, x, t)
    assert torch.equal(loss, ref)
    I, P, T = _counts(p, t)
    aI, aP, aT, _ = _acc_counts(acc)
    np.testing.assert_array_equal(aI, I.sum(0))
    np.testing.assert_array_equal(aP, P.sum(0))


@pytest.mark.parametrize("graph", [False, True])
def test_search_trainer_evaluate(graph):
    from nas_3d_unet_amd import nas
    from nas_3d_unet_amd.train import SearchTrainer
    cfg = orc.DEFAULT_CFG._replace(depth=2)
    net = nas.ShellNet(cfg.in_channels, cfg.init_n_kernels, cfg.out_channels, cfg.depth, cfg.n_nodes, False, cfg.channel_change)
    fill_module(net)
    net = net.cuda()
    tr = SearchTrainer(net, graph=graph)
    x, t = _batch(41, 2, 16)
    vx, vt = _batch(42, 2, 16)
    for rnd in range(2):
        torch.cuda.synchronize()
        state = [a.clone() for a in (tr.fp.flat, tr.fp.exp_avg, tr.fp.exp_avg_sq, tr.aflat, tr.a_m, tr.a_v)]
        loss, acc = _one_eval(tr, vx, vt)
        ref, p = _eager_eval(net, vx, vt)
        assert torch.equal(loss, ref), (rnd, float(loss), float(ref))
        I, P, T = _counts(p, vt)
        aI, aP, _, _ = _acc_counts(acc)
        np.testing.assert_array_equal(aI, I.sum(0))
        np.testing.assert_array_equal(aP, P.sum(0))
        assert all(torch.equal(a, b) for a, b in zip(state, (tr.fp.flat, tr.fp.exp_avg, tr.fp.exp_avg_sq, tr.aflat, tr.a_m, tr.a_v)))
        tr.step(x, t, vx, vt)


def test_eval_result_in_a_one_rank_group_equals_single_gpu(one_rank_group):
    from nas_3d_unet_amd.train import Trainer
    batches = [_batch(51, 2, 32), _batch(52, 2, 32), _batch(53, 1, 32)]
    out = []
    for dp in (True, False):
        forced = None if dp else os.environ.pop("N3D_FORCE_DP", None)
        try:
            net, _ = build_net("searched", "G_CONV", 4)
            tr = Trainer(net, graph=True)
            assert tr.dp_path == dp
            for x, t in batches:
                tr.evaluate(x, t)
            out.append(tr.eval_result(reset=True))
        finally:
            if forced is not None:
                os.environ["N3D_FORCE_DP"] = forced
    a, b = out
    assert a.loss == b.loss and a.n_batches == b.n_batches == 3 and a.n_samples == b.n_samples == 5
    np.testing.assert_array_equal(a.dice, b.dice)
    np.testing.assert_array_equal(a.dice_global, b.dice_global)


def _eval_batches():
    return [_batch(61 + i, 2, 16) for i in range(4)]


def _two_rank_eval_worker(rank, world, port, out):
    """one of two processes sharing cuda:0 (gloo: RCCL refuses two ranks on one device); each evaluates half of the batches"""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests"), os.path.join(root, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.pop("N3D_FORCE_DP", None)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nas_3d_unet_amd.train import Trainer
    from test_gpu_nets import build_net as bn
    net, _ = bn("searched", "G_CONV", 2)
    tr = Trainer(net, graph=True)
    assert tr.dp_path
    for i, (x, t) in enumerate(_eval_batches()):
        if i % world == rank:
            tr.evaluate(x, t)
    acc = tr.eval_accumulator().detach().cpu().clone()
    res = tr.eval_result(reset=True)
    torch.save({"acc": acc, "res": tuple(res)}, out + ".r%d" % rank)
    dist.barrier()
    dist.destroy_process_group()


def test_two_processes_each_evaluating_half_equal_one_process():
    import torch.multiprocessing as mp
    from nas_3d_unet_amd.train import Trainer
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "ev2")
        mp.spawn(_two_rank_eval_worker, args=(2, port, out), nprocs=2, join=True)
        r0, r1 = torch.load(out + ".r0", weights_only=False), torch.load(out + ".r1", weights_only=False)
    forced = os.environ.pop("N3D_FORCE_DP", None)
    try:
        net, _ = build_net("searched", "G_CONV", 2)
        tr = Trainer(net, graph=True)
        for x, t in _eval_batches():
            tr.evaluate(x, t)
        acc = tr.eval_accumulator().detach().cpu().clone()
        res = tr.eval_result(reset=True)
    finally:
        if forced is not None:
            os.environ["N3D_FORCE_DP"] = forced
    both = (r0["acc"] + r1["acc"]).numpy()
    a = acc.numpy()
    np.testing.assert_array_equal(both[1:3], a[1:3])
    for c in range(3):
        np.testing.assert_array_equal(both[4 + 4 * c:7 + 4 * c], a[4 + 4 * c:7 + 4 * c])
    np.testing.assert_allclose(both[0], a[0], rtol=1e-15)
    for r in (r0["res"], r1["res"]):
        loss, dice, dglob, nb, ns = r
        assert nb == res.n_batches == 4 and ns == res.n_samples == 8
        np.testing.assert_allclose(loss, res.loss, rtol=1e-15)
        np.testing.assert_array_equal(dglob, res.dice_global)
        np.testing.assert_allclose(dice, res.dice, rtol=1e-14)
    np.testing.assert_array_equal(r0["res"][2], r1["res"][2])
