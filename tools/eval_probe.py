"""What the trainers' evaluation pass costs against the reference's validation pattern and against a training step, batch 2:
  * evaluate() replayed (eval-mode forward + Dice + region counts, one captured graph, no host sync);
  * the eager `net.eval(); forward_loss` with float(loss) per batch (train.py:138-157: one host sync per batch);
  * one step() (replayed);
and the evaluation head alone (n3d_head_eval: conv + sigmoid + soft and hard sums + finalize / accumulate) against n3d_head_fwd's Dice
mode on the same head input, priced by its bytes (head input + targets) over 8 TB/s.
    python tools/eval_probe.py [--reps N]"""
import argparse
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
sys.path.insert(0, os.path.join(R, "tests", "golden"))
import numpy as np
import torch

from nas_3d_unet_amd import kernels as K, unet
from nas_3d_unet_amd.train import Trainer, capture_stream
from test_gpu_nets import build_net

HBM = 8e12


def wall(fn, reps):
    """seconds per call of fn (host issue + device), synchronised at the end"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def graph_us(fn, iters=20, reps=5):
    """device microseconds per call of fn, timed as a captured graph of `iters` calls"""
    s = capture_stream(torch.device("cuda", 0))
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            for _ in range(iters):
                fn()
    g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * iters)


def case(size, storage, reps, batch=2):
    rng = np.random.default_rng(size)
    x = torch.from_numpy(rng.standard_normal((batch, 4, size, size, size)).astype(np.float32)).cuda()
    t = torch.from_numpy((rng.uniform(0, 1, (batch, 3, size, size, size)) < 0.3).astype(np.float32)).cuda()
    net, _ = build_net("searched", "G_CONV", 4, keep_dropout=True)
    tr = Trainer(net, graph=True, storage=storage)
    tr.step(x, t)
    tr.evaluate(x, t)
    t_eval = wall(lambda: tr.evaluate(x, t), reps)
    tr.eval_result(reset=True)

    def eager():
        net.eval()
        with torch.no_grad():
            loss, _ = net.forward_loss(x, t)
        float(loss)
        net.train()
    t_eager = wall(eager, reps)
    t_step = wall(lambda: tr.step(x, t), reps)
    # the evaluation head alone, on the head input of this net (node-planar, as the trainers run it)
    net.eval()
    with torch.no_grad():
        body = unet.body(net, x, None, planar=unet._head_takes_planar(net))
    net.train()
    op = net.last_conv[0]
    xv = K.as_planar(body, "head input") if body.dim() == 6 else K.as_view(body, "head input", bf16_ok=True)
    acc = K.eval_acc(3, x.device)
    us_eval = graph_us(lambda: K.head_eval(xv, op.conv.weight, op.conv.bias, t, acc))
    us_fwd = graph_us(lambda: K.head_fwd(xv, op.conv.weight, op.conv.bias, None, t, want_p=False))
    esz = 2 if body.dtype == torch.bfloat16 else 4
    nbytes = batch * size ** 3 * (xv.C * esz + 3 * 4)
    name = "%s 4x%d^3 B=%d" % (storage, size, batch)
    print("%-18s evaluate() replay %7.3f ms | eager eval + sync %7.3f ms (%.2fx) | step() %7.3f ms (eval/step %.3f)"
          % (name, t_eval * 1e3, t_eager * 1e3, t_eager / t_eval, t_step * 1e3, t_eval / t_step), flush=True)
    print("%-18s head_eval %7.2f us = %.3f of %d B / 8 TB/s (floor %.2f us) | head_fwd Dice mode %7.2f us (eval/fwd %.3f)"
          % (name, us_eval, nbytes / HBM * 1e6 / us_eval, nbytes, nbytes / HBM * 1e6, us_fwd, us_eval / us_fwd), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0))
    for size, storage in ((64, "fp32"), (128, "fp32"), (128, "bf16")):
        case(size, storage, a.reps)
