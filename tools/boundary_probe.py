"""What loss.BoundaryLoss costs: the signed distance maps of a target batch (n3d_target_sdt) alone, and one Trainer.step() with and
without the boundary term.
  * n3d_target_sdt at 2 x 3 x 64^3 and 2 x 3 x 128^3, device time from captured graphs of 20 calls, on tumour-like targets (a blob
    with nested regions WT > TC > ET plus 1 % speckle in WT; float and byte storage) and on the two extremes of the walk -- empty maps
    (every column answered from its flag, no walk) and 30 % speckle (every walk ends after a step or two).  The variants ALTERNATE
    round by round; the log gives each one's median with its spread (min .. max).  Beside it: the bytes the three launches must move
    as time at 8 TB/s, the min-steps a brute-force line pass would take (2 fields x D1 + 1 x D0 per voxel) as time at the rate
    profiles/metrics_probe.log measured for that loop (0.13 G min-steps in 61 us), and a lower bound of the min-steps the bounded
    walk of the LAST pass takes (2 per step, ceil(sqrt(d2)) - 1 steps per voxel, from the finished map);
  * one replayed Trainer.step() at 4 x 64^3 and 4 x 128^3, B = 2: the default loss (launch for launch the parent commit's step: the
    default path runs no code this loss adds), TverskyBCELoss(bce_weight=0.5), and BoundaryLoss on either -- alternating the same
    way, each as a ratio to the default step of the same process;
  * with --parent DIR (a built checkout of the parent commit): the library calls of one eager default step in both trees (the
    launches the captured step holds), and `python bench.py` of this tree and of the parent, alternating.
Writes profiles/boundary_probe.log (or --out).
    python tools/boundary_probe.py [--rounds N] [--out FILE] [--parent DIR]"""
import argparse
import collections
import json
import os
import statistics
import subprocess
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
sys.path.insert(0, os.path.join(R, "tests", "golden"))
sys.path.insert(0, os.path.join(R, "tools"))

HBM = 8e12
MINSTEPS_PER_S = 0.13e9 / 61e-6      # profiles/metrics_probe.log: seg_edt_line_kernel, 0.13 G min-steps in 61 us
LINES = []

# the default step's library calls, run in either tree (the parent has no tools/boundary_probe.py): prints one JSON line
COUNT_SCRIPT = r"""
import collections, json, os, sys
R = os.getcwd()
for p in (R, os.path.join(R, "tests"), os.path.join(R, "tests", "golden"), os.path.join(R, "tools")):
    sys.path.insert(0, p)
import numpy as np, torch
import kernel_table
from nas_3d_unet_amd.train import Trainer
from test_gpu_nets import build_net
rng = np.random.default_rng(64)
x = torch.from_numpy(rng.standard_normal((2, 4, 64, 64, 64)).astype(np.float32)).cuda()
t = torch.from_numpy((rng.uniform(0, 1, (2, 3, 64, 64, 64)) < 0.3).astype(np.float32)).cuda()
net, _ = build_net("searched", "G_CONV", 4, keep_dropout=True)
tr = Trainer(net, graph=False, side_wgrad=False)
for _ in range(2):
    tr.step(x, t)
with kernel_table.Recorder() as r:
    tr.step(x, t)
torch.cuda.synchronize()
c = collections.Counter(n for n, _ in r.calls)
print(json.dumps({"calls": len(r.calls), "head": {k: v for k, v in sorted(c.items()) if "head" in k or "sdt" in k or "dice" in k}}))
"""


def say(s):
    print(s, flush=True)
    LINES.append(s)


def fmt(v, digits=2):
    return "%8.*f (%.*f .. %.*f)" % (digits, statistics.median(v), digits, min(v), digits, max(v))


def parent_series(parent, rounds):
    """library calls of one eager default step in both trees, then `python bench.py --gpus 1` of both, alternating, each in a fresh process"""
    counts = {}
    for name, root in (("parent", parent), ("branch", R)):
        out = subprocess.run([sys.executable, "-c", COUNT_SCRIPT], cwd=root, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            raise SystemExit("the launch count failed in %s (exit %d): %s" % (root, out.returncode, out.stderr[-2000:]))
        counts[name] = json.loads(out.stdout.strip().splitlines()[-1])
    say("library calls of one eager default step (fp32 4x64^3 B=2, one stream: what the captured step holds), and those of the head among them")
    for name in ("parent", "branch"):
        say("    %-7s %d calls   %s" % (name, counts[name]["calls"], counts[name]["head"]))
    series = {"branch": [], "parent": []}
    for _ in range(rounds):
        for name, root in (("parent", parent), ("branch", R)):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "60", "--warmup", "10"], cwd=root, capture_output=True,
                                 text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit("bench.py failed in %s (exit %d): %s" % (root, out.returncode, out.stderr[-2000:]))
            line = json.loads(out.stdout.strip().splitlines()[-1])
            series[name].append((line["ms_per_step"], line["config"]["schedule"], line["config"]["final_loss"]))
            print("    bench %s: %.3f ms" % (name, line["ms_per_step"]), flush=True)
    say("bench.py --gpus 1 --steps 60 --warmup 10, ms_per_step, %d alternating rounds (parent first in each round)" % rounds)
    for name in ("parent", "branch"):
        ms = [m for m, _, _ in series[name]]
        say("    %-7s %s   series %s   schedules %s   final_loss %s" % (name, fmt(ms, 3), ms, sorted({s for _, s, _ in series[name]}), sorted({l for _, _, l in series[name]})))


def main(a):
    if a.parent:
        parent_series(a.parent, max(3, a.rounds // 3))       # (first: this process has not opened the GPU yet)
    import numpy as np
    import torch

    import kernel_table
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd.loss import BoundaryLoss, TverskyBCELoss
    from nas_3d_unet_amd.train import Trainer, capture_stream
    from test_gpu_nets import build_net

    def graph_of(fn, iters):
        s = capture_stream(torch.device("cuda", 0))
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                for _ in range(iters):
                    fn()
        g.replay()
        torch.cuda.synchronize()
        return g

    def replay_us(g, iters, reps=5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (reps * iters)

    def tumour(size, batch, seed, dtype):
        """blob plus speckle, nested regions: WT > TC > ET around one centre per sample, 1 % speckle in WT"""
        gen = torch.Generator(device="cuda").manual_seed(seed)
        ax = torch.arange(size, device="cuda", dtype=torch.float32)
        t = torch.zeros((batch, 3, size, size, size), device="cuda", dtype=torch.bool)
        for b in range(batch):
            c = (0.3 + 0.4 * torch.rand(3, device="cuda", generator=gen)) * size
            r2 = (ax[:, None, None] - c[0]) ** 2 + (ax[None, :, None] - c[1]) ** 2 + (ax[None, None, :] - c[2]) ** 2
            for k, frac in enumerate((0.3, 0.2, 0.11)):
                t[b, k] = r2 <= (frac * size) ** 2
            t[b, 0] |= torch.rand((size,) * 3, device="cuda", generator=gen) < 0.01
        return t.to(dtype)

    def sdt_case(size, rounds, batch=2, iters=20):
        shape = (batch, 3, size, size, size)
        gen = torch.Generator(device="cuda").manual_seed(size)
        variants = [("tumour-like, float", tumour(size, batch, size, torch.float32)), ("tumour-like, bytes", tumour(size, batch, size, torch.uint8)),
                    ("empty maps, float", torch.zeros(shape, device="cuda")),
                    ("30 % speckle, float", (torch.rand(shape, device="cuda", generator=gen) < 0.3).float())]
        out = torch.empty(shape, device="cuda")
        graphs = [(n, t, graph_of(lambda t=t: K.target_sdt(t, out=out), iters)) for n, t in variants]
        times = {n: [] for n, _ in variants}
        for _ in range(rounds):
            for n, _, g in graphs:
                times[n].append(replay_us(g, iters))
        vox = batch * 3 * size ** 3
        brute = vox * 3 * size
        say("n3d_target_sdt %d x 3 x %d^3 (3 launches), us, median (min .. max) of %d alternating rounds of %d calls; a brute-force line pass: "
            "%.3f G min-steps = %.1f us at the metrics loop's rate" % (batch, size, rounds, iters, brute / 1e9, brute / MINSTEPS_PER_S * 1e6))
        for n, t, _ in graphs:
            phi = K.target_sdt(t).double()
            d2 = torch.where(t != 0, (1.0 - phi) ** 2, phi ** 2).round()
            d2 = torch.where((phi == 0) & (t != 0), torch.zeros_like(d2), d2)      # (a full map: no source, no walk)
            last = float((2.0 * (torch.sqrt(d2).ceil() - 1).clamp(min=0)).sum())
            nbytes = vox * (t.element_size() + 36)
            say("    %-20s %s | moves %d B: %.1f us at 8 TB/s | last pass >= %.4f G min-steps (%.1f us at that rate), %.1f %% foreground"
                % (n, fmt(times[n]), nbytes, nbytes / HBM * 1e6, last / 1e9, last / MINSTEPS_PER_S * 1e6, 100.0 * float((t != 0).float().mean())))

    def step_case(size, rounds, reps=20, batch=2):
        rng = np.random.default_rng(size)
        x = torch.from_numpy(rng.standard_normal((batch, 4, size, size, size)).astype(np.float32)).cuda()
        t = tumour(size, batch, size + 1, torch.float32)
        tv = lambda: TverskyBCELoss(0.3, 0.7, 0.75, 0.5)
        trs = []
        for name, loss in (("default (Dice)", None), ("TverskyBCELoss(0.3, 0.7, 0.75, 0.5)", tv()), ("BoundaryLoss(that TverskyBCELoss, 0.01)", BoundaryLoss(tv(), 0.01)),
                           ("BoundaryLoss(None, 0.01)", BoundaryLoss(None, 0.01))):
            net, _ = build_net("searched", "G_CONV", 4, keep_dropout=True)
            tr = Trainer(net, graph=True, loss=loss)
            for _ in range(5):
                tr.step(x, t)
            trs.append((name, tr))
        times = {n: [] for n, _ in trs}
        for _ in range(rounds):
            for n, tr in trs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    tr.step(x, t)
                torch.cuda.synchronize()
                times[n].append((time.perf_counter() - t0) / reps * 1e3)
        base = statistics.median(times["default (Dice)"])
        say("Trainer.step() fp32 4x%d^3 B=%d, tumour-like float targets, replayed, ms, median (min .. max) of %d alternating rounds of %d steps" % (size, batch, rounds, reps))
        for n, tr in trs:
            say("    %-42s %s  x%.3f of the default step   schedule: %s" % (n, fmt(times[n], 3), statistics.median(times[n]) / base,
                                                                             "side-stream" if tr._use_side else "single stream"))

    def call_case():
        """library calls of one eager step, default loss against the boundary loss: what the term adds to the captured step"""
        rng = np.random.default_rng(64)
        x = torch.from_numpy(rng.standard_normal((2, 4, 64, 64, 64)).astype(np.float32)).cuda()
        t = tumour(64, 2, 65, torch.float32)
        res = []
        for name, loss in (("default (Dice)", None), ("BoundaryLoss(TverskyBCELoss(bce_weight=0.5), 0.01)", BoundaryLoss(TverskyBCELoss(bce_weight=0.5), 0.01))):
            net, _ = build_net("searched", "G_CONV", 4, keep_dropout=True)
            tr = Trainer(net, graph=False, side_wgrad=False, loss=loss)
            for _ in range(2):
                tr.step(x, t)
            with kernel_table.Recorder() as r:
                tr.step(x, t)
            torch.cuda.synchronize()
            c = collections.Counter(n for n, _ in r.calls)
            res.append((name, len(r.calls), {k: v for k, v in sorted(c.items()) if "head" in k or "sdt" in k}))
        say("library calls of one eager step, fp32 4x64^3 B=2, one stream (n3d_target_sdt is three launches, a head forward two)")
        for name, n, head in res:
            say("    %-52s %d calls   %s" % (name, n, head))

    say("device: %s" % torch.cuda.get_device_name(0))
    for size in (64, 128):
        sdt_case(size, a.rounds)
    call_case()
    for size in (64, 128):
        step_case(size, a.rounds)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "boundary_probe.log"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: launch counts and bench.py of both trees, alternating")
    main(ap.parse_args())
