"""What rotation, linear interpolation and the intensity map cost inside the patch gather: n3d_patch_gather_warp against
n3d_patch_gather and n3d_patch_gather_aug on the SAME refs (volume, corner, isometry key), each timed as a captured graph of 20
launches, alternating in one process (rounds over all configurations), at 2 x 4 x 64^3 and 2 x 4 x 128^3 out of two 140 x 170 x 140
boxes.  Configurations:
    plain       n3d_patch_gather
    aug         n3d_patch_gather_aug, scale 1.25 and two flipped axes
    noop        n3d_patch_gather_warp with descriptors that change nothing (mode 0, A = 1, sh = 0, order 0, no intensity)
    lin         no rotation (mode 0, A = 1, sh = 0: every coordinate an integer, the eight taps are read along straight lines and seven
                of them weigh 0), linear interpolation: the cost of the taps without the slant
    rot-near    a rotation by (15, -15, 15) degrees about the patch centre (mode 1), nearest neighbour
    rot-lin     the same rotation, linear interpolation of the data (8 taps per channel)
    lin+int     the same, plus gain and bias on the nonzero voxels
What is reported is the ratio to the plain gather, median and min .. max over the rounds, next to the bytes of the batch at 8 TB/s
and the share of a 1.63 ms training step (README) the launch amounts to.
    python tools/warp_probe.py [--out FILE] [--rounds N]"""
import argparse
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from nas_3d_unet_amd import _lib, generator as G
from nas_3d_unet_amd import kernels as K

HBM = 8e12
STEP_US = 1630.0
LINES = []


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def make_graph(fn, iters=20):
    """a captured graph of `iters` calls of fn"""
    from nas_3d_unet_amd.train import capture_stream
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


def replay_us(g, iters=20, reps=5):
    """device microseconds per captured call: events around `reps` replays"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    _lib.require_device()
    dev = torch.device("cuda", 0)
    log("warp_probe: %s, %d rounds, graphs of 20 launches" % (torch.cuda.get_device_name(0), args.rounds))
    s = G.VolumeSet(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    for i in range(2):
        vol = torch.randn((4, 140, 170, 140), generator=gen, device=dev)
        truth = torch.randint(0, 5, (140, 170, 140), generator=gen, device=dev).to(torch.uint8)
        truth[truth == 3] = 0
        s.add(vol, truth)
    key = ((0, 1), 0, 1, 0, 1)
    gain, bias = np.array([1.05, 0.95, 1.1, 0.9]), np.array([0.1, -0.1, 0.05, -0.05])
    for P in (64, 128):
        refs = [(0, (30, 40, 5), key), (1, (3, 1, 7), None)]                    # inside their boxes at 64^3; 128^3 hangs over the high faces
        bufs = (K.empty_ndhwc(2, 4, P, P, P, dev, torch.float32), torch.empty((2, 3, P, P, P), device=dev))
        A, sh, identity = G.resample_params(np.eye(4), P, np.full(3, 1.25))
        matrix = G.warp_transform(np.ones(3), np.zeros(3), G.rotation_matrix((15.0, -15.0, 15.0)), P)
        configs = {
            "plain": dict(),
            "aug": dict(augment=[(A, sh, identity, [0, 2])] * 2),
            "noop": dict(warp=[(None, 0, None, None)] * 2),
            "lin": dict(warp=[(None, 1, None, None)] * 2),
            "rot-near": dict(warp=[(matrix, 0, None, None)] * 2),
            "rot-lin": dict(warp=[(matrix, 1, None, None)] * 2),
            "lin+int": dict(warp=[(matrix, 1, gain, bias)] * 2),
        }
        graphs = {k: make_graph(lambda kw=kw: s.patch_batch(refs, P, out=bufs, **kw)) for k, kw in configs.items()}
        x, _ = s.patch_batch(refs, P, **configs["rot-lin"])
        log("  P %d rotation (15, -15, 15) degrees: %.1f %% of the voxels have a source" % (P, 100.0 * float((x != 0).float().mean())))
        res = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, g in graphs.items():
                res[k].append(replay_us(g))
        wbytes = 2 * (4 + 3) * P ** 3 * 4
        rbytes = 2 * (4 * 4 + 1) * P ** 3
        log("2 x 4 x %d^3 (fp32 targets): %.1f MB written, at most %.1f MB of distinct source bytes read = %.1f us at 8 TB/s" % (
            P, wbytes / 1e6, rbytes / 1e6, (wbytes + rbytes) / HBM * 1e6))
        for k, v in res.items():
            ratios = [a / b for a, b in zip(v, res["plain"])]
            med = float(np.median(v))
            share = "   %.2f %% of the 1.63 ms step" % (100.0 * med / STEP_US) if P == 64 else ""      # the README's step is 2 x 4 x 64^3
            log("  %-9s %7.1f us (min %.1f .. max %.1f)   ratio to plain: median %.3f (min %.3f .. max %.3f)%s" % (
                k, med, min(v), max(v), float(np.median(ratios)), min(ratios), max(ratios), share))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
