"""What the scale / flip augmentation costs inside the patch gather: n3d_patch_gather_aug against n3d_patch_gather on the SAME refs
(volume, corner, isometry key), each timed as a captured graph of 20 launches, alternating in one process (rounds of plain / 0.75 /
1.0 / 1.25), at 2 x 4 x 64^3 and 2 x 4 x 128^3 out of two 140 x 170 x 140 boxes.  Scale 1.0 is a resampled patch whose coordinates
are the identity (A = 1: the fp64 arithmetic runs, the addresses are the plain gather's); scale 0.75 (A = 4/3) reads its lines
strided along z and leaves a border of zeros; scale 1.25 (A = 0.8) repeats source voxels and reads 0.8^3 of the source bytes.  What
is reported is the ratio to the plain gather, median and min .. max over the rounds, next to the bytes of the batch at 8 TB/s.
    python tools/augment_probe.py [--out FILE] [--rounds N]"""
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
    log("augment_probe: %s, %d rounds, graphs of 20 launches" % (torch.cuda.get_device_name(0), args.rounds))
    s = G.VolumeSet(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    for i in range(2):
        vol = torch.randn((4, 140, 170, 140), generator=gen, device=dev)
        truth = torch.randint(0, 5, (140, 170, 140), generator=gen, device=dev).to(torch.uint8)
        truth[truth == 3] = 0
        s.add(vol, truth)
    affine = np.eye(4)
    key = ((0, 1), 0, 1, 0, 1)
    for P in (64, 128):
        refs = [(0, (30, 40, 5), key), (1, (3, 1, 7), None)]                    # inside their boxes at 64^3; 128^3 hangs over the high faces
        bufs = (K.empty_ndhwc(2, 4, P, P, P, dev, torch.float32), torch.empty((2, 3, P, P, P), device=dev))
        graphs = {"plain": make_graph(lambda: s.patch_batch(refs, P, out=bufs))}
        for scale in (0.75, 1.0, 1.25):
            A, sh, identity = G.resample_params(affine, P, np.full(3, scale)) if scale != 1.0 else (np.ones(3), np.zeros(3), False)
            aug = [(A, sh, identity, [0, 2])] * 2
            graphs["%.2f" % scale] = make_graph(lambda aug=aug: s.patch_batch(refs, P, out=bufs, augment=aug))
            x, _ = s.patch_batch(refs, P, augment=aug)
            log("  P %d scale %.2f: A %s sh %s; %.1f %% of the voxels have a source" % (P, scale, A[0], sh[0], 100.0 * float((x != 0).float().mean())))
        res = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, g in graphs.items():
                res[k].append(replay_us(g))
        wbytes = 2 * (4 + 3) * P ** 3 * 4
        rbytes = 2 * (4 * 4 + 1) * P ** 3
        med = {k: float(np.median(v)) for k, v in res.items()}
        log("2 x 4 x %d^3 (fp32 targets): %.1f MB written, at most %.1f MB read = %.1f us at 8 TB/s" % (
            P, wbytes / 1e6, rbytes / 1e6, (wbytes + rbytes) / HBM * 1e6))
        for k, v in res.items():
            ratios = [a / b for a, b in zip(v, res["plain"])]
            log("  %-6s %7.1f us (min %.1f .. max %.1f)   ratio to plain: median %.3f (min %.3f .. max %.3f)" % (
                k, med[k], min(v), max(v), float(np.median(ratios)), min(ratios), max(ratios)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
