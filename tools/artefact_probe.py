"""What the artefact transforms cost beside the gather that feeds them: n3d_patch_artefact with ONE stage active on every patch (low
resolution at n = P / 2 and at n = 3 P / 4 on every channel; the bias field at order 3; dropout of one channel) and with all
three, against the plain n3d_patch_gather of the same batch, each timed as a captured graph of 20 calls, alternating in one process
(rounds over all configurations), at 2 x 4 x 64^3 and 2 x 4 x 128^3 out of two 140 x 170 x 140 boxes whose inner ellipsoid is brain
(about half of the patch's voxels are masked).  Every artefact call includes its mask launch.  The stages are replayed on the
same buffer: low resolution keeps smoothing it and the bias field (a small range here) keeps scaling it, neither of which changes
the work; a dropped channel has no masked voxel from the second call on, so "all three" is also timed behind a fresh gather
("gather+all").  Next to each time: the bytes the stage must move -- the mask launch reads the batch and writes a byte per voxel; the
low-resolution launch reads the (n / P)^3 of the batch its taps touch and writes 4 bytes per voxel and channel, its landing launch
reads the mask, that output and the batch and writes the masked share; the bias launch reads the mask and the batch and writes the
masked share; dropout writes the channel -- as microseconds at 8 TB/s, and the launches it takes.
    python tools/artefact_probe.py [--out FILE] [--rounds N]"""
import argparse
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from nas_3d_unet_amd import _lib, generator as G
from nas_3d_unet_amd import kernels as K
from nas_3d_unet_amd.artefact import Artefact
from warp_probe import make_graph, replay_us

HBM = 8e12
STEP_US = 1630.0
LINES = []


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    _lib.require_device()
    dev = torch.device("cuda", 0)
    log("artefact_probe: %s, %d rounds, graphs of 20 calls" % (torch.cuda.get_device_name(0), args.rounds))
    s = G.VolumeSet(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    shape = (140, 170, 140)
    g = torch.meshgrid(*[torch.arange(n, device=dev, dtype=torch.float32) for n in shape], indexing="ij")
    brain = sum(((g[a] - shape[a] / 2) / (0.45 * shape[a])) ** 2 for a in range(3)) <= 1
    for i in range(2):
        vol = torch.randn((4,) + shape, generator=gen, device=dev) * brain
        s.add(vol, None)
    a = Artefact()
    for P in (64, 128):
        refs = [(0, (30, 40, 5), None), (1, (3, 1, 7), None)]
        x = K.empty_ndhwc(2, 4, P, P, P, dev, torch.float32)
        s.patch_batch(refs, P, out=(x, None))
        masked = float((x != 0).float().mean())
        drop = np.arange(4) == 2
        one = {
            "lowres 1/2": dict(lowres=np.full(4, 0.5)), "lowres 3/4": dict(lowres=np.full(4, 0.75)),
            "bias": dict(bias=(0.02, 3, (1, 2))),
            "dropout": dict(dropout=drop),
            "all three": dict(lowres=np.full(4, 0.5), bias=(0.02, 3, (1, 2)), dropout=drop),
        }
        n = 2 * 4 * P ** 3
        rd, wr, mk = 4 * n, 4 * n * masked, n // 4             # the batch read once, its masked share written once, the mask bytes
        first = rd + mk                                         # the mask launch
        low = lambda f: first + rd * f ** 3 + rd + (mk + 2 * rd + wr)
        must = {"lowres 1/2": low(0.5), "lowres 3/4": low(0.75), "bias": first + mk + rd + wr, "dropout": first + rd // 4}
        must["all three"] = must["lowres 1/2"] + must["bias"] + must["dropout"] - 2 * first - rd // 4      # dropout rides in the bias launch
        launches = {"lowres 1/2": 3, "lowres 3/4": 3, "bias": 2, "dropout": 2, "all three": 4}
        graphs = {"gather": make_graph(lambda: s.patch_batch(refs, P, out=(x, None)))}
        for k, d in one.items():
            graphs[k] = make_graph(lambda d=d: a.apply(x, [d, d]))
        graphs["gather+all"] = make_graph(lambda: a.apply(s.patch_batch(refs, P, out=(x, None))[0], [one["all three"]] * 2))
        res = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, gr in graphs.items():
                s.patch_batch(refs, P, out=(x, None))           # every graph starts from the gathered batch
                res[k].append(replay_us(gr))
        gbytes = 4 * n + 4 * n
        log("2 x 4 x %d^3, %.0f %% of the voxels masked; the gather moves %.1f MB = %.1f us at 8 TB/s" % (P, 100 * masked, gbytes / 1e6, gbytes / HBM * 1e6))
        for k, v in res.items():
            med = float(np.median(v))
            ratios = [p / q for p, q in zip(v, res["gather"])]
            extra = ""
            if k in must:
                extra = "   must move %.1f MB = %.1f us at 8 TB/s (x %.1f), %d launches" % (must[k] / 1e6, must[k] / HBM * 1e6, med / (must[k] / HBM * 1e6), launches[k])
            share = "   %.2f %% of the 1.63 ms step" % (100.0 * med / STEP_US) if P == 64 else ""
            log("  %-10s %7.1f us (min %.1f .. max %.1f)   ratio to the gather: median %.2f%s%s" % (
                k, med, min(v), max(v), float(np.median(ratios)), extra, share))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
