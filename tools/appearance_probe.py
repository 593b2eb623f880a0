"""What the appearance transforms cost beside the gather that feeds them: n3d_patch_appearance with ONE stage active on every patch
(noise; blur at radius 2, 4 and 6; contrast; gamma) and with all four, against the plain n3d_patch_gather of the same batch, each timed
as a captured graph of 20 calls, alternating in one process (rounds over all configurations), at 2 x 4 x 64^3 and 2 x 4 x 128^3 out of
two 140 x 170 x 140 boxes whose inner ellipsoid is brain (about half of the patch's voxels are masked).  Every appearance call
includes its mask launch; the stages are idempotent enough to be replayed on the same buffer (noise is re-gathered first in the
"gather+all" row only).  Next to each time: the bytes the stage must move -- the mask launch reads the batch and writes a byte per
voxel; every further launch reads the mask and the batch, the ones that store also write the masked share; the blur writes its fp32
result and lands the masked share -- as microseconds at 8 TB/s, and the launches it takes.
    python tools/appearance_probe.py [--out FILE] [--rounds N]"""
import argparse
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from nas_3d_unet_amd import _lib, generator as G
from nas_3d_unet_amd import kernels as K
from nas_3d_unet_amd.appearance import Appearance
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
    log("appearance_probe: %s, %d rounds, graphs of 20 calls" % (torch.cuda.get_device_name(0), args.rounds))
    s = G.VolumeSet(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    shape = (140, 170, 140)
    g = torch.meshgrid(*[torch.arange(n, device=dev, dtype=torch.float32) for n in shape], indexing="ij")
    brain = sum(((g[a] - shape[a] / 2) / (0.45 * shape[a])) ** 2 for a in range(3)) <= 1
    for i in range(2):
        vol = torch.randn((4,) + shape, generator=gen, device=dev) * brain
        s.add(vol, None)
    a = Appearance()
    for P in (64, 128):
        refs = [(0, (30, 40, 5), None), (1, (3, 1, 7), None)]
        x = K.empty_ndhwc(2, 4, P, P, P, dev, torch.float32)
        s.patch_batch(refs, P, out=(x, None))
        masked = float((x != 0).float().mean())
        sig = {2: 0.5, 4: 1.0, 6: 1.5}
        one = {
            "noise": dict(noise=(0.1, (1, 2))),
            "blur r=2": dict(blur=np.full(4, sig[2])), "blur r=4": dict(blur=np.full(4, sig[4])), "blur r=6": dict(blur=np.full(4, sig[6])),
            "contrast": dict(contrast=np.full(4, 1.2)),
            "gamma": dict(gamma=np.full(4, 0.9)),
            "all four": dict(noise=(0.1, (1, 2)), blur=np.full(4, sig[4]), contrast=np.full(4, 1.2), gamma=np.full(4, 0.9)),
        }
        n = 2 * 4 * P ** 3
        rd, wr, mk = 4 * n, 4 * n * masked, n // 4             # the batch read once, its masked share written once, the mask bytes
        first, rdl = rd + mk, mk + rd                           # the mask launch; a launch that reads the mask and the batch
        must = {"noise": first + rdl + wr, "contrast": first + 2 * rdl + wr, "gamma": first + 4 * rdl + 2 * wr}
        for k in ("blur r=2", "blur r=4", "blur r=6"):          # reads x (the halo re-reads not counted), writes fp32, lands the masked share
            must[k] = first + rd + 4 * n + mk + 2 * wr
        must["all four"] = must["noise"] + must["blur r=4"] + must["contrast"] + must["gamma"] - 3 * first
        launches = {"noise": 2, "blur r=2": 3, "blur r=4": 3, "blur r=6": 3, "contrast": 3, "gamma": 5, "all four": 10}
        graphs = {"gather": make_graph(lambda: s.patch_batch(refs, P, out=(x, None)))}
        for k, d in one.items():
            graphs[k] = make_graph(lambda d=d: a.apply(x, [d, d]))
        graphs["gather+all"] = make_graph(lambda: a.apply(s.patch_batch(refs, P, out=(x, None))[0], [one["all four"]] * 2))
        res = {k: [] for k in graphs}
        for _ in range(args.rounds):
            s.patch_batch(refs, P, out=(x, None))               # every round starts from the gathered batch
            for k, gr in graphs.items():
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
