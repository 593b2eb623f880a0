"""What the elastic deformation costs inside the patch gather: n3d_patch_gather_elastic against n3d_patch_gather_warp on the SAME refs
(volume, corner, isometry key), each timed as a captured graph of 20 launches, alternating in one process (rounds over all
configurations), at 2 x 4 x 64^3 and 2 x 4 x 128^3 out of two 140 x 170 x 140 boxes.  Configurations:
    warp-near   n3d_patch_gather_warp, no rotation, nearest neighbour (the baseline of the nearest rows)
    warp-lin    n3d_patch_gather_warp, no rotation, linear interpolation (the baseline of the linear rows)
    off-near    n3d_patch_gather_elastic with `elastic` clear on both patches: the warp kernel's work behind the new entry point
    off-lin     the same, linear interpolation
    c4-near     cells 4 (a 7^3 lattice), lock 2, displacement 4 voxels, nearest neighbour
    c4-lin      the same, linear interpolation
    c8-lin      cells 8 (an 11^3 lattice: 1331 Philox blocks per workgroup), lock 2, displacement 3 voxels, linear interpolation
What is reported is the time per launch, median and min .. max over the rounds, and the ratio to the warp launch of the same
interpolation order, next to the share of a 1.63 ms training step (README) the launch amounts to.
    python tools/elastic_probe.py [--out FILE] [--rounds N]"""
import argparse
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from nas_3d_unet_amd import _lib, generator as G
from nas_3d_unet_amd import kernels as K
from warp_probe import make_graph, replay_us

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
    log("elastic_probe: %s, %d rounds, graphs of 20 launches" % (torch.cuda.get_device_name(0), args.rounds))
    s = G.VolumeSet(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    for i in range(2):
        vol = torch.randn((4, 140, 170, 140), generator=gen, device=dev)
        truth = torch.randint(0, 5, (140, 170, 140), generator=gen, device=dev).to(torch.uint8)
        truth[truth == 3] = 0
        s.add(vol, truth)
    key = ((0, 1), 0, 1, 0, 1)
    lib = _lib.load()
    for P in (64, 128):
        refs = [(0, (30, 40, 5), key), (1, (3, 1, 7), None)]                    # inside their boxes at 64^3; 128^3 hangs over the high faces
        bufs = (K.empty_ndhwc(2, 4, P, P, P, dev, torch.float32), torch.empty((2, 3, P, P, P), device=dev))
        xv = K.as_view(bufs[0])

        def off(order):
            """the elastic entry point with `elastic` clear everywhere: patch_batch would take the warp launch for such a batch"""
            descs = s._elastic_descs(refs, P, None, [(None, order, None, None)] * 2, [(4, 2, (1, 2), 4.0)] * 2)
            for d in descs:
                d.elastic = 0
            return lambda: _lib.check(lib.n3d_patch_gather_elastic(K.ptr(s.records), len(s), 4, descs, 2, P, 0, xv.p, xv.ld, K.ptr(bufs[1]),
                                                                   K.stream_ptr()), "n3d_patch_gather_elastic")

        def batch(order, elastic=None):
            kw = dict(warp=[(None, order, None, None)] * 2, elastic=elastic)
            return lambda: s.patch_batch(refs, P, out=bufs, **kw)

        c4 = [(4, 2, (0x243F6A88, 0x85A308D3), 4.0), (4, 2, (0x13198A2E, 0x03707344), 4.0)]
        c8 = [(8, 2, (0x243F6A88, 0x85A308D3), 3.0), (8, 2, (0x13198A2E, 0x03707344), 3.0)]
        configs = {"warp-near": batch(0), "warp-lin": batch(1), "off-near": off(0), "off-lin": off(1), "c4-near": batch(0, c4),
                   "c4-lin": batch(1, c4), "c8-lin": batch(1, c8)}
        graphs = {k: make_graph(fn) for k, fn in configs.items()}
        x0 = s.patch_batch(refs, P, warp=[(None, 0, None, None)] * 2)[0]
        x1 = s.patch_batch(refs, P, warp=[(None, 0, None, None)] * 2, elastic=c4)[0]
        log("  P %d cells 4, displacement 4: %.1f %% of the voxels take another source voxel than without the field" % (
            P, 100.0 * float((x0 != x1).any(dim=1).float().mean())))
        res = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, g in graphs.items():
                res[k].append(replay_us(g))
        log("2 x 4 x %d^3 (fp32 targets):" % P)
        for k, v in res.items():
            base = res["warp-near" if k.endswith("near") else "warp-lin"]
            ratios = [a / b for a, b in zip(v, base)]
            med = float(np.median(v))
            share = "   %.2f %% of the 1.63 ms step" % (100.0 * med / STEP_US) if P == 64 else ""      # the README's step is 2 x 4 x 64^3
            log("  %-9s %7.1f us (min %.1f .. max %.1f)   ratio to the warp launch: median %.3f (min %.3f .. max %.3f)%s" % (
                k, med, min(v), max(v), float(np.median(ratios)), min(ratios), max(ratios), share))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
