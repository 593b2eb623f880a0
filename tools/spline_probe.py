"""What cubic B-spline interpolation costs in the patch gather: n3d_patch_gather_spline (five launches: crop, three prefilter passes,
gather) against the single n3d_patch_gather_warp launch with linear interpolation on the SAME refs (volume, corner, isometry key) and
the same rotation, each timed as a captured graph of 20 calls, alternating in one process (rounds over all configurations), at
2 x 4 x 64^3 and 2 x 4 x 128^3 out of two 140 x 170 x 140 boxes.  Configurations:
    rot-near    n3d_patch_gather_warp, a rotation by (15, -15, 15) degrees about the patch centre, nearest neighbour
    rot-lin     the same, linear interpolation of the data (8 taps per channel)
    spline3     n3d_patch_gather_spline, the same rotation (64 fp64 taps per channel on prefiltered coefficients)
    spline3+el  the same with both patches deformed (cells 4)
    prefilter   n3d_spline_prefilter alone on the batch's 8 cubes: the three axis passes of spline3
The crop and the gather of spline3 are not reachable on their own through the C ABI: their sum is reported as spline3 - prefilter, per
round.  An fp32-coefficient variant would halve the gather's bytes but leave scipy's arithmetic; it is out of scope and not built.
Not a gate: no ratio is required of these numbers.
    python tools/spline_probe.py [--out FILE] [--rounds N]"""
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

LINES = []


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R, "profiles", "spline_probe.log"))
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    log("spline_probe: %s, %d rounds, graphs of 20 calls" % (torch.cuda.get_device_name(0), args.rounds))
    s = G.VolumeSet(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    for i in range(2):
        vol = torch.randn((4, 140, 170, 140), generator=gen, device=dev)
        truth = torch.randint(0, 5, (140, 170, 140), generator=gen, device=dev).to(torch.uint8)
        truth[truth == 3] = 0
        s.add(vol, truth)
    key = ((0, 1), 0, 1, 0, 1)
    for P in (64, 128):
        refs = [(0, (30, 40, 5), key), (1, (3, 1, 7), None)]                    # inside their boxes at 64^3; 128^3 hangs over the high faces
        bufs = (K.empty_ndhwc(2, 4, P, P, P, dev, torch.float32), torch.empty((2, 3, P, P, P), device=dev))
        matrix = G.warp_transform(np.ones(3), np.zeros(3), G.rotation_matrix((15.0, -15.0, 15.0)), P)
        el = [(4, 0, (11, 12), 0.4 * (P - 1) / 4), (4, 0, (13, 14), 0.4 * (P - 1) / 4)]
        raw = torch.randn((8, P, P, P), generator=gen, device=dev)
        coef = torch.empty((8, P, P, P), dtype=torch.float64, device=dev)
        configs = {
            "rot-near": lambda: s.patch_batch(refs, P, out=bufs, warp=[(matrix, 0, None, None)] * 2),
            "rot-lin": lambda: s.patch_batch(refs, P, out=bufs, warp=[(matrix, 1, None, None)] * 2),
            "spline3": lambda: s.patch_batch(refs, P, out=bufs, warp=[(matrix, 3, None, None)] * 2),
            "spline3+el": lambda: s.patch_batch(refs, P, out=bufs, warp=[(matrix, 3, None, None)] * 2, elastic=el),
            "prefilter": lambda: _lib.check(lib.n3d_spline_prefilter(K.ptr(raw), 8, P, K.ptr(coef), K.stream_ptr()), "n3d_spline_prefilter"),
        }
        graphs = {k: make_graph(fn) for k, fn in configs.items()}
        res = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, g in graphs.items():
                res[k].append(replay_us(g))
        res["crop+gather"] = [a - b for a, b in zip(res["spline3"], res["prefilter"])]
        log("2 x 4 x %d^3 (fp32 targets): scratch %.1f MB (12 bytes per voxel and channel)" % (
            P, lib.n3d_patch_spline_scratch_bytes(2, 4, P) / 1e6))
        for k, v in res.items():
            ratios = [a / b for a, b in zip(v, res["rot-lin"])]
            log("  %-11s %8.1f us (min %.1f .. max %.1f)   ratio to rot-lin: median %.2f (min %.2f .. max %.2f)" % (
                k, float(np.median(v)), min(v), max(v), float(np.median(ratios)), min(ratios), max(ratios)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
