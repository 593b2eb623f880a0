"""What drawing crops on the device costs: the line index of a volume (n3d_volume_line_index, once per volume) beside the summed-area
tables of the same volume (n3d_volume_sat, what VolumeSet.add already pays), and the epoch's sample launch (n3d_patch_sample) beside
the qualification of the same candidates (n3d_patch_qualify, what every epoch already pays).  Each call is timed as a captured graph
of 20 launches; the members of a pair alternate round by round in one process.  Subjects are synthetic: an ellipsoid of nonzero data
(the brain, 52 % of a box) with a tumour-sized ellipsoid of labels 2 > 1 > 4 nested in it, boxes 193 x 193 x 126 (a typical
brain-wise box) and 240 x 240 x 155 (a whole BraTS image).  The sampler draws N = 1024 crops of 128^3 from both subjects for the masks
("tumour",) and (1, 2, 4) at foreground 0, 1/3 and 1.  Reported: the time per launch, median and min .. max over the rounds, and the
ratio to the launch beside it.
    python tools/sample_probe.py [--out FILE] [--rounds N]"""
import argparse
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from nas_3d_unet_amd import _lib, generator as G, sampling
from nas_3d_unet_amd import kernels as K
from warp_probe import make_graph, replay_us

LINES = []


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def subject(shape, dev, gen):
    g = torch.meshgrid(*[torch.linspace(-1, 1, n, device=dev) for n in shape], indexing="ij")
    r2 = g[0] ** 2 + g[1] ** 2 + g[2] ** 2
    t2 = ((g[0] - 0.3) / 0.28) ** 2 + ((g[1] + 0.2) / 0.3) ** 2 + (g[2] / 0.4) ** 2
    vol = torch.randn((4,) + shape, generator=gen, device=dev) * (r2 < 1.0)
    truth = torch.zeros(shape, dtype=torch.uint8, device=dev)
    truth[t2 < 1.0] = 2
    truth[t2 < 0.45] = 1
    truth[t2 < 0.2] = 4
    return vol, truth


def report(name, v, base_name, base):
    ratios = [a / b for a, b in zip(v, base)]
    log("  %-28s %8.1f us (min %.1f .. max %.1f)   ratio to %s: median %.3f (min %.3f .. max %.3f)" % (
        name, float(np.median(v)), min(v), max(v), base_name, float(np.median(ratios)), min(ratios), max(ratios)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    _lib.require_device()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    log("sample_probe: %s, %d rounds, graphs of 20 launches" % (torch.cuda.get_device_name(0), args.rounds))
    s = G.VolumeSet(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    for shape in ((193, 193, 126), (240, 240, 155)):
        i = s.add(*subject(shape, dev, gen))
        X, Y, Z = shape
        vol, truth, sat = s.volumes[i], s.truths[i], s.tables[i]
        index = torch.empty((len(sampling.MASKS), X * Y + 1), dtype=torch.int32, device=dev)

        def build_index():
            _lib.check(lib.n3d_volume_line_index(K.ptr(vol), 4, K.ptr(truth), X, Y, Z, K.ptr(index), K.stream_ptr()), "n3d_volume_line_index")

        def build_sat():
            _lib.check(lib.n3d_volume_sat(K.ptr(vol), 4, K.ptr(truth), X, Y, Z, K.ptr(sat), K.stream_ptr()), "n3d_volume_sat")

        graphs = {"index": make_graph(build_index), "sat": make_graph(build_sat)}
        assert torch.equal(index, s.line_index(i))
        res = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, g in graphs.items():
                res[k].append(replay_us(g))
        totals = index[:, -1].tolist()
        log("subject %d x %d x %d, 4 channels: %d lines, mask totals brain %d (%.0f %%), tumour %d, labels 1 / 2 / 4: %d / %d / %d" % (
            X, Y, Z, X * Y, totals[0], 100.0 * totals[0] / (X * Y * Z), totals[1], totals[2], totals[3], totals[4]))
        log("  volume read %.1f MB, index written %.2f MB, tables written %.1f MB" % (
            X * Y * Z * 17 / 1e6, index.numel() * 4 / 1e6, sat.numel() * 4 / 1e6))
        report("n3d_volume_sat", res["sat"], "itself", res["sat"])
        report("n3d_volume_line_index", res["index"], "n3d_volume_sat", res["sat"])
    N, P, key = 1024, 128, (0x243F6A88, 0x85A308D3)
    ids = torch.tensor([0, 1], dtype=torch.int32).to(dev)
    table = s.index_table()
    log("n3d_patch_sample, N = %d crops of %d^3 from both subjects, beside n3d_patch_qualify of the same candidates:" % (N, P))
    for masks in (("tumour",), (1, 2, 4)):
        for fg in (0.0, 1 / 3, 1.0):
            bits, thr = sampling.mask_bits(masks), sampling.fg_threshold(fg)
            cand = torch.empty((N, 4), dtype=torch.int32, device=dev)
            mode = torch.empty(N, dtype=torch.uint8, device=dev)
            flags = torch.empty(N, dtype=torch.uint8, device=dev)

            def sample():
                _lib.check(lib.n3d_patch_sample(K.ptr(s.records), K.ptr(table), len(s), 4, K.ptr(ids), 2, N, P, key[0], key[1], thr, bits,
                                                K.ptr(cand), K.ptr(mode), K.stream_ptr()), "n3d_patch_sample")

            def qualify():
                _lib.check(lib.n3d_patch_qualify(K.ptr(s.records), len(s), K.ptr(cand), N, P, K.ptr(flags), K.stream_ptr()), "n3d_patch_qualify")

            graphs = {"sample": make_graph(sample), "qualify": make_graph(qualify)}
            res = {k: [] for k in graphs}
            for _ in range(args.rounds):
                for k, g in graphs.items():
                    res[k].append(replay_us(g))
            m = mode.cpu().numpy()
            log("  masks %-12s foreground %.3f: %d foreground-centred, %d uniform, %d fallback; %d of %d kept by the filters" % (
                masks, fg, int((m < 5).sum()), int((m == 255).sum()), int((m == 254).sum()), int((flags == 3).sum()), N))
            report("  n3d_patch_qualify", res["qualify"], "itself", res["qualify"])
            report("  n3d_patch_sample", res["sample"], "n3d_patch_qualify", res["qualify"])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
