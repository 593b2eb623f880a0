"""What the lesion-wise scores of one subject cost (nas_3d_unet_amd.metrics.score_lesions) on a synthetic 240x240x155 pair built like
tools/postprocess_probe.py's: the prediction is a tumour-sized blob (nested balls of radius 20 / 14 / 8 voxels) plus a few hundred
speckle components, the truth the same blob two voxels off plus a second, smaller lesion the prediction misses.  The phases of
n3d_lw_score are timed as captured graphs of repeated calls of the phases 0 .. k (a phase needs the ones before it), a phase's
time being the difference of two such graphs, medians of 9 rounds; next to it the bytes it must move at 8 TB/s.  Then the whole
score_lesions call by the wall clock and, where scipy imports, the same record from the scipy restatement
(tests/golden/make_golden_lesion.py) on the host.  No threshold is set: nobody has measured these before.
    python tools/lesion_probe.py [--out profiles/lesion_probe.log] [--no-scipy]"""
import argparse
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from nas_3d_unet_amd import _lib, metrics as M

HBM = 8e12
SHAPE = (240, 240, 155)
ROUNDS, ITERS = 9, 3
LINES = []
LISTS = 6 * 4 * M.LW_MAX_SURFACE
# bytes per voxel of the image every phase reads and writes whatever the labels are (foreground voxels add their neighbours',
# roots' and lists' words, through the cache); the dilation reads only the tiles that meet the truth's box
TRAFFIC = {"init": (0, "the 14 KB record"), "region_bits": (4, "labels of both volumes read, region and surface bits written"),
           "select": (14, "bits read; mask, sizes, match masks written"), "label_pred": (17, "n3d_cc_label: three launches"),
           "dilate": (1, "mask written; read inside the truth's box only"), "label_truth": (17, "n3d_cc_label: three launches"),
           "roots": (4, "ids read"), "ranks": (0, "64 ids"), "match": (9, "both ids and bits read"), "components": (4, "ids read"),
           "surfaces": (1, "surface bits read"), "distances": (0, "the lists, n_truth x n_pred pairs"), "order": (0, "the lists, ~25 times")}


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def graph_us(fn):
    """device microseconds per call of fn: a captured graph of ITERS calls, the median of ROUNDS replays"""
    from nas_3d_unet_amd.train import capture_stream
    s = capture_stream(torch.device("cuda", 0))
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            for _ in range(ITERS):
                fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / ITERS)
    return float(np.median(ts))


def synthetic_pair(dev, seed=1):
    X, Y, Z = SHAPE
    gx, gy, gz = torch.meshgrid(*[torch.arange(n, device=dev, dtype=torch.float32) for n in SHAPE], indexing="ij")

    def balls(cx, cy, cz, radii):
        d = ((gx - cx) ** 2 + (gy - cy) ** 2 + (gz - cz) ** 2).sqrt()
        return torch.where(d <= radii[2], 4, torch.where(d <= radii[1], 1, torch.where(d <= radii[0], 2, 0))).to(torch.uint8)

    pred = balls(0.6 * X, 0.5 * Y, 0.5 * Z, (20, 14, 8))
    g = torch.Generator(device=dev).manual_seed(seed)
    u = torch.rand(SHAPE, generator=g, device=dev)
    pred = torch.where(u < 4e-5, torch.where(u < 1e-5, torch.full_like(pred, 4), torch.full_like(pred, 2)), pred)
    truth = torch.maximum(balls(0.6 * X + 2, 0.5 * Y, 0.5 * Z - 1, (20, 14, 8)), balls(0.25 * X, 0.3 * Y, 0.7 * Z, (7, 5, 3)))
    return pred.contiguous(), truth.contiguous()


def phase_name(k):
    return ("init", "region_bits")[k] if k < 2 else M.LW_REGION_PHASES[(k - 2) % len(M.LW_REGION_PHASES)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    from nas_3d_unet_amd.train import reserve_side_streams
    _lib.require_device()
    reserve_side_streams(dev)
    log("lesion_probe: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    pred, truth = synthetic_pair(dev)
    N = SHAPE[0] * SHAPE[1] * SHAPE[2]
    scores = M.score_lesions(pred, truth)          # allocates the scratch, warms up
    torch.cuda.synchronize()
    reps = 10
    t0 = time.perf_counter()
    for _ in range(reps):
        rec, _ = M.lesion_record(pred, truth)
    wall = (time.perf_counter() - t0) / reps
    ws = M._lesion_workspaces[(pred.device, SHAPE)]
    log("one subject, %dx%dx%d uint8 labels, dilation 3; scratch %.0f MB (%.1f B per voxel); graph-timed, %d calls per graph, medians of %d" % (
        SHAPE + (ws.buf.numel() / 1e6, ws.buf.numel() / N, ITERS, ROUNDS)))
    for r in M.REGIONS:
        s = scores[r]
        log("  %s: lesion-wise Dice %.6f, HD95 %.6f; %d lesions (%d kept, %d missed), %d false positives of %d voxels; surface distances per lesion %s" % (
            r, s["lesionwise_dice"], s["lesionwise_hausdorff95"], s["n_lesions"], s["n_kept"], s["n_fn"], s["n_fp"], s["fp_voxels"],
            [int(rec.reshape(3, -1)[M.REGIONS.index(r), M.LW_HEADER_WORDS + 9 * l + 5]) for l in range(s["n_lesions"])]))
    out = torch.empty(M.LW_REC_WORDS, dtype=torch.int64, device=dev)
    cum = [graph_us(lambda k=k: M.lesion_phases(pred, truth, first=0, last=k, rec=out)) for k in range(M.LW_PHASES)]
    assert np.array_equal(out.cpu().numpy(), rec)
    us = [cum[0]] + [cum[k] - cum[k - 1] for k in range(1, len(cum))]
    for k in range(M.LW_PHASES):
        name = phase_name(k)
        b, what = TRAFFIC[name]
        region = "" if k < 2 else M.REGIONS[(k - 2) // len(M.LW_REGION_PHASES)] + " "
        log("    %2d %-16s %8.1f us | %6.1f MB (%2d B per voxel: %s) -> %5.1f us at 8 TB/s" % (
            k, region + name, us[k], b * N / 1e6, b, what, b * N / HBM * 1e6))
    per_region = [sum(us[2 + 11 * r:2 + 11 * (r + 1)]) for r in range(3)]
    log("  all %d phases (47 launches) %.1f us: init + region bits %.1f, WT %.1f, TC %.1f, ET %.1f" % (
        M.LW_PHASES, cum[-1], us[0] + us[1], per_region[0], per_region[1], per_region[2]))
    log("  lesion_record by the wall clock (one host sync, the copy of the record): %.3f ms" % (wall * 1e3))
    try:
        if args.no_scipy:
            raise ImportError
        import scipy
        sys.path.insert(0, os.path.join(R, "tests", "golden"))
        from make_golden_lesion import scipy_record
    except ImportError:
        log("  scipy: not timed here")
    else:
        p, t = pred.cpu().numpy(), truth.cpu().numpy()
        t0 = time.perf_counter()
        ref, _ = scipy_record(p, t, None, 3)
        dt = time.perf_counter() - t0
        log("  scipy %s on the host, same record (binary_dilation, label, distance_transform_edt per lesion): %.2f s = %.0fx lesion_record; "
            "records %s" % (scipy.__version__, dt, dt / wall, "equal" if np.array_equal(ref, rec) else "DIFFER"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
