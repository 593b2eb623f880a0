"""What scoring one predicted subject costs (nas_3d_unet_amd.metrics) on a synthetic 240x240x155 label volume with a tumour-sized
blob (truth: nested balls of radius 20 / 14 / 8 voxels; prediction: the same shifted by (3, -2, 2) and a little larger, plus a few
stray voxels): the four steps -- n3d_seg_regions, n3d_seg_edt (three launches), n3d_seg_sample, n3d_seg_order -- each timed as a
captured graph of repeated calls, the whole score_labels call by the wall clock (it ends in the subject's one host sync), and,
where scipy imports, the same numbers by scipy.ndimage on the host.  No threshold is set: nobody has measured these before.
    python tools/metrics_probe.py [--out profiles/metrics_probe.log]"""
import argparse
import ctypes as C
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from nas_3d_unet_amd import _lib, metrics as M
from nas_3d_unet_amd import kernels as K

HBM = 8e12
SHAPE = (240, 240, 155)
LINES = []


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def graph_us(fn, iters=20, reps=5):
    """device microseconds per call of fn, timed as a captured graph of `iters` calls (no host issue cost in the window)"""
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * iters)


def synthetic_labels(dev, seed=1):
    X, Y, Z = SHAPE
    gx, gy, gz = torch.meshgrid(*[torch.arange(n, device=dev, dtype=torch.float32) for n in SHAPE], indexing="ij")

    def balls(cx, cy, cz, scale):
        d = ((gx - cx) ** 2 + (gy - cy) ** 2 + (gz - cz) ** 2).sqrt() / scale
        return torch.where(d <= 8, 4, torch.where(d <= 14, 1, torch.where(d <= 20, 2, 0))).to(torch.uint8)

    truth = balls(0.6 * X, 0.5 * Y, 0.5 * Z, 1.0)
    pred = balls(0.6 * X + 3, 0.5 * Y - 2, 0.5 * Z + 2, 1.08)
    g = torch.Generator(device=dev).manual_seed(seed)
    stray = torch.rand(SHAPE, generator=g, device=dev) < 2e-5
    near = ((gx - 0.6 * X).abs() < 40) & ((gy - 0.5 * Y).abs() < 40) & ((gz - 0.5 * Z).abs() < 40)
    pred = torch.where(stray & near, torch.full_like(pred, 2), pred)
    return pred.contiguous(), truth.contiguous()


def scipy_scores(pred, truth):
    from scipy import ndimage
    st = ndimage.generate_binary_structure(3, 1)
    out = {}
    for name, labs in zip(M.REGIONS, ((1, 2, 4), (1, 4), (4,))):
        mp, mt = np.isin(pred, labs), np.isin(truth, labs)
        sp, stt = mp & ~ndimage.binary_erosion(mp, st, border_value=0), mt & ~ndimage.binary_erosion(mt, st, border_value=0)
        d = np.concatenate([ndimage.distance_transform_edt(~stt)[sp], ndimage.distance_transform_edt(~sp)[stt]])
        tp = int((mp & mt).sum())
        out[name] = (2 * tp / (int(mp.sum()) + int(mt.sum())), float(np.percentile(d, 95)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    from nas_3d_unet_amd.train import reserve_side_streams
    _lib.require_device()
    reserve_side_streams(dev)
    lib = _lib.load()
    log("metrics_probe: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    pred, truth = synthetic_labels(dev)
    X, Y, Z = SHAPE
    N = X * Y * Z
    scores = M.score_labels(pred, truth)          # allocates the scratch, warms up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 10
    for _ in range(reps):
        scores = M.score_labels(pred, truth)
    wall = (time.perf_counter() - t0) / reps
    ws = M._workspaces[(pred.device, SHAPE)]
    rec = ws.rec.cpu().numpy()
    bbox = rec[M.REC_BBOX:].view(np.int32).reshape(3, 6)
    log("one subject, %dx%dx%d uint8 labels; scratch %.0f MB; graph-timed, 20 calls per graph" % (X, Y, Z, ws.buf.numel() / 1e6))
    for r, name in enumerate(M.REGIONS):
        s = scores[name]
        log("  %s: tp %d fp %d fn %d | dice %.4f sens %.4f spec %.6f | surface distances %d, hd95 %.4f, hd100 %.4f | box %s..%s" % (
            name, s["tp"], s["fp"], s["fn"], s["dice"], s["sensitivity"], s["specificity"], s["n_surface"], s["hausdorff95"],
            s["hausdorff100"], bbox[r, :3].tolist(), bbox[r, 3:].tolist()))
    ext = np.maximum(bbox[:, 3:].astype(np.int64) - bbox[:, :3] + 1, 0)
    steps = int(sum(2 * int(e.prod()) * int(e.sum()) for e in ext))        # two jobs per region
    full_steps = 6 * N * (X + Y + Z)

    f3 = (C.c_int32 * 3)(*SHAPE)
    zero3 = (C.c_int32 * 3)(0, 0, 0)
    bb = C.c_void_p(ws.rec.data_ptr() + M.REC_BBOX * 8)
    ck = _lib.check
    regions = lambda: ck(lib.n3d_seg_regions(K.ptr(pred), K.ptr(truth), f3, f3, zero3, K.ptr(ws.flags), K.ptr(ws.rec), K.stream_ptr()))
    edt = lambda: ck(lib.n3d_seg_edt(K.ptr(ws.flags), 6, 3, f3, bb, K.ptr(ws.dist), K.stream_ptr()))
    sample = lambda: ck(lib.n3d_seg_sample(K.ptr(ws.flags), f3, bb, K.ptr(ws.dist), K.ptr(ws.hist), ws.hist_len, K.stream_ptr()))
    order = lambda: ck(lib.n3d_seg_order(K.ptr(ws.hist), ws.hist_len, K.ptr(ws.rec), K.stream_ptr()))
    us = {}
    us["regions"] = graph_us(regions)
    log("  %-28s %8.1f us | %5.1f MB moved (2 B read + 1 B written per voxel) -> %4.1f us at 8 TB/s" % (
        "n3d_seg_regions", us["regions"], 3 * N / 1e6, 3 * N / HBM * 1e6))
    us["edt"] = graph_us(edt)
    log("  %-28s %8.1f us | %.3f G min-steps inside the boxes (%.1f G without them: %.0fx fewer) -> %.0f G min-steps/s" % (
        "n3d_seg_edt (3 launches)", us["edt"], steps / 1e9, full_steps / 1e9, full_steps / max(steps, 1), steps / us["edt"] / 1e3))
    us["sample"] = graph_us(sample)
    log("  %-28s %8.1f us | the box around the three boxes: %d voxels of %d" % ("n3d_seg_sample", us["sample"], int(ext.max(axis=0).prod()), N))
    us["order"] = graph_us(order)
    log("  %-28s %8.1f us | three workgroups, histograms of %s bins" % (
        "n3d_seg_order", us["order"], [int((e - 1).clip(0) @ (e - 1).clip(0)) + 1 for e in ext]))
    log("  device total %.1f us; score_labels by the wall clock, host sync included: %.2f ms" % (sum(us.values()), wall * 1e3))
    try:
        import scipy
    except ImportError:
        log("  scipy: not installed here, host path not timed")
    else:
        p, t = pred.cpu().numpy(), truth.cpu().numpy()
        t0 = time.perf_counter()
        ref = scipy_scores(p, t)
        dt = time.perf_counter() - t0
        log("  scipy %s on the host, same labels (3 x 2 erosions and distance transforms): %.2f s = %.0fx score_labels" % (
            scipy.__version__, dt, dt / wall))
        for name in M.REGIONS:
            log("    %s: dice %.4f hd95 %.4f (device: %.4f %.4f)" % (name, ref[name][0], ref[name][1], scores[name]["dice"],
                                                                   scores[name]["hausdorff95"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
