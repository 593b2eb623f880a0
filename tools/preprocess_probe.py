"""What the preprocessing kernels (nas_3d_unet_amd.preprocess) cost on one BraTS-sized subject, 4 x 240x240x155 int16 of synthetic
counts (an ellipsoid brain, zero outside): the scan (n3d_brain_scan), the squared-deviation pass (n3d_brain_sqdev, two launches)
and normalise + crop (n3d_brain_normalize, with the label crop), each timed as a captured graph of repeated calls and shown beside
its traffic bound (bytes moved at 8 TB/s).  No threshold is set: nobody has measured these before.
    python tools/preprocess_probe.py [--out profiles/preprocess_probe.log]"""
import argparse
import ctypes as C
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from nas_3d_unet_amd import _lib, preprocess as P
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


def synthetic_subject(dev, seed=1):
    """(4, X, Y, Z) int16 counts 1..4000 inside an ellipsoid that fills ~0.8 of each axis (BraTS brains fill about that much of
    the 240x240x155 grid), zero outside; uint8 labels in a ball"""
    g = torch.Generator(device=dev).manual_seed(seed)
    X, Y, Z = SHAPE
    gx, gy, gz = torch.meshgrid(*[torch.arange(n, device=dev, dtype=torch.float32) for n in SHAPE], indexing="ij")
    brain = ((gx - X / 2) / (0.4 * X)) ** 2 + ((gy - Y / 2) / (0.4 * Y)) ** 2 + ((gz - Z / 2) / (0.4 * Z)) ** 2 <= 1
    raw = (torch.randint(1, 4001, (4, X, Y, Z), generator=g, device=dev) * brain).to(torch.int16).contiguous()
    d = ((gx - 0.6 * X) ** 2 + (gy - 0.5 * Y) ** 2 + (gz - 0.5 * Z) ** 2).sqrt()
    truth = (torch.where(d <= 8, 4, torch.where(d <= 14, 1, torch.where(d <= 20, 2, 0))) * brain).to(torch.uint8).contiguous()
    return raw, truth


def line(name, us, nbytes, what):
    log("  %-28s %8.1f us | %6.1f MB moved (%s) -> %5.1f us at 8 TB/s (%.0f%% of that bound)" % (
        name, us, nbytes / 1e6, what, nbytes / HBM * 1e6, 100 * nbytes / HBM * 1e6 / us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    from nas_3d_unet_amd.train import reserve_side_streams
    _lib.require_device()
    reserve_side_streams(dev)
    lib = _lib.load()
    log("preprocess_probe: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    raw, truth = synthetic_subject(dev)
    Cm, (X, Y, Z) = 4, SHAPE
    N = X * Y * Z
    log("one subject, %d x %dx%dx%d int16 (%.0f MB), brain %.0f%% of the voxels; graph-timed, 20 calls per graph" % (
        Cm, X, Y, Z, raw.numel() * 2 / 1e6, 100 * float((raw[0] != 0).float().mean())))

    totals = torch.zeros((Cm, 2), dtype=torch.int64, device=dev)
    rec = P._records(1, Cm, dev)[0]
    scan = lambda: _lib.check(lib.n3d_brain_scan(K.ptr(raw), Cm, X, Y, Z, K.ptr(totals), K.ptr(rec), K.stream_ptr()))
    line("n3d_brain_scan", graph_us(scan), 2 * Cm * N, "2 B read per voxel")

    totals.zero_()
    scan()
    t = totals.cpu().numpy()
    mean = torch.from_numpy(t[:, 1].astype(np.float64) / t[:, 0]).to(dev)
    acc = torch.zeros(Cm, dtype=torch.float64, device=dev)
    ws = torch.empty(Cm * lib.n3d_brain_sqdev_rows(N), dtype=torch.float64, device=dev)
    sq = lambda: _lib.check(lib.n3d_brain_sqdev(K.ptr(raw), Cm, N, K.ptr(mean), K.ptr(ws), K.ptr(acc), K.stream_ptr()))
    line("n3d_brain_sqdev (2 launches)", graph_us(sq), 2 * Cm * N, "2 B read per voxel")

    acc.zero_()
    sq()
    std = np.sqrt(acc.cpu().numpy() / t[:, 0])
    ms = torch.from_numpy(np.stack([mean.cpu().numpy(), std], axis=1).round(4).copy()).to(dev)
    h = rec.cpu().numpy().astype(np.int64)
    start = np.maximum(h[:, 2:5] - 1, 0).min(axis=0)
    hi = np.minimum(np.minimum(h[:, 5:8] + 1, SHAPE).max(axis=0) + 1, SHAPE)
    b = [int(v) for v in hi - start]
    nb = b[0] * b[1] * b[2]
    out = torch.empty((Cm, *b), dtype=torch.float32, device=dev)
    t_out = torch.empty(b, dtype=torch.uint8, device=dev)
    lo_c, hi_c = (C.c_int32 * 3)(*[int(v) for v in start]), (C.c_int32 * 3)(*[int(v) for v in hi])
    norm = lambda: _lib.check(lib.n3d_brain_normalize(K.ptr(raw), Cm, X, Y, Z, K.ptr(ms), K.ptr(rec), lo_c, hi_c, K.ptr(out), K.ptr(truth),
                                                      K.ptr(t_out), K.stream_ptr()))
    line("n3d_brain_normalize + crop", graph_us(norm), nb * (Cm * (2 + 4) + 2),
         "box %dx%dx%d: 2 B read + 4 B written per modality voxel, 1 + 1 B per label" % tuple(b))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
