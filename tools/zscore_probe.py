"""What the ZScore normalisation (nas_3d_unet_amd.preprocess.ZScore) costs on one BraTS-sized subject, 4 x 240x240x155 int16 of
synthetic counts (tools/preprocess_probe.py's subject: an ellipsoid brain, zero outside): the histogram (n3d_brain_hist, with the
memset of its table), the order statistics (n3d_brain_robust) and normalise + crop (n3d_brain_zscore, with the label crop), each
timed as a captured graph of repeated calls and shown beside its traffic bound (bytes moved at 8 TB/s) and beside n3d_brain_scan
on the same data.  The histogram is timed twice more: with no minimum in `rec`, where every voxel is a global atomic (what the LDS
window is there to avoid), and on counts drawn from 64 values only (contention inside the window).  No threshold is set.
    python tools/zscore_probe.py [--out profiles/zscore_probe.log]"""
import argparse
import ctypes as C
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
import numpy as np
import torch

import preprocess_probe as pp
from nas_3d_unet_amd import _lib, preprocess as P
from nas_3d_unet_amd import kernels as K

log, line, graph_us, SHAPE = pp.log, pp.line, pp.graph_us, pp.SHAPE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    from nas_3d_unet_amd.train import reserve_side_streams
    _lib.require_device()
    reserve_side_streams(dev)
    lib = _lib.load()
    log("zscore_probe: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    raw, truth = pp.synthetic_subject(dev)
    Cm, (X, Y, Z) = 4, SHAPE
    N = X * Y * Z
    brain = int((raw[0] != 0).sum())
    log("one subject, %d x %dx%dx%d int16 (%.0f MB), brain %.0f%% of the voxels, counts 1..4000; graph-timed, 20 calls per graph; "
        "LDS window %d bins" % (Cm, X, Y, Z, raw.numel() * 2 / 1e6, 100.0 * brain / N, lib.n3d_brain_hist_window()))

    totals = torch.zeros((Cm, 2), dtype=torch.int64, device=dev)
    rec = P._records(1, Cm, dev)[0]
    scan = lambda: _lib.check(lib.n3d_brain_scan(K.ptr(raw), Cm, X, Y, Z, K.ptr(totals), K.ptr(rec), K.stream_ptr()))
    line("n3d_brain_scan", graph_us(scan), 2 * Cm * N, "2 B read per voxel")

    hist = torch.empty((Cm, P.HIST_BINS), dtype=torch.int32, device=dev)
    hist_bytes = 2 * Cm * N + 4 * Cm * P.HIST_BINS
    run_hist = lambda r, rc: _lib.check(lib.n3d_brain_hist(K.ptr(r), Cm, X, Y, Z, K.ptr(rc), K.ptr(hist), K.stream_ptr()))
    line("n3d_brain_hist", graph_us(lambda: run_hist(raw, rec)), hist_bytes, "2 B read per voxel + the table's memset")
    want = torch.stack([torch.bincount(raw[c].reshape(-1).long() + 32768, minlength=P.HIST_BINS) for c in range(Cm)])
    want[:, 32768] = 0
    assert torch.equal(hist.long(), want), "the histogram is wrong"
    no_min = P._records(1, Cm, dev)[0]
    line("  .. global atomics only", graph_us(lambda: run_hist(raw, no_min)), hist_bytes, "no minimum in rec: %d atomics" % (Cm * brain))
    assert torch.equal(hist.long(), want), "the histogram is wrong"
    few = ((raw.int() % 64 + 1) * (raw != 0)).to(torch.int16).contiguous()
    rec_few = P._records(1, Cm, dev)[0]
    _lib.check(lib.n3d_brain_scan(K.ptr(few), Cm, X, Y, Z, K.ptr(totals), K.ptr(rec_few), K.stream_ptr()))
    line("  .. 64 distinct counts", graph_us(lambda: run_hist(few, rec_few)), hist_bytes, "LDS contention")
    line("  .. the same, global only", graph_us(lambda: run_hist(few, no_min)), hist_bytes, "global contention")

    run_hist(raw, rec)
    rob = torch.zeros(Cm * P.ROBUST_WORDS, dtype=torch.int64, device=dev)
    robust = lambda: _lib.check(lib.n3d_brain_robust(K.ptr(hist), Cm, 0.5, 99.5, K.ptr(rob), K.stream_ptr()))
    line("n3d_brain_robust", graph_us(robust), 4 * 4 * Cm * P.HIST_BINS, "four passes over the table, from L2; %d workgroups" % Cm)
    rr = rob.cpu().numpy().view(P.ROBUST_DTYPE)
    for c in range(Cm):
        log("    modality %d: n %d  bounds %.6g %.6g  clipped %d + %d  mean %.10g  std %.10g" % (
            c, rr[c]["count"], rr[c]["lower"], rr[c]["upper"], rr[c]["n_below"], rr[c]["n_above"], rr[c]["mean"], rr[c]["std"]))

    h = rec.cpu().numpy().astype(np.int64)
    bw, hi = P._box(h, np.array(SHAPE, np.int64))
    b = [int(v) for v in hi - bw[0]]
    nb = b[0] * b[1] * b[2]
    out = torch.empty((Cm, *b), dtype=torch.float32, device=dev)
    t_out = torch.empty(b, dtype=torch.uint8, device=dev)
    lo_c, hi_c = (C.c_int32 * 3)(*[int(v) for v in bw[0]]), (C.c_int32 * 3)(*[int(v) for v in hi])
    zs = lambda: _lib.check(lib.n3d_brain_zscore(K.ptr(raw), Cm, X, Y, Z, K.ptr(rob), lo_c, hi_c, K.ptr(out), K.ptr(truth), K.ptr(t_out),
                                                 K.stream_ptr()))
    line("n3d_brain_zscore + crop", graph_us(zs), nb * (Cm * (2 + 4) + 2),
         "box %dx%dx%d: 2 B read + 4 B written per modality voxel, 1 + 1 B per label" % tuple(b))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(pp.LINES) + "\n")


if __name__ == "__main__":
    main()
