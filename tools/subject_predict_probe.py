"""Per-subject wall time of predict.SubjectPredictor (qualify, gather, captured forward per chunk, n3d_stitch_add, n3d_stitch_finish,
labels only) against predict.Predictor.tumor (eager forward of every patch, torch.cat, n3d_stitch into an fp64 image,
n3d_tumor_labels), alternating the two in one process on the same seeded subject: a 140x170x140 brain-wide box in a 240x240x155
image, the slab x >= 2/3 X of the box empty, the benchmarked searched net (bench.py: G_conv, depth 4), batch 8; patch 128 without
overlap and patch 64 with overlap 16.  A window is one subject between two device synchronises; per path the median and the
spread (min .. max) of the windows are printed, with the forward counts behind them.
    python tools/subject_predict_probe.py [--windows N] [--out profiles/subject_predict_probe.log]"""
import argparse
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

import bench
from nas_3d_unet_amd import searched
from nas_3d_unet_amd.generator import VolumeSet
from nas_3d_unet_amd.predict import Predictor, SubjectPredictor, patching

BOX, FULL, ORIGIN, BATCH = (140, 170, 140), (240, 240, 155), (50, 35, 8), 8


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def case(net, vs, vol, patch, overlap, windows, say):
    old = Predictor(net, patch=patch, batch=BATCH)
    new = SubjectPredictor(net, patch=patch, batch=BATCH)
    run_old = lambda: old.tumor(vol, 0.5, True, overlap=overlap, full_shape=FULL, origin=ORIGIN)
    run_new = lambda: new.predict(vs, 0, overlap=overlap, full_shape=FULL, origin=ORIGIN, skull_mask=True)[0]
    for _ in range(2):          # warm-up of both paths at this shape (code objects, allocator, the capture)
        lab_old, lab_new = run_old(), run_new()
    torch.cuda.synchronize()
    skull = torch.zeros(FULL, dtype=torch.bool, device="cuda")
    skull[tuple(slice(o, o + b) for o, b in zip(ORIGIN, BOX))] = (vol != 0).any(0)
    agree = float(((lab_old * skull) == lab_new).double().mean())
    t_old, t_new = [], []
    for _ in range(windows):    # alternating, so that both see the same machine
        t_old.append(window(run_old)[0])
        t_new.append(window(run_new)[0])
    n_corners = len(patching(BOX, (patch,) * 3, overlap))
    st = new.stats
    name = "patch %d, overlap %s" % (patch, overlap)
    fmt = lambda t: "median %8.2f ms (min %8.2f .. max %8.2f, %d windows)" % (statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3, len(t))
    say("%s: %d patches, %d live; labels of the two paths agree on %.6f of the voxels (the old path masked here)" % (name, st.entries, st.live, agree))
    say("  Predictor.tumor          %s | %d eager forwards of up to %d patches, all %d run, cat + fp64 image + labels"
        % (fmt(t_old), -(-n_corners // BATCH), BATCH, n_corners))
    say("  SubjectPredictor.predict %s | %d graph replays of %d patches, %d live run, %d stitch_add + 1 stitch_finish"
        % (fmt(t_new), st.chunks, BATCH, st.live, st.chunks))
    spread = max(max(t_old) - min(t_old), max(t_new) - min(t_new))
    d = statistics.median(t_new) - statistics.median(t_old)
    verdict = "within the expectation" if d <= spread else "SLOWER than the old path by more than the window spread"
    say("  new - old median %+.2f ms, window spread %.2f ms: %s" % (d * 1e3, spread * 1e3, verdict))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "subject_predict_probe.log"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("subject: box %s in image %s at %s, x >= %d of the box empty; net: bench.py's (G_conv, depth %d), fp32, batch %d"
        % (BOX, FULL, ORIGIN, 2 * BOX[0] // 3, bench.CFG["depth"], BATCH))
    torch.manual_seed(0)
    c = bench.CFG
    net = searched.SearchedNet(c["in_channels"], c["init_n_kernels"], c["out_channels"], c["depth"], c["n_nodes"], c["channel_change"],
                               searched.Genotype(**bench.G_CONV)).cuda().eval()
    vol = np.random.default_rng(7).standard_normal((4,) + BOX).astype(np.float32)
    vol[:, 2 * BOX[0] // 3:] = 0
    vs = VolumeSet()
    vs.add(vol)
    dvol = vs.volumes[0]
    for patch, overlap in ((128, None), (64, 16)):
        case(net, vs, dvol, patch, overlap, a.windows, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
