"""What whole-image prediction (predict.ImagePredictor; prediction.py:102-119) costs on one BraTS-sized subject: a synthetic
140x170x140 brain-wide box at (50, 35, 8) in a 240x240x155 image (the slab x >= 2/3 X of the box empty), padded to 256x256x160, the
benchmarked searched net (bench.py: G_conv, depth 4, init_n_kernels 4), fp32.
  * n3d_image_embed, the captured forward and n3d_image_finish (labels with the skull mask; labels + the fp64 image), each
    graph-timed, the two kernels beside their traffic at 8 TB/s;
  * peak device memory of a subject;
  * per-subject wall time (one subject between two device synchronises; median, min .. max) against SubjectPredictor at patch 128
    without overlap, batch 8, on the same subject, the two alternating in one process;
  * with --oracle: the max abs difference of the probabilities against the CPU oracle's forward of the same padded image, run once
    (the only check at a size where 32-bit offsets could bite; recorded, no gate).
No threshold is set: nobody has measured this before.
    python tools/image_predict_probe.py [--windows N] [--oracle] [--out profiles/image_predict_probe.log]"""
import argparse
import os
import statistics
import sys
import threading
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

import bench
from nas_3d_unet_amd import poststep, searched
from nas_3d_unet_amd.generator import VolumeSet
from nas_3d_unet_amd.predict import ImagePredictor, SubjectPredictor, image_forward_tensors, image_pad, net_halvings

HBM = 8e12
BOX, FULL, ORIGIN = (140, 170, 140), (240, 240, 155), (50, 35, 8)
LINES = []


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def graph_us(fn, iters=10, reps=5):
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
    return replay_us(g, reps) / iters


def replay_us(g, reps=5):
    g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def line(name, us, nbytes, what):
    log("  %-36s %9.1f us | %6.1f MB moved (%s) -> %5.1f us at 8 TB/s (%.0f%% of that bound)" % (
        name, us, nbytes / 1e6, what, nbytes / HBM * 1e6, 100 * nbytes / HBM * 1e6 / us))


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "image_predict_probe.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_predict_probe: needs the GPU; nothing is measured without one")
    log("device: %s" % torch.cuda.get_device_name(0))
    torch.manual_seed(0)
    c = bench.CFG
    net = searched.SearchedNet(c["in_channels"], c["init_n_kernels"], c["out_channels"], c["depth"], c["n_nodes"], c["channel_change"],
                               searched.Genotype(**bench.G_CONV)).cuda().eval()
    vol = np.random.default_rng(7).standard_normal((4,) + BOX).astype(np.float32)
    vol[:, 2 * BOX[0] // 3:] = 0
    vs = VolumeSet()
    vs.add(vol)
    vs.origins[0], vs.full_shapes[0] = ORIGIN, FULL
    pad = image_pad(FULL, net_halvings(net))
    padded = tuple(f + w for f, w in zip(FULL, pad))
    widest = max(image_forward_tensors(net, 4, padded), key=lambda r: r[1] * r[2])
    log("subject: box %s at %s in image %s, x >= %d of the box empty; pad %s -> %s; net: bench.py's (G_conv, depth %d, init_n_kernels %d), fp32"
        % (BOX, ORIGIN, FULL, 2 * BOX[0] // 3, pad, padded, c["depth"], c["init_n_kernels"]))
    log("widest tensor of the forward: %s, %d voxels x %d channels x 4 B = %.0f MB (bound 2^31 B = 2147 MB)"
        % (widest[0], widest[1], widest[2], widest[1] * widest[2] * 4 / 1e6))

    ip = ImagePredictor(net, graph=True)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for _ in range(2):                      # the capture, code objects, the allocator
        labels, _ = ip.predict(vs, 0)
    torch.cuda.synchronize()
    log("peak device memory of a subject (labels only, graph and its buffers included): %.0f MB above the %.0f MB resident before"
        % ((torch.cuda.max_memory_allocated() - base) / 1e6, base / 1e6))
    log("labels: %s" % np.bincount(labels.cpu().numpy().ravel(), minlength=5).tolist())

    dvol, y = vs.volumes[0], ip._y
    FN, PN, BN = int(np.prod(FULL)), int(np.prod(padded)), int(np.prod(BOX))
    log("graph-timed (embed / finish: 10 calls per graph, 5 replays; forward: 5 replays of the predictor's own graph):")
    line("n3d_image_embed", graph_us(lambda: poststep.image_embed(dvol, ORIGIN, FULL, padded, out=ip._x)), 16 * BN + 16 * PN,
         "16 B read per box voxel, 16 B written per padded voxel")
    log("  %-36s %9.1f us" % ("forward (captured graph, weight packing included)", replay_us(ip._graph)))
    line("n3d_image_finish (labels, mask)", graph_us(lambda: poststep.image_finish(y, FULL, padded, want_probs=False, inclusive_label=True,
                                                                                     mask_box=dvol, origin=ORIGIN)),
         12 * FN + 16 * BN + FN, "12 B read + 1 B written per voxel, 16 B read per box voxel")
    line("n3d_image_finish (labels + fp64 image)", graph_us(lambda: poststep.image_finish(y, FULL, padded, want_probs=True, inclusive_label=True,
                                                                                         mask_box=dvol, origin=ORIGIN)),
         12 * FN + 16 * BN + 25 * FN, "as above + 24 B written per voxel")

    sp = SubjectPredictor(net, patch=128, batch=8)
    run_img = lambda: ip.predict(vs, 0)
    run_pat = lambda: sp.predict(vs, 0, full_shape=FULL, origin=ORIGIN)
    for _ in range(2):
        lab_p, _ = run_pat()
    agree = float((lab_p == labels).double().mean())
    t_img, t_pat = [], []
    for _ in range(a.windows):              # alternating, so that both see the same machine
        t_img.append(window(run_img))
        t_pat.append(window(run_pat))
    fmt = lambda t: "median %8.2f ms (min %8.2f .. max %8.2f, %d windows)" % (statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3, len(t))
    log("per subject, labels only, wall time between device synchronises:")
    log("  ImagePredictor.predict                       %s | 1 forward on %s" % (fmt(t_img), padded))
    log("  SubjectPredictor.predict (patch 128, no overlap) %s | %d patches, %d live, %d forwards of 8" % (fmt(t_pat), sp.stats.entries, sp.stats.live, sp.stats.chunks))
    log("  the two label volumes agree on %.4f of the voxels (different GroupNorm statistics: not expected to be equal)" % agree)

    if a.oracle:
        from oracle import ref_path as orc
        _, probs = ip.predict(vs, 0, want_probs=True)
        probs = probs.cpu().numpy()
        P = {n: q.detach().cpu() for n, q in net.named_parameters()}
        gene = orc.Genotype(bench.G_CONV["down"], bench.G_CONV["up"])
        x = np.zeros((1, 4) + padded, np.float32)
        x[(0, slice(None)) + tuple(slice(o, o + b) for o, b in zip(ORIGIN, BOX))] = vol
        res = {}

        def forward():
            with torch.no_grad():
                res["p"] = orc.searched_forward(P, torch.from_numpy(x), gene, orc.NetCfg(**c))[0].numpy()

        t0 = time.perf_counter()
        th = threading.Thread(target=forward)
        th.start()
        while th.is_alive():
            th.join(60)
            print("  (the CPU oracle's forward on %s: %.0f s so far)" % (padded, time.perf_counter() - t0), flush=True)
        ref = res["p"][:, :FULL[0], :FULL[1], :FULL[2]]
        log("probabilities against the CPU oracle's fp32 forward of the padded image (one run, %.0f s of CPU): max |diff| %.3e (no gate)"
            % (time.perf_counter() - t0, np.abs(probs - ref).max()))
    else:
        log("probabilities against the CPU oracle at this size: not measured (run with --oracle)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
