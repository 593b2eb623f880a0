"""What the on-device generator (nas_3d_unet_amd.generator) costs:
  (a) the summed-area tables of one volume (n3d_volume_sat) at 140x170x140 and 240x240x155, against their bytes at 8 TB/s;
  (b) qualifying an epoch's candidates (n3d_patch_qualify), ns per candidate, at overlap none / 32 / 48 / 60 with 64^3 patches, for
      one volume and a 16-volume set -- and, for overlap <= 32, a brute-force device reduction of the same crops (the gather of every
      candidate + a torch reduction) to show what the tables buy;
  (c) host microseconds per batch of Generator.epoch(), and the step time of the flagship 64^3 B=2 Trainer loop fed by
      epoch(out=tr.input_buffers) against the same loop fed one pre-made batch (alternated A/B/A/B).
    python tools/generator_probe.py [--out FILE] [--steps N]"""
import argparse
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from nas_3d_unet_amd import _lib, generator as G
from nas_3d_unet_amd import kernels as K

HBM = 8e12
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


def event_us(fn, reps):
    """microseconds per call of fn issued back to back from the host (events around `reps` calls, after one warm-up call): the
    device time where it exceeds the host's issue time"""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def brain_volume(shape, seed, dev):
    """(4, X, Y, Z) fp32 brain ellipsoid (zero outside) and a uint8 tumour ball towards one side, made on the device"""
    g = torch.Generator(device=dev).manual_seed(seed)
    X, Y, Z = shape
    ax = [torch.arange(n, device=dev, dtype=torch.float32) for n in shape]
    gx, gy, gz = torch.meshgrid(*ax, indexing="ij")
    brain = ((gx - X / 2) / (0.45 * X)) ** 2 + ((gy - Y / 2) / (0.45 * Y)) ** 2 + ((gz - Z / 2) / (0.45 * Z)) ** 2 <= 1
    vol = torch.randn((4, X, Y, Z), generator=g, device=dev) * brain
    off = 0.25 + 0.5 * torch.rand(3, generator=g, device=dev).cpu()
    d = ((gx - off[0] * X) ** 2 + (gy - off[1] * Y) ** 2 + (gz - off[2] * Z) ** 2).sqrt()
    truth = torch.where(d <= 6, 4, torch.where(d <= 11, 1, torch.where(d <= 16, 2, 0))) * brain
    return vol.contiguous(), truth.to(torch.uint8).contiguous()


def part_a(dev, reps):
    log("(a) summed-area tables, one volume (n3d_volume_sat: z pass + indicator, y pass, x pass; 3 launches, graph-timed)")
    lib = _lib.load()
    for shape in ((140, 170, 140), (240, 240, 155)):
        vol, truth = brain_volume(shape, 1, dev)
        X, Y, Z = shape
        sat = torch.empty((X + 1, Y + 1, Z + 1, 2), dtype=torch.int32, device=dev)
        us = graph_us(lambda: _lib.check(lib.n3d_volume_sat(K.ptr(vol), 4, K.ptr(truth), X, Y, Z, K.ptr(sat), K.stream_ptr())))
        vox, padded = X * Y * Z, (X + 1) * (Y + 1) * (Z + 1)
        nbytes = 17 * vox + 8 * padded * 5     # z: 16 B + 1 B read, 8 B written; y and x passes: 8 B read + 8 B written each
        log("  %3dx%3dx%3d: %7.1f us per volume | %5.0f MB moved -> %5.1f us at 8 TB/s (%.0f%% of that bound) | tables %5.0f MB "
            "(8 B per padded voxel) next to the volume's %4.0f MB" % (X, Y, Z, us, nbytes / 1e6, nbytes / HBM * 1e6,
                                                                     100 * nbytes / HBM * 1e6 / us, 8 * padded / 1e6, 17 * vox / 1e6))
    log()


def part_b(dev, reps):
    log("(b) qualification of an epoch's candidates, 64^3 patches on 140x170x140 boxes (n3d_patch_qualify: one thread per candidate; kernel time graph-timed)")
    sets = {}
    for n in (1, 16):
        s = G.VolumeSet(dev)
        for i in range(n):
            s.add(*brain_volume((140, 170, 140), 100 + i, dev))
        sets[n] = s
    lib = _lib.load()
    for n, s in sets.items():
        for ov in (None, 32, 48, 60):
            cand = G.candidate_table([s.box(i) for i in range(n)], list(range(n)), 64, ov)
            N = len(cand)
            cd = torch.from_numpy(cand).to(dev)
            flags = torch.empty(N, dtype=torch.uint8, device=dev)
            us = graph_us(lambda: _lib.check(lib.n3d_patch_qualify(K.ptr(s.records), n, K.ptr(cd), N, 64, K.ptr(flags), K.stream_ptr())))
            t0 = time.perf_counter()
            f = s.qualify_table(cand, 64).cpu().numpy()            # what epoch_init pays: copy up, launch, copy the flags back
            wall = time.perf_counter() - t0
            line = ("  %2d vol, overlap %4s: %8d candidates | kernel %8.1f us = %7.2f ns/candidate | with the table upload and the flag "
                    "download %8.2f ms | kept %d" % (n, ov, N, us, us * 1e3 / N, wall * 1e3, int(G.kept_mask(f, True).sum())))
            if ov is None or ov <= 32:
                def brute():
                    out = []
                    for lo in range(0, N, 64):
                        refs = [(int(r[0]), r[1:], None) for r in cand[lo:lo + 64]]
                        x, t = s.patch_batch(refs, 64, target_dtype=torch.uint8)
                        m0 = (x.view(torch.int32) & 0x7fffffff).ne(0).flatten(1).any(1)
                        m1 = t.ne(0).flatten(1).any(1)
                        out.append(m0.to(torch.uint8) | (m1.to(torch.uint8) << 1))
                    return torch.cat(out)
                assert torch.equal(brute(), torch.from_numpy(f).to(dev)), "brute force disagrees with the tables"
                bus = event_us(brute, max(1, reps // 10))
                line += " | brute force (gather every crop + torch reduce, issued from the host) %9.1f us = %8.1f ns/candidate (%.0fx)" % (
                    bus, bus * 1e3 / N, bus / us)
            log(line)
    log()
    return sets[16]


def part_c(dev, s, steps):
    from bench import CFG, G_CONV
    from nas_3d_unet_amd import searched
    from nas_3d_unet_amd.train import Trainer
    log("(c) Generator.epoch() feeding the flagship trainer (searched G_CONV net, 64^3, B = 2, graph replay), 16 volumes, "
        "patch_overlap 32 (drawn), permute, skip_health")
    gen = G.Generator(list(range(len(s))), s, 64, patch_overlap=32, batch_size=2, labels=[1, 2, 4], permute=True)
    t0 = time.perf_counter()
    gen.epoch_init()
    log("  epoch_init (overlap %s: %d candidates, %d kept, %d steps): %.2f ms host wall" %
        (gen.overlap, len(gen.candidates), gen.n_patches, gen.steps_per_epoch, (time.perf_counter() - t0) * 1e3))
    # host time of next() alone (no trainer): the pops, key draws and descriptors, one launch
    it = gen.epoch()
    ts = []
    for _ in range(min(steps, gen.steps_per_epoch - 1)):
        t0 = time.perf_counter()
        next(it)
        ts.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    it.close()
    ts = np.array(ts[5:]) * 1e6
    log("  host per batch of epoch() (no trainer): median %.1f us, p90 %.1f us over %d batches" % (np.median(ts), np.percentile(ts, 90), len(ts)))
    x0, t0_ = next(gen.epoch())
    bufs = (x0, t0_)
    gi = G.VolumeSet.patch_batch
    refs = [(0, (38, 53, 38), None), (3, (38, 53, 38), G.KEYS[5])]
    log("  one n3d_patch_gather launch, 2 x 64^3 into float targets: %.1f us device (graph-timed); %.1f us per call issued back to "
        "back from the host; %.1f us at 8 TB/s" % (graph_us(lambda: gi(s, refs, 64, out=bufs)), event_us(lambda: gi(s, refs, 64, out=bufs), 50),
                                                  2 * 64 ** 3 * (16 + 12 + 1) / HBM * 1e6))
    torch.manual_seed(1234)
    net = searched.SearchedNet(CFG["in_channels"], CFG["init_n_kernels"], CFG["out_channels"], CFG["depth"], CFG["n_nodes"],
                               CFG["channel_change"], searched.Genotype(**G_CONV)).to(dev)
    net.train()
    tr = Trainer(net, graph=True)
    for _ in range(3):
        tr.step(x0, t0_)
    bx, bt = tr.input_buffers()
    bx.copy_(x0)
    bt.copy_(t0_)

    def fed(n):
        done = 0
        while done < n:
            for x, t in gen.epoch(out=tr.input_buffers):
                if x.shape[0] != 2:
                    continue                        # (the smaller last batch: an eager step, not what is timed)
                assert x is bx
                tr.step(x, t)
                done += 1
                if done == n:
                    break
        torch.cuda.synchronize()

    def premade(n):
        for _ in range(n):
            tr.step(bx, bt)
        torch.cuda.synchronize()

    fed(10)
    premade(10)
    res = {"fed": [], "premade": []}
    for _ in range(3):
        for name, fn in (("fed", fed), ("premade", premade)):
            t0 = time.perf_counter()
            fn(steps)
            res[name].append((time.perf_counter() - t0) * 1e3 / steps)
    a, b = np.median(res["fed"]), np.median(res["premade"])
    log("  step time fed by epoch(out=tr.input_buffers): %s ms (median %.3f)" % (" ".join("%.3f" % v for v in res["fed"]), a))
    log("  step time on one pre-made batch           : %s ms (median %.3f)" % (" ".join("%.3f" % v for v in res["premade"]), b))
    log("  generator cost: %+.3f ms per step = %+.1f%% of the step" % (a - b, 100 * (a - b) / b))
    log()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    from nas_3d_unet_amd.train import reserve_side_streams
    _lib.require_device()
    reserve_side_streams(dev)
    log("generator_probe: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    log()
    part_a(dev, args.reps)
    s16 = part_b(dev, args.reps)
    part_c(dev, s16, args.steps)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
