"""What cleaning one predicted subject costs (nas_3d_unet_amd.postprocess) on a synthetic 240x240x155 label volume: a tumour-sized
blob (nested balls of radius 20 / 14 / 8 voxels, as tools/metrics_probe.py's) plus a few hundred speckle components.  The six
launches of n3d_cc_clean are timed as captured graphs of repeated calls of the launches 0 .. k (a launch needs the ones before it;
launch 0 clears what the later ones add to), a launch's time being the difference of two such graphs; next to it the bytes it
must move at 8 TB/s.  The same for the variant without the LDS tile phase (N3D_CC_GLOBAL_ONLY), a volume that is one component
throughout (the aggregated size count), the whole clean_labels call by the wall clock, and, where scipy imports,
scipy.ndimage.label plus the same rules on the host.  No threshold is set: nobody has measured these before.
    python tools/postprocess_probe.py [--out profiles/postprocess_probe.log]"""
import argparse
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from nas_3d_unet_amd import _lib, postprocess as P

HBM = 8e12
SHAPE = (240, 240, 155)
RULES = dict(connectivity=26, min_voxels=10, keep_largest=False, et_min_voxels=500)
LINES = []
# per voxel of the image: bytes every launch reads and writes whatever the labels are (foreground voxels add their neighbours'
# and roots' words, through the cache)
TRAFFIC = {"local": (13, "1 B labels read; parent, size, label-4 count written"), "merge": (4, "parent read"),
           "flatten": (8, "parent read, comp written"), "decide_max": (4, "comp read"), "decide_keep": (4, "comp read"),
           "apply": (5, "comp read, 1 B written")}


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
    d = ((gx - 0.6 * X) ** 2 + (gy - 0.5 * Y) ** 2 + (gz - 0.5 * Z) ** 2).sqrt()
    vol = torch.where(d <= 8, 4, torch.where(d <= 14, 1, torch.where(d <= 20, 2, 0))).to(torch.uint8)
    g = torch.Generator(device=dev).manual_seed(seed)
    u = torch.rand(SHAPE, generator=g, device=dev)
    vol = torch.where(u < 4e-5, torch.where(u < 1e-5, torch.full_like(vol, 4), torch.full_like(vol, 2)), vol)
    return vol.contiguous()


def launch_times(labels, out, variant):
    """cumulative graph times of the launches 0 .. k -> per-launch microseconds by difference"""
    cum = [graph_us(lambda k=k: P.run_phases(labels, out, 0, k, variant, **RULES)) for k in range(len(P.PHASES))]
    return [cum[0]] + [cum[k] - cum[k - 1] for k in range(1, len(cum))], cum


def scipy_clean(vol, connectivity, min_voxels, keep_largest, et_min_voxels):
    from scipy import ndimage
    lab, n = ndimage.label(vol != 0, ndimage.generate_binary_structure(3, P.CONNECTIVITIES.index(connectivity) + 1))
    size = np.bincount(lab.ravel(), minlength=n + 1)
    size[0] = 0
    keep = size >= max(min_voxels, 1)
    if keep_largest:
        keep &= np.arange(n + 1) == (int(np.argmax(size)) if n else -1)
    out = np.where(keep[lab], vol, 0).astype(np.uint8)
    e = int((out == 4).sum())
    if 0 < e < et_min_voxels:
        out[out == 4] = 1
    return out, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    from nas_3d_unet_amd.train import reserve_side_streams
    _lib.require_device()
    reserve_side_streams(dev)
    log("postprocess_probe: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    labels = synthetic_labels(dev)
    X, Y, Z = SHAPE
    N = X * Y * Z
    cleaned, stats = P.clean_labels(labels, return_stats=True, **RULES)        # allocates the scratch, warms up
    torch.cuda.synchronize()
    reps = 10
    t0 = time.perf_counter()
    for _ in range(reps):
        cleaned, stats = P.clean_labels(labels, return_stats=True, **RULES)
    wall = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for _ in range(reps):
        cleaned = P.clean_labels(labels, **RULES)
    torch.cuda.synchronize()
    wall_nosync = (time.perf_counter() - t0) / reps
    ws = P._workspaces[(labels.device, SHAPE)]
    log("one subject, %dx%dx%d uint8 labels, rules %s; scratch %.0f MB (%.1f B per voxel); graph-timed, 20 calls per graph" % (
        X, Y, Z, RULES, ws.buf.numel() / 1e6, ws.buf.numel() / N))
    log("  " + ", ".join("%s %s" % (k, stats[k]) for k in P.STAT_KEYS))
    out = torch.empty_like(labels)
    per = {}
    for variant, name in ((P.TILED, "tiled (8 x 8 x 32 tiles in LDS; what n3d_cc_clean runs)"), (P.GLOBAL_ONLY, "global only (no LDS tile phase)")):
        us, cum = launch_times(labels, out, variant)
        per[variant] = us
        assert torch.equal(out, cleaned) and P.stats_of(ws.rec) == stats
        log("  %s:" % name)
        for k, ph in enumerate(P.PHASES):
            b, what = TRAFFIC[ph]
            log("    %d %-12s %8.1f us | %5.1f MB (%d B per voxel: %s) -> %5.1f us at 8 TB/s" % (k, ph, us[k], b * N / 1e6, b, what, b * N / HBM * 1e6))
        log("    launches 0 .. 2 (labelling) %.1f us, all six %.1f us" % (cum[2], cum[5]))
    log("  labelling, tiled vs global only: %.1f us vs %.1f us" % (sum(per[P.TILED][:3]), sum(per[P.GLOBAL_ONLY][:3])))
    log("  clean_labels by the wall clock: %.3f ms with the statistics (one host sync), %.3f ms per call without (10 calls, one sync)" % (
        wall * 1e3, wall_nosync * 1e3))
    dense = torch.full(SHAPE, 2, dtype=torch.uint8, device=dev)
    us_dense = graph_us(lambda: P.run_phases(dense, out, 0, 5, P.TILED, **RULES), iters=5, reps=3)
    dstats = P.stats_of(ws.rec)
    assert dstats["n_components"] == 1 and dstats["largest_size"] == N and torch.equal(out, dense)
    log("  every voxel foreground (one component of %d voxels; sizes counted per wave and run of iterations): all six launches %.1f us" % (N, us_dense))
    try:
        import scipy
    except ImportError:
        log("  scipy: not installed here, host path not timed")
    else:
        vol = labels.cpu().numpy()
        t0 = time.perf_counter()
        ref, n = scipy_clean(vol, **RULES)
        dt = time.perf_counter() - t0
        same = bool(np.array_equal(ref, cleaned.cpu().numpy())) and n == stats["n_components"]
        log("  scipy %s on the host, same volume (ndimage.label, bincount, the same rules): %.3f s = %.0fx clean_labels; %d components, "
            "volumes %s" % (scipy.__version__, dt, dt / wall, n, "equal" if same else "DIFFER"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
