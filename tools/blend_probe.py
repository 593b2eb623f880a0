"""What importance-weighted blending costs next to the equal-weight stitch (nas_3d_unet_amd.poststep) on one synthetic subject: a
160x190x140 box, patch 128, overlap 64 (28 entries, 4 to a chunk, 3 label channels in the head's NDHWC layout) placed in a
240x240x155 image.  n3d_stitch_add against n3d_stitch_add_w on the same entry table and patch tensor -- all chunks of the subject
per call -- and n3d_stitch_finish against n3d_stitch_finish_w (labels with the skull mask, as the predictors call it; and with the
fp64 probability image).  Each is timed as a captured graph of repeated calls; the two of a pair alternate round by round in one
process and the medians are reported, next to the bytes the pass must move and their time at 8 TB/s.  No threshold is set: nobody
has measured these before.
    python tools/blend_probe.py [--out profiles/blend_probe.log]"""
import argparse
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from nas_3d_unet_amd import _lib, poststep as hp
from nas_3d_unet_amd.predict import patching, plan_subject

HBM = 8e12
BOX, FULL, ORIGIN = (160, 190, 140), (240, 240, 155), (40, 25, 8)
P, OVERLAP, BATCH, C_OUT, C_VOL = 128, 64, 4, 3, 4
LINES = []


def log(s=""):
    print(s, flush=True)
    LINES.append(s)


def capture(fn, iters):
    """a captured graph of `iters` calls of fn (no host issue cost in the timed window)"""
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
    torch.cuda.synchronize()
    return g


def replay_us(g, iters, reps=3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * iters)


def alternate(fa, fb, iters=10, rounds=9):
    """median device microseconds per call of fa and of fb, the two graphs replayed in turn"""
    ga, gb = capture(fa, iters), capture(fb, iters)
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(replay_us(ga, iters))
        tb.append(replay_us(gb, iters))
    return float(np.median(ta)), float(np.median(tb)), (min(ta), max(ta)), (min(tb), max(tb))


def add_traffic(corners, plan, cover_bytes):
    """bytes the chunks of the subject must move: per voxel of a chunk's clipped bounding box the running sums and the covering
    word, read and written; per covering (entry, voxel) pair the patch's channels"""
    box = np.asarray(BOX)
    vox = hits = 0
    for ch in plan.chunks:
        cs = corners[plan.corner[ch.first:ch.last]]
        lo, hi = np.maximum(cs.min(axis=0), 0), np.minimum(cs.max(axis=0) + P, box)
        vox += int(np.prod(hi - lo))
        hits += int(sum(np.prod(np.minimum(c + P, box) - np.maximum(c, 0)) for c in cs))
    return vox * 2 * (C_OUT * 8 + cover_bytes) + hits * C_OUT * 4, vox, hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    from nas_3d_unet_amd.train import reserve_side_streams
    _lib.require_device()
    reserve_side_streams(dev)
    log("blend_probe: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    corners = patching(BOX, (P, P, P), OVERLAP)
    plan = plan_subject(np.zeros(len(corners), dtype=bool), 1, BATCH)
    table = hp.entry_table([(corners[c], hp.IDENTITY, s) for c, s in zip(plan.corner, plan.slot)], dev)
    g = torch.Generator(device=dev).manual_seed(1)
    y = torch.rand((BATCH, P, P, P, C_OUT), generator=g, device=dev).permute(0, 4, 1, 2, 3)      # NDHWC storage, as the head leaves it
    vol = torch.randn((C_VOL,) + BOX, generator=g, device=dev)
    prof = torch.from_numpy(hp.blend_profile(P)).to(dev)
    sum_, cnt = hp.stitch_buffers(C_OUT, BOX, dev)
    sum_w, wsum = hp.stitch_buffers_w(C_OUT, BOX, dev)
    boxes = [(ch, corners[plan.corner[ch.first:ch.last]]) for ch in plan.chunks]

    def add():
        for ch, cs in boxes:
            hp.stitch_add(y, table, ch.first, ch.last - ch.first, cs.min(axis=0), cs.max(axis=0) + P, sum_, cnt)

    def add_w():
        for ch, cs in boxes:
            hp.stitch_add_w(y, table, ch.first, ch.last - ch.first, cs.min(axis=0), cs.max(axis=0) + P, prof, sum_w, wsum)

    log("one subject: box %s, patch %d, overlap %d: %d entries in %d chunks of %d; %d channels; image %s" % (
        BOX, P, OVERLAP, len(corners), len(plan.chunks), BATCH, C_OUT, FULL))
    log("graph-timed (10 calls per graph, 3 replays per round), medians of 9 alternating rounds [min .. max]")
    ta, tw, ra, rw = alternate(add, add_w)
    for name, t, r, cover in (("n3d_stitch_add   (int32 count)", ta, ra, 4), ("n3d_stitch_add_w (fp64 weight sum)", tw, rw, 8)):
        b, vox, hits = add_traffic(corners, plan, cover)
        log("  %-36s %8.1f us [%.1f .. %.1f] per subject (%d launches) | %6.1f MB (%d box voxels r+w, %d covering pairs) -> %5.1f us at 8 TB/s" % (
            name, t, r[0], r[1], len(plan.chunks), b / 1e6, vox, hits, b / HBM * 1e6))
    log("  weighted / unweighted: %.3f" % (tw / ta))
    # one add each from zeroed buffers: the finishing passes then see a subject's values
    for b in (sum_, cnt, sum_w, wsum):
        b.zero_()
    add()
    add_w()
    N, FN = int(np.prod(BOX)), int(np.prod(FULL))
    for what, probs in (("labels + skull mask", False), ("labels + skull mask + fp64 probabilities", True)):
        kw = dict(full_shape=FULL, origin=ORIGIN, want_probs=probs, want_labels=True, inclusive_label=True, mask_vol=vol)
        tf, tfw, rf, rfw = alternate(lambda: hp.stitch_finish(sum_, cnt, **kw), lambda: hp.stitch_finish_w(sum_w, wsum, **kw))
        for name, t, r, cover in (("n3d_stitch_finish", tf, rf, 4), ("n3d_stitch_finish_w", tfw, rfw, 8)):
            b = N * (C_OUT * 8 + cover + C_VOL * 4) + FN * (1 + (C_OUT * 8 if probs else 0))
            log("  %-20s %-42s %7.1f us [%.1f .. %.1f] | %6.1f MB -> %5.1f us at 8 TB/s" % (name, what, t, r[0], r[1], b / 1e6, b / HBM * 1e6))
    la, pa = hp.stitch_finish(sum_, cnt, want_probs=True)
    lw, pw = hp.stitch_finish_w(sum_w, wsum, want_probs=True)
    log("  gaussian vs mean on this subject (uniform(0, 1) patches): max |diff| %.3f, %d of %d labels differ" % (
        float((pa - pw).abs().max()), int((la != lw).sum()), N))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
