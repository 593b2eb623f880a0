"""A/B timing of the small pointwise conv launches (conv_point_kernel) through the C ABI, each with and without N3D_NO_POINTWISE (the
generic gather path they used to take): the forms the 64^3 train step issues -- forward with ReLU on load and statistics, data
gradient with ReLU mask + accumulate, and the two-job launches of a cell's preprocess pair.  HIP-graph replay + HIP events (kernel
time + the dependent-launch boundary).  The output-channel tile follows the rule in conv_generic.hip (point_cot).
python tools/pointwise_ab.py"""
import os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tools"))
import torch
from nas_3d_unet_amd import kernels as K, _lib
from conv_ab import timed

dev = torch.device("cuda", 0)
B = 2
# (Ci, Co, stride, size of the conv INPUT): the pointwise convs of the benchmarked net (profiles/r06_launch_table_seq_64.txt)
SHAPES = [(24, 16, 1, 16), (48, 8, 1, 16), (12, 16, 2, 32), (24, 32, 2, 16), (48, 32, 1, 8)]
FWD_PAIRS = [((12, 16, 2, 32), (24, 16, 1, 16)), ((24, 32, 2, 16), (48, 32, 1, 8))]
BWD_PAIRS = [((24, 16, 1, 16), (12, 16, 2, 32)), ((24, 32, 2, 16), (48, 32, 1, 8))]


def operands(ci, co, stride, size):
    so = (size - 1) // stride + 1
    g = K.conv_geom(B, size, size, size, ci, co, 1, stride, 1, 0)
    x = K.as_view(K.empty_ndhwc(B, ci, size, size, size, dev, torch.float32).normal_())
    dx = K.as_view(K.empty_ndhwc(B, ci, size, size, size, dev, torch.float32).normal_())
    y = K.as_view(K.empty_ndhwc(B, co, so, so, so, dev, torch.float32).normal_())
    w = torch.randn(co, ci, 1, 1, 1, device=dev) * 0.1
    stats = torch.empty((B, K.conv_stats_rows(g, False, 0, x, y), co, 2), dtype=torch.float64, device=dev)
    return g, x, dx, y, w, stats


def fwd_call(o, fl):
    g, x, dx, y, w, stats = o
    return (g, x, w, None, y, K.RELU_IN | fl, None, stats, False)


def bwd_call(o, fl):
    g, x, dx, y, w, stats = o
    return (g, y, w, dx, K.ACCUMULATE | fl, x, None, False)


if __name__ == "__main__":
    print("lib:", _lib.LIB_PATH)
    ctx = K.StepContext(dev)
    ops = {s: operands(*s) for s in set(SHAPES) | {s for p in FWD_PAIRS + BWD_PAIRS for s in p}}
    with K.step_context(ctx):
        for o in ops.values():       # first pass: records the packing jobs
            K.conv_fwd(*fwd_call(o, 0)); K.conv_bwd_data(*bwd_call(o, 0))
        ctx.freeze()
        ctx.pack_all()
        for s in SHAPES:
            t = [timed(lambda: K.conv_fwd(*fwd_call(ops[s], fl))) for fl in (K.NO_POINTWISE, 0)]
            u = [timed(lambda: K.conv_bwd_data(*bwd_call(ops[s], fl))) for fl in (K.NO_POINTWISE, 0)]
            print("%d->%d s%d %d^3: fwd relu+stats  gather %.2f us  pointwise %.2f us | dgrad mask+acc  gather %.2f us  pointwise %.2f us"
                  % (s + (t[0], t[1], u[0], u[1])), flush=True)
        for a, b in FWD_PAIRS:
            t = [timed(lambda: K.conv_fwd2([fwd_call(ops[a], fl), fwd_call(ops[b], fl)])) for fl in (K.NO_POINTWISE, 0)]
            print("fwd2  %d->%d s%d %d^3 + %d->%d s%d %d^3: two gather launches %.2f us  one two-job launch %.2f us" % (a + b + (t[0], t[1])), flush=True)
        for a, b in BWD_PAIRS:
            t = [timed(lambda: K.conv_bwd_data2([bwd_call(ops[a], fl), bwd_call(ops[b], fl)])) for fl in (K.NO_POINTWISE, 0)]
            print("bwd_data2  %d->%d s%d %d^3 + %d->%d s%d %d^3: two gather launches %.2f us  one two-job launch %.2f us" % (a + b + (t[0], t[1])), flush=True)
    print("pointwise launches / jobs:", K.conv_pointwise_counts())
