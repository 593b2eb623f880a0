"""A/B timing of the folded C = 8 node pairs of the benchmarked searched net (G_conv, 4x64^3, batch 2): each pair as ONE launch of
conv_vox_multi_kernel (n3d_conv_fwd2 / n3d_conv_bwd_data2) against its two single launches back to back, pre-packed weights, HIP-graph
replay + HIP events as tools/conv_ab.py does it (kernel time + the dependent-launch boundary).
    python tools/vox_pair_ab.py > profiles/vox_pair_ab.log
Job kinds: s1 = stride-1 conv, s2 = stride-2 gather (big -> half grid), up = the doubled-grid form (half -> big grid); @N = the big grid."""
import ctypes as C
import os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch
from nas_3d_unet_amd import kernels as K, _lib
from nas_3d_unet_amd.train import capture_stream

dev = torch.device("cuda", 0)
lib = _lib.load()
B, CH = 2, 8


def timed(fn, iters=40, reps=5):
    s = capture_stream(dev)
    g = torch.cuda.CUDAGraph()
    fn()
    torch.cuda.synchronize()
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
    return e0.elapsed_time(e1) * 1e3 / (iters * reps)


class Job:
    def __init__(self, kind, big, dil, bwd):
        self.kind, self.bwd = kind, bwd
        self.g = K.conv_geom(B, big, big, big, CH, CH, 3, 1 if kind == "s1" else 2, dil, dil)
        self.transposed = (kind == "s2") if bwd else (kind == "up")
        h = big // 2
        ss, ds = {"s1": (big, big), "s2": (big, h), "up": (h, big)}[kind]
        self.src = torch.randn((B, ss, ss, ss, CH), device=dev)
        self.dst = torch.zeros((B, ds, ds, ds, CH), device=dev)
        self.w = torch.randn((CH, CH, 3, 3, 3), device=dev) * 0.1
        self.bias = None if bwd else torch.randn((CH,), device=dev)
        rows = 0 if bwd else int(lib.n3d_conv_stats_rows(C.byref(self.g), 1 if self.transposed else 0, 0))
        self.stats = torch.zeros((B, rows, CH, 2), dtype=torch.float64, device=dev) if rows else None
        self.ws, self.n = K._ws(self.g, dev)
        self.name = "%s@%d d%d" % (kind, big, dil)
        self.single(0)      # packs the weights
        torch.cuda.synchronize()

    def single(self, flags=_lib.PREPACKED):
        g, s = self.g, K.stream_ptr()
        if not self.bwd:
            fn = lib.n3d_convT_fwd if self.transposed else lib.n3d_conv_fwd
            _lib.check(fn(C.byref(g), K.ptr(self.src), CH, K.ptr(self.w), K.ptr(self.bias), K.ptr(self.dst), CH, flags, None, K.ptr(self.stats),
                          K.ptr(self.ws), self.n, s), "conv_fwd")
        elif self.transposed:
            _lib.check(lib.n3d_convT_bwd_data(C.byref(g), K.ptr(self.src), CH, K.ptr(self.w), K.ptr(self.dst), CH, flags, K.ptr(self.ws), self.n, s), "convT_bwd_data")
        else:
            _lib.check(lib.n3d_conv_bwd_data(C.byref(g), K.ptr(self.src), CH, K.ptr(self.w), K.ptr(self.dst), CH, flags, None, 0, None, K.ptr(self.ws),
                                             self.n, s), "conv_bwd_data")

    def call(self):
        if not self.bwd:
            return K.ConvFwdCall(C.pointer(self.g), 1 if self.transposed else 0, _lib.PREPACKED, self.src.data_ptr(), CH, self.w.data_ptr(),
                                 self.bias.data_ptr(), self.dst.data_ptr(), CH, None, self.stats.data_ptr() if self.stats is not None else None,
                                 self.ws.data_ptr(), self.n)
        return K.ConvBwdCall(C.pointer(self.g), 1 if self.transposed else 0, _lib.PREPACKED, 0, 0, None, 0, self.src.data_ptr(), CH, self.w.data_ptr(),
                             self.dst.data_ptr(), CH, None, 0, None, self.ws.data_ptr(), self.n, None, None, None, None, 0, None)


def pair(a, b, bwd, where):
    ja, jb = Job(*a, bwd), Job(*b, bwd)
    ca, cb = ja.call(), jb.call()
    query, entry = (lib.n3d_conv_bwd_data2_folds, lib.n3d_conv_bwd_data2) if bwd else (lib.n3d_conv_fwd2_folds, lib.n3d_conv_fwd2)
    folds = int(query(C.byref(ca), C.byref(cb)))

    def two():
        ja.single()
        jb.single()

    def one():
        _lib.check(entry(C.byref(ca), C.byref(cb), K.stream_ptr()), "pair")
    ta, tb, t2, t1 = timed(ja.single), timed(jb.single), timed(two), timed(one)
    print("%-3s %-26s %-11s + %-11s  single %5.2f + %5.2f us, back to back %5.2f us, one call %5.2f us (%s)  saves %5.2f us"
          % ("bwd" if bwd else "fwd", where, ja.name, jb.name, ta, tb, t2, t1, "folded" if folds else "NOT folded", t2 - t1))


print("C = %d, batch %d, fp32; per launch = HIP-graph replay of 40 calls, 5 replays, HIP events" % (CH, B))
# forward: the nodes of up-cell 3 (32^3) and down-cell 0 (32^3 -> 16^3) of G_conv
pair(("s1", 32, 1), ("up", 32, 1), False, "up-cell 3 node 0")
pair(("up", 32, 1), ("s1", 32, 2), False, "up-cell 3 node 1")
pair(("s1", 32, 1), ("up", 32, 2), False, "up-cell 3 node 2")
pair(("s2", 32, 1), ("s2", 32, 2), False, "down-cell 0 node 0")
pair(("s2", 32, 1), ("s1", 16, 1), False, "down-cell 0 node 1")
pair(("s1", 16, 2), ("s1", 16, 1), False, "down-cell 0 node 2")
# backward: their data gradients (the gradient of a stride-2 conv is the up form, that of a transposed conv the stride-2 gather)
pair(("s1", 32, 1), ("s2", 32, 1), True, "up-cell 3 node 0")
pair(("s2", 32, 1), ("s1", 32, 2), True, "up-cell 3 node 1")
pair(("s1", 32, 1), ("s2", 32, 2), True, "up-cell 3 node 2")
pair(("up", 32, 1), ("up", 32, 2), True, "down-cell 0 node 0")
pair(("up", 32, 1), ("s1", 16, 1), True, "down-cell 0 node 1")
pair(("s1", 16, 2), ("s1", 16, 1), True, "down-cell 0 node 2")
