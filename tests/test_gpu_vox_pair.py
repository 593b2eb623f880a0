"""GPU: two one-plane-tile 3x3x3 convs of C in {4, 8} in ONE launch of conv_vox_multi_kernel, the stride-2 transposed ("up") form
included -- the two convs of a searched-cell node at the C <= 8 levels (n3d_conv_fwd2) and their two data gradients (n3d_conv_bwd_data2).

Every job of the folded launch runs the body of the single kernel on its own range of workgroups, so the comparison with the two single
launches (n3d_conv_fwd / n3d_convT_fwd / n3d_conv_bwd_data / n3d_convT_bwd_data, themselves pinned against CPU convs by test_gpu_conv.py
and test_gpu_conv_exact.py) is torch.equal -- a condition, not a tolerance.  Which path a call took is read from n3d_conv_fold_counts, and
the queries n3d_conv_fwd2_folds / n3d_conv_bwd_data2_folds must have said so beforehand.

Shapes: the stride-1 job on (D, H, W) = (4, 8, 32), the smallest volume with two tile columns and two tile rows; the up job from
(2, 4, 16) onto the same grid; the stride-2 job from (4, 8, 32) down to (2, 4, 16).  B = 3 gives job ranges whose workgroup counts are
not multiples of 8 (the XCD remap's remainder branch inside a job range).

Then the launch as an entry-signal carrier, and the schedule switch fused.FOLD_SMALL_PAIRS: a trainer with the side-stream schedule must
compute the same bits with the folded schedule as with the forked one."""
import ctypes as C

import pytest
import torch

from test_gpu_nets import build_net
from test_gpu_side import _batch

pytestmark = pytest.mark.gpu

BIG, SMALL = (4, 8, 32), (2, 4, 16)
STEP = 7


def _geom(K, B, c, dil, stride):
    return K.conv_geom(B, BIG[0], BIG[1], BIG[2], c, c, 3, stride, dil, dil)


class _Job:
    """one conv of a pair.  kind: "s1" stride-1, "s2" stride-2 gather (big -> small grid), "up" the doubled-grid form (small -> big);
    mode "fwd": n3d_conv_fwd / n3d_convT_fwd with bias and statistics rows, "bwd": n3d_conv_bwd_data / n3d_convT_bwd_data accumulating
    into a non-zero destination"""

    def __init__(self, kind, mode, B, c, dil, gen, pitched=False):
        from nas_3d_unet_amd import _lib, kernels as K
        self.K, self.lib, self._lib = K, _lib.load(), _lib
        self.kind, self.mode, self.c = kind, mode, c
        self.g = _geom(K, B, c, dil, 1 if kind == "s1" else 2)
        # forward: the up form is the transposed conv; data gradient: the up form is the gradient of the plain stride-2 conv
        self.transposed = (kind == "up") if mode == "fwd" else (kind == "s2")
        sshape, dshape = {"s1": (BIG, BIG), "s2": (BIG, SMALL), "up": (SMALL, BIG)}[kind]
        if pitched:      # the source as a channel slice of a node buffer (3 c channels), as a node's conv reads an earlier node
            buf = torch.randn((B,) + sshape + (3 * c,), device="cuda", generator=gen)
            self.src, self.sld = buf[..., c:2 * c], 3 * c
        else:
            self.src, self.sld = torch.randn((B,) + sshape + (c,), device="cuda", generator=gen), c
        self.w = torch.randn((c, c, 3, 3, 3), device="cuda", generator=gen) * 0.1
        self.bias = torch.randn((c,), device="cuda", generator=gen) if mode == "fwd" else None
        self.dst0 = torch.randn((B,) + dshape + (c,), device="cuda", generator=gen)      # what an accumulating data gradient adds to
        self.dshape, self.B = (B,) + dshape + (c,), B
        self.rows = int(self.lib.n3d_conv_stats_rows(C.byref(self.g), 1 if self.transposed else 0, 0)) if mode == "fwd" else 0
        if mode == "fwd":
            assert self.rows > 0
        self.ws, self.ws_bytes = K._ws(self.g, self.src.device)
        self.flags = _lib.ACCUMULATE if mode == "bwd" else 0

    def outputs(self):
        dst = self.dst0.clone()
        stats = torch.zeros((self.B, self.rows, self.c, 2), dtype=torch.float64, device="cuda") if self.rows else None
        return dst, stats

    def single(self, extra_flags=0, ws=None):
        """the single launch; returns [dst] (+ [stats])"""
        K, lib, g = self.K, self.lib, self.g
        dst, stats = self.outputs()
        ws = self.ws if ws is None else ws
        fl, s = self.flags | extra_flags, K.stream_ptr()
        if self.mode == "fwd":
            fn = lib.n3d_convT_fwd if self.transposed else lib.n3d_conv_fwd
            self._lib.check(fn(C.byref(g), K.ptr(self.src), self.sld, K.ptr(self.w), K.ptr(self.bias), K.ptr(dst), self.c, fl, None, K.ptr(stats),
                               K.ptr(ws), self.ws_bytes, s), "conv_fwd")
        elif self.transposed:
            self._lib.check(lib.n3d_convT_bwd_data(C.byref(g), K.ptr(self.src), self.sld, K.ptr(self.w), K.ptr(dst), self.c, fl, K.ptr(ws),
                                                   self.ws_bytes, s), "convT_bwd_data")
        else:
            self._lib.check(lib.n3d_conv_bwd_data(C.byref(g), K.ptr(self.src), self.sld, K.ptr(self.w), K.ptr(dst), self.c, fl, None, 0, None,
                                                  K.ptr(ws), self.ws_bytes, s), "conv_bwd_data")
        return [dst] + ([stats] if stats is not None else [])

    def call(self, dst, stats, extra_flags=0, ws=None):
        """the job as an element of the two-call entry points"""
        K, ws = self.K, (self.ws if ws is None else ws)
        fl = self.flags | extra_flags
        if self.mode == "fwd":
            return K.ConvFwdCall(C.pointer(self.g), 1 if self.transposed else 0, fl, self.src.data_ptr(), self.sld, self.w.data_ptr(),
                                 self.bias.data_ptr(), dst.data_ptr(), self.c, None, stats.data_ptr(), ws.data_ptr(), self.ws_bytes)
        return K.ConvBwdCall(C.pointer(self.g), 1 if self.transposed else 0, fl, 0, 0, None, 0, self.src.data_ptr(), self.sld, self.w.data_ptr(),
                             dst.data_ptr(), self.c, None, 0, None, ws.data_ptr(), self.ws_bytes, None, None, None, None, 0, None)


def _pair(j0, j1, extra_flags=0, ws=(None, None)):
    """both jobs through n3d_conv_fwd2 / n3d_conv_bwd_data2 -> (outputs of job 0 + outputs of job 1, the query's answer, folded launches)"""
    K, lib, _lib = j0.K, j0.lib, j0._lib
    outs = [j.outputs() for j in (j0, j1)]
    cs = [j.call(d, st, extra_flags, w) for j, (d, st), w in zip((j0, j1), outs, ws)]
    if j0.mode == "fwd":
        said = int(lib.n3d_conv_fwd2_folds(C.byref(cs[0]), C.byref(cs[1])))
        n0 = K.conv_fold_counts()["vox_multi"]
        _lib.check(lib.n3d_conv_fwd2(C.byref(cs[0]), C.byref(cs[1]), K.stream_ptr()), "n3d_conv_fwd2")
    else:
        said = int(lib.n3d_conv_bwd_data2_folds(C.byref(cs[0]), C.byref(cs[1])))
        n0 = K.conv_fold_counts()["vox_multi"]
        _lib.check(lib.n3d_conv_bwd_data2(C.byref(cs[0]), C.byref(cs[1]), K.stream_ptr()), "n3d_conv_bwd_data2")
    folded = K.conv_fold_counts()["vox_multi"] - n0
    torch.cuda.synchronize()
    return [t for d, st in outs for t in ([d] + ([st] if st is not None else []))], said, folded


def _check_pair(j0, j1):
    """not pre-packed with distinct workspaces, pre-packed, and one shared workspace without N3D_PREPACKED (two launches)"""
    _lib = j0._lib
    ref = j0.single() + j1.single()      # (also packs each job's weights into its own workspace)
    torch.cuda.synchronize()
    got, said, folded = _pair(j0, j1)
    assert (said, folded) == (1, 1), (said, folded)
    assert len(got) == len(ref) and all(torch.equal(a, b) for a, b in zip(got, ref))
    got, said, folded = _pair(j0, j1, _lib.PREPACKED)
    assert (said, folded) == (1, 1), (said, folded)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    shared = torch.empty_like(j0.ws)
    got, said, folded = _pair(j0, j1, 0, (shared, shared))
    assert (said, folded) == (0, 0), (said, folded)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))


CASES = [(B, c, dil) for B in (2, 3) for c in (4, 8) for dil in (1, 2)]


@pytest.mark.parametrize("B,c,dil", CASES)
@pytest.mark.parametrize("mode", ["fwd", "bwd"])
def test_stride1_with_up_job_both_orders(mode, B, c, dil):
    """a node of up-cell 3 (forward) / a stride-1 and a stride-2 conv's data gradients (backward): both write the (4, 8, 32) grid"""
    gen = torch.Generator(device="cuda").manual_seed(100 * B + 10 * c + dil)
    s1 = _Job("s1", mode, B, c, dil, gen, pitched=True)
    up = _Job("up", mode, B, c, 3 - dil, gen)      # (the other dilation: two different bodies in one launch)
    up_same = _Job("up", mode, B, c, dil, gen)
    _check_pair(up, s1)
    _check_pair(s1, up)
    _check_pair(s1, up_same)


@pytest.mark.parametrize("B,c,dil", CASES)
@pytest.mark.parametrize("mode", ["fwd", "bwd"])
def test_stride2_with_up_job(mode, B, c, dil):
    """the stride-2 gather next to the doubled-grid form: forward, a stride-2 conv and a stride-2 transposed conv; backward, the data
    gradient of a stride-2 transposed conv and that of a stride-2 conv (the mix of down-cell 0's backward)"""
    gen = torch.Generator(device="cuda").manual_seed(1000 + 100 * B + 10 * c + dil)
    s2 = _Job("s2", mode, B, c, dil, gen, pitched=True)
    up = _Job("up", mode, B, c, dil, gen)
    _check_pair(s2, up)
    _check_pair(up, s2)


@pytest.mark.parametrize("c", [4, 8])
def test_two_stride1_jobs_and_refusals(c):
    """two stride-1 jobs (the form the launch took before) still fold; one destination for both and a job of another channel count do not"""
    gen = torch.Generator(device="cuda").manual_seed(31 + c)
    a, b = _Job("s1", "fwd", 3, c, 1, gen), _Job("s1", "fwd", 3, c, 2, gen)
    _check_pair(a, b)
    other = _Job("up", "fwd", 3, 12 - c, 1, gen)
    ref = a.single() + other.single()
    got, said, folded = _pair(a, other)
    assert (said, folded) == (0, 0)
    assert all(torch.equal(x, y) for x, y in zip(got, ref))
    # two data gradients accumulating into ONE buffer: never one launch (n3d_conv_bwd_data2 runs them one after the other)
    d0, d1 = _Job("s1", "bwd", 2, c, 1, gen), _Job("up", "bwd", 2, c, 1, gen)
    dst = d0.dst0.clone()
    cs = [j.call(dst, None) for j in (d0, d1)]
    K = d0.K
    assert int(d0.lib.n3d_conv_bwd_data2_folds(C.byref(cs[0]), C.byref(cs[1]))) == 0
    n0 = K.conv_fold_counts()["vox_multi"]
    d0._lib.check(d0.lib.n3d_conv_bwd_data2(C.byref(cs[0]), C.byref(cs[1]), K.stream_ptr()), "n3d_conv_bwd_data2")
    torch.cuda.synchronize()
    assert K.conv_fold_counts()["vox_multi"] == n0
    want = d0.single()[0] + d1.single()[0] - d1.dst0
    assert torch.allclose(dst, want, rtol=1e-5, atol=1e-5)      # (a sum in another order: the only comparison here that is not bit for bit)


@pytest.mark.parametrize("mode", ["fwd", "bwd"])
def test_folded_pair_carries_an_entry_signal(mode):
    """a signal armed in front of a folded pre-packed pair rides in the launch's entry; an unarmed launch leaves the flag alone"""
    gen = torch.Generator(device="cuda").manual_seed(77)
    j0, j1 = _Job("s1", mode, 2, 8, 1, gen), _Job("up", mode, 2, 8, 1, gen)
    K, lib, _lib = j0.K, j0.lib, j0._lib
    ref = j0.single() + j1.single()      # packs the weights
    torch.cuda.synchronize()
    w = torch.zeros(16, dtype=torch.int32, device="cuda")      # [0] the stream's step word, [4] the flag
    w[0] = STEP
    p = lambda i: w.data_ptr() + 4 * i
    c0 = K.entry_signal_counts()
    got, said, folded = _pair(j0, j1, _lib.PREPACKED)      # unarmed
    c1 = K.entry_signal_counts()
    assert (said, folded) == (1, 1) and tuple(c1) == tuple(c0)
    assert w.tolist()[4] == 0 and w.tolist()[0] == STEP
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    _lib.check(lib.n3d_entry_signal_arm(C.c_void_p(p(4)), C.c_void_p(p(0)), 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "arm")
    assert K.entry_signal_pending() == 1
    got, said, folded = _pair(j0, j1, _lib.PREPACKED)
    assert K.entry_signal_pending() == 0
    c2 = K.entry_signal_counts()
    assert (said, folded) == (1, 1)
    assert (c2[0] - c1[0], c2[1] - c1[1]) == (1, 0), "the signal was not carried by the folded launch: %s -> %s" % (c1, c2)
    assert w.tolist()[4] == STEP and w.tolist()[0] == STEP
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    # not pre-packed: the packing launches in front of the folded one issue the signal stand-alone, as in front of a single conv
    w[4] = 0
    _lib.check(lib.n3d_entry_signal_arm(C.c_void_p(p(4)), C.c_void_p(p(0)), 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "arm")
    got, said, folded = _pair(j0, j1)
    c3 = K.entry_signal_counts()
    assert (said, folded) == (1, 1) and (c3[0] - c2[0], c3[1] - c2[1]) == (0, 1)
    assert w.tolist()[4] == STEP
    assert all(torch.equal(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize("graph,size,shared", [(False, 32, True), (True, 32, True), (True, 64, False)])
def test_folded_schedule_computes_the_forked_schedule_bits(graph, size, shared):
    """G_CONV trainer, batch 2, side-stream schedule forced: two steps with fused.FOLD_SMALL_PAIRS on and two with it off.
    The folded launch runs the single kernels' bodies and every buffer keeps its writers in program order on one stream, so loss,
    parameters and gradients are equal bit for bit -- eagerly and replayed from the captured graphs.  Patch 32^3: every pair libn3d
    folds (the C = 4 nodes of up-cell 4, stride-1 with up form; kernels.FOLD_SHARED_SIMDS, since no pair of this size leaves a SIMD to
    every wave); patch 64^3: the pairs the schedule folds by itself (down-cell 0)."""
    from nas_3d_unet_amd import fused, kernels as K
    from nas_3d_unet_amd.train import Trainer
    x, t = _batch(61, size=size)
    res = []
    prev, K.FOLD_SHARED_SIMDS = K.FOLD_SHARED_SIMDS, shared
    try:
        for fold in (True, False):
            with fused.switched(FOLD_SMALL_PAIRS=fold):
                net, _ = build_net("searched", "G_CONV", 4)
                tr = Trainer(net, graph=graph, side_wgrad="force")
                n0 = K.conv_fold_counts()["vox_multi"]
                losses = [tr.step(x, t).clone() for _ in range(2)]
                torch.cuda.synchronize()
                tr.check_sync()
                assert tr.sync_timeouts() == 0
                if graph:
                    assert tr._use_side
                res.append((losses, tr.fp.flat.clone(), tr.fp.grad.clone(), K.conv_fold_counts()["vox_multi"] - n0))
    finally:
        K.FOLD_SHARED_SIMDS = prev
    (l1, p1, g1, n1), (l0, p0, g0, n0) = res
    print("folded launches issued: FOLD_SMALL_PAIRS on %d, off %d" % (n1, n0))
    assert n1 > n0, "the switch folded nothing at this size"
    assert all(torch.equal(a, b) for a, b in zip(l1, l0))
    assert torch.equal(p1, p0)
    assert torch.equal(g1, g0)
