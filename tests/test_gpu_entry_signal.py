"""GPU: entry signals (include/n3d.h, "Entry signals") -- a stream hand-off signal stored by the NEXT kernel of its stream as that
kernel starts, instead of by a one-lane launch of its own.

1. every carrier family: the flag holds the step value, outputs are bit-identical to the unarmed call, the step word is bumped only
   when asked, two armed signals both land, and the library counts the signal as CARRIED (no stand-alone launch);
2. a launch that carries nothing, a launch on another stream and n3d_entry_signal_flush turn the armed signal into one stand-alone
   launch in front -- never lost;
3. the two-stream ping-pong of test_gpu_side.test_sync_handoff_orders_two_streams with the signals carried by the wait kernels, eager
   and replayed from captured graphs: no time-out;
4. the trainer's captured three-stream step with entry signals against the same step with every signal a launch of its own
   (kernels.ENTRY_SIGNALS = False): weights, Adam moments and losses bit-identical, no time-out, nothing left pending, and no stand-alone
   signal in front of a carrier on the main chain."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 7      # value of the signalling stream's step word in the unit tests


def _words(n=16):
    w = torch.zeros(n, dtype=torch.int32, device="cuda")   # [0] step of stream A, [1] time-outs, [2] step of stream B, [4..] flags
    w[0] = STEP
    w[2] = STEP
    return w


def _carried(call, n_signals=1, bump=False):
    """call() -> list of output tensors.  Runs it unarmed, then with n_signals armed; checks everything the carriers promise."""
    from nas_3d_unet_amd import _lib, kernels as K
    lib = _lib.load()
    ref = [t.clone() for t in call()]
    torch.cuda.synchronize()
    w = _words()
    p = lambda i: w.data_ptr() + 4 * i
    h = torch.cuda.current_stream().cuda_stream
    c0 = K.entry_signal_counts()
    for i in range(n_signals):
        _lib.check(lib.n3d_entry_signal_arm(C.c_void_p(p(4 + i)), C.c_void_p(p(0)), 1 if (bump and i == n_signals - 1) else 0, C.c_void_p(h)), "arm")
    assert K.entry_signal_pending() == n_signals
    got = call()
    assert K.entry_signal_pending() == 0
    torch.cuda.synchronize()
    c1 = K.entry_signal_counts()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (n_signals, 0), "the signal was not carried by the kernel: %s -> %s" % (c0, c1)
    ws = w.tolist()
    assert ws[4:4 + n_signals] == [STEP] * n_signals and ws[4 + n_signals] == 0, ws
    assert ws[0] == STEP + (1 if bump else 0), ws
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def _all_modes(call):
    _carried(call, 1, False)
    _carried(call, 1, True)
    _carried(call, 2, False)
    _carried(call, 2, True)


# ---- 1. carriers ----------------------------------------------------------------------------------------------------------------
def test_wait_kernels_carry():
    from nas_3d_unet_amd import kernels as K
    v = torch.zeros(8, dtype=torch.int32, device="cuda")     # [0] step, [1] time-outs, [2], [3] flags that have arrived
    v[0] = 3
    v[2] = 3
    v[3] = 3
    q = lambda i: v.data_ptr() + 4 * i

    def wait1():
        K.sync_wait(q(2), q(0), q(1), False, max_polls=1000)
        return [v[1:2]]

    def wait2():
        K.sync_wait2(q(2), q(3), q(0), q(1), False, max_polls=1000)
        return [v[1:2]]
    _all_modes(wait1)
    _all_modes(wait2)
    assert int(v[1]) == 0


def _conv_case(g, transposed=False, data_grad=False, bf16=False, seed=0):
    """a forward (or transposed forward, or data-gradient) conv through the C ABI with weights packed by a first call: the call under
    test passes N3D_PREPACKED, as every conv of a trainer step does, so it is ONE launch"""
    from nas_3d_unet_amd import _lib, kernels as K
    lib = _lib.load()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    i_shape, o_shape = (g.B, g.Di, g.Hi, g.Wi, g.Ci), (g.B, g.Do, g.Ho, g.Wo, g.Co)
    src_shape, dst_shape = (o_shape, i_shape) if (transposed != data_grad) else (i_shape, o_shape)
    dt = torch.bfloat16 if bf16 else torch.float32      # bf16: the storage twins of conv_bf16.hip (both tensors in bf16)
    src = torch.randn(src_shape, device="cuda", generator=gen).to(dt)
    w = torch.randn((g.Co, g.Ci, g.k, g.k, g.k), device="cuda", generator=gen) * 0.1
    bias = None if data_grad else torch.randn(((g.Ci if transposed else g.Co),), device="cuda", generator=gen)
    ws, n = K._ws(g, src.device)
    sld, dld = src_shape[-1], dst_shape[-1]
    bf = (_lib.SRC_BF16 | _lib.DST_BF16) if bf16 else 0
    # GroupNorm statistics rows of the forward forms, written by the same launch (n3d_conv_stats_rows: > 0 where the kernel has them)
    rows = 0 if data_grad else int(lib.n3d_conv_stats_rows(C.byref(g), 1 if transposed else 0, bf))
    if not data_grad:
        assert rows > 0, "this case is meant to run on a kernel that writes statistics rows"

    def run(flags):
        dst = torch.zeros(dst_shape, device="cuda", dtype=dt)
        stats = torch.zeros((g.B, rows, dst_shape[-1], 2), dtype=torch.float64, device="cuda") if rows > 0 else None
        flags |= bf
        s = K.stream_ptr()
        if data_grad:
            fn = lib.n3d_convT_bwd_data if transposed else lib.n3d_conv_bwd_data
            if transposed:
                _lib.check(fn(C.byref(g), K.ptr(src), sld, K.ptr(w), K.ptr(dst), dld, flags, K.ptr(ws), n, s), "convT_bwd_data")
            else:
                _lib.check(fn(C.byref(g), K.ptr(src), sld, K.ptr(w), K.ptr(dst), dld, flags, None, 0, None, K.ptr(ws), n, s), "conv_bwd_data")
        else:
            fn = lib.n3d_convT_fwd if transposed else lib.n3d_conv_fwd
            _lib.check(fn(C.byref(g), K.ptr(src), sld, K.ptr(w), K.ptr(bias), K.ptr(dst), dld, flags, None, K.ptr(stats), K.ptr(ws), n, s), "conv_fwd")
        return [dst] + ([stats] if stats is not None else [])
    run(0)                      # packs the weights into ws
    torch.cuda.synchronize()
    return lambda: run(_lib.PREPACKED)


@pytest.mark.parametrize("case", ["vox64_c4", "vox64_c8_dil2", "vox64_bwd_data", "vox_s2", "vox_up_convT", "vox_up_bwd_data", "k1", "gather_k1_s2",
                                  "vox64b_bf16", "vox_s2b_bf16", "vox_upb_bf16", "vox_s2_convT_bwd_data"])
def test_conv_kernels_carry(case):
    from nas_3d_unet_amd import kernels as K
    geom = {
        "vox64_c4": (K.conv_geom(2, 16, 16, 16, 4, 4, 3, 1, 1, 1), False, False),
        "vox64_c8_dil2": (K.conv_geom(2, 16, 16, 16, 8, 8, 3, 1, 2, 2), False, False),
        "vox64_bwd_data": (K.conv_geom(2, 16, 16, 16, 8, 8, 3, 1, 1, 1), False, True),
        "vox_s2": (K.conv_geom(2, 32, 32, 32, 8, 8, 3, 2, 1, 1), False, False),
        "vox_up_convT": (K.conv_geom(2, 32, 32, 32, 8, 8, 3, 2, 1, 1), True, False),
        "vox_up_bwd_data": (K.conv_geom(2, 32, 32, 32, 4, 4, 3, 2, 1, 1), False, True),
        "k1": (K.conv_geom(2, 32, 32, 32, 4, 12, 1, 1, 1, 0), False, False),
        "gather_k1_s2": (K.conv_geom(2, 32, 32, 32, 12, 8, 1, 2, 1, 0), False, False),
        "vox64b_bf16": (K.conv_geom(2, 16, 16, 16, 8, 8, 3, 1, 1, 1), False, False, True),
        "vox_s2b_bf16": (K.conv_geom(2, 32, 32, 32, 8, 8, 3, 2, 1, 1), False, False, True),
        "vox_upb_bf16": (K.conv_geom(2, 32, 32, 32, 8, 8, 3, 2, 1, 1), True, False, True),
        "vox_s2_convT_bwd_data": (K.conv_geom(2, 32, 32, 32, 8, 8, 3, 2, 1, 1), True, True),      # n3d_convT_bwd_data: a stride-2 gather of dy
    }[case]
    _all_modes(_conv_case(*geom))


def test_conv_pair_carries():
    """n3d_conv_fwd2 on the two pointwise convs of a cell's preprocess pair (one K-split MFMA launch)"""
    from nas_3d_unet_amd import _lib, kernels as K
    # (the deepest cell of the benchmark net at 64^3: 48 x 8^3 -> 64 x 4^3 with stride 2 next to 96 x 4^3 -> 64 x 4^3)
    g0, g1 = K.conv_geom(2, 8, 8, 8, 48, 64, 1, 2, 1, 0), K.conv_geom(2, 4, 4, 4, 96, 64, 1, 1, 1, 0)
    gen = torch.Generator(device="cuda").manual_seed(5)
    xs = [K.as_view(torch.randn((2, g.Di, g.Hi, g.Wi, g.Ci), device="cuda", generator=gen).permute(0, 4, 1, 2, 3)) for g in (g0, g1)]
    wts = [torch.randn((g.Co, g.Ci, 1, 1, 1), device="cuda", generator=gen) * 0.1 for g in (g0, g1)]
    bs = [torch.randn((64,), device="cuda", generator=gen) for _ in range(2)]
    ctx = K.StepContext(torch.device("cuda"))
    rows = [K.conv_stats_rows(g, False, 0) for g in (g0, g1)]
    assert min(rows) > 0

    def run():
        ys = [K.View(K.empty_ndhwc(2, 64, 4, 4, 4, "cuda", torch.float32), 64) for _ in range(2)]
        sts = [torch.zeros((2, r, 64, 2), dtype=torch.float64, device="cuda") for r in rows]
        with K.step_context(ctx):
            K.conv_fwd2([(g, x, w, b, y, 0, None, st, False) for g, x, w, b, y, st in zip((g0, g1), xs, wts, bs, ys, sts)])
        return [y.t for y in ys] + sts
    # weights packed once, as in a trainer: the call under test is one launch
    with K.step_context(ctx):
        for g, w in zip((g0, g1), wts):
            ctx.slot(w, g, False, 0)
    ctx.freeze()
    ctx.pack_all()
    torch.cuda.synchronize()
    _all_modes(run)


def test_k1_norm_kernels_carry():
    """stem0 in its recompute form (Ci = 4, Co = 12, the shape the step uses): n3d_conv_k1_norm_fwd -- the statistics-only pass and the
    conv-and-normalise pass, both conv_k1_kernel -- and n3d_conv_k1_norm_bwd_reduce (k1n_bwd_kernel)"""
    from nas_3d_unet_amd import kernels as K
    g = K.conv_geom(2, 32, 32, 32, 4, 12, 1, 1, 1, 0)
    assert K.conv_k1_norm_ok(g)
    gen = torch.Generator(device="cuda").manual_seed(17)
    x = K.View(K.empty_ndhwc(2, 4, 32, 32, 32, "cuda", torch.float32).normal_(generator=gen), 4)
    dout = K.View(K.empty_ndhwc(2, 12, 32, 32, 32, "cuda", torch.float32).normal_(generator=gen), 12)
    w = torch.randn((12, 4, 1, 1, 1), device="cuda", generator=gen) * 0.3
    bias = torch.randn((12,), device="cuda", generator=gen)
    a, b = torch.rand((2, 12), device="cuda", generator=gen) + 0.5, torch.randn((2, 12), device="cuda", generator=gen)
    rows = K.conv_stats_rows(g, False, 0)
    ctx = K.StepContext(torch.device("cuda"))
    with K.step_context(ctx):          # weights packed once, as in a trainer: each call under test is one launch
        ctx.slot(w, g, False, 0)
    ctx.freeze()
    ctx.pack_all()
    torch.cuda.synchronize()

    def stats_pass():
        stats = torch.zeros((2, rows, 12, 2), dtype=torch.float64, device="cuda")
        with K.step_context(ctx):
            K.conv_k1_norm_fwd(g, x, w, bias, None, None, None, stats)
        return [stats]

    def norm_pass():
        y = K.View(K.empty_ndhwc(2, 12, 32, 32, 32, "cuda", torch.float32), 12)
        with K.step_context(ctx):
            K.conv_k1_norm_fwd(g, x, w, bias, y, a, b, None)
        return [y.t]

    def bwd_reduce():
        return [K.conv_k1_norm_bwd_reduce(g, x, w, bias, dout, a, b)[0]]
    _all_modes(stats_pass)
    _all_modes(norm_pass)
    _all_modes(bwd_reduce)


def _gn_terms(B, Cc, N, G, gen):
    from nas_3d_unet_amd import kernels as K
    side = round(N ** (1 / 3))
    mk = lambda: K.View(K.empty_ndhwc(B, Cc, side, side, side, "cuda", torch.float32).normal_(generator=gen), Cc)
    terms = []
    for _ in range(2):
        terms.append(dict(raw=mk(), a=torch.rand((B, Cc), device="cuda", generator=gen) + 0.5, b=torch.randn((B, Cc), device="cuda", generator=gen),
                          mr=torch.rand((B, G, 2), device="cuda", generator=gen) + 0.5, sumraw=None,
                          gamma=torch.nn.Parameter(torch.randn((Cc,), device="cuda", generator=gen)),
                          beta=torch.nn.Parameter(torch.randn((Cc,), device="cuda", generator=gen)), wptr=None, relu=True, conv_bias=None))
    return terms, mk()


@pytest.mark.parametrize("shape", [(2, 8, 32 ** 3, 2), (2, 32, 4 ** 3, 2)], ids=["reduce2", "small"])
def test_node_backward_kernels_carry(shape):
    """the backward of a node's two GroupNorm epilogues: affine_bwd_reduce2_kernel in front (large levels), or the one-launch
    gn_bwd_small2_kernel (deep levels)"""
    from nas_3d_unet_amd import kernels as K
    B, Cc, N, G = shape
    gen = torch.Generator(device="cuda").manual_seed(11)
    terms, dout = _gn_terms(B, Cc, N, G, gen)
    assert bool(K.small_backward_mode(B, N, Cc, G)) == (N == 64)

    def run():
        for t in terms:
            t["draw"] = K.like(t["raw"])
        outs = K.affine_act_bwd_gn2(dout, terms, G)
        return [t["draw"].t for t in terms] + [o for pair in outs for o in pair[:2]]
    _all_modes(run)


def test_epilogue_backward_reduce_carries():
    from nas_3d_unet_amd import kernels as K
    gen = torch.Generator(device="cuda").manual_seed(13)
    mk = lambda: K.View(K.empty_ndhwc(2, 16, 16, 16, 16, "cuda", torch.float32).normal_(generator=gen), 16)
    dout, raw = mk(), mk()
    a, b = torch.rand((2, 16), device="cuda", generator=gen) + 0.5, torch.randn((2, 16), device="cuda", generator=gen)
    _all_modes(lambda: [K.affine_act_bwd_reduce(dout, raw, a, b, 0)[0]])      # (sums, rows)


# ---- 2. never lost --------------------------------------------------------------------------------------------------------------
def test_non_carrier_other_stream_and_flush_fall_back_to_a_launch():
    from nas_3d_unet_amd import _lib, kernels as K
    from nas_3d_unet_amd.train import reserve_side_streams
    lib = _lib.load()
    w = _words()
    p = lambda i: w.data_ptr() + 4 * i
    h = torch.cuda.current_stream().cuda_stream
    arm = lambda flag, stream: _lib.check(lib.n3d_entry_signal_arm(C.c_void_p(p(flag)), C.c_void_p(p(0)), 0, C.c_void_p(stream)), "arm")
    n = 4096
    prm, g, m, v, st = torch.ones(n, device="cuda"), torch.randn(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), K.step_counter("cuda")
    # a kernel that carries nothing
    c0 = K.entry_signal_counts()
    arm(4, h)
    K.adam_step(prm, g, m, v, st)
    assert K.entry_signal_pending() == 0
    torch.cuda.synchronize()
    c1 = K.entry_signal_counts()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (0, 1) and int(w[4]) == STEP
    # the next launch is on another stream (a carrier there): the signal goes to ITS stream, stand-alone
    other = reserve_side_streams(torch.device("cuda", torch.cuda.current_device()))[0]
    w[6] = STEP
    arm(5, h)
    with K.on_side(other):
        K.sync_wait(p(6), p(0), p(1), False, max_polls=1000)
    assert K.entry_signal_pending() == 0
    torch.cuda.synchronize()
    c2 = K.entry_signal_counts()
    assert (c2[0] - c1[0], c2[1] - c1[1]) == (0, 1) and int(w[5]) == STEP and int(w[1]) == 0
    # no next launch: flush
    arm(7, h)
    _lib.check(lib.n3d_entry_signal_flush(C.c_void_p(other.cuda_stream)), "flush")      # (another stream's flush leaves it armed)
    assert K.entry_signal_pending() == 1
    _lib.check(lib.n3d_entry_signal_flush(C.c_void_p(h)), "flush")
    assert K.entry_signal_pending() == 0
    torch.cuda.synchronize()
    c3 = K.entry_signal_counts()
    assert (c3[0] - c2[0], c3[1] - c2[1]) == (0, 1) and int(w[7]) == STEP
    # a third signal does not fit one entry: the first two go out, nothing is dropped
    for i in (8, 9, 10):
        arm(i, h)
    assert K.entry_signal_pending() == 1
    _lib.check(lib.n3d_entry_signal_flush(C.c_void_p(h)), "flush")
    torch.cuda.synchronize()
    assert w[8:11].tolist() == [STEP] * 3


# ---- 3. ping-pong ---------------------------------------------------------------------------------------------------------------
def test_ping_pong_with_signals_carried_by_the_wait_kernels_eager():
    """test_gpu_side.test_sync_handoff_orders_two_streams with every signal riding in its stream's next wait kernel"""
    from nas_3d_unet_amd import _lib, kernels as K
    from nas_3d_unet_amd.train import reserve_side_streams
    lib = _lib.load()
    w = torch.zeros(16, dtype=torch.int32, device="cuda")
    w[0] = 1
    w[2] = 1
    p = lambda i: w.data_ptr() + 4 * i
    a, b = reserve_side_streams(torch.device("cuda", torch.cuda.current_device()))[:2]
    src = torch.zeros(1 << 22, device="cuda")
    dst = torch.zeros(4, 1 << 22, device="cuda")
    torch.cuda.synchronize()
    c0 = K.entry_signal_counts()
    for r in range(4):
        with torch.cuda.stream(b):
            K.sync_wait(p(4), p(2), p(1), True)          # (from the second round on: carries b's signal of the round before)
            dst[r].copy_(src)
        with torch.cuda.stream(a):
            for _ in range(8):
                src.add_(1.0)
            _lib.check(lib.n3d_entry_signal_arm(C.c_void_p(p(4)), C.c_void_p(p(0)), 1, C.c_void_p(a.cuda_stream)), "arm")
            K.sync_wait(p(5), p(0), p(1), False)         # stores flag 4 (and bumps a's step), THEN polls flag 5
        _lib.check(lib.n3d_entry_signal_arm(C.c_void_p(p(5)), C.c_void_p(p(2)), 0, C.c_void_p(b.cuda_stream)), "arm")
    _lib.check(lib.n3d_entry_signal_flush(C.c_void_p(b.cuda_stream)), "flush")
    assert K.entry_signal_pending() == 0
    torch.cuda.synchronize()
    c1 = K.entry_signal_counts()
    assert int(w[1]) == 0, "a device-side wait timed out"
    for r in range(4):
        assert float(dst[r].min()) == float(dst[r].max()) == 8.0 * (r + 1), r
    assert int(w[0]) == 5 and int(w[2]) == 5
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (7, 1)


def test_ping_pong_with_carried_signals_under_graph_replay():
    """both streams captured (n3d_stream_capture_begin): kernels.sync_signal(entry=True) holds the signals back, the wait kernels carry
    them, the last one goes out when its capture closes; device clock stamps show the order"""
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd.train import reserve_side_streams
    assert K.ENTRY_SIGNALS
    w = torch.zeros(16, dtype=torch.int32, device="cuda")
    w[0] = 1
    w[2] = 1
    p = lambda i: w.data_ptr() + 4 * i
    rounds, replays = 4, 3
    ta, tb = torch.zeros(rounds, dtype=torch.int64, device="cuda"), torch.zeros(rounds, dtype=torch.int64, device="cuda")
    a, b = reserve_side_streams(torch.device("cuda", torch.cuda.current_device()))[:2]
    torch.cuda.synchronize()
    c0 = K.entry_signal_counts()
    execs = []
    K.stream_capture_begin(b.cuda_stream)
    K.stream_capture_begin(a.cuda_stream)
    try:
        for r in range(rounds):
            with K.on_side(b):
                K.sync_wait(p(4), p(2), p(1), True)
                K.stamp(tb.data_ptr() + 8 * r)
                K.sync_signal(p(5), p(2), False, entry=True)
            with K.on_side(a):
                K.stamp(ta.data_ptr() + 8 * r)
                K.sync_signal(p(4), p(0), True, entry=True)
                assert K.entry_signal_pending() == 2
                K.sync_wait(p(5), p(0), p(1), False)
    finally:
        execs = [(K.stream_capture_end(b.cuda_stream), b), (K.stream_capture_end(a.cuda_stream), a)]
    assert K.entry_signal_pending() == 0
    c1 = K.entry_signal_counts()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2 * rounds - 1, 0)      # b's last signal: a plain launch from the capture's end
    try:
        for k in range(replays):
            for ex, st in execs:
                K.graph_launch(ex, st.cuda_stream)
            torch.cuda.synchronize()
            assert int(w[1]) == 0, "a device-side wait timed out"
            assert int(w[0]) == 1 + rounds * (k + 1) and int(w[2]) == 1 + rounds * (k + 1)
            assert bool((tb >= ta).all()) and bool((ta[1:] >= tb[:-1]).all()), (ta.tolist(), tb.tolist())
    finally:
        for ex, _ in execs:
            K.graph_destroy(ex)


# ---- 4. the trainer ---------------------------------------------------------------------------------------------------------------
CARRIERS = {"n3d_sync_wait", "n3d_sync_wait2", "n3d_conv_fwd", "n3d_conv_fwd2", "n3d_convT_fwd", "n3d_conv_bwd_data", "n3d_convT_bwd_data",
            "n3d_affine_act_bwd_reduce", "n3d_affine_act_bwd_reduce2", "n3d_affine_act_bwd_small", "n3d_affine_act_bwd_small2",
            "n3d_conv_k1_norm_fwd", "n3d_conv_k1_norm_bwd_reduce"}


def _train(entry):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench
    from kernel_table import Recorder
    from nas_3d_unet_amd import kernels as K, programs, searched
    from nas_3d_unet_amd.train import Trainer, reserve_side_streams
    dev = torch.device("cuda", torch.cuda.current_device())
    reserve_side_streams(dev)
    prev, K.ENTRY_SIGNALS = K.ENTRY_SIGNALS, entry
    try:
        torch.manual_seed(1234)
        programs._drop_serial[0] = 0      # the Dropout3d masks are seeded by torch's seed AND a per-process module serial number
        net = searched.SearchedNet(4, 4, 3, 4, 3, True, searched.Genotype(**bench.G_CONV)).to(dev)
        net.train()
        tr = Trainer(net, graph=True, side_wgrad="force")
        assert tr.side is not None and tr.side.stream is not None, "the side stream was not accepted on this box"
        xn, tn = bench.synthetic_batch(2, 32, 1)
        x, t = bench.to_patch_layout(torch.from_numpy(xn).to(dev)), torch.from_numpy(tn).to(dev)
        c0 = K.entry_signal_counts()
        with Recorder() as rec:
            losses = [tr.step(x, t).clone()]
        assert K.entry_signal_pending() == 0
        c1 = K.entry_signal_counts()
        losses += [tr.step(x, t).clone() for _ in range(2)]
        torch.cuda.synchronize()
        tr.check_sync()
        assert tr._use_side and tr.sync_timeouts() == 0
        return dict(flat=tr.fp.flat.clone(), m=tr.fp.exp_avg.clone(), v=tr.fp.exp_avg_sq.clone(), losses=torch.stack(losses), calls=rec.calls,
                    counts=(c1[0] - c0[0], c1[1] - c0[1]))
    finally:
        K.ENTRY_SIGNALS = prev


def test_trainer_step_is_bit_identical_with_entry_signals():
    on, off = _train(True), _train(False)
    for k in ("flat", "m", "v", "losses"):
        assert torch.equal(on[k], off[k]), k
    assert bool(torch.isfinite(on["losses"]).all())
    assert off["counts"] == (0, 0), off["counts"]
    assert on["counts"][0] > 0, on["counts"]
    # the captured pass (the last one recorded that arms anything): per stream, no stand-alone signal in front of a carrier
    val = lambda a: getattr(a, "value", a)
    starts = [i for i, (n, _) in enumerate(on["calls"]) if n == "n3d_pack_batch"] + [len(on["calls"])]
    segs = [on["calls"][a:b] for a, b in zip(starts[:-1], starts[1:])]
    seg = [s for s in segs if any(n == "n3d_entry_signal_arm" for n, _ in s)][-1]
    streams = {}
    for n, a in seg:
        if a and n != "n3d_entry_signal_pending":
            streams.setdefault(val(a[-1]), []).append(n)
    main = max(streams.values(), key=len)
    armed = sum(1 for n in main if n == "n3d_entry_signal_arm")
    assert armed >= 10, armed
    # (a signal launched by kernels.flush_entry_signals -- the end of the main graph's capture; the tail graph's wait follows on the same
    # stream -- comes right behind an n3d_entry_signal_flush call: that one had no successor in ITS graph)
    bad, closing = [], 0
    for i, n in enumerate(main):
        if n != "n3d_sync_signal":
            continue
        nxt = next((q for q in main[i + 1:] if q not in ("n3d_entry_signal_arm", "n3d_entry_signal_flush")), None)
        if nxt in CARRIERS:
            if i > 0 and main[i - 1] == "n3d_entry_signal_flush":
                closing += 1
            else:
                bad.append((i, nxt))
    assert not bad and closing <= 1, (bad, closing)
    # ... and whatever was armed on the main chain is followed by a launch of that stream (nothing rides past the end of the capture)
    last_arm = max(i for i, n in enumerate(main) if n == "n3d_entry_signal_arm")
    assert any(n not in ("n3d_entry_signal_arm", "n3d_entry_signal_flush") for n in main[last_arm + 1:])
