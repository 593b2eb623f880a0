"""Inputs and fp64 references for the kernels in the form a training step runs them (kernels.step_context): the batched slab reduction
n3d_wgrad_finalize_batch on synthetic jobs, the conv family with batch-packed weights and deferred weight gradients, and the stem's
recompute kernels n3d_conv_k1_norm_*.  numpy / torch CPU only (shared by test_step_form_ref_host.py and test_gpu_step_form.py).

Slab layout of a reduction job (include/n3d.h n3d_final_job, as the kernel comments state it):
  partial[c][p], p = tile * T + ci_l * co_t + co_l, T = ci_t * co_t, tile = (tap * tci + cit) * tco + cot, ntiles = taps * tci * tco
  pbias[c][cot * co_t + co_l]
  dw[co][ci][tap] (native (Co, Ci, taps)) = sum_c partial for ci = cit * ci_t + ci_l < Ci, co = cot * co_t + co_l < Co
  dbias[co] = sum_c pbias
The references below are written from this description."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

SENTINEL = np.float32(-7.31e9)       # fills every output buffer before a call; what a kernel must not touch keeps these bits
GUARD = 64                           # floats of sentinel in front of and behind every output

# ------------------------------------------------------------------------------------------ A. n3d_wgrad_finalize_batch
# has_pb: pbias / dbias present; has_dw: dw present (False: the bias gradient alone)
FinalSpec = collections.namedtuple("FinalSpec", "name nchunks taps tci tco ci_t co_t Ci Co has_pb has_dw")
N_FINAL_JOBS = 80                    # job records of one launch (N3D_FINAL_JOBS)
MAP_UNITS, MAP_GROUP = 512, 16       # entries of the workgroup -> job map, workgroups per entry (N3D_JOB_UNITS, 1 << N3D_FINAL_GSHIFT)
DIRECT_MAX = 16                      # N3D_FINAL_DIRECT_MAX


def fspec(name, nchunks, taps, tiles, Ci, Co, tci=None, tco=None, has_pb=True, has_dw=True):
    ci_t, co_t = tiles
    tci = -(-Ci // ci_t) if tci is None else tci
    tco = -(-Co // co_t) if tco is None else tco
    return FinalSpec(name, nchunks, taps, tci, tco, ci_t, co_t, Ci, Co, has_pb, has_dw)


def final_ntiles(s):
    return s.taps * s.tci * s.tco


def final_slab_floats(s):
    """floats of ONE chunk's slab / bias row"""
    return final_ntiles(s) * s.ci_t * s.co_t, s.tco * s.co_t


def final_path(s):
    """the branch of wgrad_final_batch_kernel a job takes, from the thresholds include/n3d.h and the issue document"""
    if s.nchunks == 0:
        return "none"
    if s.nchunks <= 4 and s.ci_t * s.co_t <= 256 and s.taps <= 27:
        return "tile"
    if s.nchunks <= 4:
        return "direct4"
    if s.nchunks <= DIRECT_MAX:
        return "direct16"
    return "many%d" % (64 if s.nchunks <= 64 else (16 if s.nchunks <= 256 else (8 if s.nchunks <= 1024 else 4)))


def final_blocks(s):
    """workgroups of a job"""
    path = final_path(s)
    if path == "none":
        return 0
    if path == "tile":
        return s.tci * s.tco
    ns, nb = final_slab_floats(s)
    per = 256 if path.startswith("direct") else int(path[4:])
    return -(-(ns + nb) // per)


def final_args_ok(s):
    """the argument checks n3d_wgrad_finalize_batch documents (nchunks == 0: nothing deferred, the job is skipped)"""
    if s.nchunks == 0:
        return True
    return (s.nchunks > 0 and 0 < final_ntiles(s) < 65536 and 0 < s.Co < 65536 and 0 < s.Ci < 65536 and 0 < s.tci < 256 and 0 < s.tco < 256
            and 0 < s.ci_t < 65536 and 0 < s.co_t < 65536 and 0 < s.taps < 256 and s.tci * s.ci_t >= s.Ci and s.tco * s.co_t >= s.Co)


def final_reference(s, partial, pbias):
    """-> (dw, dw_abs, db, db_abs) in fp64: the sums over chunks and the sums of magnitudes (for the error bound), dw as (Co, Ci, taps).
    partial: (nchunks, slab floats) fp32, pbias: (nchunks, tco * co_t) fp32 or None."""
    def fold(v):
        t = v.reshape(s.taps, s.tci, s.tco, s.ci_t, s.co_t).transpose(2, 4, 1, 3, 0)        # (tco, co_t, tci, ci_t, taps)
        return np.ascontiguousarray(t).reshape(s.tco * s.co_t, s.tci * s.ci_t, s.taps)[:s.Co, :s.Ci]
    dw = fold(partial.sum(axis=0, dtype=np.float64))
    dwa = fold(np.abs(partial).sum(axis=0, dtype=np.float64))
    if pbias is None:
        return dw, dwa, None, None
    return dw, dwa, pbias.sum(axis=0, dtype=np.float64)[:s.Co], np.abs(pbias).sum(axis=0, dtype=np.float64)[:s.Co]


def final_reference_loops(s, partial, pbias):
    """the same, one element at a time straight from the index formulas (tiny jobs only)"""
    T = s.ci_t * s.co_t
    dw = np.zeros((s.Co, s.Ci, s.taps))
    for co in range(s.Co):
        for ci in range(s.Ci):
            for tap in range(s.taps):
                cot, co_l, cit, ci_l = co // s.co_t, co % s.co_t, ci // s.ci_t, ci % s.ci_t
                p = ((tap * s.tci + cit) * s.tco + cot) * T + ci_l * s.co_t + co_l
                dw[co, ci, tap] = sum(float(partial[c, p]) for c in range(s.nchunks))
    db = None
    if pbias is not None:
        db = np.array([sum(float(pbias[c, (co // s.co_t) * s.co_t + co % s.co_t]) for c in range(s.nchunks)) for co in range(s.Co)])
    return dw, db


def final_bound(s, abs_sum):
    """|fp32 sum in any order - exact sum| <= (n - 1) u sum|v| + O(u^2) <= n 2^-24 sum|v|"""
    return s.nchunks * 2.0 ** -24 * abs_sum


def final_main_jobs():
    """every branch of the reduction kernel at the smallest job that reaches it, and the NULL / empty variants of each path"""
    j = [
        # tile path: <= 4 chunks, tile <= 256 floats
        fspec("tile27_8x16", 3, 27, (8, 16), 32, 32),
        fspec("tile27_8x16_ragged", 4, 27, (8, 16), 12, 24),           # ci tile 1 half empty, co tile 1 half empty
        fspec("tile27_dw12", 1, 27, (1, 12), 1, 12),                   # depthwise form: ci_t = 1, co_t = C, one tile per tap
        fspec("tile27_dw_ragged", 3, 27, (1, 16), 1, 12),
        fspec("tile1_4x4", 4, 1, (4, 4), 12, 4),
        fspec("tile1_4x4_ragged", 1, 1, (4, 4), 10, 6),
        # direct path: the 1x1x1 form, tile = the whole 48 x 16 matrix
        fspec("direct_2", 2, 1, (48, 16), 48, 16),
        fspec("direct_5", 5, 1, (48, 16), 48, 16),
        fspec("direct_16", 16, 1, (48, 16), 48, 16),
    ]
    # many-chunk path: both sides of every positions-per-workgroup threshold, counts off the 8 S and S strides
    for n in (17, 64, 65, 200, 256, 257, 1000, 1024, 1025, 2050):
        j.append(fspec("many_%d" % n, n, 1, (4, 4), 4, 12))
    j.append(fspec("many27_65", 65, 27, (16, 16), 16, 24))            # co tile 1 half empty
    # variants, once per path
    j += [
        fspec("tile_nobias", 3, 27, (8, 16), 8, 16, has_pb=False),
        fspec("direct_nobias", 7, 1, (48, 16), 48, 16, has_pb=False),
        fspec("many_nobias", 100, 1, (4, 4), 4, 12, has_pb=False),
        fspec("tile_biasonly", 2, 27, (8, 16), 16, 16, has_dw=False),
        fspec("direct_biasonly", 9, 1, (48, 16), 48, 16, has_dw=False),
        fspec("many_biasonly", 300, 1, (4, 4), 4, 12, has_dw=False),
        fspec("tile_empty", 0, 27, (8, 16), 8, 16),
        fspec("direct_empty", 0, 1, (48, 16), 48, 16),
        fspec("many_empty", 0, 1, (4, 4), 4, 12),
    ]
    order = np.random.default_rng(20240).permutation(len(j))
    jobs = [j[i] for i in order]
    # the empty jobs sit in the middle of the batch
    for name in ("tile", "direct", "many"):
        e = next(i for i, s in enumerate(jobs) if s.name == name + "_empty")
        jobs.insert(len(jobs) // 2, jobs.pop(e))
    return jobs


def final_many_small_jobs(n=200):
    """more jobs than one launch holds: small ones of every path in turn"""
    kinds = [lambda i: fspec("s%d_tile" % i, 1 + i % 4, 27, (4, 4), 4, 4), lambda i: fspec("s%d_direct" % i, 5 + i % 12, 1, (24, 12), 24, 12),
             lambda i: fspec("s%d_many" % i, 17 + 7 * (i % 40), 1, (4, 4), 4, 12), lambda i: fspec("s%d_tile1" % i, 2, 1, (4, 8), 12, 8),
             lambda i: fspec("s%d_empty" % i, 0, 1, (4, 4), 4, 4) if i % 35 == 4 else fspec("s%d_dw" % i, 3, 27, (1, 8), 1, 8)]
    return [kinds[i % 5](i) for i in range(n)]


def final_map_overflow_jobs():
    """workgroup counts that fill the 512-entry map (16 workgroups per entry) long before 80 jobs: twelve 1600-workgroup tile jobs
    (100 entries each) with many-chunk jobs of 327 workgroups (21 entries) between them"""
    jobs = []
    for i in range(12):
        jobs.append(fspec("ov%d_tile" % i, 1 + i % 4, 1, (4, 4), 160 - (i % 3), 160 - (i % 2)))
        if i % 2:
            jobs.append(fspec("ov%d_many" % i, 1025 + i, 27, (4, 4), 4, 12))
    return jobs


def final_giant_jobs():
    """single jobs larger than the whole map (> 8192 workgroups) between ordinary ones"""
    return [fspec("g_pre", 3, 27, (8, 16), 8, 16), fspec("g_tile", 2, 1, (4, 4), 384, 384), fspec("g_mid", 20, 1, (4, 4), 4, 12),
            fspec("g_many", 257, 27, (8, 16), 64, 64), fspec("g_post", 5, 1, (48, 16), 48, 16)]


def final_launch_plan(jobs):
    """how the documented limits cut a batch into launches: [(first job, jobs)], from the job count and the map alone (all the
    addresses of these tests fit one set of segments)"""
    plan, base = [], 0
    while base < len(jobs):
        units, m = 0, 0
        while base + m < len(jobs) and m < N_FINAL_JOBS:
            u = -(-final_blocks(jobs[base + m]) // MAP_GROUP)
            if units + u > MAP_UNITS:
                break
            units, m = units + u, m + 1
        m = max(m, 1)
        plan.append((base, m))
        base += m
    return plan


# ------------------------------------------------------------------------------------------ C. the stem's recompute kernels
# raw = W x + bias is never stored (include/n3d.h, n3d_conv_k1_norm_*): the statistics pass sums it, the normalise pass writes
# y = a raw + b, the backward passes recompute it from x.  Everything below is fp64 on the operands as the device holds them.
K1Case = collections.namedtuple("K1Case", "Ci Co B shape")
K1_CASES = {
    "K1": K1Case(4, 12, 2, (32, 32, 32)),      # 512-voxel chunks
    "K2": K1Case(4, 12, 1, (32, 33, 33)),      # last chunk of 32 voxels; last forward workgroup (1024 voxels) of 32
    "K3": K1Case(4, 12, 1, (32, 35, 37)),      # last chunk of 480 voxels: the second voxel of a trip is valid for some threads only
    "K4": K1Case(8, 4, 2, (32, 32, 40)),
    "K5": K1Case(4, 8, 3, (33, 32, 32)),
    "K6": K1Case(4, 4, 1, (64, 64, 64)),       # 1024-voxel chunks
    "K7": K1Case(4, 12, 1, (64, 64, 128)),     # 2048-voxel chunks
}
K1_MIXES = ("f32->f32", "bf16->f32", "f32->bf16", "bf16->bf16")      # storage of x -> storage of y / dout
K1_BF16_CASES = ("K1", "K2")
K1_CHAIN_CASES = ("K1", "K2", "K4")
K1_MARGIN = 1e-3
K1_MAX_PASSES = 8


def k1_chunk(N):
    """voxels per workgroup of the backward kernels: 2048, halved down to 512 while a sample has fewer than 256 workgroups"""
    chunk = 2048
    while chunk > 512 and -(-N // chunk) < 256:
        chunk //= 2
    return chunk


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def k1_raw(x, w, bias):
    """(B, Co, N) fp64: raw = W x + bias on x (B, Ci, N)"""
    raw = np.matmul(w.astype(np.float64), x.astype(np.float64))
    return raw if bias is None else raw + bias.astype(np.float64)[None, :, None]


def _near_zero_voxels(xv, bidx, w, bias, a, b, margin):
    """(M,) bool for voxels xv (M, Ci) of samples bidx (M,)"""
    w64, x64 = w.astype(np.float64), xv.astype(np.float64)
    raw, mag = x64 @ w64.T, np.abs(x64) @ np.abs(w64).T
    if bias is not None:
        raw, mag = raw + bias.astype(np.float64), mag + np.abs(bias.astype(np.float64))
    av, bv = a.astype(np.float64)[bidx], b.astype(np.float64)[bidx]
    return (np.abs(av * raw + bv) < margin * (np.abs(av) * mag + np.abs(bv))).any(axis=1)


def k1_near_zero(x, w, bias, a, b, margin=K1_MARGIN):
    """(B, N) bool: voxels where some channel's z = a raw + b lies within `margin` times the magnitude of its terms,
    |a| (|bias| + sum |x| |w|) + |b|, of zero -- fp32 (whose error is a few 2^-24 of that magnitude) could take the other side of the
    ReLU there"""
    B, Ci, N = x.shape
    xv = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(B * N, Ci)
    return _near_zero_voxels(xv, np.repeat(np.arange(B), N), w, bias, a, b, margin).reshape(B, N)


def k1_margin_x(rng, x, w, bias, a, b, bf16):
    """redraw x wherever a ReLU mask could differ between fp32 and fp64, with AND without the conv bias (both forms are run), until no
    such voxel is left.  bf16: x is rounded after every redraw and the check runs on the rounded values.  After the first pass only
    the redrawn voxels are looked at again (test_step_form_ref_host.py rechecks the whole tensor).  -> (x, voxels redrawn per pass)"""
    x = bf16_round(x) if bf16 else x.copy()
    bad = k1_near_zero(x, w, bias, a, b) | k1_near_zero(x, w, None, a, b)
    bi, vi = np.nonzero(bad)
    counts = [len(bi)]
    while len(bi):
        if len(counts) > K1_MAX_PASSES:
            raise AssertionError("k1_margin_x: voxels near a ReLU threshold left after %d passes: %s" % (K1_MAX_PASSES, counts))
        fresh = rng.standard_normal((len(bi), x.shape[1])).astype(np.float32)
        fresh = bf16_round(fresh) if bf16 else fresh
        x[bi, :, vi] = fresh
        still = _near_zero_voxels(fresh, bi, w, bias, a, b, K1_MARGIN) | _near_zero_voxels(fresh, bi, w, None, a, b, K1_MARGIN)
        bi, vi = bi[still], vi[still]
        counts.append(len(bi))
    return x, counts


@functools.lru_cache(maxsize=2)
def k1_inputs(cid, mix="f32->f32"):
    """x (B, Ci, N), dout (B, Co, N) as the device holds them (bf16 mixes: representable values), fp32 weight (Co, Ci) and bias -- the
    1x1x1 streaming kernels never round weights --, random forward coefficients a in [0.5, 1.5], b ~ N(0, 1) and backward coefficients
    A, Bc, Cc ~ N(0, 1) per (sample, channel)"""
    c = K1_CASES[cid]
    rng = np.random.default_rng(7000 + 10 * list(K1_CASES).index(cid) + K1_MIXES.index(mix))
    N = int(np.prod(c.shape))
    x16, d16 = mix.startswith("bf16"), mix.endswith("bf16")
    w = (rng.standard_normal((c.Co, c.Ci)) * 0.3).astype(np.float32)
    bias = rng.standard_normal(c.Co).astype(np.float32)
    a = rng.uniform(0.5, 1.5, (c.B, c.Co)).astype(np.float32)
    b = rng.standard_normal((c.B, c.Co)).astype(np.float32)
    x, counts = k1_margin_x(rng, rng.standard_normal((c.B, c.Ci, N)).astype(np.float32), w, bias, a, b, x16)
    dout = rng.standard_normal((c.B, c.Co, N)).astype(np.float32)
    if d16:
        dout = bf16_round(dout)
    A, Bc, Cc = (rng.standard_normal((c.B, c.Co)).astype(np.float32) for _ in range(3))
    gamma = (rng.uniform(0.5, 1.5, c.Co) * np.where(rng.random(c.Co) < 0.35, -1.0, 1.0)).astype(np.float32)
    beta = (rng.standard_normal(c.Co) * 0.2).astype(np.float32)
    return dict(case=c, N=N, x=x, dout=dout, w=w, bias=bias, a=a, b=b, A=A, Bc=Bc, Cc=Cc, gamma=gamma, beta=beta, redrawn=counts)


def k1_reference(inp, with_bias):
    """fp64 results of every pass on the random coefficients: stats (B, Co, 2), y (B, Co, N), and per relu in (False, True):
    sums (B, Co, 3) = (sum g, sum g raw, sum dout z) and dW (Co, Ci) = sum_b sum_v (A g + Cc raw + Bc) x"""
    x, d = inp["x"].astype(np.float64), inp["dout"].astype(np.float64)
    col = lambda k: inp[k].astype(np.float64)[:, :, None]
    raw = k1_raw(inp["x"], inp["w"], inp["bias"] if with_bias else None)
    out = dict(stats=np.stack([raw.sum(-1), (raw * raw).sum(-1)], axis=-1), y=col("a") * raw + col("b"))
    for relu in (False, True):
        z = out["y"]
        g = np.where(z > 0, d, 0.0) if relu else d
        zz = np.maximum(z, 0.0) if relu else z
        out["sums", relu] = np.stack([g.sum(-1), (g * raw).sum(-1), (d * zz).sum(-1)], axis=-1)
        draw = col("A") * g + col("Cc") * raw + col("Bc")
        out["dw", relu] = np.einsum("bon,bcn->oc", draw, x)
    return out


def k1_chain_reference(inp, with_bias, G):
    """y = GroupNorm_G(conv1x1(x)) and its fp64 autograd under dout: y, dW, dgamma, dbeta and the conv-bias gradient"""
    c = inp["case"]
    x = torch.from_numpy(inp["x"]).double()
    w = torch.from_numpy(inp["w"]).double().requires_grad_(True)
    cb = torch.from_numpy(inp["bias"]).double() if with_bias else torch.zeros(c.Co, dtype=torch.float64)
    cb.requires_grad_(True)
    gm = torch.from_numpy(inp["gamma"]).double().requires_grad_(True)
    bt = torch.from_numpy(inp["beta"]).double().requires_grad_(True)
    raw = torch.einsum("oc,bcn->bon", w, x) + cb[None, :, None]
    y = F.group_norm(raw, G, gm, bt, 1e-5)
    (y * torch.from_numpy(inp["dout"]).double()).sum().backward()
    return dict(y=y.detach().numpy(), dw=w.grad.numpy(), dgamma=gm.grad.numpy(), dbeta=bt.grad.numpy(), dbias=cb.grad.numpy(),
                raw=raw.detach().numpy())


# ------------------------------------------------------------------------------------------ B. the conv family in trainer form
# (Cin, Cout, k, stride, dil, transposed, B, spatial of the conv INPUT, depthwise, storage): the smallest shape of every kernel family of
# tests/test_gpu_conv.py (CASES and the depthwise table) and, with bf16 storage on both sides, of tests/test_gpu_bf16.py
ConvCase = collections.namedtuple("ConvCase", "cin cout k stride dil transposed B shape depthwise bf16")
_F, _T = False, True
CONV_CASES = [ConvCase(*r, False, False) for r in [
    (4, 4, 3, 1, 1, _F, 2, (8, 10, 12)), (4, 12, 3, 2, 1, _F, 2, (8, 8, 12)), (8, 8, 3, 2, 1, _T, 2, (4, 4, 6)),
    (16, 16, 3, 1, 1, _F, 2, (8, 8, 8)), (16, 16, 3, 1, 1, _F, 2, (16, 16, 16)), (32, 32, 3, 1, 1, _F, 1, (16, 32, 32)),
    (64, 64, 3, 1, 1, _F, 2, (2, 2, 2)), (64, 32, 3, 1, 1, _F, 3, (12, 8, 8)), (16, 16, 3, 2, 1, _T, 2, (8, 16, 32)),
    (192, 64, 1, 1, 1, _F, 2, (2, 2, 2)), (12, 3, 1, 1, 1, _F, 2, (8, 8, 8)), (12, 4, 1, 1, 1, _F, 2, (32, 33, 32)),
    (4, 4, 3, 1, 1, _F, 2, (8, 8, 64)), (8, 8, 3, 2, 1, _F, 2, (8, 8, 32)), (8, 8, 3, 2, 1, _F, 2, (32, 32, 64)),
    (4, 12, 3, 2, 1, _F, 2, (64, 64, 64))]]
CONV_CASES += [ConvCase(8, 8, 3, 1, 1, _F, 2, (8, 12, 32), True, False), ConvCase(16, 16, 3, 2, 1, _T, 2, (4, 4, 6), True, False)]
CONV_CASES += [ConvCase(*r, False, True) for r in [(4, 4, 3, 1, 1, _F, 2, (8, 16, 16)), (8, 8, 3, 2, 1, _F, 2, (8, 16, 16)),
                                                   (4, 4, 3, 2, 1, _T, 2, (4, 8, 8)),
                                                   # the smallest bf16 stride-2 shape on the bf16 MFMA kernels (W / 2 >= 16): the only
                                                   # way to packed layout 5 (its data gradient), which the three rows above do not reach
                                                   (4, 4, 3, 2, 1, _F, 2, (8, 8, 32))]]


# what every row reaches today: (packed layout of the forward form, of the data-gradient form, branch of the slab reduction its deferred
# weight gradient takes).  Layouts: 0 generic, 1 gemm16, 2 vox64, 3 vox_up, 4 / 5 = 2 / 3 in bfloat16, -1 = native weights (depthwise).
# Asserted by the tests, so that a retuned kernel selection says "look at what the table still covers" instead of silently moving a row.
CONV_REACHES = {
    "4-4_k3s1_B2_8x10x12": (0, 0, "tile"), "4-12_k3s2_B2_8x8x12": (0, 0, "tile"), "8-8_k3s2T_B2_4x4x6": (0, 0, "tile"),
    "16-16_k3s1_B2_8x8x8": (1, 1, "direct16"), "16-16_k3s1_B2_16x16x16": (1, 1, "many64"), "32-32_k3s1_B1_16x32x32": (1, 1, "many64"),
    "64-64_k3s1_B2_2x2x2": (1, 1, "tile"), "64-32_k3s1_B3_12x8x8": (1, 1, "many64"), "16-16_k3s2T_B2_8x16x32": (1, 1, "many64"),
    "192-64_k1s1_B2_2x2x2": (1, 1, "tile"), "12-3_k1s1_B2_8x8x8": (0, 0, "tile"), "12-4_k1s1_B2_32x33x32": (0, 0, "many16"),
    "4-4_k3s1_B2_8x8x64": (2, 2, "direct16"), "8-8_k3s2_B2_8x8x32": (2, 3, "tile"), "8-8_k3s2_B2_32x32x64": (2, 3, "many64"),
    "4-12_k3s2_B2_64x64x64": (0, 0, "many64"), "dw8-8_k3s1_B2_8x12x32": (-1, -1, "many64"), "dw16-16_k3s2T_B2_4x4x6": (-1, -1, "tile"),
    "4-4_k3s1_B2_8x16x16_bf16": (4, 4, "direct16"), "8-8_k3s2_B2_8x16x16_bf16": (0, 0, "tile"), "4-4_k3s2T_B2_4x8x8_bf16": (0, 0, "tile"),
    "4-4_k3s2_B2_8x8x32_bf16": (4, 5, "tile"),
}


def final_path_of(nchunks, ci_t, co_t, taps):
    return final_path(FinalSpec("", nchunks, taps, 1, 1, ci_t, co_t, ci_t, co_t, True, True))


def conv_case_id(c):
    return "%s%d-%d_k%ds%d%s_B%d_%s%s" % ("dw" if c.depthwise else "", c.cin, c.cout, c.k, c.stride, "T" if c.transposed else "", c.B,
                                          "x".join(map(str, c.shape)), "_bf16" if c.bf16 else "")


def conv_padding(k, stride, dil):
    """the reference's padding rule for its conv primitives (prim_ops.py): 'same' for stride 1, half the dilated kernel otherwise"""
    return dil * (k - 1) // 2


def conv_out_shape(c):
    pad = conv_padding(c.k, c.stride, c.dil)
    if c.transposed:
        return tuple((i - 1) * c.stride - 2 * pad + c.dil * (c.k - 1) + (0 if c.stride == 1 else 1) + 1 for i in c.shape)
    return tuple((i + 2 * pad - c.dil * (c.k - 1) - 1) // c.stride + 1 for i in c.shape)


# n3d_pack_batch: 160 job records per launch, a 512-entry workgroup -> job map with 4 workgroups per entry (include/n3d.h, kernel comments)
N_PACK_JOBS, PACK_GROUP = 160, 4


def pack_blocks(Co, Ci, taps, data_grad, layout, cdp):
    """workgroups of one pack job: 3x3x3 weights go by 16 x 16 (source, destination) channel tiles, others by 256 elements of a tap"""
    Cs, Cd = (Co, Ci) if data_grad else (Ci, Co)
    if taps == 27:
        return -(-Cs // 16) * -(-(cdp if layout == 0 else Cd) // 16)
    return -(-(Cs * cdp if layout == 0 else (Cs * Cd if layout == 1 else Co * Co)) // 256)


def pack_launch_plan(blocks):
    """[(jobs of the launch, why it ended: 'table' | 'map' | 'end')] from the job cap and the map"""
    plan, base = [], 0
    while base < len(blocks):
        units, m, why = 0, 0, "end"
        while base + m < len(blocks):
            if m == N_PACK_JOBS:
                why = "table"
                break
            u = -(-blocks[base + m] // PACK_GROUP)
            if units + u > MAP_UNITS:
                why = "map"
                break
            units, m = units + u, m + 1
        plan.append((max(m, 1), why))
        base += max(m, 1)
    return plan


def _mk(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


@functools.lru_cache(maxsize=None)
def conv_weights(i):
    """weight and bias of table row i: fp32 rows as test_conv_family / test_depthwise_family draw them, bf16 rows as
    test_conv_family_bf16_storage does (weights representable in bf16)"""
    c = CONV_CASES[i]
    if c.bf16:
        rng = np.random.default_rng(c.cin * 1000 + c.cout * 10 + c.k + c.stride)
        rng.standard_normal((c.B, c.cin) + c.shape)
        w = bf16_round(rng.standard_normal((c.cin, c.cout) + (c.k,) * 3 if c.transposed else (c.cout, c.cin) + (c.k,) * 3) * 0.2)
        return w, rng.standard_normal(c.cout).astype(np.float32) * 0.1
    if c.depthwise:
        return _mk((c.cin, 1, 3, 3, 3), 2, 0.2), _mk((c.cin,), 3, 0.1)
    wshape = (c.cin, c.cout) + (c.k,) * 3 if c.transposed else (c.cout, c.cin) + (c.k,) * 3
    return _mk(wshape, 2, 1.0 / np.sqrt(c.cin * c.k ** 3)), _mk((c.cout,), 3, 0.1)


@functools.lru_cache(maxsize=2)
def conv_reference(i):
    """x, dy and the torch-CPU results y, dx, dw, db of row i, by the references of the standalone tests: fp32 rows F.conv3d /
    F.conv_transpose3d in fp32 (test_conv_family, test_depthwise_family), bf16 rows the same on bf16-rounded operands"""
    c = CONV_CASES[i]
    pad = conv_padding(c.k, c.stride, c.dil)
    wn, bn = conv_weights(i)
    if c.bf16:
        rng = np.random.default_rng(c.cin * 1000 + c.cout * 10 + c.k + c.stride)
        xn = bf16_round(rng.standard_normal((c.B, c.cin) + c.shape))
    else:
        xn = _mk((c.B, c.cin) + c.shape, 1)
    x, w, b = (torch.from_numpy(a).requires_grad_(True) for a in (xn, wn, bn))
    groups = c.cin if c.depthwise else 1
    if c.transposed:
        y = F.conv_transpose3d(x, w, b, stride=c.stride, padding=pad, output_padding=0 if c.stride == 1 else 1, dilation=c.dil, groups=groups)
    else:
        y = F.conv3d(x, w, b, stride=c.stride, padding=pad, dilation=c.dil, groups=groups)
    dyn = bf16_round(_mk(tuple(y.shape), 5)) if c.bf16 else _mk(tuple(y.shape), 5)
    y.backward(torch.from_numpy(dyn))
    return dict(x=xn, dy=dyn, w=wn, b=bn, y=y.detach().numpy(), dx=x.grad.numpy(), dw=w.grad.numpy(), db=b.grad.numpy())
