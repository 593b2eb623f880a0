"""fp64 torch-CPU restatements of the epilogue, SE-gate, pooling and depthwise-batch kernels, and the builders of their test inputs
(shared by test_epilogue_ref_host.py, which checks the builders and closed forms on the CPU, and test_gpu_epilogue_reference.py).

Formulas are those of the reference modules: GroupNorm(G, C, eps 1e-5) -> [ReLU] -> weight w -> node sum (prim_ops.py:56-63,75-80,
cell.py:29-32,76-81); SE = mean -> Linear(C, 1) -> ReLU -> Linear(1, C) -> sigmoid -> w * x * gate (prim_ops.py:133-152); avg / max
pooling with kernel 2, stride 2 (prim_ops.py:160-163); depthwise conv3d / conv_transpose3d (prim_ops.py:95-110).  Gradients are torch
autograd in fp64.  The fields of include/n3d.h that no module has are closed forms: dalpha = <dout, z>, dbias_conv = channel sum of
d(raw), sumraw = channel sum of raw, mean_rstd = (mean, 1 / sqrt(var + eps)) per (sample, group)."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
W_SCALAR = 0.37         # the device scalar behind `wptr` where a case has one


def w64(w):
    """the weight scalar as the device holds it (fp32), None = 1"""
    return 1.0 if w is None else float(np.float32(w))


def real_channels(C, G):
    """G < 0: ONE group of -G real channels stored in C zero-padded ones (include/n3d.h, "padded channels")"""
    return -G if G < 0 else C


def n_groups(G):
    return 1 if G < 0 else G


def pad_c(t, C, axis=1):
    """zero-pad the channel axis of a torch tensor to C"""
    if t.shape[axis] == C:
        return t
    shape = list(t.shape)
    shape[axis] = C - t.shape[axis]
    return torch.cat([t, torch.zeros(shape, dtype=t.dtype)], dim=axis)


# ------------------------------------------------------------------------------------------ input builders
def draw_gamma_beta(rng, C, real=None):
    """|gamma| in [0.5, 1.5] with some negative entries (so a margin pass moves z far enough), beta ~ 0.2 N(0, 1); padded entries zero"""
    real = C if real is None else real
    gamma = rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.35, -1.0, 1.0)
    gamma[1] = -abs(gamma[1])
    gamma[0] = abs(gamma[0])
    beta = rng.standard_normal(C) * 0.2
    gamma[real:] = 0.0
    beta[real:] = 0.0
    return gamma.astype(np.float32), beta.astype(np.float32)


def draw_tensor(rng, B, C, shape, real=None, scale=1.0, shift=0.0):
    t = (rng.standard_normal((B, C) + tuple(shape)) * scale + shift).astype(np.float32)
    if real is not None:
        t[:, real:] = 0.0
    return t


def gn_z(raw, G, gamma, beta):
    """z = GroupNorm(raw) of the REAL channels in fp64 (numpy fp32 in, numpy fp64 out)"""
    r = real_channels(raw.shape[1], G)
    x = torch.from_numpy(np.ascontiguousarray(raw[:, :r])).double()
    return F.group_norm(x, n_groups(G), torch.from_numpy(gamma[:r]).double(), torch.from_numpy(beta[:r]).double(), EPS).numpy()


def margin_inputs(raw, G, gamma, beta, near=1e-3, step=0.05, floor=5e-4, max_passes=4):
    """ReLU masks that agree by construction: fp32 and fp64 can only disagree on a * raw + b > 0 where |z| is of the order of the
    rounding error, so every element with |z| < `near` is moved by `step` in the direction sign(z) * sign(gamma) -- away from zero -- and
    the result must keep min|z| >= `floor` (asserted).  Returns (raw fp32, min|z|, passes)."""
    raw = np.array(raw, dtype=np.float32, copy=True)
    r = real_channels(raw.shape[1], G)
    sg = np.where(gamma[:r] < 0, -1.0, 1.0).astype(np.float32)[None, :, None, None, None]
    passes = 0
    for _ in range(max_passes):
        z = gn_z(raw, G, gamma, beta)
        close = np.abs(z) < near
        if not close.any():
            break
        move = (step * np.where(z >= 0, 1.0, -1.0) * sg).astype(np.float32)
        view = raw[:, :r]
        view[close] += move[close]
        passes += 1
    zmin = float(np.abs(gn_z(raw, G, gamma, beta)).min())
    assert zmin >= floor, "margin_inputs: min|z| = %.3e after %d passes" % (zmin, passes)
    return raw, zmin, passes


# ------------------------------------------------------------------------------------------ one epilogue term
def term_reference(raw, gamma, beta, G, relu, w, dout):
    """y = w * act(GN(raw)) (gamma None: no norm) and its backward under the output gradient dout, all fp64.  Tensors come back with the
    full (padded) channel count; on padded channels everything is 0 except `draw`, see twin_draw()."""
    B, C = raw.shape[:2]
    r, g = real_channels(C, G), n_groups(G)
    x = torch.from_numpy(np.ascontiguousarray(raw[:, :r])).double().requires_grad_(True)
    cb = torch.zeros(r, dtype=torch.float64, requires_grad=True)      # the bias of the conv that produced raw
    wt = torch.tensor(w64(w), dtype=torch.float64, requires_grad=True)
    d = torch.from_numpy(np.ascontiguousarray(dout[:, :r])).double()
    u = x + cb[None, :, None, None, None]
    out = {}
    if gamma is not None:
        gm = torch.from_numpy(gamma[:r]).double().requires_grad_(True)
        bt = torch.from_numpy(beta[:r]).double().requires_grad_(True)
        zn = F.group_norm(u, g, gm, bt, EPS)
    else:
        zn = u
    z = F.relu(zn) if relu else zn
    y = wt * z
    (y * d).sum().backward()
    xd = x.detach()
    out["y"], out["z"], out["draw"] = pad_c(y.detach(), C), pad_c(z.detach(), C), pad_c(x.grad, C)
    out["dalpha"], out["dbias_conv"] = wt.grad.reshape(1), pad_c(cb.grad, C, 0)
    out["stats"] = pad_c(torch.stack([xd.sum((2, 3, 4)), (xd * xd).sum((2, 3, 4))], dim=-1), C)          # (B, C, 2)
    out["sumraw"] = out["stats"][..., 0]
    gmask = d * (zn.detach() > 0) if relu else d
    out["sums"] = pad_c(torch.stack([gmask.sum((2, 3, 4)), (gmask * xd).sum((2, 3, 4)), (d * z.detach()).sum((2, 3, 4))], dim=-1), C)
    if gamma is not None:
        out["dgamma"], out["dbeta"] = pad_c(gm.grad, C, 0), pad_c(bt.grad, C, 0)
        xg = xd.reshape(B, g, -1)
        mean = xg.mean(-1)
        rstd = 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + EPS)
        out["mean_rstd"] = torch.stack([mean, rstd], dim=-1)                                          # (B, g, 2)
        cg = r // g
        a = gm.detach()[None, :] * rstd.repeat_interleave(cg, dim=1)
        out["a"] = pad_c(a, C)
        out["b"] = pad_c(bt.detach()[None, :] - mean.repeat_interleave(cg, dim=1) * a, C)
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def dalpha_closed(dout, z):
    """n3d.h: dalpha of a term = <dout, z_k>"""
    return float((np.asarray(dout, np.float64) * np.asarray(z, np.float64)).sum())


def dbias_conv_closed(draw):
    """n3d.h: dbias_conv = channel sum of d(raw)"""
    return np.asarray(draw, np.float64).sum(axis=(0, 2, 3, 4))


def twin_forward(x, gamma, beta, real, relu):
    """GroupNorm of the zero-padded twin: ONE group over all stored channels whose sums are divided by N * real (the padded channels
    hold zeros, so the sums are the real tensor's).  x: fp64 torch (B, C, ...), gamma / beta: fp64 torch (C,) with zero padded entries."""
    B = x.shape[0]
    n = real * int(np.prod(x.shape[2:]))
    flat = x.reshape(B, -1)
    mean = flat.sum(1) / n
    var = (flat * flat).sum(1) / n - mean * mean
    rstd = 1.0 / torch.sqrt(var + EPS)
    bc = lambda v: v[:, None, None, None, None]
    z = (x - bc(mean)) * bc(rstd) * gamma[None, :, None, None, None] + beta[None, :, None, None, None]
    return F.relu(z) if relu else z


def twin_draw(raw, gamma, beta, G, relu, w, dout):
    """d(raw) of the padded twin on ALL stored channels (fp64 autograd).  On the real channels it is GroupNorm(1, real)'s; on a padded
    channel it is the group's coupling term (the twin's mean and variance do depend on that channel), which the trainers mask."""
    x = torch.from_numpy(raw).double().requires_grad_(True)
    z = twin_forward(x, torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), real_channels(raw.shape[1], G), relu)
    (w64(w) * z * torch.from_numpy(dout).double()).sum().backward()
    return x.grad.numpy()


Single = collections.namedtuple("Single", "C shape B G fused ragged slice pitch acc w relu bias dalpha")
# (C, spatial, B, G) and what they reach: the issue's table A; fused / ragged = the regime the row mapping (ew_map) gives them today,
# which the GPU test asserts through K.stats_rows so that a retuning says "pick new shapes".  Options, each in at least two cases:
# slice = raw is a channel slice of a 3C-wide buffer, pitch = out and d(raw) have pitch C + 4, acc = N3D_ACCUMULATE onto previous
# content, w = a device weight scalar, relu, bias = dbias_conv with the forward's sumraw, dalpha.
SINGLE_CASES = {
    "A1": Single(12, (6, 10, 14), 3, 1, True, True, True, True, False, True, True, False, True),
    "A2": Single(12, (40, 42, 44), 2, 1, True, True, False, False, True, False, True, True, False),
    "A3": Single(24, (14, 18, 22), 1, 1, False, False, False, False, False, True, False, True, True),
    "A4": Single(48, (14, 18, 22), 5, 3, True, True, False, True, True, False, True, False, True),
    "A5": Single(64, (40, 42, 44), 1, 4, False, False, True, False, False, True, True, True, False),
    "A6": Single(4, (40, 42, 44), 3, 1, False, True, False, False, False, False, False, False, True),
    "A7": Single(8, (6, 10, 14), 2, -6, True, True, False, True, False, True, True, False, True),
    "A8": Single(32, (2, 2, 2), 2, 2, True, True, True, False, True, False, False, True, False),
    "A9": Single(4, (32, 32, 32), 2, 1, True, False, True, False, False, True, True, False, False),
    "A10": Single(4, (32, 32, 33), 2, 1, False, False, False, True, True, False, False, False, True),
}


@functools.lru_cache(maxsize=2)
def single_inputs(cid):
    c = SINGLE_CASES[cid]
    rng = np.random.default_rng(1000 + list(SINGLE_CASES).index(cid))
    real = real_channels(c.C, c.G)
    gamma, beta = draw_gamma_beta(rng, c.C, real)
    raw, zmin, passes = margin_inputs(draw_tensor(rng, c.B, c.C, c.shape, real, 1.5, 0.3), c.G, gamma, beta)
    # (padded channels of the output gradient are zero, as in a padded net: their consumers have zero weights)
    return dict(raw=raw, gamma=gamma, beta=beta, dout=draw_tensor(rng, c.B, c.C, c.shape, real), prev_out=draw_tensor(rng, c.B, c.C, c.shape, real),
                prev_draw=draw_tensor(rng, c.B, c.C, c.shape), zmin=zmin, passes=passes)


# ------------------------------------------------------------------------------------------ N-term node
NTerm = collections.namedtuple("NTerm", "C shape B G terms acc bias")
_MIX8 = [True, False, True, True, False, True, False, True]
# terms: (kind, relu, w): kind "gn" = GroupNorm term, "plain" = a = b = None (the node's other primitives ride in the same pass)
NTERM_CASES = {
    "B1": NTerm(4, (6, 10, 14), 3, 1, [("gn", r, 0.1 + 0.1 * k) for k, r in enumerate(_MIX8)], False, False),
    "B2": NTerm(16, (14, 18, 22), 2, 1, [("gn", True, 0.6), ("plain", False, 0.25), ("gn", False, None), ("plain", True, None), ("gn", True, 0.15)],
                True, False),
    "B3": NTerm(64, (4, 4, 6), 5, 4, [("gn", True, 0.5), ("gn", False, None), ("gn", True, 0.3)], False, True),
    "B4": NTerm(8, (40, 42, 44), 1, 1, [("gn", True, None), ("gn", False, 0.7)], False, False),
    "B5": NTerm(32, (2, 2, 2), 2, 2, [("gn", r, 0.9 - 0.1 * k) for k, r in enumerate(_MIX8)], False, True),
    # reduction rows only (n3d_affine_act_bwd_reduceN with all 16 terms) and n3d_plain_bwd_coeffsN on the plain ones
    "B6": NTerm(16, (4, 4, 6), 2, 1, [("gn", r, None) for r in _MIX8] + [("plain", not r, None) for r in _MIX8], False, False),
}


@functools.lru_cache(maxsize=2)
def nterm_inputs(cid):
    c = NTERM_CASES[cid]
    rng = np.random.default_rng(2000 + list(NTERM_CASES).index(cid))
    terms = []
    for kind, relu, w in c.terms:
        raw = draw_tensor(rng, c.B, c.C, c.shape, None, 1.5, 0.3)
        t = dict(kind=kind, relu=relu, w=w, gamma=None, beta=None, zmin=None, passes=0)
        if kind == "gn":
            t["gamma"], t["beta"] = draw_gamma_beta(rng, c.C)
            raw, t["zmin"], t["passes"] = margin_inputs(raw, c.G, t["gamma"], t["beta"])
        t["raw"] = raw
        terms.append(t)
    return dict(terms=terms, dout=draw_tensor(rng, c.B, c.C, c.shape), prev=draw_tensor(rng, c.B, c.C, c.shape))


def node_reference(inp, G, acc):
    """node = prev + sum_k w_k * act_k(GN_k(raw_k)) in fp64 and the backward of every term under the node gradient"""
    refs = [term_reference(t["raw"], t["gamma"], t["beta"], G, t["relu"], t["w"], inp["dout"]) for t in inp["terms"]]
    node = inp["prev"].astype(np.float64) if acc else 0.0
    for r in refs:
        node = node + r["y"]
    return node, refs


# ------------------------------------------------------------------------------------------ SE gates
SeCase = collections.namedtuple("SeCase", "C shape B gates w")
SE_CASES = {
    "C1": SeCase(8, (6, 10, 14), 1, 1, None),
    "C2": SeCase(16, (4, 4, 6), 2, 3, W_SCALAR),      # B = 2: the 512-thread two-sample kernels
    "C3": SeCase(64, (2, 2, 2), 3, 3, W_SCALAR),
    "C4": SeCase(4, (14, 18, 22), 2, 8, None),
}
SE_MARGIN = 0.1     # |pre-activation of the hidden unit| of every sample


def se_chain(x, w1, b1, w2, b2):
    """(mean, pre-activation, hidden, gate) of prim_ops.py:133-139,148-152 on fp64 torch tensors: w1 (1, C), b1 (1,), w2 (C, 1), b2 (C,)"""
    mean = x.mean(dim=(2, 3, 4))
    pre = mean @ w1.t() + b1              # (B, 1)
    hidden = F.relu(pre)
    gate = torch.sigmoid(hidden @ w2.t() + b2)
    return mean, pre[:, 0], hidden[:, 0], gate


def draw_se_gate(rng, B, C, shape):
    """one gate: input, fc parameters with fc[0].bias chosen so that the hidden unit's pre-activation is at least 0.2 from zero for
    every sample, with (B >= 2) at least one live and one dead sample"""
    x = draw_tensor(rng, B, C, shape, None, 1.0, 0.2)
    x += (0.5 * rng.permutation(B)).astype(np.float32)[:, None, None, None, None]      # sample means far enough apart
    w1 = (rng.standard_normal((1, C)) * 0.5).astype(np.float32)
    w2 = (rng.standard_normal((C, 1)) * 0.8).astype(np.float32)
    b2 = (rng.standard_normal(C) * 0.3).astype(np.float32)
    p = np.sort((x.astype(np.float64).mean(axis=(2, 3, 4)) @ w1.astype(np.float64).T)[:, 0])
    if B == 1:
        b1 = 0.3 - p[0]
    else:
        gaps = np.diff(p)
        k = int(np.argmax(gaps))
        if gaps[k] < 0.4:
            s = np.float32(0.4 / gaps[k] * 1.01)
            w1, p = w1 * s, p * float(s)
        b1 = -0.5 * (p[k] + p[k + 1])
    return dict(x=x, w1=w1, b1=np.array([b1], np.float32), w2=w2, b2=b2)


@functools.lru_cache(maxsize=2)
def se_inputs(cid):
    c = SE_CASES[cid]
    rng = np.random.default_rng(3000 + list(SE_CASES).index(cid))
    gates = [draw_se_gate(rng, c.B, c.C, c.shape) for _ in range(c.gates)]
    return dict(gates=gates, dout=draw_tensor(rng, c.B, c.C, c.shape))


def se_reference(g, w, dout):
    """y = w * x * gate(x) and its fp64 autograd: dx, dw1, db1, dw2, db2, dalpha; also asserts the hidden unit's margin"""
    x = torch.from_numpy(g["x"]).double().requires_grad_(True)
    p = {k: torch.from_numpy(g[k]).double().requires_grad_(True) for k in ("w1", "b1", "w2", "b2")}
    wt = torch.tensor(w64(w), dtype=torch.float64, requires_grad=True)
    mean, pre, hidden, gate = se_chain(x, p["w1"], p["b1"], p["w2"], p["b2"])
    assert float(pre.detach().abs().min()) >= SE_MARGIN, "SE hidden unit too close to its ReLU threshold"
    y = wt * x * gate[:, :, None, None, None]
    (y * torch.from_numpy(dout).double()).sum().backward()
    out = dict(mean=mean, pre=pre, hidden=hidden, gate=gate, y=y, dx=x.grad, dw1=p["w1"].grad, db1=p["b1"].grad, dw2=p["w2"].grad,
               db2=p["b2"].grad, dalpha=wt.grad.reshape(1))
    return {k: v.detach().numpy() for k, v in out.items()}


# ------------------------------------------------------------------------------------------ pooling
PoolCase = collections.namedtuple("PoolCase", "C shape B pitched")
POOL_CASES = {
    "D1": PoolCase(4, (2, 2, 2), 1, False),
    "D2": PoolCase(8, (6, 10, 14), 3, True),       # one partial block
    "D3": PoolCase(12, (8, 6, 4), 2, True),
    "D4": PoolCase(64, (4, 4, 6), 2, False),
    "D5": PoolCase(4, (16, 18, 34), 1, False),     # five blocks, the last one ragged
}
POOL_FAMILIES = ("normal", "tie", "tie_relu")
_TIE_LEVEL_P = (0.10, 0.10, 0.10, 0.10, 0.12, 0.07, 0.07, 0.09, 0.25)      # of the levels -1, -0.75, ..., 1


@functools.lru_cache(maxsize=4)
def pool_inputs(cid, family):
    c = POOL_CASES[cid]
    rng = np.random.default_rng(4000 + 10 * list(POOL_CASES).index(cid) + POOL_FAMILIES.index(family))
    shp = (c.B, c.C) + c.shape
    if family == "normal":
        x = rng.standard_normal(shp).astype(np.float32)
    else:
        # multiples of 0.25 in [-1, 1], the top level the most frequent one (most windows then hold their maximum several times); half
        # of the zeros negative; the first window of channel 0 all equal, that of channel 1 with a zero of either sign,
        x = (rng.choice(np.arange(-4, 5), size=shp, p=_TIE_LEVEL_P) * 0.25).astype(np.float32)
        x[(x == 0) & (rng.random(shp) < 0.5)] = -0.0
        if family == "tie_relu":
            x = torch.relu(torch.from_numpy(x)).numpy()
        x[:, 0, :2, :2, :2] = 0.5
        x[:, 1, 0, 0, :2] = (-0.0, 0.0)
        x[:, 2, 0, 0, :2] = 1.0                       # ... that of channel 2 with its maximum in the first two places
    out = (c.B, c.C) + tuple(s // 2 for s in c.shape)
    return dict(x=x, dy=rng.standard_normal(out).astype(np.float32), prev=rng.standard_normal(shp).astype(np.float32))


def pool_windows(x):
    """(B, C, Do, Ho, Wo, 8): the 2x2x2 windows in (d, h, w) scan order"""
    B, C, D, H, W = x.shape
    w = x.reshape(B, C, D // 2, 2, H // 2, 2, W // 2, 2)
    return np.ascontiguousarray(w.transpose(0, 1, 2, 4, 6, 3, 5, 7)).reshape(B, C, D // 2, H // 2, W // 2, 8)


def tie_fractions(x):
    """(fraction of windows with several equal maxima, number of windows whose 8 elements are all equal)"""
    w = pool_windows(x)
    several = (w == w.max(axis=-1, keepdims=True)).sum(axis=-1) > 1
    return float(several.mean()), int((w.min(axis=-1) == w.max(axis=-1)).sum())


def pool_reference(x, dy, is_max, dtype=torch.float64):
    """(y, dx) of F.avg_pool3d / F.max_pool3d (kernel 2, stride 2) under the output gradient dy, on the CPU in `dtype`; torch's max
    backward goes to the first arg-max in (d, h, w) scan order"""
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    y = F.max_pool3d(xt, 2, 2) if is_max else F.avg_pool3d(xt, 2, 2)
    (y * torch.from_numpy(dy).to(dtype)).sum().backward()
    return y.detach(), xt.grad


# ------------------------------------------------------------------------------------------ depthwise batch
DwCase = collections.namedtuple("DwCase", "C shape B")
DW_CASES = {"E1": DwCase(8, (6, 10, 14), 3), "E2": DwCase(64, (2, 2, 2), 2), "E3": DwCase(4, (8, 8, 16), 2), "E4": DwCase(16, (4, 4, 6), 1)}
DW_JOBS = (1, 3, 8)
# fwd1: y = conv(x), stride 1; fwd2: stride 2 from a source twice as large; dgrad1: data gradient of a stride-1 conv;
# convT: the transposed form (stride 2, from a source half as large)
DW_KINDS = ("fwd1", "fwd2", "dgrad1", "convT")


@functools.lru_cache(maxsize=2)
def dw_inputs(cid, njobs):
    """jobs sharing the destination shape of the case; job `acc` accumulates onto previous content, job `pitched` reads a pitched source"""
    c = DW_CASES[cid]
    ci = list(DW_CASES).index(cid)
    rng = np.random.default_rng(5000 + 10 * ci + njobs)
    jobs = []
    for j in range(njobs):
        kind = DW_KINDS[(j + ci) % 4]
        src_shape = {"fwd1": c.shape, "dgrad1": c.shape, "fwd2": tuple(2 * s for s in c.shape), "convT": tuple(s // 2 for s in c.shape)}[kind]
        jobs.append(dict(kind=kind, src=rng.standard_normal((c.B, c.C) + src_shape).astype(np.float32),
                         w=(rng.standard_normal((c.C, 1, 3, 3, 3)) * 0.2).astype(np.float32),
                         bias=None if kind == "dgrad1" else (rng.standard_normal(c.C) * 0.1).astype(np.float32),
                         acc=(j == min(1, njobs - 1)), pitched=(j == 0), prev=rng.standard_normal((c.B, c.C) + c.shape).astype(np.float32)))
    return jobs


def dw_reference(job):
    C = job["src"].shape[1]
    s, w = torch.from_numpy(job["src"]).double(), torch.from_numpy(job["w"]).double()
    b = torch.from_numpy(job["bias"]).double() if job["bias"] is not None else None
    if job["kind"] == "fwd1":
        y = F.conv3d(s, w, b, stride=1, padding=1, groups=C)
    elif job["kind"] == "fwd2":
        y = F.conv3d(s, w, b, stride=2, padding=1, groups=C)
    elif job["kind"] == "dgrad1":
        y = F.conv_transpose3d(s, w, None, stride=1, padding=1, groups=C)       # = the gradient of conv3d(x, w) w.r.t. x under dy = src
    else:
        y = F.conv_transpose3d(s, w, b, stride=2, padding=1, output_padding=1, groups=C)
    if job["acc"]:
        y = y + torch.from_numpy(job["prev"]).double()
    return y.numpy()
