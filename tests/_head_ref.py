"""Exact dyadic operands, buffer builders and fp64 references for the fused head kernels (csrc/head.hip); no GPU needed.

Operands: x integers in [-4, 4], w in {-4..4}/32, bias in {-4..4}/8, Dropout3d gate in {0, 2}, targets in {0, 1}.  Every product
w * gate * x is a multiple of 1/32 and a logit is a sum of at most 32 of them plus a multiple of 1/8, below 2^7 in magnitude: every
partial sum is an exactly representable fp32 number whatever the summation order or FMA use, so a correct kernel returns the fp64
logits bit for bit, and x stored as bf16 is exact.  A logit is 0 or at least 1/32 away from it, so the thresholded prediction
p >= 0.5 is [z >= 0] without a doubt (sigmoid(0) == 0.5 exactly in the kernel's 1 / (1 + expf(-z))): hard sums are exact integers.

Buffers follow tests/_conv_exact_ref.py: an operand is a channel slice of a wider buffer whose other channels hold 28672 (inputs) or
-12288 (outputs, the slice itself included until the kernel writes it).

`reference(case, spec, gated)` is `_loss_ref.head_reference` on the case's operands; the Dice form is the same closed form with
Spec(0.5, 0.5, 1.0, 0.0) and the call's smooth / 2 (TI = (2A + s) / (P + T + s) with the smooth doubled)."""
import collections
import functools

import numpy as np
import torch

import _loss_ref as lr

SENT_IN = 28672.0       # as _conv_exact_ref: large, finite, bf16-representable
SENT_OUT = -12288.0
DICE_SMOOTH = 1e-6      # the smooth of head_fwd / head_bwd in the GPU file
DICE = lr.Spec(0.5, 0.5, 1.0, 0.0, DICE_SMOOTH / 2)     # Tversky(0.5, 0.5) with smooth s / 2 is Dice with smooth s

Case = collections.namedtuple("Case", "ci co shape B")

# ---- A: placements.  1200 voxels: one whole 1024-voxel chunk and a partial one (the vc clamp); 1024: one whole chunk, byte-quad eligible
PLACE_SHAPES = [(5, 6, 40), (4, 8, 32)]
PLACE_CHANNELS = [(ci, 3) for ci in (4, 8, 12, 16, 24, 32)] + [(ci, co) for ci in (4, 16, 32) for co in (1, 2, 4)]
PLACE_CASES = [Case(ci, co, shape, 2) for ci, co in PLACE_CHANNELS for shape in PLACE_SHAPES]
STORAGE = [("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f32", "bf16")]     # (x, dx)
X_SLICE = dict(off=4, extra=8)       # x: channel 4 of a buffer with ld = Ci + 8
X_LAST = dict(off=8, extra=8)        # x: the last slice of its allocation
DX_SLICE = dict(off=8, extra=12)     # dx: channel 8 of a buffer with ld = Ci + 12 (another pitch than x's: a swapped pitch shows)

# ---- C: the finalize's walks.  rows = ceil(N / 1024) partial rows per (b, c) pair; rows % 256 == 0 and BC <= 64: the flat walk,
# per = rows / 256 records per pair and thread, M = BC * per records per thread in rounds of 8; anything else: one wave per pair
Walk = collections.namedtuple("Walk", "shape B co rows per BC M what")
WALKS = [
    Walk((64, 64, 64), 3, 3, 256, 1, 9, 9, "flat, per = 1, M = 9: a second unroll round"),
    Walk((64, 64, 128), 2, 3, 512, 2, 6, 12, "flat, per = 2, M = 12"),
    Walk((64, 64, 192), 1, 3, 768, 3, 3, 9, "flat, per = 3: a pair straddles two rounds"),
    Walk((64, 64, 64), 16, 4, 256, 1, 64, 64, "flat, BC = 64: the upper edge"),
    Walk((64, 64, 64), 17, 4, 256, None, 68, None, "BC = 68: wave walk, four rows per lane"),
    Walk((40, 40, 64), 2, 3, 100, None, 6, None, "wave walk, 64 < rows < 256"),
    Walk((13, 40, 128), 2, 3, 65, None, 6, None, "wave walk, one lane takes a second row"),
]
WALK_CI = 4
TVERSKY = lr.SPECS[1]      # S = 3
BCE = lr.SPECS[4]          # S = 4 (the cross-entropy sum)


def walk_case(wk):
    return Case(WALK_CI, wk.co, wk.shape, wk.B)


def walk_reach(N, B, co):
    """(rows, per, BC, M) as head.hip derives them; per and M are None off the flat walk"""
    rows, BC = -(-N // 1024), B * co
    flat = rows % 256 == 0 and BC <= 64
    return rows, (rows // 256 if flat else None), BC, (BC * (rows // 256) if flat else None)


DLOSS_CASE = Case(12, 3, (5, 6, 40), 2)      # B: dloss scaling, Co = 3 (every loss form)
DLOSS_CASE4 = Case(8, 2, (5, 6, 40), 2)      # ... and the any-channel-count instantiation
DLOSS = [None, 1.0, 0.5, -4.0]


def all_cases():
    return PLACE_CASES + [walk_case(wk) for wk in WALKS] + [DLOSS_CASE, DLOSS_CASE4]


def _seed(c):
    return 7919 * c.ci + 104729 * c.co + 31 * c.B + sum(s * k for s, k in zip(c.shape, (1, 1009, 100003)))


@functools.lru_cache(maxsize=4)
def draw(c):
    """seeded operands of a case as fp32 torch CPU tensors: x, w, bias, gate, t (x is exactly representable in bf16 too)"""
    rng = np.random.default_rng(_seed(c))
    vs = tuple(c.shape)
    x = rng.integers(-4, 5, size=(c.B, c.ci) + vs).astype(np.float32)
    w = (rng.integers(-4, 5, size=(c.co, c.ci, 1, 1, 1)) / 32.0).astype(np.float32)
    bias = (rng.integers(-4, 5, size=(c.co,)) / 8.0).astype(np.float32)
    gate = (2.0 * (rng.random((c.B, c.ci)) < 0.5)).astype(np.float32)
    gate[:, 0] = 2.0                                     # never a wholly dropped sample
    t = (rng.random((c.B, c.co) + vs) < 0.3).astype(np.float32)
    t[0, c.co - 1] = 0                                   # one pair with an empty target
    d = dict(x=x, w=w, bias=bias, gate=gate, t=t)
    return {k: torch.from_numpy(v) for k, v in d.items()}


def second_targets(c):
    """the targets of a second evaluation batch on the same x: 1 - t"""
    return 1.0 - draw(c)["t"]


@functools.lru_cache(maxsize=2)
def draw_dp(c):
    """a given d loss / d p in {-8..8}/1024, and an integer accumulate base for dx in [-4, 4] (bf16-representable)"""
    rng = np.random.default_rng(_seed(c) + 1)
    dp = (rng.integers(-8, 9, size=(c.B, c.co) + tuple(c.shape)) / 1024.0).astype(np.float32)
    base = rng.integers(-4, 5, size=(c.B, c.ci) + tuple(c.shape)).astype(np.float32)
    return torch.from_numpy(dp), torch.from_numpy(base)


# ---- buffer builders (CPU or GPU tensors alike) ------------------------------------------------------------------------------
def ndhwc_buffer(B, shape, ld, fill, dtype=torch.float32, device="cpu"):
    """(B, D, H, W, ld) storage filled with a sentinel"""
    return torch.full((B,) + tuple(shape) + (ld,), fill, dtype=dtype, device=device)


def channel_slice(buf, off, C):
    """the logical (B, C, D, H, W) tensor of channels off .. off + C of an NDHWC buffer: a view, pitch = the buffer's channel count"""
    return buf.permute(0, 4, 1, 2, 3)[:, off:off + C]


def place_ndhwc(a, off, extra, fill=SENT_IN, dtype=None):
    """a (B, C, D, H, W) as channels off .. off + C of a sentinel-filled NDHWC buffer with ld = C + extra: (buffer, view)"""
    B, C = a.shape[:2]
    buf = ndhwc_buffer(B, a.shape[2:], C + extra, fill, dtype or a.dtype, a.device)
    v = channel_slice(buf, off, C)
    v.copy_(a)
    return buf, v


def place_ncdhw(a, off, extra, fill=SENT_IN):
    """a (B, C, D, H, W) as channels off .. off + C of a sentinel-filled contiguous (B, C + extra, D, H, W) tensor: (buffer, view)"""
    B, C = a.shape[:2]
    buf = torch.full((B, C + extra) + tuple(a.shape[2:]), fill, dtype=a.dtype, device=a.device)
    v = buf[:, off:off + C]
    v.copy_(a)
    return buf, v


def place_bytes_offset(a, lead=1):
    """the bytes of a contiguous uint8 tensor starting `lead` bytes into a sentinel-filled allocation: (buffer, view)"""
    buf = torch.full((a.numel() + lead + 3,), 255, dtype=torch.uint8, device=a.device)
    v = buf[lead:lead + a.numel()].view(a.shape)
    v.copy_(a)
    return buf, v


def outside_unchanged(buf, off, C, fill):
    """every channel of an NDHWC buffer outside off .. off + C still holds the sentinel, bit for bit"""
    ld = buf.shape[-1]
    keep = torch.ones(ld, dtype=torch.bool, device=buf.device)
    keep[off:off + C] = False
    return bool((buf[..., keep] == fill).all())


def no_prefill_left(v, fill=SENT_OUT):
    return not bool((v == fill).any())


# ---- fp64 references ---------------------------------------------------------------------------------------------------------
Ref = collections.namedtuple("Ref", "c dx dw db")      # c: _loss_ref.Closed of the logits


@functools.lru_cache(maxsize=2)
def logits(c, gated):
    """(z, x * gate) in fp64"""
    d = draw(c)
    x, w, b = d["x"].double(), d["w"].double().reshape(c.co, c.ci), d["bias"].double()
    xg = x * d["gate"].double()[:, :, None, None, None] if gated else x
    return torch.einsum("oc,bcdhw->bodhw", w, xg) + b[None, :, None, None, None], xg


def _grads(c, gated, dz):
    d = draw(c)
    _, xg = logits(c, gated)
    w = d["w"].double().reshape(c.co, c.ci)
    dw = torch.einsum("bodhw,bcdhw->oc", dz, xg).reshape(c.co, c.ci, 1, 1, 1)
    dx = torch.einsum("oc,bodhw->bcdhw", w, dz)
    if gated:
        dx = dx * d["gate"].double()[:, :, None, None, None]
    return dx, dw, dz.sum((0, 2, 3, 4))


@functools.lru_cache(maxsize=8)
def reference(c, spec, gated=True, second=False, grads=True):
    """the head with loss `spec` (DICE: the Dice entry points) on the case's operands -- `_loss_ref.head_reference` with the logits shared
    between specs; second: against the targets t2"""
    z, _ = logits(c, gated)
    cl = lr.closed_form(z, second_targets(c) if second else draw(c)["t"], spec)
    return Ref(cl, *(_grads(c, gated, cl.dz) if grads else (None, None, None)))


@functools.lru_cache(maxsize=2)
def reference_dp(c, gated=True, ones=False):
    """backward from a given d loss / d p (the case's dp, or all ones: what p.sum().backward() hands on): d z = dp p (1 - p)"""
    z, _ = logits(c, gated)
    p = torch.sigmoid(z)
    dp = torch.ones_like(p) if ones else draw_dp(c)[0].double()
    return _grads(c, gated, dp * p * (1 - p))


def hard_sums(z, t):
    """(sum [z >= 0] * t, sum [z >= 0]) per (b, c): the evaluation form's hard intersection and predicted voxels, exact integers"""
    h = (z >= 0).double()
    return (h * t.double()).sum((2, 3, 4)), h.sum((2, 3, 4))


def eval_accumulator(batches, co):
    """the evaluation accumulator (include/n3d.h, N3D_EVAL_ACC_LEN) after the batches [(loss, I, P, T), ...] with I, P, T (B, Co):
    loss sum, batches, samples, unused, then per class the I, P, T totals and the sum of the per-sample hard Dice (1 where prediction and
    target are both empty), added in the kernel's order"""
    acc = np.zeros(4 + 4 * co)
    for loss, I, P, T in batches:
        I, P, T = (np.asarray(a, dtype=np.float64) for a in (I, P, T))
        acc[0] += float(loss)
        acc[1] += 1.0
        acc[2] += I.shape[0]
        for cc in range(co):
            for b in range(I.shape[0]):
                acc[4 + 4 * cc] += I[b, cc]
                acc[5 + 4 * cc] += P[b, cc]
                acc[6 + 4 * cc] += T[b, cc]
                acc[7 + 4 * cc] += 1.0 if P[b, cc] + T[b, cc] == 0 else 2.0 * I[b, cc] / (P[b, cc] + T[b, cc])
    return acc


def scaled(ref_grads, dloss):
    """d loss scaling: the gradients of dloss * loss"""
    s = 1.0 if dloss is None else float(dloss)
    return tuple(g * s for g in ref_grads)
