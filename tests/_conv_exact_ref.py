"""Exact integer data for the convolution family: seeded draws, exactness budgets and fp64 references (no GPU needed).

With small integer-valued operands every product and every partial sum of a convolution -- forward, data gradient, weight gradient,
bias gradient, the GroupNorm statistics rows -- is an exactly representable fp32 number as long as the sums of ABSOLUTE values stay
below 2^24.  A correct kernel then returns the fp64 reference bit for bit whatever its summation order, K-split, MFMA shape or launch
grouping, and the tests need no tolerance (tests/test_gpu_conv_exact.py; the budgets and the integrality of every reference are
asserted on the CPU by tests/test_conv_exact_ref_host.py, for every case of the GPU file).

Value sets of a case (all seeded by the case's index):
  wide    x in [-3, 3], weights in [-2, 2] at a density chosen per fan-in, bias in [-3, 3], dy in [-2, 2], accumulate bases in [-4, 4], a
          ReLU-mask source in [-2, 2], gates from {0.5, 1, 2}.  fp32-storage cases: one value in 61 of x and of dy (fewer on rows with
          more than 12 200 voxels, whose weight-gradient budget would not hold otherwise) is +-515, which bf16
          cannot hold and which is no rounding tie (bf16 -> 516) -- an operand wrongly rounded to bf16 changes the answer.  Where a gate
          is 0.5 the gated values are doubled (x per (sample, channel), dy per sample), so every gated reference stays an integer.
  rep     the wide set without the 515s: every value is bf16-representable (the bf16-storage cases, run 1 of N3D_MM_BF16)
  narrow  x in {-1, 0, 1}, sparse +-1 weights, bias in [-1, 1]: the statistics rows (the conv kernels accumulate sum and sum of squares
          partly in fp32 before widening, so the per-sample sum of y^2 must stay below 2^24 too)
"""
import collections
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

LIMIT = float(2 ** 24)
SENT_IN = 28672.0       # neighbour channels of an input slice: large, finite, bf16-representable -- in a sum it is off by thousands
SENT_OUT = -12288.0     # neighbour channels (and the not-yet-written slice) of an output buffer: must come back bit-unchanged
SPRINKLE = 515.0

Case = collections.namedtuple("Case", "form cin cout k stride dil transposed depthwise B shape mix mm lay")


def _c(form, cin, cout, k, stride, dil, transposed, B, shape, mix="f32", mm=False, lay=None, depthwise=False):
    return Case(form, cin, cout, k, stride, dil, transposed, depthwise, B, shape, mix, mm, lay)


# One row per kernel form, the smallest shape that reaches it (reach conditions: the plan functions of conv_mfma.hip / conv_bf16.hip /
# conv_generic.hip; the shape is that of the conv INPUT tensor).  `lay` = the packed-weight layouts n3d_conv_pack_info reports for the
# (forward, data-gradient) call of the row: 0 generic, 1 gemm16, 2 vox64 / vox_s2, 3 vox_up, 4 / 5 their bf16 forms, -1 depthwise.
CASES = [
    # ---- fp32 storage
    _c("vox64 C=4 (+ vox_wgrad)", 4, 4, 3, 1, 1, False, 2, (4, 8, 32), lay=(2, 2)),
    _c("vox64 C=4 dil 2, odd D", 4, 4, 3, 1, 2, False, 2, (3, 8, 16), lay=(2, 2)),
    _c("vox64 C=8, odd D", 8, 8, 3, 1, 1, False, 2, (3, 4, 32), lay=(2, 2)),
    _c("vox64 C=8 dil 2 (+ vox_wgrad)", 8, 8, 3, 1, 2, False, 1, (4, 8, 16), lay=(2, 2)),
    _c("vox_s2 C=8 fwd / vox_up dgrad", 8, 8, 3, 2, 1, False, 2, (6, 8, 32), lay=(2, 3)),
    _c("vox_s2 C=4 two-plane dil 2 / vox_up", 4, 4, 3, 2, 2, False, 1, (4, 16, 32), lay=(2, 3)),
    _c("transposed C=8: vox_up fwd / vox_s2 dgrad", 8, 8, 3, 2, 1, True, 2, (3, 4, 16), lay=(3, 2)),
    _c("transposed C=4 dil 2: vox_up / vox_s2", 4, 4, 3, 2, 2, True, 1, (2, 8, 16), lay=(3, 2)),
    _c("tile16 (+ LDS-tile wgrad 16)", 16, 16, 3, 1, 1, False, 2, (10, 28, 32), mm=True, lay=(1, 1)),
    _c("tile16 dil 2", 16, 16, 3, 1, 2, False, 1, (14, 28, 48), mm=True, lay=(1, 1)),
    _c("tile32 dil 2, three samples", 32, 32, 3, 1, 2, False, 3, (6, 16, 32), mm=True, lay=(1, 1)),
    _c("tile32 (+ LDS-tile wgrad 32)", 32, 32, 3, 1, 1, False, 1, (16, 16, 32), mm=True, lay=(1, 1)),
    _c("tile16_up dgrad (stride 2, 16 ch)", 16, 16, 3, 2, 1, False, 1, (16, 32, 64), mm=True, lay=(1, 1)),
    _c("tile16_up fwd (transposed, dil 2)", 16, 16, 3, 2, 2, True, 1, (8, 16, 32), mm=True, lay=(1, 1)),
    _c("gemm16 K-split 4 + LDS-tile wgrad 16", 16, 16, 3, 1, 1, False, 2, (16, 16, 16), mm=True, lay=(1, 1)),
    _c("gemm16 K-split 16 + LDS-tile wgrad 32", 32, 32, 3, 1, 1, False, 1, (8, 16, 16), mm=True, lay=(1, 1)),
    _c("gemm16 K-split 16 + LDS-tile wgrad 64 (4x4x8)", 64, 64, 3, 1, 1, False, 2, (8, 8, 8), mm=True, lay=(1, 1)),
    _c("gemm16 2^3: a tile spans two samples, odd batch", 64, 64, 3, 1, 1, False, 3, (2, 2, 2), mm=True, lay=(1, 1)),
    _c("gemm16 stride 2 + conv_wgrad16", 16, 16, 3, 2, 1, False, 2, (8, 8, 8), mm=True, lay=(1, 1)),
    _c("gemm16 transposed + conv_wgrad16", 32, 32, 3, 2, 2, True, 3, (4, 2, 2), mm=True, lay=(1, 1)),
    _c("gemm16 Ci != Co", 32, 16, 3, 1, 1, False, 2, (4, 6, 10), mm=True, lay=(1, 1)),
    _c("gemm16 1x1x1 (48 -> 16)", 48, 16, 1, 1, 1, False, 2, (4, 6, 8), mm=True, lay=(1, 1)),
    _c("gemm16 no K-split, 16-row pairs (H % 4 != 0: no tile16)", 16, 16, 3, 1, 1, False, 1, (16, 18, 64), mm=True, lay=(1, 1)),
    _c("gemm16 no K-split, two column tiles (no tile32)", 32, 32, 3, 1, 2, False, 1, (8, 18, 64), mm=True, lay=(1, 1)),
    _c("gather 3x3x3 (W % 16 != 0)", 4, 4, 3, 1, 1, False, 2, (5, 6, 10), lay=(0, 0)),
    _c("gather 4 -> 12 stride 2", 4, 12, 3, 2, 1, False, 2, (6, 8, 12), lay=(0, 0)),
    _c("gather transposed dil 2 (parity classes)", 8, 8, 3, 2, 2, True, 2, (4, 4, 6), lay=(0, 0)),
    _c("1x1x1 streaming 4 -> 12", 4, 12, 1, 1, 1, False, 2, (32, 32, 32), lay=(0, 0)),
    _c("1x1x1 streaming 12 -> 4, ragged", 12, 4, 1, 1, 1, False, 1, (32, 33, 32), lay=(0, 0)),
    _c("1x1x1 stride 2: zero-upsampling dgrad", 12, 8, 1, 2, 1, False, 2, (32, 32, 32), lay=(0, 0)),
    _c("conv_point_kernel 12 -> 8 stride 2", 12, 8, 1, 2, 1, False, 2, (8, 8, 10), lay=(0, 0)),
    _c("conv_point_kernel 24 -> 16", 24, 16, 1, 1, 1, False, 2, (4, 6, 9), lay=(0, 0)),
    _c("depthwise gather", 4, 4, 3, 1, 1, False, 2, (5, 6, 10), lay=(-1, -1), depthwise=True),
    _c("depthwise stride 2", 8, 8, 3, 2, 1, False, 2, (6, 8, 8), lay=(-1, -1), depthwise=True),
    _c("depthwise transposed", 16, 16, 3, 2, 1, True, 2, (3, 4, 6), lay=(-1, -1), depthwise=True),
    _c("depthwise LDS-tile wgrad", 8, 8, 3, 1, 1, False, 2, (8, 16, 32), lay=(-1, -1), depthwise=True),
    _c("stride-2 MFMA wgrad C=8", 8, 8, 3, 2, 1, False, 2, (32, 64, 64), lay=(2, 3)),
    _c("stride-2 MFMA wgrad, Co/4 column tiles (4 -> 12)", 4, 12, 3, 2, 1, False, 1, (64, 64, 64), lay=(0, 0)),
    # the deep-tile vox64 forms need >= 4096 tile groups: the 64^3 level itself (the benchmarked shapes)
    _c("vox64 C=4, 4-plane tiles (+ vox_wgrad, D split)", 4, 4, 3, 1, 1, False, 2, (64, 64, 64), lay=(2, 2)),
    _c("vox64 C=4 dil 2, 4-plane tiles, two waves", 4, 4, 3, 1, 2, False, 2, (64, 64, 64), lay=(2, 2)),
    _c("vox64 C=8, 2-plane tiles", 8, 8, 3, 1, 1, False, 2, (64, 32, 64), lay=(2, 2)),
    # ---- bf16 storage (the forms of test_gpu_bf16.py's list), in the storage mixes where the form exists
    _c("vox64b C=4", 4, 4, 3, 1, 1, False, 2, (4, 8, 16), "bf16->bf16", lay=(4, 4)),
    _c("vox64b C=4 dil 2, odd D", 4, 4, 3, 1, 2, False, 2, (3, 8, 16), "bf16->bf16", lay=(4, 4)),
    _c("vox64b C=8 dil 2", 8, 8, 3, 1, 2, False, 2, (4, 8, 16), "bf16->bf16", lay=(4, 4)),
    _c("vox64b C=4 dil 2, 4-plane tiles, two waves", 4, 4, 3, 1, 2, False, 2, (64, 64, 64), "bf16->bf16", lay=(4, 4)),
    _c("vox64b C=4, 4-plane tiles (the c_node = 4 cell at 64^3)", 4, 4, 3, 1, 1, False, 2, (64, 64, 64), "bf16->bf16", lay=(4, 4)),
    _c("vox64b C=8, 2-plane tiles", 8, 8, 3, 1, 1, False, 2, (64, 64, 32), "bf16->bf16", lay=(4, 4)),
    _c("vox64b C=8, odd D", 8, 8, 3, 1, 1, False, 2, (3, 4, 32), "bf16->bf16", lay=(4, 4)),
    _c("vox_s2b C=4 two-plane / vox_upb", 4, 4, 3, 2, 1, False, 2, (4, 8, 32), "bf16->bf16", lay=(4, 5)),
    _c("vox_s2b C=8 dil 2 / vox_upb", 8, 8, 3, 2, 2, False, 2, (6, 8, 32), "bf16->bf16", lay=(4, 5)),
    _c("transposed C=4: vox_upb / vox_s2b", 4, 4, 3, 2, 1, True, 2, (3, 4, 16), "bf16->bf16", lay=(5, 4)),
    _c("transposed C=8 dil 2: vox_upb / vox_s2b", 8, 8, 3, 2, 2, True, 2, (2, 4, 16), "bf16->bf16", lay=(5, 4)),
    _c("conv C=4, mixed storage (gather)", 4, 4, 3, 1, 1, False, 2, (4, 8, 16), "bf16->f32", lay=(0, 0)),
    _c("conv C=4, mixed storage (gather)", 4, 4, 3, 1, 1, False, 2, (4, 8, 16), "f32->bf16", lay=(0, 0)),
    _c("stem1 4 -> 12 stride 2 (gather)", 4, 12, 3, 2, 1, False, 2, (6, 8, 12), "f32->bf16", lay=(0, 0)),
    _c("stem1 4 -> 12 stride 2 (gather)", 4, 12, 3, 2, 1, False, 2, (6, 8, 12), "bf16->bf16", lay=(0, 0)),
    _c("1x1x1 streaming 4 -> 12", 4, 12, 1, 1, 1, False, 1, (32, 32, 32), "bf16->bf16", lay=(0, 0)),
    _c("1x1x1 streaming 12 -> 4", 12, 4, 1, 1, 1, False, 1, (32, 32, 32), "bf16->f32", lay=(0, 0)),
    _c("1x1x1 streaming 12 -> 4", 12, 4, 1, 1, 1, False, 1, (32, 32, 32), "f32->bf16", lay=(0, 0)),
    _c("1x1x1 stride-2 preprocess (gather)", 12, 8, 1, 2, 1, False, 2, (8, 8, 10), "bf16->bf16", lay=(0, 0)),
    _c("boundary conv 24 -> 16", 24, 16, 1, 1, 1, False, 2, (4, 6, 8), "bf16->f32", lay=(0, 0)),
    _c("boundary conv 24 -> 16", 24, 16, 1, 1, 1, False, 2, (4, 6, 8), "bf16->bf16", lay=(0, 0)),
    _c("stride-2 MFMA wgrad C=4, bf16", 4, 4, 3, 2, 1, False, 1, (64, 64, 64), "bf16->bf16", lay=(4, 5)),
    _c("stride-2 MFMA wgrad 4 -> 12, fp32 x / bf16 dy", 4, 12, 3, 2, 1, False, 1, (64, 64, 64), "f32->bf16", lay=(0, 0)),
]


def case_id(i):
    c = CASES[i]
    return "%02d-%dto%d-k%ds%dd%d%s%s-B%d-%s-%s" % (i, c.cin, c.cout, c.k, c.stride, c.dil, "T" if c.transposed else "", "dw" if c.depthwise else "",
                                                     c.B, "x".join(str(s) for s in c.shape), c.mix.replace("->", "_"))


def padding(k, stride, dil):
    return max(0, math.ceil((dil * (k - 1) - stride + 1) / 2))     # prim_ops._padding


def out_shape(c):
    pad = padding(c.k, c.stride, c.dil)
    if c.transposed:
        return tuple((s - 1) * c.stride - 2 * pad + c.dil * (c.k - 1) + (0 if c.stride == 1 else 1) + 1 for s in c.shape)
    return tuple((s + 2 * pad - c.dil * (c.k - 1) - 1) // c.stride + 1 for s in c.shape)


def weight_shape(c):
    if c.depthwise:
        return (c.cin, 1, c.k, c.k, c.k)
    return (c.cin, c.cout, c.k, c.k, c.k) if c.transposed else (c.cout, c.cin, c.k, c.k, c.k)


def conv(c, x, w, b=None):
    """the case's convolution in the dtype of its operands"""
    pad, groups = padding(c.k, c.stride, c.dil), (c.cin if c.depthwise else 1)
    if c.transposed:
        return F.conv_transpose3d(x, w, b, stride=c.stride, padding=pad, output_padding=0 if c.stride == 1 else 1, dilation=c.dil, groups=groups)
    return F.conv3d(x, w, b, stride=c.stride, padding=pad, dilation=c.dil, groups=groups)


def has_extras(c):
    """ReLU-on-load, gates and the ReLU mask of the data gradient exist for plain (not transposed, not depthwise) convs"""
    return not c.transposed and not c.depthwise


def round_bf16(t):
    """round to nearest even onto bfloat16 (what pack_bf16x2 documents and torch.Tensor.bfloat16() does), returned as fp64"""
    return t.float().bfloat16().double()


def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def _sprinkle(rng, a, voxels):
    # one value in 61, fewer on the many-voxel rows: the weight-gradient budget grows with voxels x E|x| x E|dy|
    m = rng.random(a.shape) < min(1.0 / 61.0, 200.0 / voxels)
    a[m] = np.where(rng.random(int(m.sum())) < 0.5, -SPRINKLE, SPRINKLE)


def _density(c):
    """weight density: about six non-zero weights per output of the wider fan-in / fan-out, never above 35 %"""
    fan = c.k ** 3 * (1 if c.depthwise else max(c.cin, c.cout))
    return min(0.35, 6.0 / fan) if fan > 27 else 0.35


@functools.lru_cache(maxsize=6)
def draw(i, kind):
    """seeded operands of case i as fp64 torch tensors: kind = "wide" | "rep" | "narrow" (module docstring)"""
    return draw_case(CASES[i], 1000 + i, kind)


def draw_case(c, seed, kind):
    assert kind in ("wide", "rep", "narrow")
    rng = np.random.default_rng(seed)
    xs, ys = (c.B, c.cin) + tuple(c.shape), (c.B, c.cout) + out_shape(c)
    narrow = kind == "narrow"
    x = _ints(rng, xs, -1, 1) if narrow else _ints(rng, xs, -3, 3)
    dens = _density(c)
    w = rng.choice([-1.0, 1.0], size=weight_shape(c)) if narrow else _ints(rng, weight_shape(c), -2, 2)
    w *= rng.random(w.shape) < dens
    bias = _ints(rng, (c.cout,), -1, 1) if narrow else _ints(rng, (c.cout,), -3, 3)
    dy = _ints(rng, ys, -2, 2)
    base_y, base_dx, rs = _ints(rng, ys, -4, 4), _ints(rng, xs, -4, 4), _ints(rng, xs, -2, 2)
    gi = rng.choice([0.5, 1.0, 2.0], size=(c.B, c.cin))
    go = rng.choice([0.5, 1.0, 2.0], size=(c.B, c.cin))
    if kind == "wide" and c.mix == "f32":
        voxels = c.B * max(int(np.prod(c.shape)), int(np.prod(out_shape(c))))
        _sprinkle(rng, x, voxels)
        _sprinkle(rng, dy, voxels)
    # gated values stay integers: x doubled where its input gate is 0.5, dy of a sample doubled where one of its output gates is
    if narrow and int(np.prod(out_shape(c))) > 65536:
        x *= rng.random(xs) < 0.5       # the 64^3 rows: half of x zeroed, or the per-sample sum of y^2 would pass 2^24
    # (the narrow set runs ungated: x stays in {-1, 0, 1})
    if not narrow:
        x *= np.where(gi == 0.5, 2.0, 1.0)[:, :, None, None, None]
        dy *= np.where((go == 0.5).any(axis=1), 2.0, 1.0)[:, None, None, None, None]
    d = dict(x=x, w=w, bias=bias, dy=dy, base_y=base_y, base_dx=base_dx, rs=rs, gi=gi, go=go)
    return {k: torch.from_numpy(v) for k, v in d.items()}


def _bc(g):
    return g[:, :, None, None, None]


def compute(c, d, dtype, with_extras=True):
    """every result the GPU file compares, from operands d, in `dtype` (fp64: the reference; fp32: torch's own kernels)"""
    t = {k: v.to(dtype) for k, v in d.items()}
    x, w, b = t["x"].clone().requires_grad_(True), t["w"].clone().requires_grad_(True), t["bias"].clone().requires_grad_(True)
    y = conv(c, x, w, b)
    (y * t["dy"]).sum().backward()
    r = dict(y=y.detach(), y_acc=t["base_y"] + y.detach(), dx=x.grad, dx_acc=t["base_dx"] + x.grad, dw=w.grad, db=b.grad)
    if with_extras and has_extras(c):
        x2, w2 = t["x"].clone().requires_grad_(True), t["w"].clone().requires_grad_(True)
        y2 = conv(c, F.relu(x2) * _bc(t["gi"]), w2)
        (y2 * t["dy"]).sum().backward()
        mask = (t["rs"] > 0).to(dtype)
        r.update(y_rg=y2.detach(), dw_rg=w2.grad, dx_relu=r["dx"] * mask, dx_gate=r["dx"] * _bc(t["go"]),
                 dx_all=t["base_dx"] + r["dx"] * mask * _bc(t["go"]))
    return r


@functools.lru_cache(maxsize=6)
def reference(i, kind):
    """fp64 results of case i on draw(i, kind); narrow: also the per-sample statistics sums (B, Co, 2)"""
    c, d = CASES[i], draw(i, kind)
    r = compute(c, d, torch.float64, with_extras=kind != "narrow")
    if kind == "narrow":
        r["stats"] = torch.stack([r["y"].sum(dim=(2, 3, 4)), (r["y"] * r["y"]).sum(dim=(2, 3, 4))], dim=-1)
    return r


def fp32_results(i, kind):
    return compute(CASES[i], draw(i, kind), torch.float32, with_extras=kind != "narrow")


@functools.lru_cache(maxsize=6)
def reference_rounded(i):
    """N3D_MM_BF16, run 2: the fp64 conv of the wide set's operands rounded to bf16 (x, w and dy: both operands of every matrix
    product; the bias is added in fp32)"""
    c, d = CASES[i], dict(draw(i, "wide"))
    for k in ("x", "w", "dy"):
        d[k] = round_bf16(d[k])
    return compute(c, d, torch.float64, with_extras=False)


def budgets(i, kind):
    """worst-case absolute sums in fp64 -- the conv of |x| with |w| plus |bias| and its two adjoints, gates at their largest, accumulate
    bases added: y, dx, dw, db; narrow: also the per-sample sum of (worst |y|)^2.  Every one must stay below 2^24."""
    return budgets_of(CASES[i], draw(i, kind), kind)


def budgets_of(c, d, kind="wide"):
    gi, go = _bc(d["gi"].clamp(min=1.0)), _bc(d["go"].clamp(min=1.0))
    if kind == "narrow":
        gi, go = torch.ones_like(gi), torch.ones_like(go)
    x, w = (d["x"].abs() * gi).requires_grad_(True), d["w"].abs().requires_grad_(True)
    y = conv(c, x, w, d["bias"].abs())
    (y * d["dy"].abs()).sum().backward()
    out = dict(y=float((y.detach() + d["base_y"].abs()).max()), dx=float((x.grad * go + d["base_dx"].abs()).max()), dw=float(w.grad.max()),
               db=float(d["dy"].abs().sum(dim=(0, 2, 3, 4)).max()))
    if kind == "narrow":
        out["sumsq"] = float((y.detach() ** 2).sum(dim=(2, 3, 4)).max())
        out["sum"] = float(y.detach().sum(dim=(2, 3, 4)).max())
    return out


def value_kinds(c):
    """the value sets the GPU file uses for case c"""
    kinds = ["wide" if c.mix == "f32" else "rep"]
    if c.mm:
        kinds.append("rep")
    if not c.depthwise:
        kinds.append("narrow")
    return kinds


# ---- folded launches on shared buffers (the production forms: fused._slice_view hands the convs of a cell node slices of ONE buffer)
def _f(cin, cout, k, stride, dil, B, shape):
    return Case("folded", cin, cout, k, stride, dil, False, False, B, shape, "f32", False, None)


FOLDED = {
    # n3d_conv_fwdN: four one-wave-tile convs reading the four node slices of one buffer (vox64 / vox_s2 bodies in one launch)
    "fwdN C=4": [_f(4, 4, 3, s, d, 2, (4, 8, 32)) for s, d in ((1, 1), (1, 2), (2, 1), (2, 2))],
    "fwdN C=8": [_f(8, 8, 3, s, d, 2, (4, 8, 32)) for s, d in ((1, 1), (1, 2), (2, 1), (2, 2))],
    # n3d_conv_fwd2: two pointwise jobs writing two interleaved node slices of one (2, 3 x 8, 8, 8, 8) buffer
    "fwd2 pointwise": [_f(12, 8, 1, 1, 1, 2, (8, 8, 8)), _f(24, 8, 1, 2, 1, 2, (16, 16, 16))],
    # n3d_conv_bwd_data2: their data-gradient counterparts, both dx (8 channels, 8^3) in one buffer; the second is the zero-upsampling form
    "bwd_data2 pointwise": [_f(8, 12, 1, 1, 1, 2, (8, 8, 8)), _f(8, 16, 1, 2, 1, 2, (8, 8, 8))],
    # two small MFMA jobs (K-split-16 gemm16 pair / combined backward)
    "mfma pair": [_f(64, 64, 3, 1, 1, 2, (4, 4, 4)), _f(64, 64, 3, 1, 2, 2, (4, 4, 4))],
}


def folded_draw(name, j):
    return draw_case(FOLDED[name][j], 5000 + 10 * sorted(FOLDED).index(name) + j, "wide")


@functools.lru_cache(maxsize=16)
def folded_reference(name, j):
    return compute(FOLDED[name][j], folded_draw(name, j), torch.float64)
