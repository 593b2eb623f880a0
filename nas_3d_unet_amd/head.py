"""Network head as fused launches (nas.py:50-52 / searched.py:91-93: `nn.Sequential(ConvOps(c, n_out, kernel_size=1,
dropout_rate=p, ops_order='weight'), nn.Sigmoid())`, and loss.py:12-14 behind it).

`run(head, x)` = Dropout3d -> 1x1x1 conv -> sigmoid in ONE kernel (n3d_head_fwd) with a one-pass backward (n3d_head_bwd);
`run_loss(head, x, t, smooth)` additionally forms the Dice sums in the forward pass and the Dice gradient inside the
backward pass, so the trainers' step has no separate sigmoid / Dice passes over (B, n_out, D, H, W).
`run_loss(..., loss=TverskyBCELoss(...))` forms the Tversky / focal / cross-entropy loss in the same two passes (n3d_head_loss_fwd / _bwd).
`run_loss(..., loss=BoundaryLoss(...))` first forms the targets' signed distance map on the current stream (n3d_target_sdt), then the base
loss plus the boundary term in the same two passes (n3d_head_bnd_fwd / _bwd); `run_eval` with a BoundaryLoss evaluates its base loss.
`run_eval(head, x, t, acc)` is the evaluation form (n3d_head_eval, no autograd): eval-mode head, Dice loss and the region counts of
the thresholded prediction in one pass, added into a device accumulator that `eval_figures` turns into an `EvalResult`.
The modules (and their state-dict names `last_conv.0.conv.*`) stay the reference's; only what runs underneath differs.
Shapes the fused kernels do not take (see include/n3d.h) fall back to the op-by-op path.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import kernels as K
from . import programs as P

KEEP_LOGITS = False   # tests: keep the pre-sigmoid activations of the last run() / run_loss() call in `last_logits`
last_logits = None


def feat_shape(x):
    """(B, C) of a feature map: a 5-D (B, C, D, H, W) tensor, or a node-planar 6-D (nn, B, cn, D, H, W) one (kernels.Planar)"""
    return (x.shape[1], x.shape[0] * x.shape[2]) if x.dim() == 6 else (x.shape[0], x.shape[1])


def fusable(head, x):
    op = head[0]
    return (len(head) == 2 and isinstance(head[1], torch.nn.Sigmoid) and getattr(op, "ops_list", None) == ["weight"]
            and not getattr(op, "depthwised", True) and op._k == 1 and op._stride == 1 and not op._transposed
            and feat_shape(x)[1] in (4, 8, 12, 16, 24, 32) and op.conv.weight.shape[0] <= 4)


def _gate(op, x):
    B, Cc = feat_shape(x)
    return P.draw_gate(op.dropout, op.training, B, Cc, x.device)


def _feat_view(x):
    return K.as_planar(x, "head input") if x.dim() == 6 else K.as_view(x, "head input", bf16_ok=True)


def _feat_like(xv):
    """gradient buffer of the head input's layout"""
    if isinstance(xv, K.Planar):
        return K.empty_planar(xv.nn, xv.B, xv.cn, xv.D, xv.H, xv.W, xv.t.device, xv.t.dtype)
    return K.as_view(K.empty_ndhwc(xv.B, xv.C, xv.D, xv.H, xv.W, xv.t.device, xv.t.dtype), bf16_ok=True)


class HeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, x, w, b):
        global last_logits
        xv = _feat_view(x)
        p, logits, _, _ = K.head_fwd(xv, w, b, gate, want_logits=KEEP_LOGITS)
        if KEEP_LOGITS:
            last_logits = logits
        ctx.xv, ctx.gate, ctx.w, ctx.b = xv, gate, w, b
        return p

    @staticmethod
    def backward(ctx, dp):
        xv, w, b = ctx.xv, ctx.w, ctx.b
        if K._bcv_strides(dp) is None:
            dp = dp.contiguous()
        dx = _feat_like(xv)
        dw, db = K.grad_target(w), K.grad_target(b)
        K.head_bwd(xv, w, b, ctx.gate, dx, dw, db, dp=dp)
        inplace = getattr(w, "_n3d_grad", None) is not None
        ctx.xv = None
        return None, dx.t, None if inplace else dw, None if inplace else db


class HeadDiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, smooth, x, t, w, b):
        global last_logits
        xv = _feat_view(x)
        if K._bcv_strides(t) is None:
            t = t.contiguous()
        # (the trainers' autograd-free pipeline sets `skip_p`: a step needs the loss, and the backward pass recomputes p from x)
        want_p = KEEP_LOGITS or not getattr(ctx, "skip_p", False)
        p, logits, sums, loss = K.head_fwd(xv, w, b, gate, t, smooth, want_logits=KEEP_LOGITS, want_p=want_p)
        if KEEP_LOGITS:
            last_logits = logits
        ctx.xv, ctx.gate, ctx.w, ctx.b, ctx.t, ctx.sums, ctx.smooth = xv, gate, w, b, t, sums, smooth
        if p is not None:
            ctx.mark_non_differentiable(p)
        return loss, p

    @staticmethod
    def backward(ctx, dloss, _dp):
        xv, w, b = ctx.xv, ctx.w, ctx.b
        dx = _feat_like(xv)
        dw, db = K.grad_target(w), K.grad_target(b)
        K.head_bwd(xv, w, b, ctx.gate, dx, dw, db, t=ctx.t, sums=ctx.sums, dloss=dloss.contiguous(), smooth=ctx.smooth)
        inplace = getattr(w, "_n3d_grad", None) is not None
        ctx.xv = ctx.t = None
        return None, None, dx.t, None, None if inplace else dw, None if inplace else db


class HeadLossFn(torch.autograd.Function):
    """HeadDiceFn for a loss.TverskyBCELoss `spec` (n3d_head_loss_fwd / n3d_head_loss_bwd): the same `skip_p` contract"""

    @staticmethod
    def forward(ctx, gate, spec, x, t, w, b):
        global last_logits
        xv = _feat_view(x)
        if K._bcv_strides(t) is None:
            t = t.contiguous()
        want_p = KEEP_LOGITS or not getattr(ctx, "skip_p", False)
        p, logits, _, coef, loss = K.head_loss_fwd(xv, w, b, gate, t, spec, want_logits=KEEP_LOGITS, want_p=want_p)
        if KEEP_LOGITS:
            last_logits = logits
        ctx.xv, ctx.gate, ctx.w, ctx.b, ctx.t, ctx.coef = xv, gate, w, b, t, coef
        if p is not None:
            ctx.mark_non_differentiable(p)
        return loss, p

    @staticmethod
    def backward(ctx, dloss, _dp):
        xv, w, b = ctx.xv, ctx.w, ctx.b
        dx = _feat_like(xv)
        dw, db = K.grad_target(w), K.grad_target(b)
        K.head_loss_bwd(xv, w, b, ctx.gate, dx, dw, db, ctx.t, ctx.coef, dloss=dloss.contiguous())
        inplace = getattr(w, "_n3d_grad", None) is not None
        ctx.xv = ctx.t = None
        return None, None, dx.t, None, None if inplace else dw, None if inplace else db


class HeadBndFn(torch.autograd.Function):
    """HeadLossFn for a loss.BoundaryLoss `bnd` (n3d_head_bnd_fwd / n3d_head_bnd_bwd) and the distance map phi of t: the same `skip_p`
    contract"""

    @staticmethod
    def forward(ctx, gate, bnd, phi, x, t, w, b):
        global last_logits
        xv = _feat_view(x)
        if K._bcv_strides(t) is None:
            t = t.contiguous()
        want_p = KEEP_LOGITS or not getattr(ctx, "skip_p", False)
        p, logits, _, coef, loss = K.head_bnd_fwd(xv, w, b, gate, t, phi, bnd.spec, bnd.weight_tensor(t.device), want_logits=KEEP_LOGITS,
                                                  want_p=want_p)
        if KEEP_LOGITS:
            last_logits = logits
        ctx.xv, ctx.gate, ctx.w, ctx.b, ctx.t, ctx.phi, ctx.coef = xv, gate, w, b, t, phi, coef
        if p is not None:
            ctx.mark_non_differentiable(p)
        return loss, p

    @staticmethod
    def backward(ctx, dloss, _dp):
        xv, w, b = ctx.xv, ctx.w, ctx.b
        dx = _feat_like(xv)
        dw, db = K.grad_target(w), K.grad_target(b)
        K.head_bnd_bwd(xv, w, b, ctx.gate, dx, dw, db, ctx.t, ctx.phi, ctx.coef, dloss=dloss.contiguous())
        inplace = getattr(w, "_n3d_grad", None) is not None
        ctx.xv = ctx.t = ctx.phi = None
        return None, None, None, dx.t, None, None if inplace else dw, None if inplace else db


def _is_boundary(loss):
    from .loss import BoundaryLoss
    return isinstance(loss, BoundaryLoss)


def target_phi(loss, t):
    """the signed distance map of the targets t for the loss.BoundaryLoss `loss`, on the current stream: the map a trainer formed at the
    start of its step for this very tensor (loss.prepared), or a new one"""
    prep = getattr(loss, "prepared", None)
    if prep is not None and prep[0] is t:
        loss.prepared = None
        return prep[1]
    return K.target_sdt(t)


def prepare_phi(loss, t):
    """trainers: form phi of t now -- at the start of the step, on the main chain -- for the head that runs at its end"""
    if _is_boundary(loss):
        loss.prepared = (t, K.target_sdt(t))


def _dice_like(loss):
    """is `loss` (None, a loss.WeightedDiceLoss or a loss.TverskyBCELoss) the Dice loss of the existing entry points?"""
    from .loss import BoundaryLoss, TverskyBCELoss, WeightedDiceLoss
    if loss is None or isinstance(loss, WeightedDiceLoss):
        return True
    if not isinstance(loss, (TverskyBCELoss, BoundaryLoss)):
        raise K.N3DError("head: loss must be a WeightedDiceLoss, a TverskyBCELoss or a BoundaryLoss (got %s)" % type(loss).__name__)
    return False


def check_loss_head(head, loss):
    """raise unless the head can form `loss`: a cross-entropy term (bce_weight > 0) and the boundary term of a BoundaryLoss are built
    inside the fused three-channel head only"""
    if _is_boundary(loss):
        op = head[0]
        ci, co = op.conv.weight.shape[1], op.conv.weight.shape[0]
        if co != 3:
            raise K.N3DError("BoundaryLoss: the boundary kernels are built for a three-channel head (out_channels=%d)" % co)
        if not fusable(head, torch.empty((1, ci, 1, 1, 1), device="meta")):
            raise K.N3DError("BoundaryLoss: the boundary term is formed inside the fused head, and this head is not one it takes "
                             "(1x1x1 conv of 4..32 channels to 3, sigmoid; %d -> %d here)" % (ci, co))
        return
    if _dice_like(loss) or not loss.bce_weight > 0:
        return
    op = head[0]
    ci, co = op.conv.weight.shape[1], op.conv.weight.shape[0]
    if not fusable(head, torch.empty((1, ci, 1, 1, 1), device="meta")):
        raise K.N3DError("TverskyBCELoss(bce_weight=%g): the cross-entropy term is formed from logits inside the fused head, and this "
                         "head is not one it takes (1x1x1 conv of 4..32 channels to <= 4, sigmoid; %d -> %d here)" % (loss.bce_weight, ci, co))
    if co != 3:
        raise K.N3DError("TverskyBCELoss(bce_weight=%g): the cross-entropy kernels are built for a three-channel head (out_channels=%d)"
                         % (loss.bce_weight, co))


def run(head, x):
    """probabilities of the head on features x"""
    if not fusable(head, x):
        return head(x)
    op = head[0]
    return HeadFn.apply(_gate(op, x), x, op.conv.weight, op.conv.bias)


def run_loss(head, x, t, smooth=1e-6, loss=None):
    """(loss, probabilities) of the head on features x against the target t.  loss: None or a WeightedDiceLoss -- the Dice loss with
    `smooth` -- or a TverskyBCELoss, which carries its own smooth, or a BoundaryLoss: the signed distance map of t is formed on the
    current stream first, and the fused head adds weight * mean(p * phi) to the BoundaryLoss's base loss.  The probabilities are returned for
    inspection only and carry NO gradient on either path (the fused kernels form the loss gradient inside the head's backward
    pass): a caller who wants another loss on them uses run() and differentiates through that."""
    fused = fusable(head, x)
    byte_ok = fused and t.dtype == torch.uint8 and head[0].conv.weight.shape[0] == 3      # {0, 1} bytes: the three-channel head kernels read them as they are
    dice = _dice_like(loss)
    if not dice:
        check_loss_head(head, loss)
    if _is_boundary(loss):
        if not fused or not (t.dtype == torch.float32 or byte_ok):
            raise K.N3DError("BoundaryLoss: the fused three-channel head forms it from float32 or uint8 {0, 1} targets (got %s)" % t.dtype)
        op = head[0]
        return HeadBndFn.apply(_gate(op, x), loss, target_phi(loss, t), x, t, op.conv.weight, op.conv.bias)
    if not fused or not (t.dtype == torch.float32 or byte_ok):
        from .loss import WeightedDiceLoss
        if not dice and loss.bce_weight > 0:
            raise K.N3DError("TverskyBCELoss(bce_weight=%g): targets are float32, or uint8 {0, 1} bytes (got %s)" % (loss.bce_weight, t.dtype))
        p = head(x)
        fn = WeightedDiceLoss(smooth=smooth) if dice else loss
        return fn(p, t if t.dtype == torch.float32 else t.to(torch.float32)), p.detach()
    op = head[0]
    if not dice:
        return HeadLossFn.apply(_gate(op, x), loss, x, t, op.conv.weight, op.conv.bias)
    return HeadDiceFn.apply(_gate(op, x), float(smooth), x, t, op.conv.weight, op.conv.bias)


class EvalResult(NamedTuple):
    """figures of an evaluation pass (trainers' eval_result()): loss = mean batch Dice loss (unrounded); dice = per class the mean
    over samples of the hard Dice of the region p >= thr (1 when prediction and target are both empty); dice_global = per class
    2 I / (P + T) over every voxel of the pass (1 when both are empty)"""
    loss: float
    dice: np.ndarray
    dice_global: np.ndarray
    n_batches: int
    n_samples: int


def eval_figures(acc):
    """EvalResult of an evaluation accumulator (host array of N3D_EVAL_ACC_LEN(co) doubles, include/n3d.h: loss sum, batches,
    samples, unused, then per class (I, P, T, sum of per-sample hard Dice))"""
    a = np.asarray(acc, dtype=np.float64).reshape(-1)
    if a.size < 8 or (a.size - 4) % 4:
        raise ValueError("eval_figures: an accumulator holds 4 + 4 * out_channels values, got %d" % a.size)
    nb, ns = a[1], a[2]
    if nb <= 0 or ns <= 0:
        raise ValueError("eval_figures: no batch was evaluated")
    per = a[4:].reshape(-1, 4)
    i, p, t, dsum = per[:, 0], per[:, 1], per[:, 2], per[:, 3]
    den = p + t
    glob = np.where(den > 0, 2.0 * i / np.where(den > 0, den, 1.0), 1.0)
    return EvalResult(float(a[0] / nb), dsum / ns, glob, int(round(nb)), int(round(ns)))


def run_eval(head, x, t, acc, smooth=1e-6, thr=0.5, loss=None):
    """eval-mode head on features x (no Dropout3d, no autograd): the loss against t -- bit for bit run_loss's in eval mode, Dice or
    the TverskyBCELoss `loss` -- with the region counts of p >= thr, both added into acc (kernels.eval_acc).  Returns the batch loss
    (0-d device tensor).  Only the fused head kernel takes this path: another head shape is an error.
    A BoundaryLoss is evaluated as its BASE loss: the boundary weight moves during training, so the figure a plateau scheduler steps
    on, and the one compared between epochs, must be a loss whose definition does not."""
    op = head[0]
    if _is_boundary(loss):
        check_loss_head(head, loss)
        loss = loss.base
        smooth = getattr(loss, "smooth", smooth)
    if not fusable(head, x):
        raise K.N3DError("evaluate: the head is not one the fused evaluation kernel takes (1x1x1 conv of 4..32 channels to <= 4, sigmoid)")
    if not (t.dtype == torch.float32 or (t.dtype == torch.uint8 and op.conv.weight.shape[0] == 3)):
        raise K.N3DError("evaluate: targets are float32, or uint8 {0, 1} bytes for a three-channel head (got %s)" % t.dtype)
    if K._bcv_strides(t) is None:
        t = t.contiguous()
    if not _dice_like(loss):
        check_loss_head(head, loss)
        return K.head_loss_eval(_feat_view(x), op.conv.weight, op.conv.bias, t, acc, loss, thr)[0]
    return K.head_eval(_feat_view(x), op.conv.weight, op.conv.bias, t, acc, smooth, thr)[0]
