"""Dice loss (drop-in for the reference's loss.py:6-14) on libn3d reduction kernels."""
import torch
import torch.nn as nn

from . import kernels as K
from ._lib import N3DError


class _DiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t, smooth):
        if not p.is_cuda:
            raise N3DError("WeightedDiceLoss: predictions are on %s; no CPU fallback" % p.device)
        if p.dtype != torch.float32 or t.dtype != torch.float32:
            raise N3DError("WeightedDiceLoss: fp32 tensors expected")
        if K._bcv_strides(p) is None:
            p = p.contiguous()
        if K._bcv_strides(t) is None:
            t = t.contiguous()
        loss, sums = K.dice_fwd(p, t, smooth)
        ctx.save_for_backward(p, t, sums)
        ctx.smooth = smooth
        return loss

    @staticmethod
    def backward(ctx, dloss):
        p, t, sums = ctx.saved_tensors
        dp = torch.empty_like(p)  # preserves p's (NDHWC) strides
        if K._bcv_strides(dp) is None:
            dp = torch.empty(p.shape, device=p.device, dtype=p.dtype)
        K.dice_bwd(p, t, ctx.smooth, sums, dloss.contiguous(), dp)
        return dp, None, None


class _TverskyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t, spec):
        if not p.is_cuda:
            raise N3DError("TverskyBCELoss: predictions are on %s; no CPU fallback" % p.device)
        if p.dtype != torch.float32 or t.dtype != torch.float32:
            raise N3DError("TverskyBCELoss: fp32 tensors expected")
        if K._bcv_strides(p) is None:
            p = p.contiguous()
        if K._bcv_strides(t) is None:
            t = t.contiguous()
        loss, _, coef = K.tversky_fwd(p, t, spec)
        ctx.save_for_backward(p, t, coef)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        p, t, coef = ctx.saved_tensors
        dp = torch.empty_like(p)  # preserves p's (NDHWC) strides
        if K._bcv_strides(dp) is None:
            dp = torch.empty(p.shape, device=p.device, dtype=p.dtype)
        K.tversky_bwd(t, coef, dloss.contiguous(), dp)
        return dp, None, None


class TverskyBCELoss(nn.Module):
    """mean_{b,c} u^gamma + bce_weight * mean_{b,c,v} BCE-with-logits(z, t), with u = max(1 - TI, 0) and the Tversky index
    TI = (A + s) / (A + alpha (P - A) + beta (T - A) + s) of A = sum(p*t), P = sum(p), T = sum(t) over the last three dims.
    alpha weighs false positives, beta false negatives; gamma != 1 is the focal form.  A pair with u == 0 contributes 0 and a ZERO
    gradient for every gamma (torch.pow's derivative is infinite there for gamma < 1).  alpha = beta = 0.5, gamma = 1, smooth = s / 2
    is WeightedDiceLoss(smooth=s).

    The trainers and `forward_loss(..., loss=...)` form the loss inside the fused head, from the logits.  Called as a module on
    probabilities -- the reference's training-loop form -- it takes the Tversky / focal term only: the cross-entropy term is formed
    from logits and exists in the fused head only, so bce_weight > 0 raises N3DError here."""

    def __init__(self, alpha=0.5, beta=0.5, gamma=1.0, bce_weight=0.0, smooth=1e-6):
        super().__init__()
        if not (alpha >= 0 and beta >= 0 and alpha + beta > 0 and gamma > 0 and bce_weight >= 0 and smooth > 0):
            raise ValueError("TverskyBCELoss: alpha, beta >= 0, alpha + beta > 0, gamma > 0, bce_weight >= 0 and smooth > 0 are required "
                             "(alpha=%r beta=%r gamma=%r bce_weight=%r smooth=%r)" % (alpha, beta, gamma, bce_weight, smooth))
        self.alpha, self.beta, self.gamma, self.bce_weight, self.smooth = float(alpha), float(beta), float(gamma), float(bce_weight), float(smooth)

    def forward(self, y_pred, y_truth):
        if self.bce_weight > 0:
            raise N3DError("TverskyBCELoss: the cross-entropy term is formed from logits and exists in the fused head only "
                           "(bce_weight=%g): train through Trainer(loss=...) or forward_loss(..., loss=...)" % self.bce_weight)
        return _TverskyFn.apply(y_pred, y_truth, self)


class BoundaryLoss(nn.Module):
    """base + weight * mean_{b,c,v} (p * phi): the boundary loss of Kervadec et al. (MIDL 2019) on top of a region loss.  phi is the
    signed distance map of the targets, formed on the device from every batch (`signed_distance`): the Euclidean distance to the nearest
    foreground voxel on the background, -(the distance to the nearest background voxel - 1) on the foreground -- scipy's
    distance_transform_edt under one_hot2dist, bit for bit -- and 0 where the patch holds no voxel of the wanted kind, so an empty map
    and a full map contribute nothing.

    base: None (WeightedDiceLoss()), a WeightedDiceLoss or a TverskyBCELoss.  weight >= 0 lives in a one-element device tensor that the
    head's loss launch reads: `set_weight(w)` (or a trainer's `set_boundary_weight(w)`) moves it between the replays of a captured
    step without a recapture -- the usual schedule raises it as training goes on.

    The term is formed inside the fused three-channel head (Trainer(loss=...), SearchTrainer(loss=...), forward_loss(..., loss=...)).
    `evaluate()` reports `base` alone: the weight moves during training, and a plateau scheduler must step on a loss whose definition
    does not.  Called as a module on probabilities it raises N3DError."""

    def __init__(self, base=None, weight=0.01):
        super().__init__()
        if base is None:
            base = WeightedDiceLoss()
        if not isinstance(base, (WeightedDiceLoss, TverskyBCELoss)):
            raise TypeError("BoundaryLoss: base must be None, a WeightedDiceLoss or a TverskyBCELoss (got %s)" % type(base).__name__)
        if not weight >= 0:
            raise ValueError("BoundaryLoss: weight >= 0 is required (weight=%r)" % (weight,))
        self.base = base
        self.weight = float(weight)
        self._wdev = None
        self.prepared = None      # (targets, their phi) a trainer formed at the start of its step (head.prepare_phi)

    @property
    def spec(self):
        """the base loss as the head's loss kernels take it (a TverskyBCELoss; the Dice loss with smooth s is alpha = beta = 0.5,
        gamma = 1, smooth = s / 2)"""
        b = self.base
        if isinstance(b, TverskyBCELoss):
            return b
        sp = getattr(self, "_dice_spec", None)
        if sp is None or sp.smooth != float(b.smooth) / 2:
            sp = self._dice_spec = TverskyBCELoss(0.5, 0.5, 1.0, 0.0, float(b.smooth) / 2)
        return sp

    @property
    def smooth(self):
        return self.base.smooth

    def set_weight(self, w):
        """move the weight: fills the device scalar in place (no recapture of a captured step that reads it)"""
        if not w >= 0:
            raise ValueError("BoundaryLoss: weight >= 0 is required (weight=%r)" % (w,))
        self.weight = float(w)
        if self._wdev is not None:
            self._wdev.fill_(self.weight)

    def weight_tensor(self, device):
        """the device scalar the head reads, created on first use on the targets' device"""
        if self._wdev is None or self._wdev.device != device:
            self._wdev = torch.full((1,), self.weight, dtype=torch.float32, device=device)
        return self._wdev

    @staticmethod
    def signed_distance(t):
        """phi of (B, C, D0, D1, D2) targets, float32 or uint8 {0, 1}, on their device (kernels.target_sdt)"""
        if not t.is_cuda:
            raise N3DError("BoundaryLoss.signed_distance: targets are on %s; no CPU fallback" % t.device)
        return K.target_sdt(t)

    def forward(self, y_pred, y_truth):
        raise N3DError("BoundaryLoss: the boundary term is formed inside the fused head, next to the targets' distance map, and has no "
                       "form on probabilities: train through Trainer(loss=...) or forward_loss(..., loss=...)")


def signed_distance(t):
    """signed distance maps of (B, C, D0, D1, D2) targets: BoundaryLoss.signed_distance"""
    return BoundaryLoss.signed_distance(t)


class WeightedDiceLoss(nn.Module):
    """1 - mean_{b,c} (2*sum(p*t)+eps) / (sum(p)+sum(t)+eps), sums over the last three dims."""

    def __init__(self, axis=(-1, -2, -3), smooth=1e-6):
        super().__init__()
        if tuple(sorted(a % 5 for a in axis)) != (2, 3, 4):
            raise NotImplementedError("WeightedDiceLoss: only the spatial axes (-1,-2,-3) are built")
        self.axis = axis
        self.smooth = smooth

    def forward(self, y_pred, y_truth):
        return _DiceFn.apply(y_pred, y_truth, float(self.smooth))
