"""fp64 reference of loss.TverskyBCELoss (include/n3d.h, n3d_loss) on the CPU.

For a (b, c) pair, sums over the sample's voxels: A = sum p*t, P = sum p, T = sum t, with the logit z and p = sigmoid(z):

    TI = (A + s) / (A + alpha (P - A) + beta (T - A) + s),   u = max(1 - TI, 0)
    L  = mean_bc u^gamma + w * mean_bcv [max(z, 0) - z t + log1p(exp(-|z|))]

Convention: where u == 0 the pair contributes 0 to the loss and a ZERO gradient for every gamma (torch.pow's derivative is infinite
there for gamma < 1); `torch_loss` masks the power the same way, so autograd and the closed form agree there too.

`closed_form` evaluates the loss and the gradient formula the kernels implement; `torch_loss` is the literal formula, differentiable,
for autograd comparisons and for the oracle's network forwards (orc.searched_forward / orc.supernet_forward with return_logits=True)."""
from collections import namedtuple

import torch
import torch.nn.functional as F

Spec = namedtuple("Spec", "alpha beta gamma bce_weight smooth", defaults=(0.5, 0.5, 1.0, 0.0, 1e-6))

# the (alpha, beta, gamma, bce_weight) sets the tests run
SPECS = [Spec(0.5, 0.5, 1.0, 0.0), Spec(0.3, 0.7, 1.0, 0.0), Spec(0.3, 0.7, 0.75, 0.0), Spec(0.7, 0.3, 2.0, 0.5), Spec(0.5, 0.5, 1.0, 1.0)]

Closed = namedtuple("Closed", "loss sums u k2 k0 kb dz")
_AX = (-1, -2, -3)


def _bce_voxels(z, t):
    return torch.clamp(z, min=0) - z * t + torch.log1p(torch.exp(-z.abs()))


def closed_form(z, t, spec):
    """loss, sums (B, C, 4) = (A, P, T, sum of the voxels' cross-entropy), u (B, C), the coefficients k2 / k0 (B, C) and kb, and
    d loss / d z = (k2 t + k0) p (1 - p) + kb (p - t).  z, t: (B, C, D, H, W); evaluated in fp64 without autograd."""
    with torch.no_grad():
        z, t = z.detach().double(), t.detach().double()
        a, b, g, w, s = (float(v) for v in spec)
        B, Cc = z.shape[:2]
        N = z[0, 0].numel()
        BC = B * Cc
        p = torch.sigmoid(z)
        A, Ps, T, CE = (p * t).sum(_AX), p.sum(_AX), t.sum(_AX), _bce_voxels(z, t).sum(_AX)
        num = A + s
        den = A + a * (Ps - A) + b * (T - A) + s
        u = torch.clamp(1 - num / den, min=0)
        pos = u > 0
        us = torch.where(pos, u, torch.ones_like(u))
        term = torch.where(pos, us ** g, torch.zeros_like(u))
        f = torch.where(pos, g * us ** (g - 1) / BC, torch.zeros_like(u))
        k2 = -f * (den - num * (1 - a - b)) / den ** 2
        k0 = f * num * a / den ** 2
        kb = w / (BC * N)
        loss = term.mean() + w * CE.sum() / (BC * N)
        e = (slice(None), slice(None), None, None, None)
        dz = (k2[e] * t + k0[e]) * p * (1 - p) + kb * (p - t)
        return Closed(loss, torch.stack([A, Ps, T, CE], dim=-1), u, k2, k0, kb, dz)


def closed_form_probs(p, t, spec):
    """the Tversky / focal term on PROBABILITIES (the module's forward): (loss, d loss / d p = k2 t + k0), fp64"""
    with torch.no_grad():
        p, t = p.detach().double(), t.detach().double()
        a, b, g, _, s = (float(v) for v in spec)
        BC = p.shape[0] * p.shape[1]
        A, Ps, T = (p * t).sum(_AX), p.sum(_AX), t.sum(_AX)
        num = A + s
        den = A + a * (Ps - A) + b * (T - A) + s
        u = torch.clamp(1 - num / den, min=0)
        pos = u > 0
        us = torch.where(pos, u, torch.ones_like(u))
        f = torch.where(pos, g * us ** (g - 1) / BC, torch.zeros_like(u))
        k2 = -f * (den - num * (1 - a - b)) / den ** 2
        k0 = f * num * a / den ** 2
        e = (slice(None), slice(None), None, None, None)
        return torch.where(pos, us ** g, torch.zeros_like(u)).mean(), k2[e] * t + k0[e]


def torch_loss(logits, t, spec):
    """the literal formula on logits, differentiable: binary_cross_entropy_with_logits plus (1 - TI).clamp(min=0).pow(gamma), the power
    masked where u == 0 (see the module docstring)"""
    a, b, g, w, s = (float(v) for v in spec)
    p = torch.sigmoid(logits)
    A, Ps, T = (p * t).sum(_AX), p.sum(_AX), t.sum(_AX)
    u = (1 - (A + s) / (A + a * (Ps - A) + b * (T - A) + s)).clamp(min=0)
    pos = u > 0
    term = torch.where(pos, torch.where(pos, u, torch.ones_like(u)).pow(g), torch.zeros_like(u))
    loss = term.mean()
    if w > 0:
        loss = loss + w * F.binary_cross_entropy_with_logits(logits, t)
    return loss


def head_reference(x, w, b, gate, t, spec):
    """the fused head (Dropout3d gate -> 1x1x1 conv -> sigmoid -> loss) in fp64 from the closed form: (Closed of the logits, dx, dw, db).
    x (B, Ci, D, H, W), w (Co, Ci, 1, 1, 1), b (Co,), gate (B, Ci) or None, t (B, Co, D, H, W)"""
    x, w, b, t = x.double(), w.double().reshape(w.shape[0], -1), b.double(), t.double()
    xg = x * gate.double()[:, :, None, None, None] if gate is not None else x
    z = torch.einsum("oc,bcdhw->bodhw", w, xg) + b[None, :, None, None, None]
    c = closed_form(z, t, spec)
    dw = torch.einsum("bodhw,bcdhw->oc", c.dz, xg).reshape(w.shape[0], -1, 1, 1, 1)
    db = c.dz.sum((0, 2, 3, 4))
    dx = torch.einsum("oc,bodhw->bcdhw", w, c.dz)
    if gate is not None:
        dx = dx * gate.double()[:, :, None, None, None]
    return c, dx, dw, db
