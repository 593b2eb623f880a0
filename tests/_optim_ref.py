"""fp64 numpy restatement of the reference's optimiser options (adabound.py:50-118 AdaBound, 164-234 AdaBoundW), of torch's Adam as
the trainers use it, and of torch.nn.utils.clip_grad_norm_ (norm type 2): the ground truth of tests/test_gpu_optim.py, itself
pinned to the reference's own classes by tests/golden/optim.npz (test_optim_ref_host.py).  One call is one optimiser step on one
flat parameter vector; every array is float64 and nothing is modified in place."""
import math

import numpy as np


def clip_coef(g, max_norm, grad_scale=1.0):
    """(norm, coefficient) of clip_grad_norm_(max_norm) on the gradient grad_scale * g"""
    x = np.asarray(g, np.float64) * grad_scale
    norm = math.sqrt(float(np.sum(x * x)))
    return norm, min(1.0, max_norm / (norm + 1e-6))


def bounds(t, lr, base_lr, final_lr, gamma, betas=(0.9, 0.999)):
    """(step_size, lower bound, upper bound) of step t (1-based): adabound.py:104-112"""
    bc1 = 1 - betas[0] ** t
    bc2 = 1 - betas[1] ** t
    step_size = lr * math.sqrt(bc2) / bc1
    final = final_lr * lr / base_lr
    return step_size, final * (1 - 1 / (gamma * t + 1)), final * (1 + 1 / (gamma * t))


def adabound_step(p, g, m, v, vmax, t, lr, base_lr=None, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, final_lr=0.1, gamma=1e-3,
                  amsbound=False, decoupled=False, coef=1.0, grad_scale=1.0):
    """step t (1-based) -> (p, m, v, vmax); vmax is passed through when amsbound is off.  decoupled: AdaBoundW"""
    b1, b2 = betas
    base_lr = lr if base_lr is None else base_lr
    g = np.asarray(g, np.float64) * (coef * grad_scale)
    if weight_decay != 0 and not decoupled:
        g = g + weight_decay * p
    m = m * b1 + (1 - b1) * g
    v = v * b2 + (1 - b2) * g * g
    if amsbound:
        vmax = np.maximum(vmax, v)
        denom = np.sqrt(vmax) + eps
    else:
        denom = np.sqrt(v) + eps
    step_size, lo, hi = bounds(t, lr, base_lr, final_lr, gamma, betas)
    upd = np.clip(step_size / denom, lo, hi) * m
    if weight_decay != 0 and decoupled:
        p = (p - upd) - p * weight_decay
    else:
        p = p - upd
    return p, m, v, vmax


def adam_step(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, coef=1.0, grad_scale=1.0):
    """torch.optim.Adam defaults (no weight decay, no amsgrad) -> (p, m, v)"""
    b1, b2 = betas
    g = np.asarray(g, np.float64) * (coef * grad_scale)
    m = m * b1 + (1 - b1) * g
    v = v * b2 + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    return p - (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps), m, v


def regimes(m, v_hat, t, lr, base_lr, final_lr, gamma, eps=1e-8, betas=(0.9, 0.999)):
    """fractions (below the lower bound, above the upper bound, unclamped) of step t among the entries with m != 0"""
    step_size, lo, hi = bounds(t, lr, base_lr, final_lr, gamma, betas)
    q = (step_size / (np.sqrt(v_hat) + eps))[m != 0]
    return float(np.mean(q < lo)), float(np.mean(q > hi)), float(np.mean((q >= lo) & (q <= hi)))


def run_case(case, p0, grads, lr_of_step, base_lr, record=()):
    """the whole trajectory of one fixture case (make_golden_optim.CASES) -> final (p, m, v, vmax), {step: state} for the steps in
    `record`, the clip norms per step (empty without max_norm)"""
    p = np.asarray(p0, np.float64).copy()
    m, v, vmax = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)
    kept, norms = {}, []
    for t in range(1, len(grads) + 1):
        g, coef = grads[t - 1], 1.0
        if case["max_norm"] is not None:
            norm, coef = clip_coef(g, case["max_norm"])
            norms.append(norm)
        p, m, v, vmax = adabound_step(p, g, m, v, vmax, t, lr_of_step(t), base_lr, weight_decay=case["weight_decay"], final_lr=case["final_lr"],
                                      gamma=case["gamma"], amsbound=case["amsbound"], decoupled=case["decoupled"], coef=coef)
        if t in record:
            kept[t] = (p, m, v, vmax)
    return (p, m, v, vmax), kept, np.array(norms)
