"""fp64 numpy restatement of the training-recipe rules, operation by operation as include/n3d.h states them: torch.optim.SGD
(n3d_sgd_step), torch.optim.AdamW (n3d_adamw_step), the warm-up + polynomial / cosine learning-rate schedule (n3d_lr_schedule) and
the exponential moving average of the weights (n3d_ema_step).  The ground truth of tests/test_gpu_recipe.py, itself held to torch's
own classes in fp64 by tests/test_recipe_ref_host.py.  One call is one step on one flat vector; every array is float64 and nothing
is modified in place.  `torch_run` / `torch_ema_run` run torch's classes on the CPU in a given dtype: the authority the helper is
compared with (float64) and the measure of what fp32 arithmetic costs on a trajectory (float32 against float64)."""
import math

import numpy as np

from _optim_ref import clip_coef

STEPS = 24
HALVE_AFTER = 12
LR = 1e-2


def lr_of_step(t):
    return LR if t <= HALVE_AFTER else LR * 0.5


def _sgd(**kw):
    return dict(dict(kind="sgd", momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, max_norm=None), **kw)


def _adamw(**kw):
    return dict(dict(kind="adamw", betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None), **kw)


CASES = {
    "sgd_plain": _sgd(),
    "sgd_mom_damp": _sgd(momentum=0.9, dampening=0.5),                 # pins buf = g at the first step
    "sgd_nesterov_wd": _sgd(momentum=0.99, nesterov=True, weight_decay=3e-3),
    "sgd_clip": _sgd(momentum=0.9, max_norm=0.05),
    "adamw_wd": _adamw(),
    "adamw_wd0": _adamw(weight_decay=0.0),
}
ARRAYS = {"sgd": ("p", "buf"), "adamw": ("p", "m", "v")}
EMA_DECAYS = (0.9, 0.999)


# ------------------------------------------------------------------------------------------------ the rules
def sgd_step(p, g, buf, t, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, coef=1.0, grad_scale=1.0):
    """step t (1-based) -> (p, buf); buf is passed through when momentum == 0"""
    g = np.asarray(g, np.float64) * (coef * grad_scale)
    if weight_decay != 0:
        g = g + weight_decay * p
    if momentum != 0:
        buf = g.copy() if t == 1 else momentum * buf + (1 - dampening) * g
        g = g + momentum * buf if nesterov else buf
    return p - lr * g, buf


def adamw_step(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, coef=1.0, grad_scale=1.0):
    """step t (1-based) -> (p, m, v)"""
    b1, b2 = betas
    g = np.asarray(g, np.float64) * (coef * grad_scale)
    p = p * (1 - lr * weight_decay)
    m = m * b1 + (1 - b1) * g
    v = v * b2 + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    return p - (lr / bc1) * (m / (np.sqrt(v) / math.sqrt(bc2) + eps)), m, v


def schedule_lr(kind, s, base, total_steps, power=0.9, warmup_steps=0, warmup_start=0.1, min_lr=0.0):
    """the rate of the update issued after s applied updates (float64)"""
    W, T, a = warmup_steps, total_steps, warmup_start
    if s < W:
        return base * (a + (1 - a) * s / W)
    n = T - W
    u = min(s - W, n)
    if kind == "poly":
        return max(min_lr, base * (1 - u / n) ** power)
    c = math.cos(math.pi * u / n) if u < n else -1.0
    return min_lr + (base - min_lr) * (1 + c) / 2


def ema_step(ema, p, n_averaged, decay):
    """-> (ema, n_averaged) after one update with the parameters p"""
    p = np.asarray(p, np.float64)
    if n_averaged == 0:
        return p.copy(), 1
    return ema + (1 - decay) * (p - ema), n_averaged + 1


# ------------------------------------------------------------------------------------------------ trajectories
def apply_case(case, state, g, t, lr, coef=1.0, grad_scale=1.0):
    """one step of a CASES entry on state = (p, buf) / (p, m, v)"""
    if case["kind"] == "sgd":
        return sgd_step(state[0], g, state[1], t, lr, case["momentum"], case["dampening"], case["weight_decay"], case["nesterov"], coef, grad_scale)
    return adamw_step(state[0], g, state[1], state[2], t, lr, case["betas"], case["eps"], case["weight_decay"], coef, grad_scale)


def run_case(case, p0, grads, lr_of=lr_of_step):
    """the helper's trajectory of a case -> final state tuple in ARRAYS[kind] order"""
    p = np.asarray(p0, np.float64).copy()
    state = (p,) + tuple(np.zeros_like(p) for _ in ARRAYS[case["kind"]][1:])
    for t in range(1, len(grads) + 1):
        coef = clip_coef(grads[t - 1], case["max_norm"])[1] if case["max_norm"] is not None else 1.0
        state = apply_case(case, state, grads[t - 1], t, lr_of(t), coef)
    return state


def ema_inputs(p0, grads):
    """a drifting parameter: (steps, n) fp32-representable values p_t = p0 + 0.05 * (g_1 + .. + g_t)"""
    return (np.asarray(p0)[None] + 0.05 * np.cumsum(grads, axis=0)).astype(np.float32).astype(np.float64)


def run_ema(params, decay):
    ema, n = np.zeros_like(params[0]), 0
    for p in params:
        ema, n = ema_step(ema, p, n, decay)
    return ema


def torch_run(case, p0, grads, dtype, lr_of=lr_of_step, trace=None):
    """torch.optim.SGD / AdamW (and clip_grad_norm_) on the CPU in `dtype` -> final state tuple as float64 arrays (a momentum buffer
    torch never made reads as zeros); trace: a list that receives the state tuple after every step"""
    import torch
    p = torch.nn.Parameter(torch.from_numpy(np.asarray(p0, np.float64).copy()).to(dtype))
    if case["kind"] == "sgd":
        opt = torch.optim.SGD([p], lr=LR, momentum=case["momentum"], dampening=case["dampening"], weight_decay=case["weight_decay"],
                              nesterov=case["nesterov"])
    else:
        opt = torch.optim.AdamW([p], lr=LR, betas=case["betas"], eps=case["eps"], weight_decay=case["weight_decay"])
    for t in range(1, len(grads) + 1):
        opt.param_groups[0]["lr"] = lr_of(t)
        p.grad = torch.from_numpy(np.asarray(grads[t - 1], np.float64).copy()).to(dtype)
        if case["max_norm"] is not None:
            torch.nn.utils.clip_grad_norm_([p], case["max_norm"])
        opt.step()
        if trace is not None:
            trace.append(_torch_state(case, opt, p))
    return _torch_state(case, opt, p), opt


def _torch_state(case, opt, p):
    import torch
    st = opt.state[p]
    keys = ("momentum_buffer",) if case["kind"] == "sgd" else ("exp_avg", "exp_avg_sq")
    out = [p.detach()] + [st[k] if st.get(k) is not None else torch.zeros_like(p) for k in keys]
    return tuple(x.detach().double().numpy().copy() for x in out)


def torch_ema_run(params, decay, dtype):
    """torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)) over the parameter sequence -> (ema, n_averaged)"""
    import torch
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

    class One(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(params.shape[1], dtype=dtype))

    model = One()
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))
    for p in params:
        with torch.no_grad():
            model.w.copy_(torch.from_numpy(p).to(dtype))
        avg.update_parameters(model)
    return avg.module.w.detach().double().numpy().copy(), int(avg.n_averaged)
