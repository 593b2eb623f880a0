#!/usr/bin/env python3
"""Generate tests/golden/optim.npz by running the REFERENCE's own optimiser classes (adabound.py: AdaBound, AdaBoundW) and torch's
clip_grad_norm_ (the call the reference keeps commented out at train.py:126-127 / search.py:236-237, config.yml:49).

Runs only where the reference checkout is present: adabound.py is imported from it at run time and nothing of it is stored.  The
inputs are regenerated from SEED by `optim_inputs` (the tests call it too); every case runs once on an fp64 parameter and once on an
fp32 one.  The fixture holds, per case, the fp64 run's p / exp_avg / exp_avg_sq / max_exp_avg_sq after the first and after the last
step, per array the scalar max|fp32 run - fp64 run| at the last step (the measure of what fp32 arithmetic costs on this trajectory:
the GPU tests' tolerance), the clip norms per step of the clipped case, and the key names of the reference's state_dict().
Usage:  python tests/golden/make_golden_optim.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

SEED = 4100
N = 257
STEPS = 24
LR = 1e-3
HALVE_AFTER = 12          # the param group's lr becomes LR / 2 after this step (what ReduceLROnPlateau(factor=0.5) does)
ARRAYS = ("p", "m", "v", "vmax")


def _case(decoupled, wd, ams, gamma=1e-3, max_norm=None):
    return dict(decoupled=decoupled, weight_decay=wd, amsbound=ams, gamma=gamma, final_lr=0.1, max_norm=max_norm)


CASES = {}
for _dec in (False, True):
    for _wd in (0.0, 1e-2):
        for _ams in (False, True):
            CASES["%s_wd%d_ams%d" % ("w" if _dec else "b", _wd != 0, _ams)] = _case(_dec, _wd, _ams)
CASES["b_wd1_ams0_g2"] = _case(False, 1e-2, False, gamma=1e-2)
CASES["w_wd1_ams1_g2"] = _case(True, 1e-2, True, gamma=1e-2)
CASES["w_wd1_ams1_clip"] = _case(True, 1e-2, True, max_norm=0.05)


def lr_of_step(t):
    return LR if t <= HALVE_AFTER else LR * 0.5


def optim_inputs(n=N, steps=STEPS, seed=SEED):
    """(p0 (n,), grads (steps, n)) as float64 arrays of fp32-representable values.  Gradients are N(0,1) * exp(U(-14, 0)) with the
    magnitude drawn once per ENTRY -- six decades, so that step_size / (sqrt(v) + eps) lands below, inside and above the bounds (a
    magnitude drawn anew in every step leaves v at the largest of the draws, and nothing but the zero-gradient entries reaches the
    upper bound) -- with every 17th entry exactly 0 in every step (a parameter that never receives a gradient)"""
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal((steps, n)) * np.exp(rng.uniform(-14.0, 0.0, n))).astype(np.float32)
    g[:, ::17] = 0.0
    return p0.astype(np.float64), g.astype(np.float64)


def run_reference(case, p0, grads, dtype):
    import torch
    sys.path.insert(0, REF)
    try:
        import adabound
    finally:
        sys.path.remove(REF)
    cls = adabound.AdaBoundW if case["decoupled"] else adabound.AdaBound
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(dtype))
    opt = cls([p], lr=LR, final_lr=case["final_lr"], gamma=case["gamma"], weight_decay=case["weight_decay"], amsbound=case["amsbound"])
    first, norms = None, []
    for t in range(1, len(grads) + 1):
        p.grad = torch.from_numpy(grads[t - 1].copy()).to(dtype)      # (clip_grad_norm_ scales it in place)
        if case["max_norm"] is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_([p], case["max_norm"])))
        opt.step()
        st = opt.state[p]
        assert st["step"] == t
        if t == 1:
            first = _state(p, st)
        if t == HALVE_AFTER:
            opt.param_groups[0]["lr"] = LR * 0.5
    sd = opt.state_dict()
    return _state(p, opt.state[p]), first, np.array(norms), sd


def _state(p, st):
    z = st.get("max_exp_avg_sq")
    return tuple(x.detach().double().numpy().copy() for x in (p, st["exp_avg"], st["exp_avg_sq"], z if z is not None else st["exp_avg_sq"] * 0))


def main():
    p0, grads = optim_inputs()
    out = {"cases": np.array(list(CASES))}
    for name, case in CASES.items():
        last64, first64, norms64, sd = run_reference(case, p0, grads, __import__("torch").float64)
        last32, _, norms32, _ = run_reference(case, p0, grads, __import__("torch").float32)
        for a, x64, x1, x32 in zip(ARRAYS, last64, first64, last32):
            out["%s/%s" % (name, a)] = x64
            out["%s/%s1" % (name, a)] = x1
            out["%s/d32/%s" % (name, a)] = np.float64(np.abs(x32 - x64).max())
        if case["max_norm"] is not None:
            out["%s/norms" % name] = norms64
        keys = sorted(sd["state"][0])
        out["%s/state_keys" % name] = np.array(keys)
        out["%s/group_keys" % name] = np.array(sorted(sd["param_groups"][0]))
        rel = ["%s %.2e" % (a, float(out["%s/d32/%s" % (name, a)]) / max(float(np.abs(out["%s/%s" % (name, a)]).max()), 1e-300)) for a in ARRAYS]
        print("%-16s moved %.2e  |fp32 - fp64| / max|x|: %s  state %s" % (name, float(np.abs(last64[0] - p0).max()), "  ".join(rel), keys))
    path = os.path.join(HERE, "optim.npz")
    np.savez_compressed(path, **out)
    print("wrote %s  (%d arrays, %.1f KB)" % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    sys.exit(main())
