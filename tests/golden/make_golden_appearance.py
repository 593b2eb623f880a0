#!/usr/bin/env python3
"""Generate tests/golden/appearance.npz: the fp64 answers of the four appearance transforms of n3d_patch_appearance (include/n3d.h,
n3d_appear_desc), each on its own on inputs made from seeds (tests/_appearance_ref.make_data: integers 10 .. 110, non-integers, about
30 % background), rounded to float32.  Only results are stored.  Per case (P, Cv, seed) and stage:

  * noise     Philox4x32-10 in Python integers, Box-Muller with numpy's log / cos / sin on the words, x + sigma * z in float64;
  * blur      scipy.ndimage.gaussian_filter(x as float64, sigma_c, mode="reflect", truncate=4.0) of each channel's whole patch;
  * contrast  plain numpy on float64: m = mean, lo = min, hi = max of the masked voxels, clip((x - m) * f + m, lo, hi);
  * gamma     plain numpy on float64: mean / std of the masked voxels, the power map rounded to float32, its mean / std, the map back;

each written to the masked voxels only (the mask is x != 0).  Nothing here comes from another project.

It also evaluates every noise and gamma case with the staged helper (tests/_appearance_ref.py: the same formulas with the rule's fixed
summation order) and records, as tol/noise and tol/gamma, the largest deviation of the helper from the fp64 answer, in float32 steps
of the channel's largest magnitude; and it asserts what tests/test_appearance_ref_host.py asserts for blur and contrast: the helper
is within one float32 step of the answer.  Needs scipy (1.15.3 wrote the committed file).
Usage:  python tests/golden/make_golden_appearance.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _appearance_ref as ap  # noqa: E402

# P = 7 with sigma 1.5 / 1.6: radius 6, reflection at both ends of every line; 0.12: radius 0.  P = 12: ragged against the 8-wide tile
CASES = [
    dict(name="p7", P=7, Cv=4, seed=11, noise=(4.0, (0x243F6A88, 0x85A308D3)), blur=[1.5, 1.6, 0.12, 1.0], contrast=[0.65, 1.5, 1.0, 1.2],
         gamma=[0.7, 1.5, 1.0, 0.9]),
    dict(name="p12", P=12, Cv=3, seed=12, noise=(9.5, (1, 0xFFFFFFFF)), blur=[0.5, 0.8, 1.3], contrast=[0.75, 1.25, 1.4], gamma=[1.3, 0.8, 1.1]),
    dict(name="p16", P=16, Cv=1, seed=13, noise=(0.5, (0xDEADBEEF, 0)), blur=[1.1], contrast=[0.9], gamma=[1.45]),
    dict(name="p20", P=20, Cv=1, seed=14, noise=(2.0, (7, 9)), blur=[0.7], contrast=[1.35], gamma=[0.75]),
]


def case_input(case):
    return ap.make_data(case["seed"], (case["Cv"],) + (case["P"],) * 3)


def answer_noise(x, sigma, key):
    Cv, n = x.shape[0], x[0].size
    words = np.array([ap.philox4x32_10((v, 0, 0, 0), key) for v in range(n)], dtype=np.float64)      # (n, 4)
    z = np.empty((4, n))
    for h in range(2):
        u1, u2 = (words[:, 2 * h] + 1.0) * 2.0 ** -32, words[:, 2 * h + 1] * 2.0 ** -32
        rho = np.sqrt(-2.0 * np.log(u1))
        z[2 * h], z[2 * h + 1] = rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)
    y = x.astype(np.float64) + sigma * z[:Cv].reshape(x.shape)
    return np.where(x != 0, y.astype(np.float32), x)


def answer_blur(x, sigmas):
    from scipy.ndimage import gaussian_filter
    y = np.stack([gaussian_filter(x[c].astype(np.float64), sigmas[c], mode="reflect", truncate=4.0) for c in range(x.shape[0])])
    return np.where(x != 0, y.astype(np.float32), x)


def answer_contrast(x, factors):
    y = x.copy()
    for c in range(x.shape[0]):
        mask, xc = x[c] != 0, x[c].astype(np.float64)
        m, lo, hi = xc[mask].mean(), xc[mask].min(), xc[mask].max()
        y[c] = np.where(mask, np.clip((xc - m) * factors[c] + m, lo, hi).astype(np.float32), x[c])
    return y


def answer_gamma(x, gammas):
    y = x.copy()
    for c in range(x.shape[0]):
        mask, xc = x[c] != 0, x[c].astype(np.float64)
        v = xc[mask]
        m, sd, lo, hi = v.mean(), v.std(), v.min(), v.max()
        v1 = (np.power((v - lo) / ((hi - lo) + 1e-7), gammas[c]) * (hi - lo) + lo).astype(np.float32).astype(np.float64)
        out = ((v1 - v1.mean()) / (v1.std() + 1e-8) * sd + m).astype(np.float32)
        y[c][mask] = out
    return y


def channel_steps(a, b):
    """the largest deviation per case, in float32 steps of each channel's largest magnitude (of b, the recorded answer)"""
    return max(float(ap.steps(a[c], b[c], np.abs(b[c]).max()).max()) for c in range(b.shape[0]))


def main():
    out, config, tol = {}, [], {"noise": 0.0, "gamma": 0.0}
    for case in CASES:
        x = case_input(case)
        mask = ap.entry_mask(x)
        assert 0.2 < 1 - mask.mean() < 0.4 and (x != np.round(x)).any() and (x[mask] >= 10).all()
        rw = [ap.blur_weights(s) for s in case["blur"]]
        answers = {"noise": answer_noise(x, *case["noise"]), "blur": answer_blur(x, case["blur"]),
                   "contrast": answer_contrast(x, case["contrast"]), "gamma": answer_gamma(x, case["gamma"])}
        helper = {"noise": ap.noise(x, mask, *case["noise"]), "blur": ap.blur(x, mask, [r for r, _ in rw], [w for _, w in rw]),
                  "contrast": ap.contrast(x, mask, case["contrast"]), "gamma": ap.gamma(x, mask, case["gamma"])}
        line = "%-4s P %2d Cv %d radii %s:" % (case["name"], case["P"], case["Cv"], [r for r, _ in rw])
        for stage, y in answers.items():
            assert y.dtype == np.float32 and np.isfinite(y).all() and (y[~mask] == 0).all() and not np.array_equal(y[mask], x[mask])
            dev = channel_steps(helper[stage], y)
            if stage in tol:
                tol[stage] = max(tol[stage], dev)
            else:
                # one float32 step of the VALUE: the two fp64 evaluations differ by rounding-order noise, then one rounding to float32
                assert (np.abs(helper[stage].astype(np.float64) - y) <= np.spacing(np.abs(y))).all(), (case["name"], stage)
            line += "  %s %.2f steps, %d voxels differ" % (stage, dev, int((helper[stage] != y).sum()))
            out["%s/%s" % (case["name"], stage)] = y
        print(line)
        config.append(case)
    out["config"] = np.array(json.dumps({"cases": config}))
    out["tol/noise"], out["tol/gamma"] = np.float64(tol["noise"]), np.float64(tol["gamma"])
    print("tol/noise %.3f  tol/gamma %.3f  (float32 steps of the channel's largest magnitude)" % (tol["noise"], tol["gamma"]))
    path = os.path.join(HERE, "appearance.npz")
    np.savez_compressed(path, **out)
    print("wrote %s  (%d cases, %.1f KB)" % (path, len(config), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    sys.exit(main())
