"""CPU: the evaluation accumulator's reduction to the reported figures (head.eval_figures) against a numpy restatement, and the C ABI
surface of the evaluation head (header, ctypes prototypes and library exports name the same entry points)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("n3d_head_eval", "n3d_comm_allreduce_sum_f64")


def _acc_from_batches(batches, thr=0.5):
    """accumulator layout of include/n3d.h (N3D_EVAL_ACC_LEN) built from per-batch (loss, probabilities, targets)"""
    co = batches[0][1].shape[1]
    acc = np.zeros(4 + 4 * co)
    for loss, p, t in batches:
        acc[0] += loss
        acc[1] += 1
        acc[2] += p.shape[0]
        h = (p >= thr).astype(np.float64)
        for c in range(co):
            for b in range(p.shape[0]):
                i, pp, tt = (h[b, c] * t[b, c]).sum(), h[b, c].sum(), t[b, c].sum()
                acc[4 + 4 * c:8 + 4 * c] += (i, pp, tt, 1.0 if pp + tt == 0 else 2 * i / (pp + tt))
    return acc


def _restated(batches, thr=0.5):
    """(mean loss, per-class mean per-sample Dice, per-class global Dice) straight from the batches"""
    loss = np.mean([b[0] for b in batches])
    p = np.concatenate([b[1] for b in batches]) >= thr
    t = np.concatenate([b[2] for b in batches]).astype(np.float64)
    ax = (2, 3, 4)
    i, pp, tt = (p * t).sum(ax), p.sum(ax), t.sum(ax)
    per = np.where(pp + tt == 0, 1.0, 2 * i / np.maximum(pp + tt, 1e-300))
    it, pt, tq = i.sum(0), pp.sum(0), tt.sum(0)
    glob = np.where(pt + tq == 0, 1.0, 2 * it / np.maximum(pt + tq, 1e-300))
    return loss, per.mean(0), glob


@pytest.mark.parametrize("co", [3, 2, 4])
def test_eval_figures_match_numpy(co):
    from nas_3d_unet_amd.head import EvalResult, eval_figures
    rng = np.random.default_rng(co)
    batches = []
    for b in (2, 2, 1):
        p = rng.uniform(0, 1, (b, co, 4, 4, 4)).astype(np.float32)
        t = (rng.uniform(0, 1, (b, co, 4, 4, 4)) < 0.3).astype(np.float32)
        batches.append((float(rng.uniform(0.2, 0.8)), p, t))
    # one sample with both regions of class 0 empty (Dice 1), one with an empty target but a prediction (Dice 0)
    batches[0][1][0, 0] = 0.1
    batches[0][2][0, 0] = 0.0
    batches[1][1][0, 0] = 0.9
    batches[1][2][0, 0] = 0.0
    res = eval_figures(_acc_from_batches(batches))
    assert isinstance(res, EvalResult)
    loss, dice, glob = _restated(batches)
    assert res.n_batches == 3 and res.n_samples == 5
    assert res.dice.shape == (co,) and res.dice_global.shape == (co,)
    np.testing.assert_allclose(res.loss, loss, rtol=1e-15)
    np.testing.assert_allclose(res.dice, dice, rtol=1e-14)
    np.testing.assert_allclose(res.dice_global, glob, rtol=1e-14)


def test_eval_figures_empty_regions_and_no_batches():
    from nas_3d_unet_amd.head import eval_figures
    acc = np.zeros(16)
    acc[0], acc[1], acc[2] = 0.5, 1, 2
    acc[4 + 4 * 1:8 + 4 * 1] = (0, 0, 0, 2.0)      # class 1: both samples empty-and-empty
    acc[4 + 4 * 2:8 + 4 * 2] = (3, 4, 2, 1.0)
    res = eval_figures(acc)
    assert res.dice[1] == 1.0 and res.dice_global[1] == 1.0
    assert res.dice[2] == 0.5 and res.dice_global[2] == 1.0
    with pytest.raises(ValueError):
        eval_figures(np.zeros(16))                 # no batch evaluated
    with pytest.raises(ValueError):
        eval_figures(np.zeros(13))                 # not 4 + 4 * out_channels


def test_eval_symbols_are_declared_bound_and_exported():
    from nas_3d_unet_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "n3d.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(n3d_[a-zA-Z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert "N3D_EVAL_ACC_LEN" in hdr


def test_eval_accumulator_length():
    from nas_3d_unet_amd import kernels as K
    assert [K.eval_acc_len(c) for c in (1, 3, 4)] == [8, 16, 20]
