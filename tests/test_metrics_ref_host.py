"""CPU: the numpy restatement of the segmentation metrics (tests/_metrics_ref.py) against scipy's and numpy's answers
(tests/golden/metrics.npz, written by make_golden_metrics.py), and the host half of nas_3d_unet_amd.metrics -- finish, write_csv --
on its own.  Every integer is compared with ==, HD95 exactly."""
import csv
import math
import os
import re

import numpy as np
import pytest

import _metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("n3d_seg_workspace_bytes", "n3d_seg_regions", "n3d_seg_edt", "n3d_seg_sample", "n3d_seg_order")


def _case(g, name):
    o = g[name + "/origin"]
    return g[name + "/pred"], g[name + "/truth"], (None if o[0] < 0 else tuple(int(v) for v in o))


def _same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def test_fixture_matches_its_generator(golden):
    """the inputs the fixture stores are the ones make_golden_metrics.metric_cases() builds (numpy only: no scipy needed)"""
    import make_golden_metrics as mg
    g = golden("metrics")
    cases = mg.metric_cases()
    assert [c[0] for c in cases] == list(g["names"])
    for name, pred, truth, origin in cases:
        p, t, o = _case(g, name)
        assert np.array_equal(p, pred) and np.array_equal(t, truth) and o == origin
    for name, mask in mg.edt_cases():
        assert np.array_equal(g[name + "/mask"], mask)


def test_helper_equals_scipy(golden):
    from nas_3d_unet_amd import metrics as M
    g = golden("metrics")
    ts = []
    for name in g["names"]:
        pred, truth, origin = _case(g, name)
        s = R.score(pred, truth, origin)
        assert np.array_equal(s["flags"], g[name + "/flags"]), name
        assert np.array_equal(s["counts"], g[name + "/counts"]), name
        assert np.array_equal(s["order"], g[name + "/order"]), name
        for r, reg in enumerate(M.REGIONS):
            assert np.array_equal(s["d2"][r], g["%s/d2_%d" % (name, r)]), (name, reg)
            assert _same_float(s["scores"][reg]["hausdorff95"], float(g[name + "/hd95"][r])), (name, reg)
            assert _same_float(s["scores"][reg]["hausdorff100"], float(g[name + "/hd100"][r])), (name, reg)
            if s["order"][r, 0]:
                ts.append(R.interp_t(int(s["order"][r, 0])))
    # both forms of numpy's interpolation occur among the cases, and one case interpolates between distinct values
    assert any(t >= 0.5 for t in ts) and any(0 < t < 0.5 for t in ts), ts
    assert any(o[1] != o[2] for name in g["names"] for o in g[name + "/order"])


def test_helper_edt_equals_scipy(golden):
    g = golden("metrics")
    for name in g["edt_names"]:
        assert np.array_equal(R.edt_sq(g[name + "/mask"]), g[name + "/d2"]), name
    assert (R.edt_sq(np.zeros((3, 4, 5), np.uint8)) == R.INF).all()


def test_hd_from_order_is_numpy_percentile():
    """finish's interpolation against np.percentile on random multisets of squared distances, sizes chosen to land t on both
    sides of 0.5 and on k + 1 == n - 1"""
    from nas_3d_unet_amd import metrics as M
    rng = np.random.default_rng(11)
    for n in list(range(1, 45)) + [100, 101, 1261, 4959]:
        D = np.sort(rng.integers(0, 3000, n))
        got = M.hd_from_order(*R.order_of(D)[:3])
        assert got == float(np.percentile(np.sqrt(D.astype(np.float64)), 95)), n


def test_finish_rules():
    from nas_3d_unet_amd import metrics as M
    nv = 1000
    # WT: both empty.  TC: prediction empty.  ET: truth empty.
    s = M.finish([[0, 0, 0], [0, 0, 7], [0, 5, 0]], nv, np.zeros((3, 4), np.int64))
    assert s["WT"]["dice"] == 1.0 and s["WT"]["hausdorff95"] == 0.0 and s["WT"]["hausdorff100"] == 0.0
    assert math.isnan(s["WT"]["sensitivity"]) and s["WT"]["specificity"] == 1.0 and s["WT"]["tn"] == nv
    assert s["TC"]["dice"] == 0.0 and s["TC"]["sensitivity"] == 0.0 and math.isnan(s["TC"]["hausdorff95"])
    assert s["ET"]["dice"] == 0.0 and math.isnan(s["ET"]["sensitivity"]) and math.isnan(s["ET"]["hausdorff95"])
    assert s["ET"]["specificity"] == (nv - 5) / nv
    # ordinary integers: the ratios are single fp64 quotients
    s = M.finish([[30, 10, 5], [1, 0, 0], [2, 1, 1]], nv, [[40, 9, 16, 25], [2, 0, 0, 0], [6, 4, 4, 4]])
    assert s["WT"]["dice"] == 60 / 75 and s["WT"]["sensitivity"] == 30 / 35 and s["WT"]["specificity"] == 955 / 965
    assert (s["WT"]["tp"], s["WT"]["fp"], s["WT"]["fn"], s["WT"]["tn"], s["WT"]["n_surface"]) == (30, 10, 5, 955, 40)
    t = 39 * 0.95 - math.floor(39 * 0.95)
    assert t < 0.5 and s["WT"]["hausdorff95"] == 3.0 + (4.0 - 3.0) * t and s["WT"]["hausdorff100"] == 5.0
    assert s["TC"]["dice"] == 1.0 and s["TC"]["hausdorff95"] == 0.0
    assert s["ET"]["hausdorff95"] == 2.0
    # everything is foreground: TN + FP == 0
    assert math.isnan(M.finish([[8, 0, 0]] * 3, 8, [[8, 0, 0, 0]] * 3)["WT"]["specificity"])


def test_write_csv_round_trips_through_the_plot_slicing(tmp_path):
    """plot.py:154-156: [x for x in df[criteria + '_' + region] if not isnan(x)][:-5] -- the five trailing rows go, NaN entries go"""
    from nas_3d_unet_amd import metrics as M
    nan = float("nan")
    subjects = [M.finish([[30, 10, 5], [20, 3, 4], [2, 1, 1]], 1000, [[40, 9, 16, 25], [12, 1, 2, 5], [6, 4, 4, 4]]),
                M.finish([[50, 2, 9], [10, 0, 6], [0, 0, 3]], 1000, [[33, 1, 1, 9], [9, 2, 2, 3], [0, 0, 0, 0]]),      # ET: HD95 NaN
                M.finish([[41, 7, 7], [11, 2, 2], [0, 0, 0]], 1000, [[50, 4, 5, 36], [10, 1, 1, 1], [0, 0, 0, 0]])]     # ET: both empty
    rows = [M.row_of("sub%d" % i, s) for i, s in enumerate(subjects)]
    path = str(tmp_path / "scores.csv")
    M.write_csv(path, rows)
    with open(path, newline="") as f:
        table = list(csv.reader(f))
    assert tuple(table[0]) == M.COLUMNS and M.COLUMNS[1:4] == ("Dice_ET", "Dice_WT", "Dice_TC")
    assert [r[0] for r in table[1:]] == ["sub0", "sub1", "sub2", "Mean", "StdDev", "Median", "25quantile", "75quantile"]
    col = {c: [float(r[j]) if r[j] != "" else nan for r in table[1:]] for j, c in enumerate(table[0]) if j}
    for crit in M.CRITERIA:
        for reg in M.REGIONS:
            want = [s[reg][crit.lower()] for s in subjects]
            kept = [x for x in col["%s_%s" % (crit, reg)] if not np.isnan(x)][:-5]
            assert kept == [x for x in want if not math.isnan(x)], (crit, reg)
    v = np.array([s["ET"]["hausdorff95"] for s in subjects])
    v = v[~np.isnan(v)]
    assert len(v) == 2
    assert col["Hausdorff95_ET"][3:] == [float(v.mean()), float(v.std()), float(np.median(v)), float(np.percentile(v, 25)),
                                         float(np.percentile(v, 75))]
    # a column that is NaN throughout stays NaN in the summary rows
    only = [M.row_of("a", subjects[1])]
    only[0]["Hausdorff95_ET"] = nan
    assert all(math.isnan(r["Hausdorff95_ET"]) for r in M.summary_rows(only))


def test_symbols_declared_bound_and_exported():
    from nas_3d_unet_amd import _lib, metrics
    hdr = open(os.path.join(ROOT, "include", "n3d.h")).read()
    assert "Segmentation metrics" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared in include/n3d.h" % name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    for k, v in (("N3D_SEG_REC_WORDS", metrics.REC_WORDS), ("N3D_SEG_REC_ORDER", metrics.REC_ORDER), ("N3D_SEG_REC_BBOX", metrics.REC_BBOX),
                 ("N3D_SEG_MAX_AXIS", metrics.MAX_AXIS)):
        assert int(re.search(r"#define %s (\d+)" % k, hdr).group(1)) == v, k
    assert re.search(r"#define N3D_SEG_INF \(1 << 29\)", hdr) and metrics.INF == 1 << 29
    assert metrics.REGIONS == ("WT", "TC", "ET")
    # host-side queries run without a device
    off = (_lib.C.c_int64 * 5)()
    n = 240 * 240 * 155
    total = lib.n3d_seg_workspace_bytes(240, 240, 155, off)
    assert off[4] == 2 * 239 ** 2 + 154 ** 2 + 1 and list(off[:2]) == [0, 256]
    assert off[2] >= off[1] + n and off[3] >= off[2] + 24 * n and total >= off[3] + 12 * off[4]
    assert lib.n3d_seg_workspace_bytes(0, 4, 4, None) == 0 and lib.n3d_seg_workspace_bytes(2048, 1024, 1024, None) == 0


def test_arguments_are_validated_without_a_device():
    import torch
    from nas_3d_unet_amd import metrics as M
    from nas_3d_unet_amd._lib import N3DError
    host = torch.zeros((4, 4, 4), dtype=torch.uint8)
    with pytest.raises(N3DError, match="HIP device"):
        M.score_labels(host, host)
    with pytest.raises(N3DError, match="HIP device"):
        M.surfaces_and_counts(host, host)
    with pytest.raises(N3DError, match="HIP device"):
        M.edt_sq(host)
    with pytest.raises(N3DError, match="HIP device"):
        M.score_labels(np.zeros((4, 4, 4), np.uint8), host)
