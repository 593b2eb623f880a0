"""CPU: the numpy restatement of the lesion-wise metrics (tests/_lesion_ref.py) and the host half of the product
(nas_3d_unet_amd.metrics.finish_lesions, write_csv) against scipy's answers (tests/golden/lesion.npz,
tests/golden/make_golden_lesion.py).  Records are integers and compared with ==; the folded floats are compared with == too: the
fixture and finish_lesions form them by the same fp64 operations in the same order."""
import numpy as np
import pytest

import _lesion_ref as R
import _metrics_ref as MR
from make_golden_lesion import EXTRA_DILATIONS, FOLDS, lesion_cases
from nas_3d_unet_amd import metrics as M
from nas_3d_unet_amd._lib import N3DError

CASES = ("gaps", "diagonal", "bridge", "rim", "fps", "threshold", "box", "nested", "both_empty", "pred_empty", "truth_empty", "cap64")


def _origin(g, name):
    o = tuple(int(v) for v in g[name + "/origin"])
    return None if o[0] < 0 else o


def test_fixture_holds_the_cases(golden):
    g = golden("lesion")
    assert tuple(g["names"]) == CASES and g["folds"].tolist() == [list(f) for f in FOLDS]
    for name, pred, truth, origin in lesion_cases():
        assert np.array_equal(g[name + "/pred"], pred) and np.array_equal(g[name + "/truth"], truth) and _origin(g, name) == origin
        assert g[name + "/record"].shape == (R.REC_WORDS,) and g[name + "/record"].dtype == np.int64


@pytest.mark.parametrize("name", CASES)
def test_helper_equals_scipy(golden, name):
    g = golden("lesion")
    pred, truth, origin = g[name + "/pred"], g[name + "/truth"], _origin(g, name)
    wt = MR.embed(truth, pred.shape, origin) != 0
    for d in range(6):
        assert np.array_equal(R.dilate(wt, d), g[name + "/dilated"][d] != 0), (name, d)
    assert np.array_equal(R.record(pred, truth, origin), g[name + "/record"]), name
    for d in EXTRA_DILATIONS.get(name, ()):
        assert np.array_equal(R.record(pred, truth, origin, d), g["%s/record_d%d" % (name, d)]), (name, d)


def test_offsets_and_components_of_the_helper():
    assert len(R.offsets(3)) == 263 and len(R.offsets(1)) == 19 and R.offsets(0) == [(0, 0, 0)]
    m = np.zeros((4, 5, 6), bool)
    for p in ((1, 1, 5), (1, 2, 0), (2, 2, 1), (3, 4, 5)):
        m[p] = True
    ids = R.label26(m)
    # (1, 1, 5) and (1, 2, 0) follow each other in linear index and are no neighbours in space
    assert ids[1, 1, 5] == 41 and ids[1, 2, 0] == ids[2, 2, 1] == 42 and ids[3, 4, 5] == 119 and (ids[~m] == -1).all()


@pytest.mark.parametrize("name", CASES)
def test_finish_lesions_gives_the_golden_floats(golden, name):
    g = golden("lesion")
    rec = g[name + "/record"]
    for i, (mv, pen) in enumerate(FOLDS):
        s = M.finish_lesions(rec, min_lesion_voxels=mv, penalty_hd95=pen)
        want = g["%s/folded_%d" % (name, i)]
        got = R.folded(s)
        assert got.tobytes() == want.tobytes(), (name, mv, pen, got.tolist(), want.tolist())
        for r, reg in enumerate(M.REGIONS):
            assert s[reg]["n_lesions"] == int(rec.reshape(3, -1)[r, 0]) == len(s[reg]["lesions"])
            assert s[reg]["n_kept"] == sum(l["gt_voxels"] > mv for l in s[reg]["lesions"])
            assert s[reg]["n_fn"] == sum(l["gt_voxels"] > mv and l["n_matched"] == 0 for l in s[reg]["lesions"])
    assert M.finish_lesions(rec) == M.finish_lesions(rec, 50, 374.0)            # the defaults


def _record(regions):
    """regions: per region (n_fp, fp_voxels, rows) -> a record"""
    rec = np.zeros((3, R.REGION_WORDS), np.int64)
    for r, (n_fp, fp_voxels, rows) in enumerate(regions):
        rec[r, :4] = [len(rows), n_fp + sum(row[4] for row in rows), n_fp, fp_voxels]
        for l, row in enumerate(rows):
            rec[r, R.HEADER_WORDS + R.ROW_WORDS * l:][:R.ROW_WORDS] = row
    return rec.ravel()


def test_rules_of_the_fold_on_hand_made_records():
    matched = [7, 100, 60, 80, 1, 10, 4, 9, 16]             # Dice 120 / 180, n = 10: k = 8, t = 0.55 -> 3 - 1 * 0.45
    hd = M.hd_from_order(10, 4, 9)
    assert hd == 3.0 - 1.0 * (1 - (np.float64(9) * np.float64(0.95) - 8))
    # den == 0: no lesion at all, or only sub-threshold ones whose components are neither scored nor false positives
    s = M.finish_lesions(_record([(0, 0, []), (0, 0, [[3, 50, 20, 30, 1, 10, 4, 9, 16]]), (0, 0, [[3, 2, 0, 0, 0, 0, 0, 0, 0]])]))
    for reg in M.REGIONS:
        assert (s[reg]["lesionwise_dice"], s[reg]["lesionwise_hausdorff95"], s[reg]["n_kept"]) == (1.0, 0.0, 0)
    assert s["TC"]["n_lesions"] == 1 and s["TC"]["lesions"][0]["dice"] == 40 / 80
    # the threshold is strict: 50 voxels are dropped at 50 and kept at 49; 51 are kept at 50
    at50 = [3, 50, 20, 30, 1, 10, 4, 9, 16]
    rec = _record([(0, 0, [at50]), (0, 0, [[3, 51, 20, 30, 1, 10, 4, 9, 16]]), (0, 0, [])])
    s = M.finish_lesions(rec)
    assert s["WT"]["n_kept"] == 0 and s["WT"]["lesionwise_dice"] == 1.0 and s["TC"]["n_kept"] == 1 and s["TC"]["lesionwise_dice"] == 40 / 81
    s = M.finish_lesions(rec, min_lesion_voxels=49)
    assert s["WT"]["n_kept"] == 1 and s["WT"]["lesionwise_dice"] == 40 / 80 and s["WT"]["lesionwise_hausdorff95"] == hd
    # an unmatched kept lesion: Dice 0 and the penalty; false positives: the penalty each, and they count in the denominator
    missed = [900, 70, 0, 0, 0, 0, 0, 0, 0]
    rec = _record([(0, 0, [matched, missed]), (2, 11, [matched, missed]), (3, 5, [])])
    s = M.finish_lesions(rec)
    assert s["WT"]["lesionwise_dice"] == (np.float64(120) / np.float64(180) + 0.0) / 2 and s["WT"]["lesionwise_hausdorff95"] == (hd + 374.0) / 2
    assert s["WT"]["n_fn"] == 1 and s["WT"]["lesions"][1]["hausdorff95"] == 374.0 and s["WT"]["lesions"][1]["dice"] == 0.0
    assert s["TC"]["lesionwise_dice"] == (np.float64(120) / np.float64(180)) / 4
    assert s["TC"]["lesionwise_hausdorff95"] == ((np.float64(hd) + 374.0) + 374.0 * 2) / 4 and s["TC"]["n_fp"] == 2 and s["TC"]["fp_voxels"] == 11
    assert (s["ET"]["lesionwise_dice"], s["ET"]["lesionwise_hausdorff95"]) == (0.0, 374.0)
    s = M.finish_lesions(rec, penalty_hd95=100.0)
    assert s["WT"]["lesionwise_hausdorff95"] == (hd + 100.0) / 2 and s["ET"]["lesionwise_hausdorff95"] == 100.0


def test_one_lesion_all_matched_equals_the_whole_image_scores(golden):
    """one lesion, every predicted voxel in its matched components, no false positive: the lesion-wise values are metrics.finish's"""
    g = golden("lesion")
    pred, truth = g["nested/pred"], g["nested/truth"]
    whole = MR.score(pred, truth)["scores"]["WT"]
    s = R.score(pred, truth, min_lesion_voxels=0)["WT"]
    assert s["n_lesions"] == 1 and s["n_fp"] == 0 and s["lesions"][0]["n_matched"] == 1
    assert s["lesionwise_dice"] == whole["dice"] and s["lesionwise_hausdorff95"] == whole["hausdorff95"]
    assert s["lesions"][0]["hausdorff100"] == whole["hausdorff100"] and s["lesions"][0]["tp"] == whole["tp"]


def test_overflow_bits_and_bad_arguments_raise():
    rec = np.zeros(R.REC_WORDS, np.int64)
    for bit, region, words in ((1, 0, ("N3D_LW_MAX_LESIONS", "WT")), (2, 1, ("N3D_LW_MAX_SURFACE", "TC", "truth")),
                               (4, 2, ("N3D_LW_MAX_SURFACE", "ET", "prediction"))):
        bad = rec.copy()
        bad[region * R.REGION_WORDS + 4] = bit
        bad[region * R.REGION_WORDS] = 65 if bit == 1 else 0
        with pytest.raises(N3DError) as e:
            M.finish_lesions(bad)
        assert all(w in str(e.value) for w in words), str(e.value)
    with pytest.raises(N3DError, match="min_lesion_voxels"):
        M.finish_lesions(rec, min_lesion_voxels=-1)
    with pytest.raises(N3DError, match="penalty_hd95"):
        M.finish_lesions(rec, penalty_hd95=-1.0)
    with pytest.raises(N3DError, match="must hold"):
        M.finish_lesions(rec[:-1])
    for fn in (lambda: M.dilate_mask(np.zeros((2, 2, 2), np.uint8)), lambda: M.lesion_record(np.zeros((2, 2, 2), np.uint8), None)):
        with pytest.raises(N3DError, match="HIP device"):
            fn()


def test_write_csv_default_columns_ignore_the_extra_keys(tmp_path):
    rng = np.random.default_rng(3)
    rows = []
    for i in range(4):
        row = {"Label": "s%d" % i}
        row.update({c: float(rng.uniform(0, 1)) for c in M.COLUMNS[1:]})
        rows.append(row)
    rows[1]["Hausdorff95_ET"] = float("nan")
    M.write_csv(tmp_path / "plain.csv", rows)
    extra = [dict(r, **{c: float(rng.uniform(0, 300)) for c in M.LESION_COLUMNS}) for r in rows]
    extra[2]["LesionWise_Hausdorff95_TC"] = float("nan")
    M.write_csv(tmp_path / "default.csv", extra)
    assert (tmp_path / "plain.csv").read_bytes() == (tmp_path / "default.csv").read_bytes()
    M.write_csv(tmp_path / "lesion.csv", extra, M.COLUMNS + M.LESION_COLUMNS)
    plain = (tmp_path / "plain.csv").read_text().splitlines()
    lines = (tmp_path / "lesion.csv").read_text().splitlines()
    assert len(lines) == len(plain) == 1 + 4 + 5 and lines[0].split(",") == list(M.COLUMNS + M.LESION_COLUMNS)
    assert len(M.LESION_COLUMNS) == 6 and all(l.startswith(p + ",") for l, p in zip(lines, plain))
    assert lines[3].split(",")[-1] == "" and lines[1].split(",")[-6] == repr(extra[0]["LesionWise_Dice_ET"])
    assert lines[5].split(",")[-6] == repr(float(np.mean([r["LesionWise_Dice_ET"] for r in extra])))
