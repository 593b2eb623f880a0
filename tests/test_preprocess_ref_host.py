"""CPU: the numpy restatement of the reference's preprocessing (tests/_preprocess_ref.py) equals the fixture the reference's own
functions produced (tests/golden/preprocess.npz, make_golden_preprocess.py) bit for bit, and the fixture meets the precondition
the GPU tests lean on: no std sits near a rounding boundary of round(., 4)."""
import numpy as np
import pytest

import _preprocess_ref as pr
import make_golden_preprocess as mp


@pytest.fixture(scope="module")
def subjects():
    return mp.preprocess_subjects()


def test_inputs_are_what_the_fixture_was_made_from(golden, subjects):
    g = golden("preprocess")
    assert tuple(g["mods"]) == mp.MODS
    assert [s[0].shape[1:] for s in subjects] == mp.SHAPES
    for raw, truth in subjects:
        assert raw.dtype == np.int16 and truth.dtype == np.uint8 and raw.shape[0] == len(mp.MODS)
        assert (raw < 0).any() and raw.max() <= 4000
    # one modality sees half of the brain only: the outlines differ between modalities
    raw = subjects[1][0]
    assert not np.array_equal(pr.outline(raw[mp.HALF_MOD]), pr.outline(raw[0]))


def test_dataset_statistics_equal_the_fixture(golden, subjects):
    g = golden("preprocess")
    count, total, mean, std = pr.dataset_stats([s[0] for s in subjects])
    np.testing.assert_array_equal(count, g["count"])
    np.testing.assert_array_equal(total, g["sum"])
    assert mean.tobytes() == g["unrounded"][:, 0].tobytes()
    assert std.tobytes() == g["unrounded"][:, 1].tobytes()
    d = np.array([[pr.rounded(m), pr.rounded(s)] for m, s in zip(mean, std)])
    assert d.tobytes() == g["dict"].tobytes()


def test_std_is_clear_of_every_rounding_boundary(golden):
    """|std * 1e4 - (k + 1/2)| >= 1e-3 for every integer k: a relative change of the sum of squares of n * 2^-53 (n < 1e4 voxels
    here: ~1e-12, i.e. ~1e-5 on std * 1e4 ~ 1e7) cannot move the rounded value, whatever the order of summation"""
    g = golden("preprocess")
    for c, m in enumerate(mp.MODS):
        scaled = g["unrounded"][c, 1] * 1e4
        assert abs(scaled - np.floor(scaled) - 0.5) >= 1e-3, (m, scaled)


@pytest.mark.parametrize("i", range(len(mp.SHAPES)))
def test_normalised_volumes_and_brain_width_equal_the_fixture(golden, subjects, i):
    g = golden("preprocess")
    raw = subjects[i][0]
    norm = np.stack([pr.normalize(raw[c], g["dict"][c, 0], g["dict"][c, 1]) for c in range(raw.shape[0])])
    np.testing.assert_array_equal(norm, g["sub%d/normalized" % i].astype(np.int16))
    bw = pr.brain_width(norm)
    np.testing.assert_array_equal(bw, g["sub%d/brain_width" % i])
    # normalised brain voxels are 10..110, so the outline of the raw array is the outline of the normalised one
    np.testing.assert_array_equal(pr.brain_width(raw), bw)


def test_touching_subject_clamps(golden, subjects):
    g = golden("preprocess")
    bw, shape = g["sub%d/brain_width" % mp.TOUCHING], mp.SHAPES[mp.TOUCHING]
    assert bw[0, 0] == 0 and bw[1, 2] == shape[2]
    sl = pr.box_slices(bw, shape)
    assert sl[2].stop == shape[2] and sl[0].stop == bw[1, 0] + 1
