"""CPU: the numpy statement of the device's crop sampling (tests/_sample_ref.py; include/n3d.h, n3d_volume_line_index and
n3d_patch_sample) against brute force -- np.cumsum for the line index, np.argwhere for the selected voxel --, its corner rule, its
reduction, its mask choice and fallbacks, a known-answer table that pins the statement itself (tests/test_gpu_sample.py holds the
kernels to the statement with ==, so the two cannot drift together), uniformity as a condition, and the host options
(nas_3d_unet_amd.sampling)."""
import numpy as np
import pytest

import _sample_ref as sr
from _appearance_ref import philox4x32_10

KEY = sr.KEY


@pytest.fixture(scope="module")
def four():
    vols, truths = sr.four_volumes()
    return vols, truths, sr.prepare(vols, truths)


def test_line_index_rows_equal_cumsum(four):
    vols, truths, prep = four
    for v, t, (m5, index) in zip(vols, truths, prep):
        X, Y, Z = v.shape[1:]
        brute = [(np.abs(v) > 0).any(0) | np.isnan(v).any(0), t != 0, t == 1, t == 2, t == 4]
        for m in range(5):
            want = np.concatenate(([0], np.cumsum(brute[m].reshape(X * Y, Z).sum(1))))
            assert index.dtype == np.int32 and np.array_equal(index[m], want), m
    bare = sr.line_index(vols[0], None)
    assert bare[0, -1] > 0 and not bare[1:].any()
    assert [int(i[4, -1]) for _, i in prep][1:3] == [0, 0] and int(prep[2][1][1, -1]) == 0          # the absent classes are absent


def test_nonzero_is_the_data_steps_rule():
    v = np.zeros((2, 1, 2, 4), np.float32)
    v[1, 0, 0] = (-0.0, np.nan, np.inf, 1e-45)          # only the last channel decides; 1e-45 is a denormal
    v[0, 0, 1] = (0.0, -0.0, -np.inf, -1e-45)
    assert sr.masks_of(v, None)[0].reshape(-1).tolist() == [False, True, True, True, False, False, True, True]


def test_selected_voxel_is_argwhere_for_every_r(four):
    vols, truths, prep = four
    for v in (0, 3):
        m5, index = prep[v]
        for m in range(5):
            where = np.argwhere(m5[m])
            assert len(where) == index[m, -1]
            for r in range(len(where)) if len(where) < 400 else list(range(0, len(where), 7)) + [len(where) - 1]:
                assert sr.select_voxel(m5, index, m, r) == tuple(where[r]), (v, m, r)
    m5, index = prep[3]
    assert [sr.select_voxel(m5, index, 1, r) for r in range(8)] == [(0, 0, z) for z in (63, 64, 127, 128)] + [(8, 16, z) for z in (63, 64, 127, 128)]


def test_reduce_ends_and_bias():
    for R in (1, 2, 3, 7, 1000, 2 ** 31 - 1, 2 ** 31):
        assert sr.reduce(0, R) == 0 and sr.reduce(0xFFFFFFFF, R) == R - 1
    # value i is taken by floor or ceil of 2^32 / R words
    R = 7
    edges = [-(-(i << 32) // R) for i in range(R + 1)]
    assert all(sr.reduce(e, R) == i and sr.reduce(e - 1, R) == i - 1 for i, e in enumerate(edges[1:-1], 1))
    assert {b - a for a, b in zip(edges, edges[1:])} <= {2 ** 32 // R, 2 ** 32 // R + 1}


def test_corner_rule_small_equal_and_larger_boxes():
    P = 8
    assert sr.corner_bounds(5, P) == (-1, -1) and sr.corner_bounds(4, P) == (-2, -2)       # odd and even difference
    assert sr.corner_bounds(7, P) == (0, 0) and sr.corner_bounds(8, P) == (0, 0) and sr.corner_bounds(9, P) == (0, 1)
    # through sample(): one tumour voxel on each face of a box with all four kinds of axes, always foreground
    for D in ((5, 8, 9), (4, 9, 8), (9, 9, 9)):
        for a in range(3):
            for face in (0, D[a] - 1):
                vox = [d // 2 for d in D]
                vox[a] = face
                vol, t = np.ones((1,) + D, np.float32), np.zeros(D, np.uint8)
                t[tuple(vox)] = 4
                cand, mode = sr.sample([vol], [t], [0], 3, P, KEY, 1 << 32, sr.mask_bits((4,)))
                want = [min(max(x - 4, lo), hi) for x, (lo, hi) in zip(vox, (sr.corner_bounds(d, P) for d in D))]
                assert (mode == 4).all() and (cand == [0] + want).all(), (D, a, face)
                for b in range(3):
                    if D[b] >= P:
                        assert 0 <= want[b] <= D[b] - P and want[b] <= vox[b] < want[b] + P      # the voxel is inside the patch
    # uniform corners stay in [lo, hi] and reach both ends
    vol = np.ones((1, 5, 8, 10), np.float32)
    cand, mode = sr.sample([vol], [None], [0], 200, P, KEY, 0, 0)
    assert (mode == 255).all() and (cand[:, 1] == -1).all() and (cand[:, 2] == 0).all() and set(cand[:, 3]) == {0, 1, 2}


def test_mask_choice_with_absent_classes_and_fallbacks(four):
    vols, truths, prep = four
    always = 1 << 32
    # volume 1 has no label 4: (1, 2, 4) chooses between masks 2 and 3 only; (4,) falls back; volume 2 has no tumour at all
    _, mode = sr.sample(vols, truths, [1], 400, 8, KEY, always, sr.mask_bits((1, 2, 4)), prep)
    assert set(mode) == {2, 3} and 150 < (mode == 2).sum() < 250
    cand, mode = sr.sample(vols, truths, [1], 50, 8, KEY, always, sr.mask_bits((4,)), prep)
    uni, umode = sr.sample(vols, truths, [1], 50, 8, KEY, 0, sr.mask_bits((4,)), prep)
    assert (mode == 254).all() and (umode == 255).all() and np.array_equal(cand, uni)            # a fallback uses the uniform words
    _, mode = sr.sample(vols, truths, [2], 50, 8, KEY, always, sr.mask_bits(("tumour", 1, 2, 4)), prep)
    assert (mode == 254).all()
    _, mode = sr.sample(vols, truths, [2], 50, 8, KEY, always, sr.mask_bits(("brain", 4)), prep)
    assert (mode == 0).all()
    # an id outside the set: (id, 0, 0, 0), mode 253, whatever the other arguments
    cand, mode = sr.sample(vols, truths, [7, 0, -2], 60, 8, KEY, always, sr.mask_bits(("tumour",)), prep)
    bad = mode == 253
    assert 20 < bad.sum() < 55 and set(cand[bad, 0]) == {7, -2} and not cand[bad, 1:].any() and set(mode[~bad]) == {1}
    # the foreground decision: u1 < threshold, so threshold 0 is never and 2^32 always, for every word
    assert (sr.sample(vols, truths, [0], 50, 8, KEY, 0, 2, prep)[1] == 255).all()
    assert (sr.sample(vols, truths, [0], 50, 8, KEY, always, 2, prep)[1] == 1).all()


def test_draws_use_counter_words_2_and_3():
    d = sr.draws(3, KEY)
    assert d[2] == (philox4x32_10((2, 2, 0, 0), KEY), philox4x32_10((2, 3, 0, 0), KEY))
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)     # Random123's known answer


KNOWN = dict(ids=[3, 1, 0, 2], N=8, P=8, fg=3 << 30, masks=("brain", 1, 4))
KNOWN_CAND = [[2, 0, 0, 2], [2, 3, 0, 0], [3, 1, 0, 50], [3, 0, 0, 33], [0, -1, 0, 0], [2, 9, 11, 0], [0, -1, 0, 0], [1, 7, 2, 5]]
KNOWN_MODE = [0, 0, 0, 0, 255, 0, 4, 255]


def test_known_answers(four):
    vols, truths, prep = four
    k = KNOWN
    cand, mode = sr.sample(vols, truths, k["ids"], k["N"], k["P"], KEY, k["fg"], sr.mask_bits(k["masks"]), prep)
    assert cand.tolist() == KNOWN_CAND and mode.tolist() == KNOWN_MODE


def test_uniformity_over_seven_voxels_and_the_foreground_share():
    """conditions, not measurements: N = 7000 draws over exactly 7 tumour voxels, each count within 6 sigma of 1000 (binomial sigma
    = sqrt(7000 * 1/7 * 6/7) = 29.3); with foreground = 1/3 and N = 6000 the foreground samples within 6 sigma of 2000 (sigma =
    sqrt(6000 * 1/3 * 2/3) = 36.5).  With the key fixed here the statement gives 1010, 996, 959, 996, 1026, 978, 1035 and 1981:
    tests/test_gpu_sample.py asks the same of the kernel's output under this key"""
    P = 8
    vol, t = sr.seven_voxel_volume()
    prep = sr.prepare([vol], [t])
    cand, mode = sr.sample([vol], [t], [0], 7000, P, KEY, 1 << 32, sr.mask_bits(("tumour",)), prep)
    assert (mode == 1).all()
    _, mode3 = sr.sample([vol], [t], [0], 6000, P, KEY, int(round(2 ** 32 / 3)), sr.mask_bits(("tumour",)), prep)
    counts, share = sr.uniformity_counts(cand, mode3)
    assert sum(counts) == 7000 and all(abs(c - 1000) <= 6 * 29.3 for c in counts), counts
    assert set(mode3) == {1, 255} and abs(share - 2000) <= 6 * 36.5, share


def test_random_crop_options_are_validated():
    from nas_3d_unet_amd import sampling as S
    from nas_3d_unet_amd._lib import N3DError
    assert S.MASKS == sr.MASKS and (S.MODE_UNIFORM, S.MODE_FALLBACK, S.MODE_BAD_ID) == (255, 254, 253)
    c = S.RandomCrop(24)
    assert (c.patches_per_epoch, c.masks, c.mask_bits, c.fg_threshold) == (24, ("tumour",), 2, int(round(2 ** 32 / 3))) and c.needs_truth()
    assert S.RandomCrop(1, 1.0, (1, 2, 4)).mask_bits == 28 == sr.mask_bits((1, 2, 4)) and S.RandomCrop(1, 1.0, (4,)).fg_threshold == 2 ** 32
    assert not S.RandomCrop(5, 0.5, ("brain",)).needs_truth() and S.RandomCrop(5, 0.0, ()).mask_bits == 0
    for bad in (dict(patches_per_epoch=0), dict(patches_per_epoch=2 ** 24 + 1), dict(patches_per_epoch=2.0), dict(patches_per_epoch=True),
                dict(foreground=-0.1), dict(foreground=1.5), dict(foreground=float("nan")), dict(masks=(3,)), dict(masks=("tumor",)),
                dict(masks="tumour"), dict(masks=(True,)), dict(masks=()), dict(masks=(1.0,))):
        with pytest.raises(N3DError):
            S.RandomCrop(**{"patches_per_epoch": 8, **bad})

    class Rec:
        def __init__(self):
            self.calls = []

        def randint(self, *a, **k):
            self.calls.append((a, k))
            return np.array([7, 2 ** 32 - 1], np.uint32)

    r = Rec()
    assert c.draw(r) == (7, 2 ** 32 - 1) and r.calls == [((0, 2 ** 32, 2), {"dtype": np.uint32})]


def test_generator_signature_gains_only_sampling():
    import inspect
    from nas_3d_unet_amd.generator import Generator, VolumeSet
    params = list(inspect.signature(Generator.__init__).parameters.values())
    assert params[-1].name == "sampling" and params[-1].default is None and params[-2].name == "augment_elastic"
    assert hasattr(VolumeSet, "line_index") and hasattr(VolumeSet, "sample")


def test_generator_refuses_a_volume_set_that_cannot_sample():
    from nas_3d_unet_amd.generator import Generator
    from nas_3d_unet_amd.sampling import RandomCrop

    class NoSample:
        channels, has_truth = 4, True

    with pytest.raises(NotImplementedError, match="sample"):
        Generator([0], NoSample(), 8, sampling=RandomCrop(4))
