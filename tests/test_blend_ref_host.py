"""CPU: the numpy restatement of the importance-weighted stitch (tests/_blend_ref.py) against the oracle's mean stitch and against a
per-voxel loop, and poststep.blend_profile: formula, exact symmetry, rejections."""
import math

import numpy as np
import pytest

import _blend_ref as br
from oracle import post_step as ps


@pytest.mark.parametrize("P", [6, 7])
def test_ones_profile_is_the_oracle_mean_stitch(P):
    c = br.case(P)
    S, W = br.blend(c["on_grid"], c["corners"], br.SHAPE, np.ones(P))
    assert np.array_equal(br.mean(S, W), ps.stitch(c["on_grid"], c["corners"], br.SHAPE))
    assert (W == 0).any() and (W > 1).any()              # covered and uncovered voxels both occur
    assert np.array_equal(W, np.round(W))                # the weight sum of a ones profile is the covering count


@pytest.mark.parametrize("P", [6, 7])
def test_sliced_reference_equals_per_voxel_loop(P):
    from nas_3d_unet_amd import poststep as hp
    c = br.case(P, with_dead=True)
    prof = hp.blend_profile(P)
    S, W = br.blend(c["on_grid"], c["corners"], br.SHAPE, prof)
    S2, W2 = br.blend_per_voxel(c["on_grid"], c["corners"], br.SHAPE, prof)
    assert (S == S2).all() and (W == W2).all()


@pytest.mark.parametrize("P", [6, 7])
def test_gaussian_result_differs_from_the_mean(P):
    from nas_3d_unet_amd import poststep as hp
    c = br.case(P)
    g = br.mean(*br.blend(c["on_grid"], c["corners"], br.SHAPE, hp.blend_profile(P, "gaussian")))
    m = br.mean(*br.blend(c["on_grid"], c["corners"], br.SHAPE, hp.blend_profile(P, "mean")))
    d = np.abs(g - m).max(axis=0)
    print("P %d: gaussian vs mean: %d of %d voxels differ, max |diff| %.3f" % (P, int((d > 0).sum()), d.size, d.max()))
    # wherever two patches overlap the two blends are different convex combinations of uniform(0, 1) values: a result of the
    # weighted path cannot be mistaken for the unweighted one's
    assert (d > 0).sum() > d.size // 4 and d.max() > 0.1


@pytest.mark.parametrize("P", [6, 7, 16, 128])
def test_blend_profile_formula_and_symmetry(P):
    from nas_3d_unet_amd import poststep as hp
    g = hp.blend_profile(P)
    assert g.dtype == np.float64 and g.shape == (P,)
    assert np.array_equal(g, g[::-1]) and (g > 0).all()
    f = lambda i, s: math.exp(-0.5 * ((i - (P - 1) / 2) / (s * P)) ** 2)
    assert g[0] == pytest.approx(f(0, 0.125), rel=1e-14) and g[P // 2] == pytest.approx(f(P // 2, 0.125), rel=1e-14)
    assert g.max() == g[P // 2] and g.min() == g[0] and (g[P // 2] == 1.0) == (P % 2 == 1)      # not normalised: 1 at a centre voxel
    assert (np.diff(g[:(P + 1) // 2]) > 0).all()
    wide = hp.blend_profile(P, "gaussian", sigma_scale=0.25)
    assert wide[0] == pytest.approx(f(0, 0.25), rel=1e-14) and wide[0] > g[0]
    assert np.array_equal(hp.blend_profile(P, "mean"), np.ones(P))
    own = np.concatenate((np.arange(1, P // 2 + 1), np.arange(1, P - P // 2 + 1)[::-1])).astype(np.float32)
    assert np.array_equal(hp.blend_profile(P, own), own.astype(np.float64))
    assert np.array_equal(hp.blend_profile(P, list(own)), own.astype(np.float64))


def test_blend_profile_rejections():
    from nas_3d_unet_amd import poststep as hp
    from nas_3d_unet_amd._lib import N3DError
    bad = {
        "wrong length": np.ones(5),
        "two-dimensional": np.ones((6, 1)),
        "a zero": [1, 2, 0, 0, 2, 1],
        "a negative": [1, -2, 3, 3, -2, 1],
        "a NaN": [1, 2, float("nan"), float("nan"), 2, 1],
        "an infinity": [1, float("inf"), 3, 3, float("inf"), 1],
        "asymmetric": [1, 2, 3, 3, 2, 1.0000000000000002],
        "unknown name": "triangle",
        "not numbers": ["a"] * 6,
    }
    for what, kind in bad.items():
        with pytest.raises(N3DError):
            hp.blend_profile(6, kind)
            pytest.fail("no error for " + what)
    with pytest.raises(N3DError):
        hp.blend_profile(6, "gaussian", sigma_scale=0.0)
