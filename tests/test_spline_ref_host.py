"""CPU: the numpy statement of n3d_patch_gather_spline's rule (tests/_spline_ref.py) against tests/golden/spline.npz -- scipy's
map_coordinates(order=3, mode="constant") and spline_filter(order=3, mode="mirror"), written by make_golden_spline.py -- and the host
side of the option: the generator's argument, its limits, the routing of VolumeSet.patch_batch.  No scipy and no device here."""
import inspect
import os
import random
import re
import types

import numpy as np
import pytest

import _elastic_ref as er
import _spline_ref as sr
import _warp_ref as wr
import make_golden_augment as mga
import make_golden_generator as mg
from make_golden_elastic import case_inputs
from test_generator_host import _NoVolumes
from test_warp_ref_host import _HostVolumes, _Recorder

# the largest |statement - scipy.ndimage.spline_filter| / max|x| over the fixture's crops is 3.775e-15 (make_golden_spline.py prints
# it); the two differ in the order of operations only, and four times the measured value is allowed
COEF_BOUND = 4 * 3.775e-15


def test_the_statement_gives_scipys_answers_where_the_mask_keeps_a_voxel_and_zero_elsewhere(golden):
    """one float32 step at every kept voxel (order 1's criterion; 0 of the fixture's 28 287 kept voxels differ at all), exactly 0
    at every dropped one, never 0 at a kept one; the cases are the elastic fixture's (P 8, 12, 16, a crop hanging out of the volume,
    flips, both modes) with their displacement, and three of them without it"""
    recs = sr.records(golden("spline"))
    assert sorted({c["P"] for c, *_ in recs}) == [8, 12, 16] and {c["mode"] for c, *_ in recs} == {0, 1}
    assert any(any(c["flips"]) for c, *_ in recs) and any(min(c["corner"]) < 0 for c, *_ in recs)
    assert sum(c["elastic"] for c, *_ in recs) >= 8 and sum(not c["elastic"] for c, *_ in recs) >= 3
    differ = total = 0
    for c, k, x3 in recs:
        data, _ = case_inputs(c)
        coords = er.coordinates(c["P"], c["mode"], k, sr.case_elastic(c))
        have = sr.spline_patch(data, c["mode"], k, sr.case_elastic(c), c["flips"])
        keep = sr.mask(sr.flipped(data, c["flips"]), coords)
        assert have.dtype == np.float32 and 0.1 < keep.mean() < 0.9, c["name"]
        assert wr.one_step(have, x3)[keep].all(), c["name"]
        assert not have[~keep].any() and not np.signbit(have[~keep]).any() and (have[keep] != 0).all(), c["name"]
        # scipy itself is nonzero on the background the mask drops: the mask is not a no-op
        inside = np.broadcast_to(sr.nearest(c["P"], coords)[0], keep.shape)
        assert (x3[~keep & inside] != 0).mean() > 0.9, c["name"]
        differ += int((have != x3)[keep].sum())
        total += int(keep.sum())
    assert total > 20000 and differ * 1000 <= total


def test_the_mask_is_the_nonzero_set_of_order_0_and_a_zero_sum_becomes_flt_min():
    P = 8
    data, _ = case_inputs({"P": P, "corner": (0, 0, 0)})
    k = wr.coefficients(0, np.ones(3), np.full(3, 0.3))
    c = er.coordinates(P, 0, k)
    have, near = sr.resample(data, c), er.resample(data, c, 0)
    assert np.array_equal(have != 0, near != 0) and (near == 0).any() and (near != 0).any()
    # a kept voxel whose spline value rounds to 0 in float32 stays nonzero: one voxel holding the smallest denormal, read 0.45 voxels
    # away on every axis (the cardinal spline is about 0.6 there per axis: 0.2 of a value that has no smaller neighbour but 0)
    raw = np.zeros((1, P, P, P), np.float32)
    raw[0, 2, 2, 2] = np.float32(1e-45)
    c45 = er.coordinates(P, 0, wr.coefficients(0, np.ones(3), np.full(3, 0.45)))
    assert raw[0, 2, 2, 2] != 0 and 0 < sr.spline_values(sr.coefficients(raw), c45)[0, 2, 2, 2] < 0.7e-45
    out = sr.resample(raw, c45)
    assert out[0, 2, 2, 2] == sr.FLT_MIN > 0 and (out != 0).sum() == 1
    # gain and bias act on the kept voxels only
    g, b = np.array([1.5, 0.5]), np.array([-2.0, 3.0])
    shaded = sr.resample(data, c, gain=g, bias=b)
    keep = have != 0
    want = have * g.astype(np.float32)[:, None, None, None] + b.astype(np.float32)[:, None, None, None]
    assert np.array_equal(shaded[keep], want[keep]) and not shaded[~keep].any()


def test_coefficients_equal_spline_filter_within_four_times_the_measured_difference(golden):
    """measured over the fixture's five crops: 3.775e-15 * max|x| (the README quotes it); allowed: four times that"""
    crops = sr.crops(golden("spline"))
    assert len(crops) >= 5
    worst = 0.0
    for c, want in crops:
        data, _ = case_inputs(c)
        raw = sr.flipped(data, c["flips"])
        have = sr.coefficients(raw)
        assert have.dtype == np.float64 and have.shape == want.shape
        worst = max(worst, float(np.abs(have - want).max() / np.abs(raw).max()))
    print("largest |statement - spline_filter| / max|x| = %.3e" % worst)
    assert worst <= COEF_BOUND


@pytest.mark.parametrize("P", [4, 5, 8, 12, 16, 64])
def test_coefficients_of_a_constant_line_are_that_constant(P):
    for value in (1.0, -3.25, 110.0):
        have = sr.filter_axis(np.full((P, 3), value), 0)
        assert np.abs(have - value).max() <= COEF_BOUND * abs(value)
    cube = sr.coefficients(np.full((P, P, P), 7.5, np.float32)) if P <= 16 else np.full(1, 7.5)
    assert np.abs(cube - 7.5).max() <= 3 * COEF_BOUND * 7.5             # three passes


def test_constants_are_the_host_modules_and_the_filter_is_an_inverse():
    from nas_3d_unet_amd import spline
    from nas_3d_unet_amd._lib import N3DError
    for P in (4, 7, 16, 64, 128):
        a, b = spline.constants(P), sr.constants(P)
        assert all(np.float64(x).tobytes() == np.float64(y).tobytes() for x, y in zip(a, b))
        z, gain, zn, inv0, anti = b
        assert abs(z - (np.sqrt(3) - 2)) == 0 and abs(gain - 6.0) < 1e-14 and abs(zn - z ** (P - 1)) <= 1e-15 * abs(zn)
    with pytest.raises(N3DError, match="at least 4"):
        spline.constants(3)
    # sampling the spline on the integers gives the line back: (c[i-1] + 4 c[i] + c[i+1]) / 6 with mirrored ends
    rs = np.random.RandomState(3)
    x = rs.uniform(10, 110, (9, 5))
    c = sr.filter_axis(x, 0)
    ext = np.concatenate((c[1:2], c, c[-2:-1]))
    assert np.abs((ext[:-2] + 4 * ext[1:-1] + ext[2:]) / 6 - x).max() < 1e-12


def test_constructor_validation_without_a_device():
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd._lib import N3DError
    aff = mga.BRATS_AFFINE
    with pytest.raises(N3DError, match="augment=True"):
        G.Generator([0], _NoVolumes(), 8, augment_interpolation="spline3")
    with pytest.raises(N3DError, match="N3D_PATCH_ELASTIC_MAX_BATCH"):
        G.Generator([0], _NoVolumes(), 8, augment=True, affine=aff, batch_size=9, augment_interpolation="spline3")
    with pytest.raises(N3DError, match="at least 4"):
        G.Generator([0], _NoVolumes(), 3, augment=True, affine=aff, augment_interpolation="spline3")
    with pytest.raises(N3DError, match="interpolation"):
        G.Generator([0], _NoVolumes(), 8, augment=True, affine=aff, augment_interpolation="cubic")
    # batch_size 8 passes the checks and reaches the volumes; 9 stays legal for "linear"
    for kw in (dict(batch_size=8, augment_interpolation="spline3"), dict(batch_size=9, augment_interpolation="linear")):
        with pytest.raises(NotImplementedError, match="patch_batch"):
            G.Generator([0], _NoVolumes(), 8, augment=True, affine=aff, **kw)
    np_rng = _Recorder(1)
    with pytest.raises(NotImplementedError, match="warp"):
        G.Generator([0], _HostVolumes(mg.generator_volumes(), with_warp=False), 8, augment=True, affine=aff, np_rng=np_rng,
                    augment_interpolation="spline3")
    assert np_rng.calls == [] and G.INTERPOLATION_ORDER == {"nearest": 0, "linear": 1, "spline3": 3}


def test_the_generator_draws_what_linear_draws_and_hands_order_3_to_patch_batch():
    from nas_3d_unet_amd import generator as G
    volumes = mg.generator_volumes()
    kw = dict(indices_list=[3, 0], patch_shape=8, patch_overlap=3, batch_size=2, permute=True, augment=True, labels=[1, 2, 4],
              affine=mga.BRATS_AFFINE, augment_rotation=(15, 10, 5), augment_intensity_scale=0.1)
    runs = {}
    for name in ("linear", "spline3"):
        s, rec = _HostVolumes(volumes), _Recorder(131)
        gen = G.Generator(volumes=s, rng=random.Random(35), np_rng=rec, augment_interpolation=name, **kw)
        spe = gen.steps_per_epoch                       # (a drawn overlap: the epoch's end draws the next one)
        assert gen.warped and len(list(gen.epoch())) == spe
        runs[name] = (s.batches, rec.calls)
    (lin, lin_calls), (spl, spl_calls) = runs["linear"], runs["spline3"]
    assert lin_calls == spl_calls and len(lin) == len(spl) >= 2
    for (r1, a1, w1), (r3, a3, w3) in zip(lin, spl):
        assert repr(r1) == repr(r3) and repr(a1) == repr(a3) and len(w1) == len(w3)
        for (m1, o1, g1, b1), (m3, o3, g3, b3) in zip(w1, w3):
            assert (o1, o3) == (1, 3) and b1 is None and b3 is None
            assert all(np.array_equal(x, y) for x, y in zip(m1, m3)) and np.array_equal(g1, g3)


def test_patch_batch_refuses_mixed_orders():
    """on a stand-in for the set: the descriptor table is built on the host"""
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd._lib import N3DError
    s = types.SimpleNamespace(channels=2)
    refs = [(0, (0, 0, 0), None)] * 3
    three, one = (None, 3, None, None), (None, 1, None, None)
    assert [d.order for d in G.VolumeSet._warp_descs(s, refs, 8, None, [three] * 3)] == [3, 3, 3]
    assert [d.order for d in G.VolumeSet._warp_descs(s, refs, 8, None, [one, None, one])] == [1, 0, 1]
    for warp in ([three, one, three], [three, None, three], [(None, 0, None, None), three, three]):
        with pytest.raises(N3DError, match="order 3"):
            G.VolumeSet._warp_descs(s, refs, 8, None, warp)
    with pytest.raises(N3DError, match="interpolation order"):
        G.VolumeSet._warp_descs(s, refs, 8, None, [(None, 2, None, None)] * 3)
    assert "warp" in inspect.signature(G.VolumeSet.patch_batch).parameters


def test_the_abi_declares_the_exports():
    from nas_3d_unet_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "n3d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("n3d_patch_spline_scratch_bytes", "n3d_spline_prefilter", "n3d_patch_gather_spline"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.PROTOTYPES
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.n3d_patch_spline_scratch_bytes(2, 4, 64) == 12 * 2 * 4 * 64 ** 3
        assert lib.n3d_patch_spline_scratch_bytes(8, 4, 128) == 12 * 8 * 4 * 128 ** 3 and lib.n3d_patch_spline_scratch_bytes(0, 4, 8) == 0
