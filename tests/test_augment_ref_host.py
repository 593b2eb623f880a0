"""CPU: the scale / flip augmentation of the generator (nas_3d_unet_amd.generator: draw_augment, scale_affine, resample_transform,
resample_params, epoch_order(augment=...)) and the numpy statement of the device rule (tests/_augment_ref.py) against the
reference's own do_augment and Generator, run over scipy by tests/golden/make_golden_augment.py into augment.npz.  No scipy here."""
import random

import numpy as np
import pytest

import _augment_ref as ar
import make_golden_augment as mga
import make_golden_generator as mg
from test_generator_host import _NoVolumes, brute_flags


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def test_helper_equals_the_reference_operator(golden):
    recs = ar.operator_records(golden("augment"))
    assert len(recs) == len(mga.operator_cases())
    resampled = 0
    for cfg, scale, flips, A, b, identity, x, y in recs:
        data, truth = mga.operator_inputs(cfg["P"])
        A_, sh = ar.params_of(A, b, identity)
        got_x, got_y = ar.augment_patch(data, A_, sh, identity, flips), ar.augment_patch(truth, A_, sh, identity, flips)
        assert got_x.dtype == np.float32 and got_y.dtype == np.uint8
        assert np.array_equal(got_x, x) and np.array_equal(got_y, y), cfg["name"]
        resampled += int(not identity)
        if not identity or flips.any():
            assert not np.array_equal(x, data), cfg["name"]
    assert resampled >= 6


def test_helper_equals_scipy_where_the_textbook_formula_does_not(golden):
    recs = ar.adversarial_records(golden("augment"))
    assert len(recs) >= 4
    kinds = set()
    for P, axis, A, b, src in recs:
        assert np.array_equal(ar.axis_table(P, A, np.float64(b) / np.float64(A), False, False), src), (P, A, b)
        c = np.float64(A) * np.arange(P, dtype=np.float64) + np.float64(b)
        naive = np.where((c >= 0) & (c <= P - 1), np.floor(c + 0.5), -1).astype(np.int64)
        assert not np.array_equal(naive, src)
        kinds.add("bound" if ((naive < 0) != (src < 0)).any() else "voxel")
    assert kinds == {"bound", "voxel"}


def test_host_functions_reproduce_the_recorded_transforms(golden):
    from nas_3d_unet_amd import generator as G
    recs = ar.operator_records(golden("augment"))
    for case, (cfg, scale, flips, A, b, identity, _, _) in zip(mga.operator_cases(), recs):
        M = G.check_affine(mga.AFFINES[cfg["affine"]])
        A2, b2, id2 = G.resample_transform(M, cfg["P"], scale)
        assert id2 == identity and np.array_equal(_bits(A2), _bits(A)) and np.array_equal(_bits(b2), _bits(b)), cfg["name"]
        A3, sh3, id3 = G.resample_params(M, cfg["P"], scale)
        assert id3 == identity and np.array_equal(_bits(A3), _bits(A)), cfg["name"]
        assert np.array_equal(_bits(sh3), _bits(np.asarray(b) / np.asarray(A))), cfg["name"]
        name, P, aff, dev, flip, draws = case
        if isinstance(draws, int):                  # the seeded cases: the package draws what the reference drew
            s2, axes = G.draw_augment(np.random.RandomState(draws), dev, flip)
            assert (s2 is None) == (scale is None) and (scale is None or np.array_equal(_bits(s2), _bits(scale))), name
            assert [int(a in (axes or [])) for a in range(3)] == flips.tolist() and (axes is None) == (not flip), name
    # no draw at all without a factor and without flips, and the order: the scale first
    rs = np.random.RandomState(9)
    state = rs.get_state()[1].copy()
    assert G.draw_augment(rs, None, False) == (None, None) and np.array_equal(rs.get_state()[1], state)
    a, b = np.random.RandomState(9), np.random.RandomState(9)
    s, axes = G.draw_augment(a, 0.25, True)
    assert np.array_equal(s, b.normal(1, 0.25, 3)) and axes == [d for d in range(3) if b.choice([True, False])]


def test_epoch_order_with_augmentation_reproduces_the_reference_generator(golden):
    from nas_3d_unet_amd import generator as G
    volumes = mg.generator_volumes()
    boxes = [v.shape[1:] for v, _ in volumes]
    seen = {"flip": False, "noflip": False, "noscale": False, "key": False}
    recs = ar.generator_records(golden("augment"))
    assert len(recs) == len(mga.generator_cases())
    for cfg, rows, scales, _, _ in recs:
        kw = cfg["kwargs"]
        P, B, po = kw["patch_shape"], kw["batch_size"], kw["patch_overlap"]
        rng, np_rng = random.Random(cfg["seed"]), np.random.RandomState(cfg["np_seed"])
        draws = (np_rng, kw.get("augment_distortion_factor", 0.25), kw.get("augment_flip", True))
        overlaps = [G.draw_overlap(po, rng)]
        for e in range(cfg["epochs"]):
            cand = G.candidate_table(boxes, kw["indices_list"], P, overlaps[-1], kw.get("both_ps", False))
            flags = brute_flags(volumes, cand, P, True)
            assert -(-int(G.kept_mask(flags, True).sum()) // B) == cfg["spe"][e], (cfg["name"], e)
            got_rows, got_scales = [], []
            for b, batch in enumerate(G.epoch_order(flags, B, rng, True, kw.get("shuffle_index_list", True), kw.get("permute", False),
                                                    augment=draws)):
                for i, key, (scale, axes) in batch:
                    k = [-1] * 6 if key is None else [key[0][0], key[0][1], key[1], key[2], key[3], key[4]]
                    got_rows.append([e, b, *cand[i].tolist(), *k, *[int(a in (axes or [])) for a in range(3)]])
                    got_scales.append(np.full(3, np.nan) if scale is None else scale)
            want = rows[rows[:, 0] == e]
            np.testing.assert_array_equal(np.asarray(got_rows, np.int32).reshape(-1, 15), want, err_msg=cfg["name"])
            assert np.array_equal(_bits(np.asarray(got_scales).reshape(-1, 3)), _bits(scales[rows[:, 0] == e])), cfg["name"]
            if po:
                overlaps.append(G.draw_overlap(po, rng))
        assert overlaps == cfg["overlap"][:len(overlaps)], (cfg["name"], overlaps)
        seen["flip"] |= bool(rows[:, 12:].any())
        seen["noflip"] |= not kw.get("augment_flip", True) and not rows[:, 12:].any()
        seen["noscale"] |= bool(np.isnan(scales).all())
        seen["key"] |= bool((rows[:, 6] >= 0).any())
    assert all(seen.values()), seen


def test_augment_constructor_validation_without_a_device():
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd._lib import N3DError
    with pytest.raises(N3DError, match="32"):
        G.Generator([0], _NoVolumes(), 8, augment=True, batch_size=33)
    skew = np.eye(4)
    skew[0, 1] = 0.1
    with pytest.raises(N3DError, match="diagonal"):
        G.Generator([0], _NoVolumes(), 8, augment=True, affine=skew)
    with pytest.raises(N3DError):
        G.Generator([0], _NoVolumes(), 8, augment=True, affine=np.eye(3))
    # a stand-in for the volume set that cannot make augmented batches is refused at construction, before any draw
    with pytest.raises(NotImplementedError, match="patch_batch"):
        G.Generator([0], _NoVolumes(), 8, augment=True, affine=mga.BRATS_AFFINE)
    assert "augment" in __import__("inspect").signature(G.VolumeSet.patch_batch).parameters
    # without augment neither limit applies before the volumes are touched: batch_size 33 is legal, the affine is not looked at
    with pytest.raises(AssertionError, match="touched"):
        G.Generator([0], _NoVolumes(), 8, batch_size=33, affine=skew)
    # a zero scale makes the scaled affine singular: numpy.linalg.inv raises, as in the reference
    with pytest.raises(np.linalg.LinAlgError):
        G.resample_transform(np.eye(4), 8, np.array([1.0, 0.0, 1.0]))
    # a negative scale is legal
    A, sh, identity = G.resample_params(np.eye(4), 8, np.array([-1.0, 1.0, 1.0]))
    assert not identity and A[0] == -1.0 and sh[0] == -8.0
