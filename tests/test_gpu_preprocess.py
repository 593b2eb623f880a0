"""GPU: raw int16 scans to the mean / std dictionary and to normalised brain-wise boxes (nas_3d_unet_amd.preprocess; n3d_brain_scan,
n3d_brain_sqdev, n3d_brain_normalize) against what the reference's own cal_mean_std / create_h5 produced
(tests/golden/preprocess.npz).  Integer quantities, means, the rounded dictionary, brain_width and the normalised boxes are
compared exactly (the boxes bit for bit); the unrounded std within a derived bound.

Shapes (make_golden_preprocess.SHAPES): (13, 11, 7) -- 1001 voxels, so modalities 1 and 3 start off a 16-byte boundary, with head
and tail voxels; (40, 36, 31) x 4 -- several workgroups per modality and an odd last axis; (22, 18, 15) -- the brain touches
x = 0 and the high z face (start clamps to 0, end == shape, the box is clipped); the data set is these three together."""
import random

import numpy as np
import pytest
import torch

import _preprocess_ref as pr
import make_golden_preprocess as mp

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def subjects():
    return mp.preprocess_subjects()


@pytest.fixture(scope="module")
def mean_std(golden):
    g = golden("preprocess")
    return {"%s_%s" % (m, k): np.float64(g["dict"][c, j]) for c, m in enumerate(mp.MODS) for j, k in enumerate(("mean", "std"))}


def _expected_box(g, i, truth):
    bw, shape = g["sub%d/brain_width" % i], mp.SHAPES[i]
    sl = pr.box_slices(bw, shape)
    return g["sub%d/normalized" % i][(slice(None),) + sl].astype(np.float32), truth[sl], bw


@pytest.mark.parametrize("i", range(len(mp.SHAPES)))
@pytest.mark.parametrize("offset", [0, 3])
def test_scan_equals_numpy(subjects, i, offset):
    """n3d_brain_scan alone: count, sum, extrema and index bounds per modality; added to running totals; also from a base that is
    only 2-byte aligned (offset 3 voxels into an allocation)"""
    from nas_3d_unet_amd import _lib, preprocess as P
    from nas_3d_unet_amd import kernels as K
    raw = subjects[i][0]
    Cm, X, Y, Z = raw.shape
    buf = torch.zeros(raw.size + 16, dtype=torch.int16, device="cuda")
    buf[offset:offset + raw.size] = torch.from_numpy(raw).cuda().reshape(-1)
    r = buf[offset:offset + raw.size]
    totals = torch.tensor([[5, -7]] * Cm, dtype=torch.int64, device="cuda")
    rec = P._records(1, Cm, "cuda")[0]
    _lib.check(_lib.load().n3d_brain_scan(K.ptr(r), Cm, X, Y, Z, K.ptr(totals), K.ptr(rec), K.stream_ptr()))
    totals, rec = totals.cpu().numpy(), rec.cpu().numpy()
    for c in range(Cm):
        idx = np.asarray(np.nonzero(raw[c]))
        vals = raw[c][np.nonzero(raw[c])].astype(np.int64)
        assert totals[c].tolist() == [5 + len(vals), -7 + int(vals.sum())]
        assert rec[c].tolist() == [vals.min(), vals.max(), *idx.min(axis=1), *idx.max(axis=1)]


def _assert_stats(st, count, total, mean, std):
    """count, sum: equal.  mean: equal bits (one correctly rounded quotient of two exactly converted integers on both sides).
    std, with u = 2^-53 and n the modality's brain voxels: every term fl(fl(x - mean)^2) is the same double on both sides (same
    operands, IEEE operations, no contraction), so the two sums S differ only by their order of addition.  A sum of n positive
    terms in any order is within (n - 1) u relative of the exact one, so the two S are within 2 (n - 1) u of each other; the square
    root halves that: (n - 1) u.  S / n and the root add one rounding each on each side, the quotient's halved by the root:
    2 (u / 2 + u) = 3 u.  Total (n + 2) u, inside the (n + 4) u asserted."""
    np.testing.assert_array_equal(st.count, count)
    np.testing.assert_array_equal(st.sum, total)
    assert st.mean.dtype == np.float64 and st.mean.tobytes() == np.asarray(mean, np.float64).tobytes()
    for c in range(len(count)):
        rel = abs(st.std[c] - std[c]) / std[c]
        print("modality %d: n %d  std %.17g  expected %.17g  rel %.3g  bound %.3g" % (c, count[c], st.std[c], std[c], rel, (count[c] + 4) * U))
        assert rel <= (count[c] + 4) * U


def test_dataset_statistics_equal_the_fixture(golden, subjects):
    from nas_3d_unet_amd import preprocess as P
    g = golden("preprocess")
    st = P.dataset_stats([s[0] for s in subjects])
    _assert_stats(st, g["count"], g["sum"], g["unrounded"][:, 0], g["unrounded"][:, 1])


@pytest.mark.parametrize("i", [0, 1])
def test_single_subject_statistics(subjects, i):
    """each shape as a data set of its own, against the restatement the CPU half pins to the fixture; raw given as a device tensor"""
    from nas_3d_unet_amd import preprocess as P
    raw = subjects[i][0]
    st = P.dataset_stats([torch.from_numpy(raw).cuda()])
    _assert_stats(st, *pr.dataset_stats([raw]))


def test_dictionary_equals_the_fixture_and_repeats_bit_for_bit(golden, subjects):
    from nas_3d_unet_amd import preprocess as P
    g = golden("preprocess")
    raws = [s[0] for s in subjects]
    d = P.cal_mean_std(raws)
    assert list(d) == ["%s_%s" % (m, k) for m in mp.MODS for k in ("mean", "std")]
    for c, m in enumerate(mp.MODS):
        assert type(d[m + "_mean"]) is np.float64 and type(d[m + "_std"]) is np.float64
        assert d[m + "_mean"] == g["dict"][c, 0] and d[m + "_std"] == g["dict"][c, 1]
    a, b = P.dataset_stats(raws), P.dataset_stats(raws)
    assert a.std.tobytes() == b.std.tobytes() and a.mean.tobytes() == b.mean.tobytes()
    assert P.cal_mean_std(raws) == d


@pytest.mark.parametrize("i", range(len(mp.SHAPES)))
def test_normalised_box_is_bit_identical(golden, subjects, mean_std, i):
    from nas_3d_unet_amd import preprocess as P
    g = golden("preprocess")
    raw, truth = subjects[i]
    want, want_t, bw = _expected_box(g, i, truth)
    vol, t, brain_width = P.normalize_subject(raw, mean_std, truth)
    assert vol.dtype == torch.float32 and vol.is_contiguous() and t.dtype == torch.uint8
    np.testing.assert_array_equal(brain_width, bw)
    assert brain_width.shape == (2, 3)
    got = vol.cpu().numpy()
    assert got.shape == want.shape
    assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    np.testing.assert_array_equal(t.cpu().numpy(), want_t)
    # without truth, truth as (1, X, Y, Z), raw as a device tensor
    vol2, t2, _ = P.normalize_subject(torch.from_numpy(raw).cuda(), mean_std)
    assert t2 is None and torch.equal(vol2, vol)
    _, t3, _ = P.normalize_subject(raw, mean_std, truth[None])
    assert torch.equal(t3, t)


def test_touching_subject_box_is_clipped(golden, subjects, mean_std):
    from nas_3d_unet_amd import preprocess as P
    i = mp.TOUCHING
    raw, truth = subjects[i]
    vol, _, bw = P.normalize_subject(raw, mean_std, truth)
    X, Y, Z = mp.SHAPES[i]
    assert bw[0, 0] == 0 and bw[1, 2] == Z                              # as the reference stores it: end == shape
    assert tuple(vol.shape[1:]) == (bw[1, 0] + 1, bw[1, 1] + 1 - bw[0, 1], Z - bw[0, 2])


def test_add_subject_records_box_origin_and_shape(golden, subjects, mean_std):
    from nas_3d_unet_amd.generator import VolumeSet
    g = golden("preprocess")
    vs = VolumeSet()
    for i, (raw, truth) in enumerate(subjects):
        assert vs.add_subject(raw, truth, mean_std) == i
    for i, (raw, truth) in enumerate(subjects):
        want, want_t, bw = _expected_box(g, i, truth)
        assert vs.box(i) == want.shape[1:]
        assert vs.origins[i] == tuple(bw[0].tolist()) and vs.full_shapes[i] == mp.SHAPES[i]
        assert np.array_equal(vs.volumes[i].cpu().numpy(), want) and np.array_equal(vs.truths[i].cpu().numpy(), want_t)
    j = vs.add(vs.volumes[0], vs.truths[0])                          # add() keeps working next to it: nothing known about its image
    assert vs.origins[j] is None and vs.full_shapes[j] is None and len(vs.origins) == len(vs) == 4


def test_degenerate_modalities_and_float_input_raise(subjects, mean_std):
    from nas_3d_unet_amd import preprocess as P
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.generator import VolumeSet
    raw = subjects[0][0]
    empty = raw.copy()
    empty[2] = 0
    with pytest.raises(N3DError, match="flair has no nonzero voxel"):
        P.normalize_subject(empty, mean_std)
    with pytest.raises(N3DError, match="flair has no nonzero voxel"):
        P.cal_mean_std([empty])
    flat = raw.copy()
    flat[3][flat[3] != 0] = 1234
    with pytest.raises(N3DError, match="t2 has a single nonzero value"):
        P.normalize_subject(flat, mean_std)
    for call in (lambda: P.normalize_subject(raw.astype(np.float32), mean_std), lambda: P.cal_mean_std([raw.astype(np.float32)]),
                 lambda: VolumeSet().add_subject(torch.from_numpy(raw).float().cuda(), None, mean_std)):
        with pytest.raises(N3DError, match="int16"):
            call()


def test_generator_over_add_subject_equals_generator_over_fixture_boxes(golden, subjects, mean_std):
    """end to end: raw scans -> add_subject -> Generator(patch 8) gives the batch the same generator gives over add() of the
    reference-made boxes"""
    from nas_3d_unet_amd.generator import Generator, VolumeSet
    g = golden("preprocess")
    a, b = VolumeSet(), VolumeSet()
    for i in (1, 2):
        raw, truth = subjects[i]
        a.add_subject(raw, truth, mean_std)
        want, want_t, _ = _expected_box(g, i, truth)
        b.add(want, np.ascontiguousarray(want_t))
    batches = []
    for vs in (a, b):
        gen = Generator([0, 1], vs, 8, patch_overlap=None, batch_size=3, labels=[1, 2, 4], permute=True, rng=random.Random(9))
        assert gen.steps_per_epoch >= 1
        batches.append(next(gen.epoch()))
    (xa, ta), (xb, tb) = batches
    assert xa.shape[0] == 3 and float(xa.abs().max()) >= 10 and float(ta.max()) == 1
    assert torch.equal(xa, xb) and torch.equal(ta, tb)


def test_predict_needs_nothing_from_outside_after_add_subject(subjects, mean_std):
    """sp.predict(vs, i, origin=vs.origins[i], full_shape=vs.full_shapes[i]) writes the box's prediction where the box sits in
    the subject's own image (the net of tests/test_gpu_subject_predict.py)"""
    from _util import fill_module
    from nas_3d_unet_amd import searched
    from nas_3d_unet_amd.generator import VolumeSet
    from nas_3d_unet_amd.predict import SubjectPredictor
    gene = searched.Genotype(down=[("down_conv", 0), ("down_dil_conv", 1), ("down_conv", 1), ("conv", 2), ("dil_conv", 2), ("conv", 3)],
                             up=[("conv", 0), ("up_conv", 1), ("up_conv", 1), ("dil_conv", 2), ("conv", 3), ("up_dil_conv", 1)])
    net = searched.SearchedNet(4, 4, 3, 2, 3, True, gene)
    fill_module(net)
    net = net.cuda().eval()
    vs = VolumeSet()
    raw, truth = subjects[1]
    i = vs.add_subject(raw, truth, mean_std)
    sp = SubjectPredictor(net, patch=16, batch=5)
    lab_box, p_box = sp.predict(vs, i, overlap=4, want_probs=True)
    lab, p = sp.predict(vs, i, overlap=4, origin=vs.origins[i], full_shape=vs.full_shapes[i], want_probs=True)
    assert tuple(lab.shape) == mp.SHAPES[1] and tuple(p.shape) == (3,) + mp.SHAPES[1]
    sl = tuple(slice(o, o + b) for o, b in zip(vs.origins[i], vs.box(i)))
    exp = torch.zeros_like(p)
    exp[(slice(None),) + sl] = p_box
    assert torch.equal(p, exp) and torch.equal(lab[sl], lab_box) and int((lab != 0).sum()) == int((lab_box != 0).sum())
    # the labels vanish wherever every raw modality is zero: the skull mask of the normalised box is the raw one
    assert not lab.cpu().numpy()[~np.any(raw != 0, axis=0)].any()
