"""GPU: segmentation metrics on the device (nas_3d_unet_amd.metrics; n3d_seg_regions, n3d_seg_edt, n3d_seg_sample, n3d_seg_order)
against scipy's answers (tests/golden/metrics.npz) and the numpy restatement (tests/_metrics_ref.py).  Flag bytes, counts,
bounding boxes, squared distances and order statistics are integers and compared with ==; the floats are metrics.finish on those
integers on both sides and compared exactly.  No tolerance anywhere.

Shapes (make_golden_metrics): (13, 9, 21) with a (9, 7, 12) box at (2, 1, 5) -- odd sizes, truth addressed through the origin;
(70, 5, 66) -- more than a wave in x and z, several workgroups, three z tiles of the line passes; (3, 130, 4) -- a line longer
than 128.  The distance transform alone also at (260, 3, 9), (2, 300, 3), (2, 3, 300): lines beyond 256, where the line passes
switch to 8 columns per workgroup and a lane of the z pass takes a second round of outputs."""
import numpy as np
import pytest
import torch

import _metrics_ref as R

pytestmark = pytest.mark.gpu

CASES = ("box", "wide", "tall", "faces", "single", "full", "equal", "both_empty", "pred_empty", "truth_empty", "no_et", "two_blobs")


def _case(g, name):
    o = g[name + "/origin"]
    return g[name + "/pred"], g[name + "/truth"], (None if o[0] < 0 else tuple(int(v) for v in o))


@pytest.fixture(scope="module")
def refs(golden):
    """name -> the helper's answer, computed once and left alone"""
    g = golden("metrics")
    assert tuple(g["names"]) == CASES
    return {name: R.score(*_case(g, name)) for name in CASES}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", CASES)
def test_surfaces_and_counts(golden, refs, name):
    from nas_3d_unet_amd import metrics as M
    g = golden("metrics")
    pred, truth, origin = _case(g, name)
    flags, counts = M.surfaces_and_counts(_dev(pred), _dev(truth), origin)
    assert flags.dtype == torch.uint8 and counts.dtype == torch.int64 and tuple(counts.shape) == (3, 3)
    flags, counts = flags.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(flags, g[name + "/flags"]) and np.array_equal(flags, refs[name]["flags"])
    assert np.array_equal(counts, g[name + "/counts"]) and np.array_equal(counts, refs[name]["counts"])


@pytest.mark.parametrize("name", CASES)
def test_score_labels(golden, refs, name):
    from nas_3d_unet_amd import metrics as M
    g = golden("metrics")
    pred, truth, origin = _case(g, name)
    p, t = _dev(pred), _dev(truth)
    rec, nvox = M.score_record(p, t, origin)
    ref = refs[name]
    assert nvox == pred.size and rec.dtype == np.int64 and rec.shape == (M.REC_WORDS,)
    assert np.array_equal(rec[:9].reshape(3, 3), g[name + "/counts"])
    assert np.array_equal(rec[M.REC_BBOX:].view(np.int32).reshape(3, 6), ref["bbox"])
    assert np.array_equal(rec[M.REC_ORDER:M.REC_BBOX].reshape(3, 4), g[name + "/order"])
    assert np.array_equal(rec[M.REC_ORDER:M.REC_BBOX].reshape(3, 4), ref["order"])
    s = M.score_labels(p, t, origin)
    assert R.same_scores(s, ref["scores"])
    for r, reg in enumerate(M.REGIONS):
        for key, want in (("hausdorff95", g[name + "/hd95"][r]), ("hausdorff100", g[name + "/hd100"][r])):
            assert (np.isnan(want) and np.isnan(s[reg][key])) or s[reg][key] == float(want), (reg, key)
    if name == "equal":
        assert all(s[reg]["dice"] == 1.0 and s[reg]["hausdorff95"] == 0.0 for reg in M.REGIONS)
    if name == "both_empty":
        assert all(s[reg]["dice"] == 1.0 and s[reg]["hausdorff95"] == 0.0 and s[reg]["n_surface"] == 0 for reg in M.REGIONS)


def test_score_labels_twice_gives_identical_records(golden):
    """the scratch is reused: a second subject of another shape in between, then the first again"""
    from nas_3d_unet_amd import metrics as M
    g = golden("metrics")
    (p, t, o), (p2, t2, o2) = _case(g, "wide"), _case(g, "box")
    p, t, p2, t2 = _dev(p), _dev(t), _dev(p2), _dev(t2)
    a, _ = M.score_record(p, t, o)
    b, _ = M.score_record(p, t, o)
    other, _ = M.score_record(p2, t2, o2)
    c, _ = M.score_record(p, t, o)
    assert np.array_equal(a, b) and np.array_equal(a, c) and not np.array_equal(a, other)
    assert R.same_scores(M.score_labels(p, t, o), M.score_labels(p, t, o))


def test_sparse_image_larger_than_the_grids():
    """(104, 110, 193): small cubes in opposite corners, so every region's box is the whole image -- more voxels than one sweep of
    the regions launch (256 x 1024 x 8), more tiles per distance pass than workgroups per job (512) and more z rows than the
    sampling launch has waves (2048): every grid-stride loop goes round again.  Few surface voxels, so the brute-force reference
    stays cheap."""
    from nas_3d_unet_amd import metrics as M
    shape = (104, 110, 193)
    pred, truth = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    pred[:3, :3, :3] = 4
    pred[-4:, -2:, -3:] = 4
    pred[50, 60, 100] = 1
    truth[:2, :4, :3] = 4
    truth[-3:, -3:, -5:] = 4
    truth[0, 109, 0] = 4
    truth[103, 0, 192] = 2
    ref = R.score(pred, truth)
    assert all(ref["bbox"][r].tolist() == [0, 0, 0, 103, 109, 192] for r in (0, 2)) and pred.size > 256 * 1024 * 8
    rec, _ = M.score_record(_dev(pred), _dev(truth))
    assert np.array_equal(rec[:9].reshape(3, 3), ref["counts"])
    assert np.array_equal(rec[M.REC_BBOX:].view(np.int32).reshape(3, 6), ref["bbox"])
    assert np.array_equal(rec[M.REC_ORDER:M.REC_BBOX].reshape(3, 4), ref["order"])
    flags, counts = M.surfaces_and_counts(_dev(pred), _dev(truth))
    assert np.array_equal(flags.cpu().numpy(), ref["flags"])
    sparse = np.zeros(shape, np.uint8)
    sparse[3, 100, 7] = sparse[99, 2, 180] = sparse[50, 50, 96] = 1
    assert np.array_equal(M.edt_sq(_dev(sparse)).cpu().numpy(), R.edt_sq(sparse))


def test_sample_histograms(golden):
    """n3d_seg_edt + n3d_seg_sample through the C ABI with boxes given by the caller -- the whole image for WT, the surfaces' own box
    for TC and ET: the histograms hold exactly the fixture's distances, and nothing is counted past hist_len"""
    import ctypes as C
    from nas_3d_unet_amd import _lib, metrics as M
    from nas_3d_unet_amd import kernels as K
    g = golden("metrics")
    pred, truth, origin = _case(g, "wide")
    full = (C.c_int32 * 3)(*pred.shape)
    n = pred.size
    flags, _ = M.surfaces_and_counts(_dev(pred), _dev(truth), origin)
    ref = R.score(pred, truth, origin)
    boxes = np.array([[0, 0, 0] + [s - 1 for s in pred.shape], ref["bbox"][1], ref["bbox"][2]], dtype=np.int32)
    bbox = _dev(boxes)
    dist = torch.empty(6 * n, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    _lib.check(lib.n3d_seg_edt(K.ptr(flags), 6, 3, full, K.ptr(bbox), K.ptr(dist), K.stream_ptr()))
    for hl in (int(max(int(g["wide/d2_%d" % r].max()) for r in range(3))) + 1, 12):
        h = torch.zeros(3 * hl + 8, dtype=torch.int32, device="cuda")
        _lib.check(lib.n3d_seg_sample(K.ptr(flags), full, K.ptr(bbox), K.ptr(dist), K.ptr(h), hl, K.stream_ptr()))
        h = h.cpu().numpy()
        assert not h[3 * hl:].any()
        for r in range(3):
            assert np.array_equal(h[r * hl:(r + 1) * hl], np.bincount(g["wide/d2_%d" % r], minlength=hl)[:hl])


@pytest.mark.parametrize("name", ["edt_box", "edt_wide", "edt_tall"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.bool])
def test_edt_sq_equals_scipy(golden, name, dtype):
    from nas_3d_unet_amd import metrics as M
    g = golden("metrics")
    d = M.edt_sq(_dev(g[name + "/mask"]).to(dtype))
    assert d.dtype == torch.int32
    assert np.array_equal(d.cpu().numpy(), g[name + "/d2"])


@pytest.mark.parametrize("shape", [(260, 3, 9), (2, 300, 3), (2, 3, 300)])
def test_edt_sq_long_lines(shape):
    from nas_3d_unet_amd import metrics as M
    rng = np.random.default_rng(sum(shape))
    mask = (rng.uniform(0, 1, shape) < 0.004).astype(np.uint8)
    mask[tuple(s - 1 for s in shape)] = 1
    assert np.array_equal(M.edt_sq(_dev(mask)).cpu().numpy(), R.edt_sq(mask))


def test_edt_sq_empty_mask_and_limits():
    from nas_3d_unet_amd import metrics as M
    from nas_3d_unet_amd._lib import N3DError
    d = M.edt_sq(torch.zeros((13, 9, 21), dtype=torch.uint8, device="cuda"))
    assert d.dtype == torch.int32 and bool((d == M.INF).all())
    one = torch.zeros((1, 1, 1), dtype=torch.uint8, device="cuda")
    assert int(M.edt_sq(one + 1)[0, 0, 0]) == 0 and int(M.edt_sq(one)[0, 0, 0]) == M.INF
    with pytest.raises(N3DError, match="1025"):
        M.edt_sq(torch.zeros((1025, 1, 2), dtype=torch.uint8, device="cuda"))
    with pytest.raises(N3DError, match="1025"):
        M.score_labels(torch.zeros((2, 1025, 1), dtype=torch.uint8, device="cuda"), torch.zeros((2, 1025, 1), dtype=torch.uint8, device="cuda"))


def test_arguments(golden):
    from nas_3d_unet_amd import metrics as M
    from nas_3d_unet_amd._lib import N3DError
    g = golden("metrics")
    pred, truth, origin = _case(g, "box")
    p, t = _dev(pred), _dev(truth)
    with pytest.raises(N3DError, match="not inside the image"):
        M.score_labels(p, t, (5, 1, 5))
    with pytest.raises(N3DError, match="not inside the image"):
        M.score_labels(p, t)                       # no origin: the box must be the image
    with pytest.raises(N3DError, match="uint8"):
        M.score_labels(p.to(torch.int32), t, origin)
    with pytest.raises(N3DError, match="HIP device"):
        M.score_labels(p, t.cpu(), origin)


class _Stub:
    """a predictor that returns fixture labels"""

    def __init__(self, labels):
        self.labels, self.calls = labels, []

    def predict(self, volumes, index, **kw):
        self.calls.append((index, kw))
        return self.labels[index], None


def test_score_subject_and_set(golden, refs, tmp_path):
    from nas_3d_unet_amd import metrics as M
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.generator import VolumeSet
    g = golden("metrics")
    rng = np.random.default_rng(3)
    vs, labels, names = VolumeSet(), [], ["wide", "box", "two_blobs"]
    for name in names:
        pred, truth, origin = _case(g, name)
        i = vs.add(rng.standard_normal((2,) + truth.shape).astype(np.float32), truth)
        if origin is not None:
            vs.origins[i] = origin                 # set by hand, as add_subject would
            vs.full_shapes[i] = pred.shape
        labels.append(_dev(pred))
    for i, name in enumerate(names):
        assert R.same_scores(M.score_subject(vs, i, labels[i]), refs[name]["scores"])
    stub = _Stub(labels)
    rows = M.score_set(stub, vs, [2, 0, 1], names=["c", "a", "b"], threshold=0.5)
    assert stub.calls == [(2, {"threshold": 0.5}), (0, {"threshold": 0.5}), (1, {"threshold": 0.5})]
    assert [r["Label"] for r in rows] == ["c", "a", "b"]
    for row, name in zip(rows, ["two_blobs", "wide", "box"]):
        assert set(row) == set(M.COLUMNS)
        for reg in M.REGIONS:
            assert row["Dice_" + reg] == refs[name]["scores"][reg]["dice"]
            assert row["Sensitivity_" + reg] == refs[name]["scores"][reg]["sensitivity"]
            assert row["Specificity_" + reg] == refs[name]["scores"][reg]["specificity"]
            assert row["Hausdorff95_" + reg] == refs[name]["scores"][reg]["hausdorff95"]
    assert [r["Label"] for r in M.score_set(stub, vs, [1])] == ["1"]
    M.write_csv(str(tmp_path / "fold.csv"), rows)
    assert len(open(str(tmp_path / "fold.csv")).read().splitlines()) == 1 + 3 + 5
    with pytest.raises(N3DError, match="do not hold"):
        M.score_subject(vs, 1, labels[0])          # the wide image for the boxed subject
    with pytest.raises(N3DError, match="do not hold"):
        M.score_subject(vs, 0, labels[1])
    with pytest.raises(N3DError, match="outside the set"):
        M.score_subject(vs, 3, labels[0])
    bare = VolumeSet()
    bare.add(rng.standard_normal((2, 5, 6, 7)).astype(np.float32))
    with pytest.raises(N3DError, match="no truth"):
        M.score_subject(bare, 0, torch.zeros((5, 6, 7), dtype=torch.uint8, device="cuda"))
