"""GPU: the lesion-wise metrics on the device (nas_3d_unet_amd.metrics: dilate_mask, lesion_record, score_lesions; n3d_lw_dilate,
n3d_lw_score) against scipy's answers (tests/golden/lesion.npz) and the numpy restatement (tests/_lesion_ref.py).  Every device
result is an integer and compared with ==; the folded floats are finish_lesions' of those integers and compared with == too.  No
tolerance anywhere.

The dilation works on 8 x 8 x 32 tiles (x, y, z) with a halo of d in LDS, the component labelling on the same tiles; the streaming
launches have at most 1024 workgroups of 256 threads, the tile walk at most 1024 workgroups.  Shapes (make_golden_lesion): apart
from cap64 none has an axis that is a multiple of its tile edge; gaps (12, 11, 45) -- the lesion line crosses the tile face z = 31 | 32 and the
halo carries the dilation over it; diagonal (21, 19, 13) -- the pair's dilations meet at a corner across the tile faces x 7 | 8
and y 7 | 8, and A's dilation is clipped at z = 0; box (13, 9, 21) -- truth addressed through an origin, dilation clipped at the
image's x and y faces; cap64 (40, 40, 24) -- 5 x 5 x 1 tiles, every lesion row of the record in use."""
import numpy as np
import pytest
import torch

import _lesion_ref as R
import _metrics_ref as MR
from make_golden_lesion import BOX_ORIGIN, EXTRA_DILATIONS, FOLDS, cap_case

pytestmark = pytest.mark.gpu

CASES = ("gaps", "diagonal", "bridge", "rim", "fps", "threshold", "box", "nested", "both_empty", "pred_empty", "truth_empty", "cap64")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _origin(g, name):
    o = tuple(int(v) for v in g[name + "/origin"])
    return None if o[0] < 0 else o


@pytest.fixture(scope="module")
def refs(golden):
    """name -> the helper's record at the default dilation, computed once and left alone"""
    g = golden("lesion")
    assert tuple(g["names"]) == CASES
    return {name: R.record(g[name + "/pred"], g[name + "/truth"], _origin(g, name)) for name in CASES}


@pytest.mark.parametrize("name", CASES)
def test_dilate_mask(golden, name):
    from nas_3d_unet_amd import metrics as M
    g = golden("lesion")
    wt = MR.embed(g[name + "/truth"], g[name + "/pred"].shape, _origin(g, name))       # labels {0, 1, 2, 4}: any nonzero byte is set
    for mask in (_dev(wt), _dev(wt != 0)):
        for d in range(6):
            out = M.dilate_mask(mask, d)
            assert out.dtype == torch.uint8 and tuple(out.shape) == wt.shape and out.data_ptr() != mask.data_ptr()
            assert np.array_equal(out.cpu().numpy(), g[name + "/dilated"][d]), (name, d)
    assert np.array_equal(M.dilate_mask(_dev(wt)).cpu().numpy(), g[name + "/dilated"][3])          # the default


@pytest.mark.parametrize("name", CASES)
def test_lesion_record(golden, refs, name):
    from nas_3d_unet_amd import metrics as M
    g = golden("lesion")
    pred, truth, origin = _dev(g[name + "/pred"]), _dev(g[name + "/truth"]), _origin(g, name)
    rec, voxels = M.lesion_record(pred, truth, origin)
    assert rec.dtype == np.int64 and rec.shape == (M.LW_REC_WORDS,) and voxels == g[name + "/pred"].size
    assert np.array_equal(rec, g[name + "/record"]), (name, np.flatnonzero(rec != g[name + "/record"])[:20])
    assert np.array_equal(rec, refs[name]), name
    for d in EXTRA_DILATIONS.get(name, ()):
        assert np.array_equal(M.lesion_record(pred, truth, origin, dilation=d)[0], g["%s/record_d%d" % (name, d)]), (name, d)
    assert np.array_equal(pred.cpu().numpy(), g[name + "/pred"]) and np.array_equal(truth.cpu().numpy(), g[name + "/truth"])


@pytest.mark.parametrize("name", CASES)
def test_score_lesions(golden, name):
    from nas_3d_unet_amd import metrics as M
    g = golden("lesion")
    pred, truth, origin = _dev(g[name + "/pred"]), _dev(g[name + "/truth"]), _origin(g, name)
    for i, (mv, pen) in enumerate(FOLDS):
        s = M.score_lesions(pred, truth, origin, min_lesion_voxels=mv, penalty_hd95=pen)
        assert R.folded(s).tobytes() == g["%s/folded_%d" % (name, i)].tobytes(), (name, mv, pen)
    assert R.folded(M.score_lesions(pred, truth, origin)).tobytes() == g[name + "/folded_0"].tobytes()


def test_cap64_ids_ascend_and_cap65_overflows(golden):
    from nas_3d_unet_amd import metrics as M
    from nas_3d_unet_amd._lib import N3DError
    g = golden("lesion")
    rec = M.lesion_record(_dev(g["cap64/pred"]), _dev(g["cap64/truth"]))[0].reshape(3, -1)
    for r in range(3):
        ids = rec[r, M.LW_HEADER_WORDS:].reshape(64, 9)[:, 0]
        assert rec[r, 0] == 64 and rec[r, 4] == 0 and (np.diff(ids) > 0).all()
    pred, truth = cap_case(65)
    with pytest.raises(N3DError, match="N3D_LW_MAX_LESIONS") as e:
        M.score_lesions(_dev(pred), _dev(truth))
    assert "WT" in str(e.value)
    rec = M.lesion_record(_dev(pred), _dev(truth))[0]
    assert np.array_equal(rec, R.record(pred, truth))                       # n_lesions = 65, the overflow bit and nothing else
    assert rec.reshape(3, -1)[:, 0].tolist() == [65] * 3 and rec.reshape(3, -1)[:, 4].tolist() == [1] * 3 and np.count_nonzero(rec) == 6
    # a normal case right after it, another shape and the same
    assert np.array_equal(M.lesion_record(_dev(g["fps/pred"]), _dev(g["fps/truth"]))[0], g["fps/record"])
    assert np.array_equal(M.lesion_record(_dev(g["cap64/pred"]), _dev(g["cap64/truth"]))[0], g["cap64/record"])


def test_surface_cap_overflows_and_the_next_subject_is_right(golden):
    """(130, 64, 64): the prediction is a checkerboard, one 26-connected component of 266240 voxels, every one of them on the
    surface, that touches the truth's one lesion: more entries than N3D_LW_MAX_SURFACE = 262144.  The counts are still there."""
    from nas_3d_unet_amd import metrics as M
    from nas_3d_unet_amd._lib import N3DError
    shape = (130, 64, 64)
    pred = np.where(np.indices(shape).sum(axis=0) % 2 == 0, 2, 0).astype(np.uint8)
    truth = np.zeros(shape, np.uint8)
    truth[60:64, 30:34, 30:34] = 2
    assert (pred != 0).sum() == 266240 > M.LW_MAX_SURFACE
    p, t = _dev(pred), _dev(truth)
    with pytest.raises(N3DError, match="N3D_LW_MAX_SURFACE") as e:
        M.score_lesions(p, t)
    assert "WT" in str(e.value) and "prediction" in str(e.value)
    rec = M.lesion_record(p, t)[0].reshape(3, -1)
    assert rec[0, :5].tolist() == [1, 1, 0, 0, 4] and rec[0, M.LW_HEADER_WORDS:][:9].tolist() == [rec[0, 8], 64, 32, 266240, 1, 0, 0, 0, 0]
    assert not rec[1:].any()
    g = golden("lesion")
    assert np.array_equal(M.lesion_record(_dev(g["gaps/pred"]), _dev(g["gaps/truth"]))[0], g["gaps/record"])


def test_the_same_record_twice_and_after_another_shape(golden):
    """the scratch is reused: a second subject of another shape in between, then the first again"""
    from nas_3d_unet_amd import metrics as M
    g = golden("lesion")
    a, b = (_dev(g["gaps/pred"]), _dev(g["gaps/truth"])), (_dev(g["nested/pred"]), _dev(g["nested/truth"]))
    r1, r2 = M.lesion_record(*a)[0], M.lesion_record(*a)[0]
    ro = M.lesion_record(*b)[0]
    r3 = M.lesion_record(*a)[0]
    assert np.array_equal(r1, r2) and np.array_equal(r1, r3) and np.array_equal(r1, g["gaps/record"]) and np.array_equal(ro, g["nested/record"])
    assert len(M._lesion_workspaces) == 1                   # one shape at a time
    # the phases in two pieces on the shared scratch give the same record
    rec = M.lesion_phases(*a, first=0, last=12)
    M.lesion_phases(*a, first=13, last=M.LW_PHASES - 1, rec=rec)
    assert np.array_equal(rec.cpu().numpy(), r1)


def test_sparse_image_larger_than_the_grids():
    """(104, 110, 193), as the component labelling's test: 13 x 14 x 7 = 1274 tiles -- more than the 1024 workgroups of the
    dilation's tile walk -- and 2.2 M voxels -- more than eight sweeps of the streaming launches' 1024 x 256 threads (region bits,
    select, roots, match, components, surface lists).  The distance launch's 1024 x 256 threads are the lists' capacity, so its
    sweep cannot be exceeded; the order launch has a workgroup per lesion row.  Small cubes in opposite corners, the second truth
    cube's dilation clipped by three image faces; a missed voxel and a stray one in the middle."""
    from nas_3d_unet_amd import metrics as M
    shape = (104, 110, 193)
    truth, pred = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    truth[:3, :3, :3] = 2
    truth[-4:, -2:, -3:] = 4
    truth[50, 50, 100] = 1
    pred[1:4, :3, :3] = 2
    pred[-4:, -2:, -5:-2] = 4
    pred[60, 70, 90] = 1
    assert pred.size > 8 * 1024 * 256 and 13 * 14 * 7 > 1024
    want = R.record(pred, truth)
    rec = M.lesion_record(_dev(pred), _dev(truth))[0]
    assert np.array_equal(rec, want)
    w = want.reshape(3, -1)
    assert w[:, 0].tolist() == [3, 2, 1] and w[:, 2].tolist() == [1, 1, 0] and w[0, M.LW_HEADER_WORDS] == 0
    wt = truth != 0
    assert np.array_equal(M.dilate_mask(_dev(wt)).cpu().numpy() != 0, R.dilate(wt, 3))


class _Stub:
    """a predictor that returns stored labels: no net is run"""

    def __init__(self, labels):
        self.labels = labels

    def predict(self, volumes, index, **kw):
        return self.labels[index], None


def _same(a, b):
    return a == b or (isinstance(a, float) and np.isnan(a) and np.isnan(b))


def test_score_set_lesionwise(golden, tmp_path):
    from nas_3d_unet_amd import metrics as M
    from nas_3d_unet_amd.generator import VolumeSet
    g = golden("lesion")
    rng = np.random.default_rng(4)
    names = ["gaps", "box", "fps"]
    vs, labels = VolumeSet(), []
    for name in names:
        truth = g[name + "/truth"]
        i = vs.add(rng.standard_normal((2,) + truth.shape).astype(np.float32), truth)
        if name == "box":
            vs.origins[i] = BOX_ORIGIN
        labels.append(_dev(g[name + "/pred"]))
    stub = _Stub(labels)
    plain = M.score_set(stub, vs, [2, 0, 1], names=["c", "a", "b"])
    rows = M.score_set(stub, vs, [2, 0, 1], names=["c", "a", "b"], lesionwise=True)
    rows5 = M.score_set(stub, vs, [2, 0, 1], names=["c", "a", "b"], lesionwise=True, dilation=3, min_lesion_voxels=0, penalty_hd95=100.0)
    for p, r, r5, i in zip(plain, rows, rows5, [2, 0, 1]):
        assert set(p) == set(M.COLUMNS) and set(r) == set(M.COLUMNS + M.LESION_COLUMNS) == set(r5)
        assert all(_same(p[c], r[c]) and _same(p[c], r5[c]) for c in M.COLUMNS)
        for k, fold in ((r, 0), (r5, 2)):
            want = g["%s/folded_%d" % (names[i], fold)]
            for j, reg in enumerate(M.REGIONS):
                assert k["LesionWise_Dice_" + reg] == want[j, 0] and k["LesionWise_Hausdorff95_" + reg] == want[j, 1], (names[i], reg)
    one = M.score_subject(vs, 1, labels[1], lesionwise=True)
    assert set(one) == set(M.REGIONS) | set(M.LESION_COLUMNS) and one["LesionWise_Dice_WT"] == g["box/folded_0"][0, 0]
    assert set(M.score_subject(vs, 1, labels[1])) == set(M.REGIONS)
    M.write_csv(tmp_path / "plain.csv", plain)
    M.write_csv(tmp_path / "rows.csv", rows)
    assert (tmp_path / "plain.csv").read_bytes() == (tmp_path / "rows.csv").read_bytes()
    M.write_csv(tmp_path / "lesion.csv", rows, M.COLUMNS + M.LESION_COLUMNS)
    assert (tmp_path / "lesion.csv").read_text().splitlines()[0].endswith(",".join(M.LESION_COLUMNS))


def test_arguments_on_the_device():
    from nas_3d_unet_amd import metrics as M
    from nas_3d_unet_amd._lib import N3DError
    vol = torch.zeros((4, 5, 6), dtype=torch.uint8, device="cuda")
    with pytest.raises(N3DError, match="HIP device"):
        M.lesion_record(vol.cpu(), vol)
    with pytest.raises(N3DError, match="uint8"):
        M.lesion_record(vol.to(torch.int32), vol)
    with pytest.raises(N3DError, match="uint8 or bool"):
        M.dilate_mask(vol.to(torch.float32))
    for d in (-1, 6, 2.0, True):
        with pytest.raises(N3DError, match="dilation"):
            M.lesion_record(vol, vol, dilation=d)
        with pytest.raises(N3DError, match="dilation"):
            M.dilate_mask(vol, d)
    with pytest.raises(N3DError, match="min_lesion_voxels"):
        M.score_lesions(vol, vol, min_lesion_voxels=-1)
    with pytest.raises(N3DError, match="not inside the image"):
        M.lesion_record(vol, vol[:2], origin=(3, 0, 0))
    with pytest.raises(N3DError, match="axes up to 1024"):
        M.lesion_record(torch.zeros((1, 1, 1025), dtype=torch.uint8, device="cuda"), torch.zeros((1, 1, 1025), dtype=torch.uint8, device="cuda"))
    with pytest.raises(N3DError, match="lesionwise=True"):
        M.score_subject(None, 0, vol, dilation=2)
    # a view that is not contiguous is scored as the volume it shows; a single voxel is its own lesion and match
    big = torch.zeros((4, 5, 12), dtype=torch.uint8, device="cuda")
    big[1, 2, 4] = 4
    s = M.score_lesions(big[:, :, ::2], big[:, :, ::2], min_lesion_voxels=0)
    assert all(s[r]["lesionwise_dice"] == 1.0 and s[r]["lesionwise_hausdorff95"] == 0.0 and s[r]["n_lesions"] == 1 for r in M.REGIONS)
    assert int(M.dilate_mask(big[:, :, ::2], 1).sum()) == 19
