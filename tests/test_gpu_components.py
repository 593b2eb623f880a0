"""GPU: the label clean-up on the device (nas_3d_unet_amd.postprocess; n3d_cc_label, n3d_cc_clean) against scipy's answers
(tests/golden/components.npz) and the numpy restatement (tests/_components_ref.py).  Component ids, cleaned volumes and statistics
are integers and compared with ==.  No tolerance anywhere.

The local phase labels 8 x 8 x 32 tiles (x, y, z) with 256 threads; the launches are capped at 1024 workgroups.  Shapes
(make_golden_components): (13, 9, 21) -- odd sizes, 2 x 2 x 1 tiles with ragged edges; (70, 5, 66) -- 9 x 1 x 3 tiles, the
serpentine crosses an x face at every turn and two z faces per line; (3, 130, 4) -- a line through 17 tiles along y; (40, 40, 3)
-- the spiral's chain of parents runs through 25 tiles; diag -- the face, edge and corner pairs each straddle a tile face
(x 7 | 8, y 7 | 8, z 31 | 32), so the merge phase is what joins or separates them; full (17, 9, 40) -- 3 x 2 x 2 tiles, one
component, the aggregated size count; checker (10, 9, 35) -- 1575 components at 6, one at 18 / 26.  (104, 110, 193) has 1274 tiles
and 8625 workgroups' worth of voxels -- more than twice what four voxels per thread cover in one sweep: every grid-stride loop goes
round again.  In a tile every z row is half a wave whose foreground runs come from one ballot: box and checker hold runs of
every length and start, full and spiral whole-row runs, wide runs that cross z faces."""
import numpy as np
import pytest
import torch

import _components_ref as R

pytestmark = pytest.mark.gpu

CASES = ("box", "wide", "tall", "spiral", "diag", "wrap", "full", "checker", "empty", "single", "tie", "et_rule")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rules(g):
    return [dict(connectivity=int(c), min_voxels=int(mv), keep_largest=bool(kl), et_min_voxels=int(em)) for c, mv, kl, em in g["rules"]]


@pytest.fixture(scope="module")
def refs(golden):
    """name -> the helper's ids per connectivity and (volume, statistics) per rule set, computed once and left alone"""
    g = golden("components")
    assert tuple(g["names"]) == CASES
    out = {}
    for name in CASES:
        labels = g[name + "/labels"]
        out[name] = ({c: R.label(labels, c) for c in R.CONNECTIVITIES}, [R.clean(labels, **r) for r in _rules(g)])
    return out


@pytest.mark.parametrize("name", CASES)
def test_label_components(golden, refs, name):
    from nas_3d_unet_amd import postprocess as P
    g = golden("components")
    labels = g[name + "/labels"]
    for dtype in (torch.uint8, torch.bool):
        mask = _dev(labels) if dtype == torch.uint8 else _dev(labels != 0)
        for c in R.CONNECTIVITIES:
            ids = P.label_components(mask, c)
            assert ids.dtype == torch.int32 and tuple(ids.shape) == labels.shape
            ids = ids.cpu().numpy()
            assert np.array_equal(ids, g["%s/ids_%d" % (name, c)]), (name, c)
            assert np.array_equal(ids, refs[name][0][c]), (name, c)
    assert np.array_equal(P.label_components(_dev(labels)).cpu().numpy(), g[name + "/ids_26"])     # the default connectivity


@pytest.mark.parametrize("name", CASES)
def test_clean_labels(golden, refs, name):
    from nas_3d_unet_amd import postprocess as P
    g = golden("components")
    labels = g[name + "/labels"]
    dev = _dev(labels)
    for k, r in enumerate(_rules(g)):
        out, stats = P.clean_labels(dev, return_stats=True, **r)
        assert out.dtype == torch.uint8 and tuple(out.shape) == labels.shape and out.data_ptr() != dev.data_ptr()
        out = out.cpu().numpy()
        assert np.array_equal(out, g["%s/clean_%d" % (name, k)]), (name, k)
        assert np.array_equal(out, refs[name][1][k][0]), (name, k)
        assert stats == refs[name][1][k][1], (name, k)
        assert np.array_equal(R.stats_row(stats), g["%s/stats_%d" % (name, k)]), (name, k)
        assert np.array_equal(P.clean_labels(dev, **r).cpu().numpy(), out)         # without the statistics: the volume alone
    assert np.array_equal(dev.cpu().numpy(), labels)                               # the input is untouched


def test_defaults_return_the_input_and_count(golden):
    from nas_3d_unet_amd import postprocess as P
    g = golden("components")
    labels = g["box/labels"]
    out, stats = P.clean_labels(_dev(labels), return_stats=True)
    assert np.array_equal(out.cpu().numpy(), labels)
    assert stats["n_components"] == stats["n_kept"] == 3 and stats["voxels_in"] == stats["voxels_kept"] == int((labels != 0).sum())
    assert stats["et_in"] == stats["et_kept"] == int((labels == 4).sum()) and stats["et_relabelled"] is False


def test_clean_labels_twice_gives_identical_results(golden):
    """the scratch is reused: a second subject of another shape in between, then the first again"""
    from nas_3d_unet_amd import postprocess as P
    g = golden("components")
    a, b = _dev(g["wide/labels"]), _dev(g["box/labels"])
    rules = dict(connectivity=6, min_voxels=3, et_min_voxels=10 ** 6)
    v1, r1 = P.clean_record(a, **rules)
    v2, r2 = P.clean_record(a, **rules)
    vo, ro = P.clean_record(b, **rules)
    v3, r3 = P.clean_record(a, **rules)
    assert torch.equal(v1, v2) and torch.equal(v1, v3) and torch.equal(r1, r2) and torch.equal(r1, r3) and not torch.equal(r1, ro)
    assert r1.data_ptr() != r2.data_ptr()                  # a record of its own per call: the next call does not overwrite it
    assert len(P._workspaces) == 1                         # one shape at a time
    want, stats = R.clean(g["wide/labels"], **rules)
    assert np.array_equal(v3.cpu().numpy(), want) and P.stats_of(r3) == stats
    assert np.array_equal(vo.cpu().numpy(), R.clean(g["box/labels"], **rules)[0])


@pytest.mark.parametrize("name", ["box", "wide", "spiral", "full", "checker", "et_rule"])
def test_phases_and_the_global_only_variant(golden, name):
    """n3d_cc_phases: the pipeline in two pieces (labelling, then the rules) on the shared scratch, and the variant without the LDS
    tile phase, give n3d_cc_clean's volume and record"""
    from nas_3d_unet_amd import postprocess as P
    g = golden("components")
    dev = _dev(g[name + "/labels"])
    for k in (5, 10):
        r = _rules(g)[k]
        want = g["%s/clean_%d" % (name, k)]
        out = torch.full_like(dev, 255)
        P.run_phases(dev, out, 0, 2, **r)
        rec = P.run_phases(dev, out, 3, 5, **r)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(rec.cpu().numpy()[:9], g["%s/stats_%d" % (name, k)])
        out.fill_(255)
        rec = P.run_phases(dev, out, variant=P.GLOBAL_ONLY, **r)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(rec.cpu().numpy()[:9], g["%s/stats_%d" % (name, k)])
    from nas_3d_unet_amd._lib import N3DError
    with pytest.raises(N3DError, match="phases 2 .. 1"):
        P.run_phases(dev, out, 2, 1)
    with pytest.raises(N3DError, match="phases 0 .. 6"):
        P.run_phases(dev, out, 0, 6)
    with pytest.raises(N3DError, match="variant 2"):
        P.run_phases(dev, out, variant=2)


def test_sparse_image_larger_than_the_grids():
    """(104, 110, 193): small cubes in opposite corners, a thin rod along the diagonal between them (each step a corner neighbour:
    one component at 26, single voxels at 6 and 18) -- more tiles than the local launch has workgroups and more voxels than one
    sweep of the other launches."""
    from nas_3d_unet_amd import postprocess as P
    shape = (104, 110, 193)
    labels = np.zeros(shape, np.uint8)
    labels[:3, :3, :3] = 2
    labels[-4:, -2:, -3:] = 4
    for t in range(5, 100):
        labels[t, t + 3, t + 60] = 1 if t % 7 else 4
    labels[50, 5, 190] = 4
    assert labels.size > 1024 * 256 and 13 * 14 * 7 > 1024
    dev = _dev(labels)
    assert np.array_equal(P.label_components(dev, 26).cpu().numpy(), R.label(labels, 26))
    for rules in (dict(connectivity=26, min_voxels=2, et_min_voxels=40), dict(connectivity=18, keep_largest=True)):
        out, stats = P.clean_labels(dev, return_stats=True, **rules)
        want, ref = R.clean(labels, **rules)
        assert np.array_equal(out.cpu().numpy(), want) and stats == ref, rules
    assert ref["largest_size"] == 27 and ref["largest_id"] == 0 and ref["n_components"] == 3 + 95


class _Stub:
    """a predictor that returns fixture labels and something more"""

    def __init__(self, labels):
        self.labels, self.calls = labels, []

    def predict(self, volumes, index, **kw):
        self.calls.append((index, kw))
        return self.labels[index], "probs-%d" % index


def test_cleaned_predictor_and_score_set(golden):
    from nas_3d_unet_amd import metrics as M, postprocess as P
    from nas_3d_unet_amd.generator import VolumeSet
    g = golden("components")
    rng = np.random.default_rng(4)
    names = ["et_rule", "box", "tie"]
    rules = dict(connectivity=26, min_voxels=10, et_min_voxels=8)
    vs, labels = VolumeSet(), []
    for name in names:
        pred = g[name + "/labels"]
        truth = np.roll(pred, 1, axis=2)                    # something to score against
        vs.add(rng.standard_normal((2,) + pred.shape).astype(np.float32), truth)
        labels.append(_dev(pred))
    stub = _Stub(labels)
    cp = P.CleanedPredictor(stub, **rules)
    got = cp.predict(vs, 0, threshold=0.5)
    assert stub.calls == [(0, {"threshold": 0.5})] and got[1:] == ("probs-0",) and isinstance(got, tuple)
    want, stats = R.clean(g["et_rule/labels"], **rules)
    assert np.array_equal(got[0].cpu().numpy(), want) and not np.array_equal(want, g["et_rule/labels"])
    assert cp.last_stats.is_cuda and cp.last_stats.dtype == torch.int64 and cp.stats() == stats and stats["et_relabelled"] is True
    assert np.array_equal(labels[0].cpu().numpy(), g["et_rule/labels"])      # the predictor's own volume is untouched
    rows = M.score_set(cp, vs, [2, 0, 1], names=["c", "a", "b"])
    assert [r["Label"] for r in rows] == ["c", "a", "b"] and cp.stats() == R.clean(g["box/labels"], **rules)[1]
    for row, i in zip(rows, [2, 0, 1]):
        cleaned = _dev(R.clean(g[names[i] + "/labels"], **rules)[0])
        assert _same_row(row, M.row_of(row["Label"], M.score_labels(cleaned, vs.truths[i]))), names[i]
    # the rules move the scores: without them the rows differ for the subject they change
    raw = M.score_set(stub, vs, [0])
    assert not _same_row(raw[0], dict(rows[1], Label="0"))


def _same_row(a, b):
    return set(a) == set(b) and all(a[k] == b[k] or (isinstance(a[k], float) and np.isnan(a[k]) and np.isnan(b[k])) for k in a)


def test_arguments_on_the_device():
    from nas_3d_unet_amd import postprocess as P
    from nas_3d_unet_amd._lib import N3DError
    vol = torch.zeros((4, 5, 6), dtype=torch.uint8, device="cuda")
    with pytest.raises(N3DError, match="uint8 volume"):
        P.clean_labels(vol.to(torch.int32))
    with pytest.raises(N3DError, match="is empty"):
        P.clean_labels(vol[:0])
    with pytest.raises(N3DError, match="is empty"):
        P.label_components(vol[:, :0])
    with pytest.raises(N3DError, match=r"X \* Y \* Z < 2\^31"):
        P.clean_labels(torch.zeros(1, dtype=torch.uint8, device="cuda").expand(2048, 1024, 1024))
    # a view that is not contiguous is labelled as the volume it shows
    big = torch.zeros((4, 5, 12), dtype=torch.uint8, device="cuda")
    big[1, 2, 0] = big[1, 2, 2] = big[2, 3, 4] = 2
    view = big[:, :, ::2]
    assert np.array_equal(P.label_components(view, 6).cpu().numpy(), R.label(view.cpu().numpy(), 6))
    one = torch.ones((1, 1, 1), dtype=torch.uint8, device="cuda")
    assert int(P.label_components(one)[0, 0, 0]) == 0 and int(P.label_components(one * 0)[0, 0, 0]) == -1
