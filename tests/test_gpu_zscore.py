"""GPU: the ZScore normalisation scheme (preprocess.ZScore; n3d_brain_hist, n3d_brain_robust, n3d_brain_zscore) against numpy:
the histogram against np.bincount, the per-modality record and the normalised box against tests/_zscore_ref.py, which restates the
rule of include/n3d.h operation by operation (tests/test_zscore_ref_host.py pins it to np.percentile / mean / std).  Everything is
compared exactly: integers with ==, bounds, mean, std and the stored fp32 boxes bit for bit.

Shapes: the three preprocessing fixture subjects (make_golden_preprocess.SHAPES: a head and a tail, 2-byte-aligned modality
bases, several workgroups, negative counts, a brain that touches two faces) and small hand-made volumes for the cases the
fixtures do not reach (counts on both sides of the LDS window, one dominant count, n = 2, ties, all-negative counts, a count
equal to the mean)."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import _preprocess_ref as pr
import _zscore_ref as R
import make_golden_preprocess as mp

pytestmark = pytest.mark.gpu

PAIRS = [(0.5, 99.5), (0, 100), (2, 98), (25, 75)]
BIG = (40, 36, 31)


@pytest.fixture(scope="module")
def subjects():
    return mp.preprocess_subjects()


@pytest.fixture(scope="module")
def mean_std(golden):
    g = golden("preprocess")
    return {"%s_%s" % (m, k): np.float64(g["dict"][c, j]) for c, m in enumerate(mp.MODS) for j, k in enumerate(("mean", "std"))}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32).tobytes()


# ---- n3d_brain_hist

def _hist(raw, offset=0, scan=True):
    """the histogram of raw (Cm, X, Y, Z) int16 placed `offset` voxels into an allocation; scan=False leaves rec as the caller
    initialises it (no minimum known: every voxel takes the global path)"""
    from nas_3d_unet_amd import _lib, preprocess as P
    from nas_3d_unet_amd import kernels as K
    lib = _lib.load()
    Cm, X, Y, Z = raw.shape
    buf = torch.zeros(raw.size + 16, dtype=torch.int16, device="cuda")
    buf[offset:offset + raw.size] = torch.from_numpy(np.ascontiguousarray(raw)).cuda().reshape(-1)
    r = buf[offset:offset + raw.size]
    rec = P._records(1, Cm, "cuda")[0]
    if scan:
        totals = torch.zeros((Cm, 2), dtype=torch.int64, device="cuda")
        _lib.check(lib.n3d_brain_scan(K.ptr(r), Cm, X, Y, Z, K.ptr(totals), K.ptr(rec), K.stream_ptr()))
    hist = torch.full((Cm, P.HIST_BINS), 77, dtype=torch.int32, device="cuda")      # the entry point zeroes it
    _lib.check(lib.n3d_brain_hist(K.ptr(r), Cm, X, Y, Z, K.ptr(rec), K.ptr(hist), K.stream_ptr()))
    return hist.cpu().numpy()


def _assert_hist(raw, **kw):
    got = _hist(raw, **kw)
    for c, m in enumerate(raw):
        want = np.bincount(m[m != 0].astype(np.int64) + 32768, minlength=65536)
        assert np.array_equal(got[c], want), "modality %d: %d bins differ" % (c, int((got[c] != want).sum()))


def _brain(shape, seed):
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return sum(((g[a] - shape[a] / 2) / (0.42 * shape[a])) ** 2 for a in range(3)) <= 1.0, rng


@pytest.mark.parametrize("i", range(len(mp.SHAPES)))
@pytest.mark.parametrize("offset", [0, 3])
def test_histogram_equals_bincount(subjects, i, offset):
    _assert_hist(subjects[i][0], offset=offset)


def test_histogram_of_counts_spread_over_all_of_int16():
    """most voxels lie outside the LDS window: the global path, every bin of the table in use, -32768 and 32767 among them"""
    brain, rng = _brain(BIG, 11)
    val = rng.integers(-32768, 32768, BIG)
    val.reshape(-1)[:2] = (-32768, 32767)
    raw = np.where(brain | (np.arange(val.size).reshape(BIG) < 2), val, 0).astype(np.int16)[None]
    assert raw.min() == -32768 and raw.max() == 32767
    _assert_hist(raw)


def test_histogram_on_both_sides_of_the_window():
    """counts min, min + W - 1 (the last LDS bin) and min + W (the first global one) exactly, and their neighbours"""
    from nas_3d_unet_amd import _lib
    W = int(_lib.load().n3d_brain_hist_window())
    assert 0 < W < 65536 and 2 * 4 * W <= 160 * 1024          # two workgroups' windows fit in a CU's LDS
    brain, rng = _brain(BIG, 12)
    for mn in (-100, 1, 32767 - W - 1):
        pick = np.array([mn, mn + W - 2, mn + W - 1, mn + W, mn + W + 1])
        pick = pick[pick != 0]
        raw = np.where(brain, rng.choice(pick, BIG), 0).astype(np.int16)[None]
        raw[0, 20, 18, 15] = mn
        assert raw.min() == min(mn, 0) and raw.max() == mn + W + 1
        _assert_hist(raw)


def test_histogram_with_one_dominant_count():
    """90 % of the brain voxels share one count: every lane of a wave adds to one LDS bin"""
    brain, rng = _brain(BIG, 13)
    val = np.where(rng.uniform(0, 1, (2,) + BIG) < 0.9, 1234, rng.integers(1, 4001, (2,) + BIG))
    raw = np.where(brain[None], val, 0).astype(np.int16)
    _assert_hist(raw)
    _assert_hist(raw, scan=False)      # without a minimum in rec the same counts arrive through global atomics


# ---- n3d_brain_robust through subject_stats

def _assert_stats(raw, pair):
    from nas_3d_unet_amd import metrics as M
    from nas_3d_unet_amd import preprocess as P
    got = P.subject_stats(raw, P.ZScore(*pair))
    again = P.subject_stats(torch.from_numpy(raw).cuda(), P.ZScore(*pair))
    want = R.subject_stats(raw, *pair)
    assert len(got) == len(want) == raw.shape[0]
    for c, (g, w) in enumerate(zip(got, want)):
        print("modality %d %s: n %d order %s bounds %.17g %.17g clipped %d %d mean %.17g std %.17g (expected %.17g %.17g)" % (
            c, pair, g.count, g.order, g.lower_bound, g.upper_bound, g.n_below, g.n_above, g.mean, g.std, w.mean, w.std))
        assert (g.count, g.order, g.n_below, g.n_above) == (w.count, w.order, w.n_below, w.n_above)
        assert all(type(v) is int for v in (g.count, g.n_below, g.n_above) + g.order)
        for name in ("lower_bound", "upper_bound", "mean", "std"):
            a, b = getattr(g, name), getattr(w, name)
            assert type(a) is np.float64 and a.tobytes() == b.tobytes(), "%s of modality %d: %.17g, expected %.17g" % (name, c, a, b)
        assert again[c] == g and all(getattr(again[c], n).tobytes() == getattr(g, n).tobytes() for n in ("mean", "std"))
        # the bounds follow from the record's integers by the package's own host statement of rule 1
        assert M.percentile_from_order(g.count, pair[0], *g.order[:2]) == g.lower_bound
        assert M.percentile_from_order(g.count, pair[1], *g.order[2:]) == g.upper_bound


@pytest.mark.parametrize("i", range(len(mp.SHAPES)))
@pytest.mark.parametrize("pair", PAIRS)
def test_subject_stats_equal_the_helper(subjects, i, pair):
    _assert_stats(subjects[i][0], pair)


def _special_subject():
    """(4, 5, 6, 7): two voxels {5, 9}; heavy ties (7 x 150, 9 x 20, 8 x 3); every count negative; {1, 2, 3} x 4"""
    rng = np.random.default_rng(21)
    raw = np.zeros((4, 5 * 6 * 7), np.int16)
    raw[0, [17, 140]] = (5, 9)
    raw[1, rng.permutation(210)[:173]] = np.repeat([7, 9, 8], [150, 20, 3])
    raw[2, rng.permutation(210)[:120]] = -rng.integers(1, 3001, 120)
    raw[3, rng.permutation(210)[:12]] = np.tile([1, 2, 3], 4)
    return raw.reshape(4, 5, 6, 7)


@pytest.mark.parametrize("pair", [(0.5, 99.5), (0, 100), (25, 75), (40, 100)])
def test_subject_stats_on_small_and_tied_modalities(pair):
    """n = 2; upper = 100 (k + 1 clamps to n - 1); a[k] and a[k + 1] in one bin; all counts negative"""
    _assert_stats(_special_subject(), pair)


# ---- normalize_subject(scheme=ZScore)

@pytest.mark.parametrize("i", range(len(mp.SHAPES)))
@pytest.mark.parametrize("pair", [(0.5, 99.5), (0, 100), (25, 75)])
def test_zscore_box_is_bit_identical(subjects, mean_std, i, pair):
    from nas_3d_unet_amd import preprocess as P
    raw, truth = subjects[i]
    want, want_t, bw = R.normalize_subject(raw, truth, *pair)
    vol, t, brain_width = P.normalize_subject(raw, None, truth, scheme=P.ZScore(*pair))
    assert vol.dtype == torch.float32 and vol.is_contiguous() and t.dtype == torch.uint8
    assert brain_width.shape == (2, 3) and brain_width.dtype == np.int64 and np.array_equal(brain_width, bw)
    got = vol.cpu().numpy()
    assert got.shape == want.shape and _bits(got) == _bits(want)
    assert np.array_equal(t.cpu().numpy(), want_t)
    # the same box as the reference scheme's, and nonzero exactly where raw is
    ref_vol, ref_t, ref_bw = P.normalize_subject(raw, mean_std, truth)
    assert np.array_equal(ref_bw, brain_width) and ref_vol.shape == vol.shape and torch.equal(ref_t, t)
    sl = (slice(None),) + pr.box_slices(bw, raw.shape[1:])
    assert np.array_equal(got != 0, raw[sl] != 0) and torch.equal(vol != 0, ref_vol != 0)
    # without truth, raw as a device tensor, truth as (1, X, Y, Z); twice the same bits
    vol2, t2, _ = P.normalize_subject(torch.from_numpy(raw).cuda(), None, scheme=P.ZScore(*pair))
    assert t2 is None and torch.equal(vol2, vol)
    _, t3, _ = P.normalize_subject(raw, None, truth[None], scheme=P.ZScore(*pair))
    assert torch.equal(t3, t)


def test_touching_subject_is_clipped_the_same_way(subjects, mean_std):
    from nas_3d_unet_amd import preprocess as P
    i = mp.TOUCHING
    raw, truth = subjects[i]
    vol, _, bw = P.normalize_subject(raw, None, truth, scheme=P.ZScore())
    X, Y, Z = mp.SHAPES[i]
    assert bw[0, 0] == 0 and bw[1, 2] == Z
    assert tuple(vol.shape[1:]) == (bw[1, 0] + 1, bw[1, 1] + 1 - bw[0, 1], Z - bw[0, 2])
    assert np.array_equal(P.normalize_subject(raw, mean_std, truth)[2], bw)


def test_a_count_equal_to_the_mean_stores_flt_min():
    from nas_3d_unet_amd import preprocess as P
    raw = np.zeros((4, 6, 5, 4), np.int16)
    for c in range(4):
        raw[c, 2, 1:4, 1:3] = np.array([[1, 2], [3, 1], [2, 3]]) * (c + 1)
    vol, _, bw = P.normalize_subject(raw, None, scheme=P.ZScore(0, 100))
    got = vol.cpu().numpy()
    want, _, _ = R.normalize_subject(raw, None, 0, 100)
    assert _bits(got) == _bits(want)
    sl = (slice(None),) + pr.box_slices(bw, raw.shape[1:])
    assert ((got.view(np.uint32) == 0x00800000) == (raw[sl] == 2 * np.arange(1, 5).reshape(4, 1, 1, 1))).all()
    assert int((got.view(np.uint32) == 0x00800000).sum()) == 8 and np.array_equal(got != 0, raw[sl] != 0)


def test_default_scheme_is_the_old_path(subjects, mean_std):
    """scheme=None (and no scheme argument at all) returns what the two launches of the reference scheme return when they are
    called as normalize_subject called them before it knew of schemes"""
    from nas_3d_unet_amd import _lib, preprocess as P
    from nas_3d_unet_amd import kernels as K
    lib = _lib.load()
    raw, truth = subjects[1]
    Cm, X, Y, Z = raw.shape
    r, t = torch.from_numpy(raw).cuda(), torch.from_numpy(truth).cuda()
    ms = torch.tensor([[mean_std["%s_mean" % m], mean_std["%s_std" % m]] for m in mp.MODS], dtype=torch.float64, device="cuda")
    rec = P._records(1, Cm, "cuda")[0]
    _lib.check(lib.n3d_brain_scan(K.ptr(r), Cm, X, Y, Z, K.ptr(torch.zeros((Cm, 2), dtype=torch.int64, device="cuda")), K.ptr(rec),
                                  K.stream_ptr()))
    h = rec.cpu().numpy().astype(np.int64)
    start = np.maximum(h[:, 2:5] - 1, 0).min(axis=0)
    end = np.minimum(h[:, 5:8] + 1, [X, Y, Z]).max(axis=0)
    hi = np.minimum(end + 1, [X, Y, Z])
    b = [int(v) for v in hi - start]
    out = torch.empty((Cm, *b), dtype=torch.float32, device="cuda")
    t_out = torch.empty(b, dtype=torch.uint8, device="cuda")
    _lib.check(lib.n3d_brain_normalize(K.ptr(r), Cm, X, Y, Z, K.ptr(ms), K.ptr(rec), (C.c_int32 * 3)(*[int(v) for v in start]),
                                       (C.c_int32 * 3)(*[int(v) for v in hi]), K.ptr(out), K.ptr(t), K.ptr(t_out), K.stream_ptr()))
    for call in (lambda: P.normalize_subject(raw, mean_std, truth), lambda: P.normalize_subject(raw, mean_std, truth, scheme=None),
                 lambda: P.normalize_subject(raw, mean_std, truth, mp.MODS, None)):
        vol, tt, bw = call()
        assert torch.equal(vol, out) and torch.equal(tt, t_out) and np.array_equal(bw, np.vstack((start, end)))


# ---- errors

def test_errors(subjects, mean_std):
    from nas_3d_unet_amd import preprocess as P
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.generator import VolumeSet
    raw, truth = subjects[0]
    flat = raw.copy()
    flat[3][flat[3] != 0] = 1234
    with pytest.raises(N3DError, match="t2 has a single value"):
        P.normalize_subject(flat, None, scheme=P.ZScore())
    tied = _special_subject()
    tied[0] = tied[2]
    with pytest.raises(N3DError, match="t1ce has a single value"):       # {7 x 150, 9 x 20, 8 x 3}: everything clips to 7
        P.normalize_subject(tied, None, scheme=P.ZScore(0, 50))
    one = raw.copy()
    one[2] = 0
    one[2, 6, 5, 3] = 17
    with pytest.raises(N3DError, match="flair has 1 nonzero voxel"):
        P.normalize_subject(one, None, scheme=P.ZScore())
    empty = raw.copy()
    empty[2] = 0
    for call in (lambda: P.normalize_subject(empty, None, scheme=P.ZScore()), lambda: P.subject_stats(empty, P.ZScore())):
        with pytest.raises(N3DError, match="flair has no nonzero voxel"):
            call()
    with pytest.raises(N3DError, match="not both"):
        P.normalize_subject(raw, mean_std, scheme=P.ZScore())
    with pytest.raises(N3DError, match="not both"):
        VolumeSet().add_subject(raw, truth, mean_std, scheme=P.ZScore())
    with pytest.raises(N3DError, match="mean_std .* or scheme|dictionary .* or a scheme"):
        VolumeSet().add_subject(raw, truth)
    with pytest.raises(N3DError, match="or a scheme"):
        P.normalize_subject(raw, None)
    with pytest.raises(N3DError, match="ZScore"):
        P.normalize_subject(raw, None, scheme="zscore")
    for call in (lambda: P.normalize_subject(raw.astype(np.float32), None, scheme=P.ZScore()),
                 lambda: P.subject_stats(raw.astype(np.float32), P.ZScore()),
                 lambda: VolumeSet().add_subject(torch.from_numpy(raw).float().cuda(), None, scheme=P.ZScore())):
        with pytest.raises(N3DError, match="int16"):
            call()
    with pytest.raises(N3DError, match="truth must be"):
        P.normalize_subject(raw, None, truth[1:], scheme=P.ZScore())
    with pytest.raises(N3DError, match="modalities"):
        P.normalize_subject(raw[:3], None, scheme=P.ZScore())


# ---- end to end

def test_generator_over_zscored_subjects(subjects):
    """raw scans -> add_subject(scheme=ZScore()) -> Generator(patch 8): the batch the same generator gives over add() of the
    helper's boxes, so its background is exactly 0 and its brain voxels have the helper's values"""
    from nas_3d_unet_amd import preprocess as P
    from nas_3d_unet_amd.generator import Generator, VolumeSet
    a, b = VolumeSet(), VolumeSet()
    boxes = []
    for n, i in enumerate((1, 2)):
        raw, truth = subjects[i]
        assert a.add_subject(raw, truth, scheme=P.ZScore()) == n
        want, want_t, bw = R.normalize_subject(raw, truth, 0.5, 99.5)
        b.add(want, want_t)
        boxes.append(want)
        assert a.box(n) == want.shape[1:] and a.origins[n] == tuple(bw[0].tolist()) and a.full_shapes[n] == mp.SHAPES[i]
        assert _bits(a.volumes[n].cpu().numpy()) == _bits(want)
    batches = []
    for vs in (a, b):
        gen = Generator([0, 1], vs, 8, patch_overlap=None, batch_size=3, labels=[1, 2, 4], permute=True, rng=random.Random(9))
        assert gen.steps_per_epoch >= 1
        batches.append(next(gen.epoch()))
    (xa, ta), (xb, tb) = batches
    assert xa.shape[0] == 3 and torch.equal(xa, xb) and torch.equal(ta, tb)
    x = xa.cpu().numpy()
    assert (x == 0).any() and (x != 0).any() and float(ta.max()) == 1
    assert np.isin(x[x != 0], np.concatenate([v[v != 0] for v in boxes])).all()


def test_prediction_over_a_zscored_subject_vanishes_outside_the_brain(subjects):
    """the skull mask of the z-scored box is the raw one (the net of tests/test_gpu_preprocess.py's last test)"""
    from _util import fill_module
    from nas_3d_unet_amd import preprocess as P
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
    i = vs.add_subject(raw, truth, scheme=P.ZScore())
    sp = SubjectPredictor(net, patch=16, batch=5)
    lab = sp.predict(vs, i, overlap=4, origin=vs.origins[i], full_shape=vs.full_shapes[i])
    lab = (lab[0] if isinstance(lab, tuple) else lab).cpu().numpy()
    print("labelled voxels: %d of %d brain voxels" % (int((lab != 0).sum()), int(np.any(raw != 0, axis=0).sum())))
    assert lab.shape == mp.SHAPES[1] and lab.any()
    assert not lab[~np.any(raw != 0, axis=0)].any()
