"""GPU: importance-weighted stitching (n3d_stitch_add_w / n3d_stitch_finish_w), predict.SubjectPredictor(blend=...) and
predict.EnsemblePredictor.  Kernel level: bit for bit against tests/_blend_ref.py (chunked, every isometry brought back, dead
entries), against the unweighted kernels under a ones profile, label fusion and skull mask in the finishing pass, argument
errors.  Predictor level: against the reference-style patch-by-patch loop blended by the same restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

import _blend_ref as br
from oracle import data_step as ds
from oracle import post_step as ps

pytestmark = pytest.mark.gpu


def _layout(t, layout):
    if layout == "ndhwc":
        return t.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)   # the layout the net's head produces
    return t


def _add_in_chunks(c, sizes, layout, profile=None):
    """the entry list of br.case through n3d_stitch_add_w (profile: a device tensor) or n3d_stitch_add (None) `sizes` entries at a
    time, each chunk with a tensor of its live patches only (none at all for an all-dead chunk).  Returns the running buffers."""
    from nas_3d_unet_amd import poststep as hp
    n, P, dead, corners, patches = c["n"], c["P"], c["dead"], c["corners"], c["patches"]
    assert sum(sizes) == n
    slots, at = [], 0
    for m in sizes:
        k = 0
        for e in range(at, at + m):
            slots.append(-1 if dead[e] else k)
            k += not dead[e]
        at += m
    table = hp.entry_table([(corners[e], br.iso(c["keys"][e]), slots[e]) for e in range(n)], "cuda")
    bufs = (hp.stitch_buffers if profile is None else hp.stitch_buffers_w)(br.SHAPE[0], br.SHAPE[1:], "cuda")
    at = 0
    for m in sizes:
        live = [patches[e] for e in range(at, at + m) if not dead[e]]
        t = _layout(torch.from_numpy(np.stack(live)).cuda(), layout) if live else (None, P)
        cs = np.asarray(corners[at:at + m])
        if profile is None:
            hp.stitch_add(t, table, at, m, cs.min(axis=0), cs.max(axis=0) + P, *bufs)
        else:
            hp.stitch_add_w(t, table, at, m, cs.min(axis=0), cs.max(axis=0) + P, profile, *bufs)
        at += m
    return bufs


@pytest.mark.parametrize("P", [6, 7])              # the profile's centre between two voxels / on a voxel
@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc"])
def test_stitch_add_w_in_uneven_chunks_vs_reference(layout, P):
    from nas_3d_unet_amd import poststep as hp
    c = br.case(P, with_dead=True)
    assert any(c["dead"]) and not all(c["dead"]) and c["dead"][7] and br.SIZES[1] == 1
    prof = hp.blend_profile(P, "gaussian")
    dprof = torch.from_numpy(prof).cuda()
    sum_, wsum = _add_in_chunks(c, br.SIZES, layout, dprof)
    S, W = br.blend(c["on_grid"], c["corners"], br.SHAPE, prof)
    assert sum_.dtype == wsum.dtype == torch.float64
    assert (wsum.cpu().numpy() == W).all() and (sum_.cpu().numpy() == S).all()
    _, probs = hp.stitch_finish_w(sum_, wsum, want_probs=True, want_labels=False)
    ref = br.mean(S, W)
    assert probs.dtype == torch.float64 and (probs.cpu().numpy() == ref).all()
    assert (W == 0).any() and (ref != ps.stitch(c["on_grid"], c["corners"], br.SHAPE)).any()
    # other chunkings of the same list: the same bits
    for other in ((49,), (1,) * 49, (20, 20, 9)):
        s2, w2 = _add_in_chunks(c, other, layout, dprof)
        assert torch.equal(s2, sum_) and torch.equal(w2, wsum)


@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc"])
def test_ones_profile_is_the_unweighted_stitch(layout):
    from nas_3d_unet_amd import poststep as hp
    c = br.case(6, with_dead=True)
    ones = torch.from_numpy(hp.blend_profile(6, "mean")).cuda()
    sum_w, wsum = _add_in_chunks(c, br.SIZES, layout, ones)
    sum_, cnt = _add_in_chunks(c, br.SIZES, layout, None)
    assert torch.equal(sum_w, sum_) and torch.equal(wsum, cnt.double()) and int(cnt.max()) > 1 and int(cnt.min()) == 0
    kw = dict(full_shape=(22, 17, 19), origin=(3, 2, 1), want_probs=True, want_labels=True)
    lab_w, probs_w = hp.stitch_finish_w(sum_w, wsum, **kw)
    lab, probs = hp.stitch_finish(sum_, cnt, **kw)
    assert torch.equal(probs_w, probs) and torch.equal(lab_w, lab)


def test_stitch_finish_w_labels_skull_mask_and_placement():
    from nas_3d_unet_amd import poststep as hp
    c = br.case(7, with_dead=True)
    prof = hp.blend_profile(7)
    sum_, wsum = _add_in_chunks(c, br.SIZES, "ndhwc", torch.from_numpy(prof).cuda())
    keep_sum, keep_wsum = sum_.clone(), wsum.clone()
    X, Y, Z = br.SHAPE[1:]
    full, org = (22, 17, 19), (3, 2, 1)
    inside = (slice(org[0], org[0] + X), slice(org[1], org[1] + Y), slice(org[2], org[2] + Z))
    _, probs = hp.stitch_finish_w(sum_, wsum, full_shape=full, origin=org, want_probs=True, want_labels=False)
    got = probs.cpu().numpy()
    exp = np.zeros((3,) + full)
    exp[(slice(None),) + inside] = br.mean(*br.blend(c["on_grid"], c["corners"], br.SHAPE, prof))
    assert (got == exp).all()
    uncovered = wsum.cpu().numpy() == 0
    assert uncovered.any() and not np.isnan(got).any() and (got[(slice(None),) + inside][:, uncovered] == 0).all()
    rng = np.random.default_rng(43)
    vol = rng.standard_normal((4, X, Y, Z)).astype(np.float32)
    vol[:, :6] = 0
    vol[:, :, :, 11:] = 0
    vol[1:, 10, 5, 5] = 0                      # one channel left: not skull
    vol[:, 11, 5, 5] = [0.0, -0.0, 0.0, -0.0]  # -0.0 is zero
    vol[:, 12, 5, 5] = [0.0, 1e-42, 0.0, 0.0]  # a denormal is not
    skull = np.any(vol != 0, axis=0)
    assert not skull[11, 5, 5] and skull[12, 5, 5] and skull[10, 5, 5]
    dvol = torch.from_numpy(vol).cuda()
    changed = False
    for thr, inclusive in ((0.5, True), (0.5, False), (0.3, False)):
        lab, none = hp.stitch_finish_w(sum_, wsum, full_shape=full, origin=org, want_probs=False, threshold=thr, inclusive_label=inclusive)
        ref = ps.tumor_labels(got, thr, inclusive)
        assert none is None and lab.dtype == torch.uint8 and np.array_equal(lab.cpu().numpy(), ref)
        assert torch.equal(lab, hp.tumor_labels(probs, thr, inclusive))
        masked, _ = hp.stitch_finish_w(sum_, wsum, full_shape=full, origin=org, want_probs=False, threshold=thr, inclusive_label=inclusive,
                                       mask_vol=dvol)
        exp_lab = np.zeros(full, np.uint8)
        exp_lab[inside] = ref[inside] * skull
        assert np.array_equal(masked.cpu().numpy(), exp_lab) and (ref[inside] != 0).any()
        changed = changed or (exp_lab != ref).any()
    assert changed
    # nothing but the outputs was written
    assert torch.equal(sum_, keep_sum) and torch.equal(wsum, keep_wsum)


def test_argument_errors_name_the_entry_point():
    from nas_3d_unet_amd import _lib, poststep as hp
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd._lib import N3DError
    lib = _lib.load()
    P = 6
    table = hp.entry_table([((0, 0, 0), br.IDENT, 0)], "cuda")
    patches = torch.zeros((1, 3, P, P, P), dtype=torch.float32, device="cuda")
    sb, sc, sv = K._bcv_strides(patches)
    sum_, wsum = hp.stitch_buffers_w(3, (8, 8, 8), "cuda")
    prof = torch.from_numpy(hp.blend_profile(P)).cuda()
    i3 = lambda *v: (C.c_int32 * 3)(*v)

    def raw(profile=K.ptr(prof), Cc=3, Pp=P):
        _lib.check(lib.n3d_stitch_add_w(K.ptr(patches), sb, sc, sv, Cc, Pp, 1, K.ptr(table), 1, profile, i3(0, 0, 0), i3(P, P, P), 8, 8, 8,
                                        K.ptr(sum_), K.ptr(wsum), K.stream_ptr()), "n3d_stitch_add_w")

    raw()                                                            # the arguments are good as they stand
    for bad in (dict(profile=None), dict(Pp=1025), dict(Cc=5)):     # every one of them is refused before anything is launched
        with pytest.raises(N3DError, match="n3d_stitch_add_w"):
            raw(**bad)
    with pytest.raises(N3DError, match="n3d_stitch_finish_w"):
        _lib.check(lib.n3d_stitch_finish_w(K.ptr(sum_), K.ptr(wsum), 5, 8, 8, 8, K.ptr(sum_), None, 0.5, 0, None, 0, 8, 8, 8, 0, 0, 0,
                                           K.stream_ptr()), "n3d_stitch_finish_w")
    with pytest.raises(N3DError, match="n3d_stitch_finish_w"):       # neither output
        _lib.check(lib.n3d_stitch_finish_w(K.ptr(sum_), K.ptr(wsum), 3, 8, 8, 8, None, None, 0.5, 0, None, 0, 8, 8, 8, 0, 0, 0,
                                           K.stream_ptr()), "n3d_stitch_finish_w")
    # the Python layer: a profile of the wrong length, a count buffer where the weight sum belongs, records outside the table
    add = lambda **kw: hp.stitch_add_w(**{**dict(patches=patches, table=table, first=0, count=1, lo=(0, 0, 0), hi=(P, P, P),
                                                 profile_dev=prof, sum_=sum_, wsum=wsum), **kw})
    add()
    with pytest.raises(N3DError, match="stitch_add_w"):
        add(profile_dev=torch.ones(P + 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(N3DError, match="stitch_add_w"):
        add(profile_dev=prof.float())
    with pytest.raises(N3DError, match="stitch_add_w"):
        add(count=2)
    with pytest.raises(N3DError, match="weight sum"):
        add(wsum=torch.zeros((8, 8, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(N3DError, match="stitch_finish_w"):
        hp.stitch_finish_w(sum_, wsum, want_probs=False, want_labels=False)
    torch.cuda.synchronize()


# ---- predictor level: the net, volume (with its empty slab), patch, overlap and batch of test_gpu_subject_predict.py
P, OVERLAP, BATCH = 16, 4, 5
TOL = 2e-6      # batch-of-5 vs batch-of-1 forward (test_gpu_subject_predict.py); a weighted mean is a convex combination of the same
                # per-patch predictions and cannot enlarge their largest error


def _net(prefix=""):
    from nas_3d_unet_amd import searched
    from _util import fill_module
    gene = searched.Genotype(down=[("down_conv", 0), ("down_dil_conv", 1), ("down_conv", 1), ("conv", 2), ("dil_conv", 2), ("conv", 3)],
                             up=[("conv", 0), ("up_conv", 1), ("up_conv", 1), ("dil_conv", 2), ("conv", 3), ("up_dil_conv", 1)])
    net = searched.SearchedNet(4, 4, 3, 2, 3, True, gene)
    fill_module(net, prefix=prefix)
    return net.cuda().eval()


def _volume(shape=(40, 21, 30), empty_from=18, seed=5):
    vol = np.random.default_rng(seed).standard_normal((4,) + shape).astype(np.float32)
    vol[:, :, :, empty_from:] = 0     # some patches are entirely empty
    return vol


def _volume_set(vol, truth=None):
    from nas_3d_unet_amd.generator import VolumeSet
    vs = VolumeSet()
    vs.add(vol, truth)
    return vs


def _loop_preds(net, vol, keys=(None,)):
    """reference-style loop (prediction.py:120-148): host crop, one patch at a time, per isometry key on the host-transformed crop
    with the inverse applied to its prediction; zeros for an all-zero crop.  Returns (predictions on the volume's grid, corners)."""
    from nas_3d_unet_amd.predict import patching
    corners = [tuple(int(v) for v in c) for c in patching(vol.shape[1:], (P, P, P), overlap=OVERLAP)]
    preds = []
    with torch.no_grad():
        for key in keys:
            for c in corners:
                data = ds.crop_zero_pad(vol, c, P)
                if np.all(data == 0):
                    preds.append(np.zeros((3, P, P, P), dtype=np.float32))
                    continue
                q = np.ascontiguousarray(ds.apply_isometry(data, *br.iso(key)))
                preds.append(br.inverse_iso(net(torch.from_numpy(q[None]).cuda())[0].cpu().numpy(), key))
    return preds, corners * len(keys)


def _blended(preds, corners, vol, profile):
    return br.mean(*br.blend(preds, corners, (3,) + tuple(vol.shape[1:]), profile))


@pytest.fixture(scope="module")
def subject():
    """net a, net b (other weights), the volume, and each net's patch-by-patch loop predictions: computed once, not modified"""
    net_a, net_b, vol = _net(), _net("b."), _volume()
    loop_a, corners = _loop_preds(net_a, vol)
    loop_b, _ = _loop_preds(net_b, vol)
    return dict(net_a=net_a, net_b=net_b, vol=vol, loop_a=loop_a, loop_b=loop_b, corners=corners)


def test_subject_predictor_gaussian_blend(subject):
    from nas_3d_unet_amd import poststep as hp
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.predict import SubjectPredictor
    net, vol = subject["net_a"], subject["vol"]
    vs = _volume_set(vol)
    sp = SubjectPredictor(net, patch=P, batch=BATCH)
    lab_m, probs_m = sp.predict(vs, 0, overlap=OVERLAP, want_probs=True)
    # a ones profile through the weighted kernels: the unweighted result, bit for bit
    lab_1, probs_1 = sp.predict(vs, 0, overlap=OVERLAP, want_probs=True, blend=np.ones(P))
    assert torch.equal(probs_1, probs_m) and torch.equal(lab_1, lab_m)
    lab, probs = sp.predict(vs, 0, overlap=OVERLAP, want_probs=True, blend="gaussian")
    ref = _blended(subject["loop_a"], subject["corners"], vol, hp.blend_profile(P))
    err = np.abs(probs.cpu().numpy() - ref).max()
    moved = float((probs - probs_m).abs().max())
    print("gaussian blend vs patch-by-patch loop: max |diff| %.3e; gaussian vs mean %.3e" % (err, moved))
    assert err < TOL and moved > 1e-4
    skull = np.any(vol != 0, axis=0)
    assert np.array_equal(lab.cpu().numpy(), ps.tumor_labels(probs.cpu().numpy(), 0.5, True) * skull) and (lab != 0).any()
    # the profile as an array, and another sigma
    _, probs_a = sp.predict(vs, 0, overlap=OVERLAP, want_probs=True, blend=hp.blend_profile(P))
    assert torch.equal(probs_a, probs)
    _, probs_s = sp.predict(vs, 0, overlap=OVERLAP, want_probs=True, blend="gaussian", sigma_scale=0.25)
    assert np.abs(probs_s.cpu().numpy() - _blended(subject["loop_a"], subject["corners"], vol, hp.blend_profile(P, "gaussian", 0.25))).max() < TOL
    assert float((probs_s - probs).abs().max()) > 1e-5
    # mean again: today's path, the same bits; one capture served all of it and each profile went up once
    lab_m2, probs_m2 = sp.predict(vs, 0, overlap=OVERLAP, want_probs=True, blend="mean")
    assert torch.equal(probs_m2, probs_m) and torch.equal(lab_m2, lab_m)
    assert sp.stats.captures == 1 and len(sp._profiles._dev) == 3
    with pytest.raises(N3DError):
        sp.predict(vs, 0, overlap=OVERLAP, blend="triangle")
    with pytest.raises(N3DError):
        sp.predict(vs, 0, overlap=OVERLAP, blend=np.ones(P + 1))


def test_gaussian_blend_with_isometry_keys(subject):
    from nas_3d_unet_amd import poststep as hp
    from nas_3d_unet_amd.predict import SubjectPredictor
    net, vol = subject["net_a"], subject["vol"]
    keys = (None, ds.permutation_keys()[30])
    assert br.iso(keys[1])[0] != [0, 1, 2] or any(br.iso(keys[1])[1])
    sp = SubjectPredictor(net, patch=P, batch=BATCH)
    _, probs = sp.predict(_volume_set(vol), 0, overlap=OVERLAP, keys=keys, want_probs=True, blend="gaussian")
    preds, corners = _loop_preds(net, vol, keys)
    err = np.abs(probs.cpu().numpy() - _blended(preds, corners, vol, hp.blend_profile(P))).max()
    print("gaussian blend, 2 keys, vs per-key loop: max |diff| %.3e" % err)
    assert err < TOL


def test_ensemble_predictor(subject):
    from nas_3d_unet_amd import metrics, postprocess, poststep as hp
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.predict import EnsemblePredictor, SubjectPredictor
    vol = subject["vol"]
    truth = np.random.default_rng(9).choice(np.array([0, 1, 2, 4], np.uint8), size=vol.shape[1:], p=[0.7, 0.1, 0.1, 0.1])
    vs = _volume_set(vol, truth)
    sa = SubjectPredictor(subject["net_a"], patch=P, batch=BATCH)
    sb = SubjectPredictor(subject["net_b"], patch=P, batch=3)
    kw = dict(overlap=OVERLAP, want_probs=True)
    # one member: that member, bit for bit
    solo = EnsemblePredictor([sa])
    for blend in ("mean", "gaussian"):
        la, pa = sa.predict(vs, 0, blend=blend, **kw)
        le, pe = solo.predict(vs, 0, blend=blend, **kw)
        assert torch.equal(pe, pa) and torch.equal(le, la)
    ens = EnsemblePredictor([sa, sb])
    _, pa = sa.predict(vs, 0, **kw)
    _, pb = sb.predict(vs, 0, **kw)
    assert float((pa - pb).abs().max()) > 1e-3                      # two different models
    lab, pm = ens.predict(vs, 0, **kw)
    # the pooled mean against the mean of the members' means: two orderings of < 1000 fp64 additions of values in [0, 1]
    err = float((pm - (pa + pb) / 2).abs().max())
    print("ensemble mean vs (pa + pb) / 2: max |diff| %.3e" % err)
    assert err < 1e-12
    assert ens.stats.qualifies == 1 and ens.stats.members == 2
    assert (ens.stats.entries, ens.stats.live) == (sa.stats.entries, sa.stats.live) == (sb.stats.entries, sb.stats.live)
    assert sa.stats.chunks == -(-sa.stats.live // BATCH) and sb.stats.chunks == -(-sb.stats.live // 3) and sa.stats.live < sa.stats.entries
    skull = np.any(vol != 0, axis=0)
    assert np.array_equal(lab.cpu().numpy(), ps.tumor_labels(pm.cpu().numpy(), 0.5, True) * skull)
    _, pg = ens.predict(vs, 0, blend="gaussian", **kw)
    ref = _blended(subject["loop_a"] + subject["loop_b"], subject["corners"] * 2, vol, hp.blend_profile(P))
    err = np.abs(pg.cpu().numpy() - ref).max()
    print("ensemble gaussian vs pooled loop: max |diff| %.3e" % err)
    assert err < TOL and ens.stats.qualifies == 1
    assert sa.stats.captures == 1 and sb.stats.captures == 1
    # the keyword reaches a scorer through CleanedPredictor and score_set as they stand
    rows = metrics.score_set(postprocess.CleanedPredictor(ens), vs, [0], blend="gaussian")
    assert len(rows) == 1 and rows[0]["Label"] == "0"
    for bad in ([], [sa, SubjectPredictor(subject["net_b"], patch=8, batch=3)], [sa, object()]):
        with pytest.raises(N3DError):
            EnsemblePredictor(bad)
    with pytest.raises(N3DError):
        ens.predict(vs, 0, blend="triangle", **kw)
