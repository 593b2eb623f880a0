"""GPU: whole-image inference (predict.ImagePredictor; prediction.py:102-119, predict(no_patch=True)).  Kernel level: n3d_image_embed,
n3d_image_add and n3d_image_finish are bit-exact against the numpy restatement (tests/_image_ref.py) -- flips, pitch gap, -0.0,
threshold equality, argmax ties, skull mask, the key-order fp64 sum.  Predictor level: the reference's own prediction of a small
subject (tests/golden/fullimage.npz), graph against eager, a second padded shape, the all-zero subject, the flip ensemble, the
trainer's entry point (padded twin included) and the size bound."""
import functools
import itertools

import numpy as np
import pytest
import torch

import _image_ref as ir
from _util import fill_module
from oracle import data_step as ds
from oracle import post_step as ps
from oracle import ref_path as orc

pytestmark = pytest.mark.gpu

FLIPS = list(itertools.product((False, True), repeat=3))
FULL, PADDED = (17, 12, 15), (32, 16, 16)       # odd sizes, no multiple of the 256-thread block, 32 blocks on the padded grid


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pitched(Cv, pitch, padded):
    """a NaN-filled (1, Cv, PX, PY, PZ) NDHWC tensor whose voxel pitch is `pitch` >= Cv, and its whole storage"""
    store = torch.full((1,) + tuple(padded) + (pitch,), float("nan"), device="cuda")
    return store[..., :Cv].permute(0, 4, 1, 2, 3), store


# ---- 1. embed ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cv,pitch", [(4, 8), (4, 4), (4, 6), (2, 2), (3, 5)])      # the 16-byte store (pitch of whole quads) and the scalar one
@pytest.mark.parametrize("box,origin", [((11, 9, 13), (3, 0, 2)),      # inside, touching one low face
                                        ((17, 12, 15), (0, 0, 0)),      # the box is the image
                                        ((11, 9, 13), (6, 3, 2))])      # touching the high faces
def test_embed_bit_for_bit(Cv, pitch, box, origin):
    from nas_3d_unet_amd import poststep as hp
    rng = np.random.default_rng(sum(box) + pitch)
    vol = rng.standard_normal((Cv,) + box).astype(np.float32)
    vol[:, ::3, 1::2, ::4] = -0.0
    vol[0, 1, 1, 1] = 0.0
    assert np.signbit(vol[vol == 0]).any() and not np.signbit(vol[vol == 0]).all()
    dvol = torch.from_numpy(vol).cuda()
    for flip in FLIPS:
        out, store = _pitched(Cv, pitch, PADDED)
        res = hp.image_embed(dvol, origin, FULL, PADDED, flip, out=out)
        assert res is out
        ref = ir.embed(vol, origin, FULL, PADDED, flip)
        got = store.cpu().numpy()[0]                                 # (PX, PY, PZ, pitch)
        assert np.array_equal(_bits(got[..., :Cv].transpose(3, 0, 1, 2)), _bits(ref)), flip      # every voxel written, -0.0 kept, pad +0.0
        assert np.isnan(got[..., Cv:]).all()                         # the pitch gap is not touched (n3d_patch_batch's convention)
    # a fresh output in the net's layout
    x = hp.image_embed(dvol, origin, FULL, PADDED)
    assert tuple(x.shape) == (1, Cv) + PADDED and np.array_equal(_bits(x.cpu().numpy()[0]), _bits(ir.embed(vol, origin, FULL, PADDED)))


def test_argument_checks_follow_the_neighbours():
    import ctypes as C
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd import poststep as hp
    from nas_3d_unet_amd._lib import N3DError
    vol = torch.zeros((4, 5, 5, 5), device="cuda")
    for origin, full, padded in (((4, 0, 0), (8, 8, 8), (8, 8, 8)),      # box outside the image
                                 ((-1, 0, 0), (8, 8, 8), (8, 8, 8)),
                                 ((0, 0, 0), (8, 8, 8), (8, 7, 8))):     # P < F
        with pytest.raises(N3DError):
            hp.image_embed(vol, origin, full, padded)
    y = torch.zeros((1, 5, 8, 8, 8), device="cuda")
    with pytest.raises(N3DError):
        hp.image_finish(y, (8, 8, 8), (8, 8, 8), want_labels=False)       # C <= 4
    with pytest.raises(N3DError):
        hp.image_finish(y[:, :2], (8, 8, 8), (8, 8, 8))                   # labels fuse 3 channels
    with pytest.raises(N3DError):
        hp.image_finish(y[:, :3], (8, 8, 8), (8, 8, 8), want_probs=False, want_labels=False)
    # FX * FY * FZ >= 2^31 is refused at the C ABI before anything is launched (no tensor of that size is made here)
    i3 = lambda *v: (C.c_int32 * 3)(*v)
    out = torch.zeros(16, device="cuda")
    big = i3(2048, 1024, 1024)
    assert _lib.load().n3d_image_embed(K.ptr(vol), 4, 5, 5, 5, i3(0, 0, 0), big, big, i3(0, 0, 0), K.ptr(out), 4, K.stream_ptr()) != 0
    assert b"too large" in _lib.load().n3d_last_error()


# ---- 2. finish ----------------------------------------------------------------------------------------------------------------
def _special_y(rng, shape):
    """fp32 values from a small set: exactly 0.5, its lower neighbour, float32(0.3) and both of its neighbours (0.3 as a double lies
    between float32(0.3) and the one below), so threshold equality and -- equal values across channels -- argmax ties occur"""
    h, t = np.float32(0.5), np.float32(0.3)
    vals = np.array([h, np.nextafter(h, np.float32(0)), np.nextafter(h, np.float32(1)), t, np.nextafter(t, np.float32(0)),
                     np.nextafter(t, np.float32(1)), 0.1, 0.7, 0.9], dtype=np.float32)
    return vals[rng.integers(0, len(vals), shape)]


def _layout(t, layout):
    if layout == "ndhwc":
        return t.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)      # the layout the net's head produces
    return t


def _mask_box(rng, box):
    vol = rng.standard_normal((4,) + box).astype(np.float32)
    vol[:, :3] = 0
    vol[:, :, :, 9:] = 0
    vol[1:, 5, 4, 4] = 0                       # one channel left: not skull
    vol[:, 6, 4, 4] = [0.0, -0.0, 0.0, -0.0]   # -0.0 is zero
    vol[:, 7, 4, 4] = [0.0, 1e-42, 0.0, 0.0]   # a denormal is not
    return vol


@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc"])
def test_finish_single_key_bit_for_bit(layout):
    from nas_3d_unet_amd import poststep as hp
    rng = np.random.default_rng(51)
    y = _special_y(rng, (3,) + PADDED)
    dy = _layout(torch.from_numpy(y[None]).cuda(), layout)
    box, origin = (11, 9, 13), (3, 0, 2)
    vol = _mask_box(rng, box)
    dvol = torch.from_numpy(vol).cuda()
    skull = ir.skull(vol, origin, FULL)
    assert skull[3 + 5, 4, 6] and not skull[3 + 6, 4, 6] and skull[3 + 7, 4, 6] and not skull[:3].any()
    crop = y[:, :FULL[0], :FULL[1], :FULL[2]]
    ties = 0
    for thr, inclusive in ((0.5, True), (0.5, False), (0.3, False), (0.3, True)):
        lab, probs = hp.image_finish(dy, FULL, PADDED, threshold=thr, inclusive_label=inclusive)
        assert probs.dtype == torch.float64 and lab.dtype == torch.uint8
        p = probs.cpu().numpy()
        assert np.array_equal(_bits(p.astype(np.float32)), _bits(crop)) and np.array_equal(p, crop.astype(np.float64))      # exactly (double)y, cropped
        ref = ps.tumor_labels(p, thr, inclusive)
        assert np.array_equal(lab.cpu().numpy(), ref)
        masked, none = hp.image_finish(dy, FULL, PADDED, want_probs=False, threshold=thr, inclusive_label=inclusive, mask_box=dvol, origin=origin)
        assert none is None and np.array_equal(masked.cpu().numpy(), ref * skull)
        assert (ref * skull != ref).any()
        rl, rp = ir.finish(y, FULL, threshold=thr, inclusive=inclusive, mask_box=vol, origin=origin)
        assert np.array_equal(masked.cpu().numpy(), rl) and np.array_equal(p, rp)
        both = (p >= thr).sum(axis=0) >= 2
        ties += int((both & ((p[0] == p[1]) | (p[0] == p[2]) | (p[1] == p[2]))).sum())
        assert (p == thr).any() or thr == 0.3       # 0.5 is a float32: equality occurs; 0.3 is none: its two neighbours straddle it
    assert ties > 50
    # under a flip the prediction comes back mirrored; probabilities only (labels NULL) and any channel count up to 4
    for flip in FLIPS[1:]:
        lab, probs = hp.image_finish(dy, FULL, PADDED, flip, threshold=0.3, inclusive_label=False, mask_box=dvol, origin=origin)
        rl, rp = ir.finish(y, FULL, flip, threshold=0.3, inclusive=False, mask_box=vol, origin=origin)
        assert np.array_equal(lab.cpu().numpy(), rl) and np.array_equal(probs.cpu().numpy(), rp)
    y4 = _special_y(rng, (4,) + PADDED)
    _, p4 = hp.image_finish(_layout(torch.from_numpy(y4[None]).cuda(), layout), FULL, PADDED, FLIPS[5], want_labels=False)
    assert np.array_equal(p4.cpu().numpy(), ir.unflip_crop(y4, FULL, FLIPS[5]).astype(np.float64))


@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc"])
def test_finish_three_keys_sum_in_key_order(layout):
    from nas_3d_unet_amd import poststep as hp
    from nas_3d_unet_amd._lib import N3DError
    rng = np.random.default_rng(52)
    flips = (FLIPS[0], FLIPS[6], FLIPS[3])
    ys = [_special_y(rng, (3,) + PADDED) for _ in flips]
    dys = [_layout(torch.from_numpy(y[None]).cuda(), layout) for y in ys]
    box, origin = (11, 9, 13), (6, 3, 2)
    vol = _mask_box(rng, box)
    dvol = torch.from_numpy(vol).cuda()
    rs = None
    for y, f in zip(ys[:-1], flips[:-1]):
        rs = ir.add(rs, y, FULL, f)

    def run():
        s = hp.image_add(dys[0], FULL, PADDED, flips[0])                       # the first key writes: a fresh, uncleared buffer
        s2 = hp.image_add(dys[1], FULL, PADDED, flips[1], s)
        assert s2 is s
        return s, s.clone()

    s, kept = run()
    assert np.array_equal(s.cpu().numpy(), rs)
    outs = []
    for thr, inclusive in ((0.5, True), (0.5, False), (0.3, False), (0.3, True)):
        lab, probs = hp.image_finish(dys[2], FULL, PADDED, flips[2], s, 3, threshold=thr, inclusive_label=inclusive, mask_box=dvol, origin=origin)
        rl, rp = ir.finish(ys[2], FULL, flips[2], rs, 3, thr, inclusive, vol, origin)
        assert np.array_equal(probs.cpu().numpy(), rp) and np.array_equal(lab.cpu().numpy(), rl)
        nomask, _ = hp.image_finish(dys[2], FULL, PADDED, flips[2], s, 3, want_probs=False, threshold=thr, inclusive_label=inclusive)
        assert np.array_equal(nomask.cpu().numpy(), ps.tumor_labels(rp, thr, inclusive))
        outs.append((lab, probs))
    assert torch.equal(s, kept)                                                # finish reads the sum, it does not write it
    # the same inputs give the same bits
    s_again, _ = run()
    assert torch.equal(s_again, s)
    lab2, probs2 = hp.image_finish(dys[2], FULL, PADDED, flips[2], s_again, 3, threshold=0.3, inclusive_label=True, mask_box=dvol, origin=origin)
    assert torch.equal(lab2, outs[3][0]) and torch.equal(probs2, outs[3][1])
    # a running sum goes with K > 1, and only with it
    with pytest.raises(N3DError):
        hp.image_finish(dys[2], FULL, PADDED, flips[2], s, 1)
    with pytest.raises(N3DError):
        hp.image_finish(dys[2], FULL, PADDED, flips[2], None, 3)


# ---- predictor level -----------------------------------------------------------------------------------------------------------
def _fixture_net():
    from nas_3d_unet_amd import searched
    net = searched.SearchedNet(4, 4, 3, ir.FIX_DEPTH, 3, True, searched.Genotype(*getattr(orc, ir.FIX_GENE)))
    fill_module(net)
    return net.cuda().eval()


def _volume_set(*subjects):
    """subjects: (box array, origin or None, full shape or None) -- what VolumeSet.add_subject records"""
    from nas_3d_unet_amd.generator import VolumeSet
    vs = VolumeSet()
    for vol, origin, full in subjects:
        i = vs.add(vol)
        vs.origins[i], vs.full_shapes[i] = origin, full
    return vs


SECOND_FULL, SECOND_BOX, SECOND_ORIGIN = (24, 27, 56), (20, 27, 41), (4, 0, 9)


def _second_box():
    vol = np.random.default_rng(77).standard_normal((4,) + SECOND_BOX).astype(np.float32)
    vol[:, :, 10:13, 30:] = 0
    return vol


@functools.lru_cache(maxsize=None)
def _oracle_second():
    """the CPU oracle's prediction of the second subject on its padded image (32, 32, 64), cropped: computed once"""
    gene = getattr(orc, ir.FIX_GENE)
    cfg = orc.DEFAULT_CFG._replace(depth=ir.FIX_DEPTH)
    P = orc.make_params(orc.searched_param_specs(cfg, gene))
    x = ir.embed(_second_box(), SECOND_ORIGIN, SECOND_FULL, (32, 32, 64))
    with torch.no_grad():
        p = orc.searched_forward(P, torch.from_numpy(x[None]), gene, cfg)[0].numpy()
    F = SECOND_FULL
    return p[:, :F[0], :F[1], :F[2]]


def test_fixture_end_to_end_graph_eager_and_a_second_shape(golden):
    from nas_3d_unet_amd.predict import ImagePredictor, image_pad, net_halvings
    g = golden("fullimage")
    net = _fixture_net()
    assert image_pad(ir.FIX_FULL, net_halvings(net)) == ir.FIX_PAD == tuple(g["pad"])
    box = ir.fixture_box()
    vs = _volume_set((box, ir.FIX_ORIGIN, ir.FIX_FULL), (_second_box(), SECOND_ORIGIN, SECOND_FULL))
    ip = ImagePredictor(net, graph=True)
    lab, probs = ip.predict(vs, 0, want_probs=True)
    assert (ip.stats.captures, ip.stats.replays, ip.stats.forwards) == (1, 1, 1)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == ir.FIX_FULL and probs.dtype == torch.float64 and tuple(probs.shape) == (3,) + ir.FIX_FULL
    p, ref = probs.cpu().numpy(), g["y"].astype(np.float64)
    err = np.abs(p - ref).max()
    print("whole-image prediction vs the reference's: max |diff| %.3e" % err)
    assert err < ir.TOL
    # labels: exactly the fusion of the returned probabilities, skull-masked; the reference's wherever they do not hang on the tolerance
    skull = ir.skull(box, ir.FIX_ORIGIN, ir.FIX_FULL)
    assert np.array_equal(lab.cpu().numpy(), ps.tumor_labels(p, 0.5, True) * skull)
    near = (np.abs(ref - 0.5) <= ir.TOL).any(axis=0)
    print("voxels within %.0e of the threshold: %d of %d" % (ir.TOL, near.sum(), near.size))
    assert near.mean() <= 1e-3
    assert np.array_equal(lab.cpu().numpy()[~near], g["labels/inclusive"][~near])
    lab_x, none = ip.predict(vs, 0, inclusive_label=False)
    assert none is None and np.array_equal(lab_x.cpu().numpy(), ps.tumor_labels(p, 0.5, False) * skull)
    assert np.array_equal(lab_x.cpu().numpy()[~near], g["labels/exclusive"][~near])
    lab_n, _ = ip.predict(vs, 0, threshold=0.3, inclusive_label=False, skull_mask=False)
    assert np.array_equal(lab_n.cpu().numpy(), ps.tumor_labels(p, 0.3, False))
    assert (ip.stats.captures, ip.stats.replays, ip.stats.forwards) == (1, 3, 3)
    # origin / full shape given explicitly override what the set recorded; the same numbers give the same bits
    lab_e, probs_e = ip.predict(vs, 0, full_shape=ir.FIX_FULL, origin=ir.FIX_ORIGIN, pad=ir.FIX_PAD, want_probs=True)
    assert torch.equal(lab_e, lab) and torch.equal(probs_e, probs) and ip.stats.captures == 1
    # eager: the same bits
    ie = ImagePredictor(net, graph=False)
    le, pe = ie.predict(vs, 0, want_probs=True)
    assert torch.equal(le, lab) and torch.equal(pe, probs)
    assert (ie.stats.captures, ie.stats.replays, ie.stats.forwards) == (0, 0, 1)
    # another padded shape: (24, 27, 56) -> (32, 32, 64), a new capture (one entry is kept)
    lab2, probs2 = ip.predict(vs, 1, want_probs=True)
    assert ip.stats.captures == 2 and tuple(probs2.shape) == (3,) + SECOND_FULL
    err2 = np.abs(probs2.cpu().numpy() - _oracle_second().astype(np.float64)).max()
    print("second subject vs the CPU oracle: max |diff| %.3e" % err2)
    assert err2 < ir.TOL
    assert np.array_equal(lab2.cpu().numpy(), ps.tumor_labels(probs2.cpu().numpy(), 0.5, True) * ir.skull(_second_box(), SECOND_ORIGIN, SECOND_FULL))
    le2, pe2 = ie.predict(vs, 1, want_probs=True)
    assert torch.equal(le2, lab2) and torch.equal(pe2, probs2)
    # back to the first shape: the first result, bit for bit
    lab3, probs3 = ip.predict(vs, 0, want_probs=True)
    assert ip.stats.captures == 3 and torch.equal(lab3, lab) and torch.equal(probs3, probs)
    assert not net.training
    net.train()
    ip.predict(vs, 0)
    assert net.training and all(m.training for m in net.modules()) and ip.stats.captures == 3      # the caller's mode is restored
    net.eval()


def test_box_without_origin_is_the_image_and_weights_moved_recapture():
    from nas_3d_unet_amd.predict import ImagePredictor
    net = _fixture_net()
    vol = np.random.default_rng(3).standard_normal((4, 20, 9, 33)).astype(np.float32)
    vs = _volume_set((vol, None, None))
    ip = ImagePredictor(net, graph=True)
    lab, probs = ip.predict(vs, 0, want_probs=True)
    assert tuple(lab.shape) == (20, 9, 33) and ip.stats.captures == 1
    with torch.no_grad():
        net.last_conv[0].conv.bias.add_(0.25)                  # in place: same storage, the captured graph stays
    _, moved = ip.predict(vs, 0, want_probs=True)
    assert ip.stats.captures == 1 and float((moved - probs).abs().max()) > 1e-3
    _, pe = ImagePredictor(net, graph=False).predict(vs, 0, want_probs=True)
    assert torch.equal(moved, pe)
    with torch.no_grad():
        for q in net.parameters():
            q.data = q.data.clone()                            # parameters in other storage: a new capture
    _, again = ip.predict(vs, 0, want_probs=True)
    assert ip.stats.captures == 2 and torch.equal(again, pe)


def test_all_zero_subject_runs_no_forward():
    from nas_3d_unet_amd.predict import ImagePredictor
    net = _fixture_net()
    zero = np.zeros((4, 10, 12, 9), np.float32)
    zero[1, 2, 3, 4] = -0.0                                    # -0.0 is zero (np.all(data == 0), prediction.py:114)
    vs = _volume_set((zero, (1, 2, 3), (14, 15, 16)), (np.ones((4, 3, 3, 3), np.float32), (0, 0, 0), (14, 15, 16)))
    ip = ImagePredictor(net, graph=True)
    lab, probs = ip.predict(vs, 0, want_probs=True)
    assert tuple(lab.shape) == (14, 15, 16) and lab.dtype == torch.uint8 and not lab.any()
    assert tuple(probs.shape) == (3, 14, 15, 16) and probs.dtype == torch.float64 and not probs.any()
    assert (ip.stats.captures, ip.stats.replays, ip.stats.forwards) == (0, 0, 0)
    ip.predict(vs, 1)
    before = vars(ip.stats).copy()
    assert before["forwards"] == 1
    lab, none = ip.predict(vs, 0)
    assert none is None and not lab.any() and vars(ip.stats) == before


def test_flip_ensemble_is_the_key_order_mean():
    from nas_3d_unet_amd.predict import ImagePredictor
    from nas_3d_unet_amd._lib import N3DError
    net = _fixture_net()
    box = ir.fixture_box()
    vs = _volume_set((box, ir.FIX_ORIGIN, ir.FIX_FULL))
    fx, fz = ((0, 0), 1, 0, 0, 0), ((0, 0), 0, 0, 1, 0)
    ip = ImagePredictor(net, graph=True)
    singles = [ip.predict(vs, 0, keys=(k,), want_probs=True)[1].cpu().numpy() for k in (None, fx, fz)]
    assert np.abs(singles[1] - singles[0]).max() > 1e-4 and np.abs(singles[2] - singles[0]).max() > 1e-4      # the net is no even function
    lab, probs = ip.predict(vs, 0, keys=(None, fx, fz), want_probs=True)
    mean = ((singles[0] + singles[1]) + singles[2]) / 3.0
    assert np.array_equal(probs.cpu().numpy(), mean)
    assert np.array_equal(lab.cpu().numpy(), ps.tumor_labels(mean, 0.5, True) * ir.skull(box, ir.FIX_ORIGIN, ir.FIX_FULL))
    assert ip.stats.captures == 1 and ip.stats.forwards == 6
    forwards = ip.stats.forwards
    for bad in (((0, 1), 0, 0, 0, 0), ((0, 0), 1, 0, 0, 1), "fx"):
        with pytest.raises(N3DError):
            ip.predict(vs, 0, keys=(None, bad))
    with pytest.raises(N3DError):
        ip.predict(vs, 0, keys=())
    with pytest.raises(N3DError):
        ip.predict(vs, 0, pad=(16, 8, 5))                     # (64, 48, 32): 48 is no multiple of 32
    assert ip.stats.forwards == forwards


# ---- the trainer's entry point: the net, patch and batch of test_trainer_predictor_predicts_with_the_moved_weights
TRAIN_DOWN = [("down_conv", 0), ("down_dil_conv", 1), ("down_conv", 1), ("conv", 2), ("dil_conv", 2), ("conv", 3)]
TRAIN_UP = [("conv", 0), ("up_conv", 1), ("up_conv", 1), ("dil_conv", 2), ("conv", 3), ("up_dil_conv", 1)]


@pytest.mark.parametrize("init_n_kernels", [4, 6])
def test_trainer_image_predictor_predicts_with_the_stepped_weights(init_n_kernels):
    from nas_3d_unet_amd import searched
    from nas_3d_unet_amd.predict import ImagePredictor, SubjectPredictor
    from nas_3d_unet_amd.train import Trainer
    net = searched.SearchedNet(4, init_n_kernels, 3, 2, 3, True, searched.Genotype(down=TRAIN_DOWN, up=TRAIN_UP))
    fill_module(net)
    net = net.cuda().train()
    net.last_conv[0].dropout = None
    assert bool(net._n3d_padded) == (init_n_kernels == 6)
    rng = np.random.default_rng(12)
    full, origin = (20, 14, 11), (3, 1, 0)
    vol = rng.standard_normal((4, 15, 12, 11)).astype(np.float32)
    vol[:, 4:6] = 0
    vs = _volume_set((vol, origin, full))
    tr = Trainer(net, graph=True)
    ip = tr.predictor(no_patch=True)
    assert isinstance(ip, ImagePredictor) and ip.use_graph and isinstance(tr.predictor(16, 5), SubjectPredictor)
    _, before = ip.predict(vs, 0, want_probs=True)
    x = torch.from_numpy(rng.standard_normal((2, 4, 16, 16, 16)).astype(np.float32)).cuda()
    t = torch.from_numpy((rng.uniform(0, 1, (2, 3, 16, 16, 16)) < 0.3).astype(np.float32)).cuda()
    tr.step(x, t)
    lab, probs = ip.predict(vs, 0, want_probs=True)          # the predictor made before the step: a replay
    assert ip.stats.captures == 1 and net.training
    assert float((probs - before).abs().max()) > 1e-6
    tr.check_sync()      # (padded twin: the trained parameters back in the user's module)
    le, pe = ImagePredictor(net, graph=False).predict(vs, 0, want_probs=True)
    if init_n_kernels == 4:
        assert torch.equal(probs, pe) and torch.equal(lab, le)
    else:
        # the module's own twin is embedded afresh from the cut-back parameters: the same numbers through the same kernels
        assert float((probs - pe).abs().max()) < 2e-6
    # against the CPU oracle with the stepped parameters (fp64: test_gpu_nets.py evaluates it so for channel counts that are no
    # multiples of 4, and holds such a net's probabilities to 3e-5 of it; the unpadded net's to 2e-5)
    gene = orc.Genotype(TRAIN_DOWN, TRAIN_UP)
    cfg = orc.NetCfg(4, init_n_kernels, 3, 2, 3, True)
    P = {n: q.detach().cpu().double() for n, q in net.named_parameters()}
    padded = (24, 16, 16)                                     # D = 8: (4, 2, 5)
    xin = ir.embed(vol, origin, full, padded)
    with torch.no_grad():
        ref = orc.searched_forward(P, torch.from_numpy(xin[None]).double(), gene, cfg)[0].numpy()[:, :20, :14, :11]
    err = np.abs(probs.cpu().numpy() - ref).max()
    print("trainer's whole-image predictor (init_n_kernels %d) vs the fp64 oracle: max |diff| %.3e" % (init_n_kernels, err))
    assert err < (3e-5 if init_n_kernels == 6 else 2e-5)
    assert np.array_equal(lab.cpu().numpy(), ps.tumor_labels(probs.cpu().numpy(), 0.5, True) * ir.skull(vol, origin, full))


def test_oversized_request_is_refused_before_any_launch():
    from nas_3d_unet_amd.predict import ImagePredictor, check_image_size
    from nas_3d_unet_amd._lib import N3DError
    net = _fixture_net()
    vs = _volume_set((np.ones((4, 8, 8, 8), np.float32), (0, 0, 0), (1000, 1000, 600)))
    ip = ImagePredictor(net, graph=True)
    with pytest.raises(N3DError, match=r"\d+ voxels x \d+ channels x 4 bytes = \d+ bytes"):
        ip.predict(vs, 0)                                     # (1024, 1024, 608): the 12-channel stem alone would be 30.6e9 bytes
    assert (ip.stats.captures, ip.stats.replays, ip.stats.forwards) == (0, 0, 0) and ip._x is None and ip._graph is None
    check_image_size(net, 4, (256, 256, 160))                 # the reference's own size passes
