"""CPU: host side of the whole-image predictor (predict.ImagePredictor; prediction.py:102-119) -- the pad rule, the key rule, the
size bound, the C ABI of the three kernels, the numpy restatement of the passes (tests/_image_ref.py) and the fixture
tests/golden/fullimage.npz against the oracle's forward and against that restatement.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest
import torch

import _image_ref as ir
from oracle import data_step as ds
from oracle import post_step as ps
from oracle import ref_path as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(8)


def test_image_pad_rule():
    from nas_3d_unet_amd import predict
    from nas_3d_unet_amd._lib import N3DError
    # the depth-4 net halves its grid five times (stem1 and four down cells): D = 32; the reference's literal widths (prediction.py:116)
    assert predict.image_pad((240, 240, 155), 5) == (16, 16, 5)
    assert predict.image_pad((48, 40, 27), 5) == ir.FIX_PAD == (16, 24, 5)
    assert predict.image_pad((24, 27, 56), 5) == (8, 5, 8)
    # D = 16 (a net that halves four times)
    assert predict.image_pad((240, 240, 155), 4) == (16, 16, 5)
    assert predict.image_pad((48, 40, 27), 4) == (16, 8, 5)
    # every axis gets 1..D voxels: a multiple of D gets D more
    assert predict.image_pad((32, 64, 1), 5) == (32, 32, 31)
    # explicit widths: every padded axis a multiple of D, else an error
    assert predict.image_pad((48, 40, 27), 5, (16, 24, 37)) == (16, 24, 37)
    assert predict.image_pad((32, 64, 96), 5, (0, 0, 0)) == (0, 0, 0)
    for bad in ((16, 8, 5), (16, 24, 4), (-16, 24, 5), (16, 24)):
        with pytest.raises(N3DError):
            predict.image_pad((48, 40, 27), 5, bad)
    with pytest.raises(N3DError):
        predict.image_pad((48, 0, 27), 5)


def test_net_halvings_is_depth_plus_one():
    from nas_3d_unet_amd import predict, searched
    for depth in (2, 4):
        net = searched.SearchedNet(4, 4, 3, depth, 3, True, searched.Genotype(*orc.G_CONV))
        assert predict.net_halvings(net) == depth + 1


def test_key_rule_accepts_the_flips_and_nothing_else():
    from nas_3d_unet_amd import datastep, predict
    from nas_3d_unet_amd._lib import N3DError
    keys = ds.permutation_keys()
    assert len(keys) == 48 and set(keys) == datastep.generate_permutation_keys()
    assert predict.image_flip_of_key(None) == (False, False, False)
    ok, bad = [], []
    for k in keys:
        try:
            ok.append((k, predict.image_flip_of_key(k)))
        except N3DError:
            bad.append(k)
    assert len(ok) == 8 and len(bad) == 40
    assert sorted(f for _, f in ok) == sorted((bool(a), bool(b), bool(c)) for a in (0, 1) for b in (0, 1) for c in (0, 1))
    for k, f in ok:
        assert k[0] == (0, 0) and k[4] == 0 and f == (bool(k[1]), bool(k[2]), bool(k[3]))
        # the flip IS the reference's permute_data for that key (oracle.data_step.apply_isometry restates it)
        x = np.arange(2 * 4 * 4 * 4, dtype=np.float32).reshape(2, 4, 4, 4)
        assert np.array_equal(ds.apply_isometry(x, *ds.isometry_of_key(k)), ir.embed(x, (0, 0, 0), (4, 4, 4), (4, 4, 4), f))
    for k in bad:
        assert k[0] != (0, 0) or k[4] != 0
    for junk in ("flip", 3, ((0, 0), 1, 0), ((0, 0), 2, 0, 0, 0)):
        with pytest.raises(N3DError):
            predict.image_flip_of_key(junk)


def test_size_bound():
    from nas_3d_unet_amd import predict, searched
    from nas_3d_unet_amd._lib import N3DError
    N = 256 * 256 * 160
    assert predict.image_tensor_fits(N, 12) and predict.image_tensor_fits(N, 51)
    assert not predict.image_tensor_fits(N, 52) and not predict.image_tensor_fits(N, 64)
    assert not predict.image_tensor_fits(2 ** 31, 1, 1)
    # the default net (init_n_kernels = 4) fits at the reference's padded size; a 24-wide one does not (72-channel stems)
    gene = searched.Genotype(*orc.G_CONV)
    net = searched.SearchedNet(4, 4, 3, 4, 3, True, gene)
    rows = predict.image_forward_tensors(net, 4, (256, 256, 160))
    assert max(v * c for _, v, c in rows) == N * 12 and ("stem0", N, 12) in rows and ("down_cells.3", 8 * 8 * 5, 192) in rows
    predict.check_image_size(net, 4, (256, 256, 160))
    with pytest.raises(N3DError, match="stem0.*72 channels"):
        predict.check_image_size(searched.SearchedNet(4, 24, 3, 4, 3, True, gene), 4, (256, 256, 160))
    # channel counts that are no multiples of 4 count as the padded twin's
    odd = predict.image_forward_tensors(searched.SearchedNet(4, 6, 3, 2, 3, True, gene), 4, (32, 32, 32))
    assert ("stem0", 32 ** 3, 20) in odd and ("up_cells.2", 32 ** 3, 24) in odd


def test_image_kernels_are_declared_and_bound():
    from nas_3d_unet_amd import _lib, poststep, predict, train
    import inspect
    hdr = open(os.path.join(ROOT, "include", "n3d.h")).read()
    for name in ("n3d_image_embed", "n3d_image_add", "n3d_image_finish"):
        assert re.search(r"\bint %s\s*\(" % name, hdr)
        assert name in _lib.PROTOTYPES
    assert all(callable(getattr(poststep, f)) for f in ("image_embed", "image_add", "image_finish"))
    assert inspect.signature(train.Trainer.predictor).parameters["no_patch"].default is False
    ip = predict.ImagePredictor(None, graph=False)
    assert vars(ip.stats) == dict(captures=0, replays=0, forwards=0)
    assert issubclass(predict.ImagePredictor, predict._ForwardHost) and issubclass(predict.SubjectPredictor, predict._ForwardHost)


def test_reference_embed_is_pad_of_the_flipped_image():
    rng = np.random.default_rng(7)
    box = rng.standard_normal((2, 4, 3, 5)).astype(np.float32)
    full, origin, padded = (7, 5, 6), (2, 1, 0), (8, 8, 8)
    img = ir.place(box, origin, full)
    assert np.array_equal(img[:, 2:6, 1:4, 0:5], box) and np.count_nonzero(img) == box.size
    for flip in ((False,) * 3, (True, False, True), (True, True, True)):
        e = ir.embed(box, origin, full, padded, flip)
        assert e.shape == (2,) + padded
        assert not e[:, 7:].any() and not e[:, :, 5:].any() and not e[:, :, :, 6:].any()          # the pad stays at the high end
        assert np.array_equal(ir.unflip_crop(e, full, flip), img)                                  # a mirror is its own inverse


def test_reference_finish_sums_in_key_order():
    rng = np.random.default_rng(8)
    full, padded = (5, 4, 3), (8, 8, 4)
    flips = ((False,) * 3, (True, False, False), (False, True, True))
    ys = [rng.uniform(0, 1, (3,) + padded).astype(np.float32) for _ in flips]
    s = None
    for y, f in zip(ys[:-1], flips[:-1]):
        s = ir.add(s, y, full, f)
    lab, mean = ir.finish(ys[-1], full, flips[-1], s, 3, 0.5, False)
    t = [ir.unflip_crop(y, full, f).astype(np.float64) for y, f in zip(ys, flips)]
    assert np.array_equal(mean, ((t[0] + t[1]) + t[2]) / 3.0)
    assert np.array_equal(lab, ps.tumor_labels(mean, 0.5, False))
    lab1, mean1 = ir.finish(ys[0], full, flips[0])
    assert np.array_equal(mean1, ys[0][:, :5, :4, :3].astype(np.float64)) and mean1.dtype == np.float64


def test_oracle_forward_on_the_padded_fixture_input(golden):
    """the oracle's searched net on np.pad of the fixture's image, cropped, against the reference's own prediction at the tolerance
    test_oracle_golden.py holds the oracle's probabilities to (1e-4 of max|ref|)"""
    g = golden("fullimage")
    assert int(g["seed"]) == ir.FIX_SEED and tuple(g["pad"]) == ir.FIX_PAD
    box = ir.fixture_box()
    padded = tuple(f + w for f, w in zip(ir.FIX_FULL, ir.FIX_PAD))
    assert padded == (64, 64, 32)
    x = ir.embed(box, ir.FIX_ORIGIN, ir.FIX_FULL, padded)
    gene = getattr(orc, ir.FIX_GENE)
    cfg = orc.DEFAULT_CFG._replace(depth=ir.FIX_DEPTH)
    P = orc.make_params(orc.searched_param_specs(cfg, gene))
    with torch.no_grad():
        p = orc.searched_forward(P, torch.from_numpy(x[None]), gene, cfg)[0].numpy()
    F = ir.FIX_FULL
    ref = g["y"]
    assert ref.dtype == np.float32 and ref.shape == (3,) + F
    err = np.abs(p[:, :F[0], :F[1], :F[2]].astype(np.float64) - ref).max() / np.abs(ref).max()
    print("oracle vs fixture: max err / max|ref| = %.3e" % err)
    assert err <= 1e-4


@pytest.mark.parametrize("name,inclusive", [("labels/inclusive", True), ("labels/exclusive", False)])
def test_reference_finish_gives_the_fixture_labels(golden, name, inclusive):
    g = golden("fullimage")
    box = ir.fixture_box()
    F = ir.FIX_FULL
    assert (box == 0).all(axis=0).sum() > 100 and ir.skull(box, ir.FIX_ORIGIN, F).sum() < np.prod(ir.FIX_BOX)
    # finish takes the net's output on the padded grid: the fixture's cropped y in the low corner of it
    padded = tuple(f + w for f, w in zip(F, ir.FIX_PAD))
    y = np.full((3,) + padded, np.float32(0.9))
    y[:, :F[0], :F[1], :F[2]] = g["y"]
    lab, probs = ir.finish(y, F, threshold=0.5, inclusive=inclusive, mask_box=box, origin=ir.FIX_ORIGIN)
    assert lab.dtype == np.uint8 and np.array_equal(lab, g[name])
    assert np.array_equal(probs, g["y"].astype(np.float64))
    assert set(np.unique(g[name]).tolist()) == {0, 1, 2, 4}
    # the cap the GPU test relies on: voxels whose label hangs on less than its tolerance are rare
    near = (np.abs(g["y"].astype(np.float64) - 0.5) <= ir.TOL).any(axis=0)
    assert near.mean() <= 1e-3
