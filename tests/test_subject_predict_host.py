"""CPU: host side of the subject predictor (predict.SubjectPredictor) -- the entry / chunk planner, the inverse of the 48 cube
isometries that the GPU tests build their expectation with, and the C ABI of the stitching kernels.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest

from oracle import data_step as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_plan(dead, n_keys, batch):
    from nas_3d_unet_amd.predict import plan_subject
    dead = np.asarray(dead, dtype=bool)
    nc = len(dead)
    plan = plan_subject(dead, n_keys, batch)
    n = nc * n_keys
    # key-major: for key in keys: for corner in corners
    assert plan.corner.tolist() == [c for _ in range(n_keys) for c in range(nc)]
    assert plan.key.tolist() == [k for k in range(n_keys) for _ in range(nc)]
    # dead entries -- under every key -- have slot < 0, live ones a slot of their chunk's tensor
    assert len(plan.slot) == n
    assert np.array_equal(plan.slot < 0, dead[plan.corner])
    live = np.flatnonzero(plan.slot >= 0)
    assert len(plan.chunks) == -(-len(live) // batch)
    # the chunks' table ranges tile the list in order; each holds exactly its own live entries, at distinct slots 0, 1, ...
    at = 0
    seen = []
    for ch in plan.chunks:
        assert ch.first == at and ch.last > ch.first
        at = ch.last
        assert len(ch.refs) == batch          # the net always runs at one batch shape
        mine = [e for e in range(ch.first, ch.last) if plan.slot[e] >= 0]
        assert 1 <= len(mine) <= batch
        assert [int(plan.slot[e]) for e in mine] == list(range(len(mine)))
        assert ch.refs[:len(mine)] == mine    # slot s of the input holds the entry whose table record says s
        # padding repeats a live patch, and no table record points at a padding slot
        assert all(plan.slot[e] >= 0 for e in ch.refs[len(mine):])
        assert all(plan.slot[e] < len(mine) for e in range(ch.first, ch.last))
        seen += mine
    assert seen == live.tolist()              # live entries in list order, batch at a time
    assert all(len([e for e in range(c.first, c.last) if plan.slot[e] >= 0]) == batch for c in plan.chunks[:-1])
    if plan.chunks:
        assert at == n
    return plan


@pytest.mark.parametrize("batch", [1, 3, 5, 8])
@pytest.mark.parametrize("n_keys", [1, 4])
def test_plan_is_key_major_and_skips_dead_entries(batch, n_keys):
    rng = np.random.default_rng(100 * batch + n_keys)
    for nc in (1, 7, 26):
        for p_dead in (0.0, 0.4, 0.9):
            _check_plan(rng.uniform(0, 1, nc) < p_dead, n_keys, batch)
    # dead entries at either end and in a row
    _check_plan([1, 1, 0, 0, 1, 1, 1, 0, 1], n_keys, batch)
    # live count an exact multiple of the batch: no padding
    plan = _check_plan([0] * batch * 2 + [1], n_keys, batch)
    assert all(len(set(ch.refs)) == batch for ch in plan.chunks[:2])


def test_plan_without_a_live_entry_has_no_chunk():
    plan = _check_plan([1, 1, 1], 2, 4)
    assert plan.chunks == [] and (plan.slot < 0).all()


def test_inverse_of_every_isometry_round_trips():
    """inv_perm[b] = perm.index(b), inv_flip[b] = flip[inv_perm[b]] undoes the isometry the gather applies, for the 48 keys and the
    identity, exactly (indices only: no arithmetic)"""
    from nas_3d_unet_amd import datastep
    keys = [None] + ds.permutation_keys()
    assert len(keys) == 49 and set(keys[1:]) == datastep.generate_permutation_keys()
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 5, 5, 5)).astype(np.float32)
    images = set()
    for key in keys:
        perm, flip = ([0, 1, 2], [False] * 3) if key is None else datastep.isometry_of_key(key)
        if key is not None:
            assert (perm, flip) == ds.isometry_of_key(key)
        inv_perm, inv_flip = datastep.inverse_isometry(perm, flip)
        assert inv_perm == [list(perm).index(b) for b in range(3)]
        assert inv_flip == [flip[inv_perm[b]] for b in range(3)]
        q = ds.apply_isometry(x, perm, flip)
        assert np.array_equal(ds.apply_isometry(q, inv_perm, inv_flip), x)
        assert np.array_equal(ds.apply_isometry(ds.apply_isometry(x, inv_perm, inv_flip), perm, flip), x)
        images.add(q.tobytes())
    assert len(images) == 48          # the 48 keys are the 48 distinct isometries (the identity is one of them)


def test_stitch_kernels_are_declared_and_bound():
    from nas_3d_unet_amd import _lib
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "n3d.h")).read()
    for name in ("n3d_stitch_add", "n3d_stitch_finish"):
        assert re.search(r"\bint %s\s*\(" % name, hdr)
        assert name in _lib.PROTOTYPES
    # the table record is the gather's descriptor plus the slot: ten int32
    assert C.sizeof(_lib.StitchEntry) == 40 == C.sizeof(_lib.GatherDesc)


def test_entry_table_rejects_what_is_no_permutation():
    from nas_3d_unet_amd import poststep
    from nas_3d_unet_amd._lib import N3DError
    with pytest.raises(N3DError):
        poststep.entry_table([((0, 0, 0), ([0, 0, 2], [False] * 3), 0)], "cpu")
    t = poststep.entry_table([((1, -2, 3), ([2, 0, 1], [True, False, True]), -1), ((4, 5, 6), poststep.IDENTITY, 1)], "cpu")
    assert t.numpy().view(np.int32).reshape(2, 10).tolist() == [[1, -2, 3, 2, 0, 1, 1, 0, 1, -1], [4, 5, 6, 0, 1, 2, 0, 0, 0, 1]]


def test_predictor_surface():
    from nas_3d_unet_amd import predict, train
    from nas_3d_unet_amd._lib import N3DError
    assert callable(train.Trainer.predictor)
    with pytest.raises(N3DError):
        predict.SubjectPredictor(None, 16, 65)
    sp = predict.SubjectPredictor(None, 16, 5, graph=False)
    assert vars(sp.stats) == dict(entries=0, live=0, chunks=0, captures=0, replays=0, forwards=0)
