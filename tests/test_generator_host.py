"""CPU: the generator's epoch logic (nas_3d_unet_amd.generator) against the reference's own Generator class, run by
tests/golden/make_golden_generator.py into generator.npz.  Fed qualification flags computed by brute force in numpy (every candidate
cropped with oracle.data_step.crop_zero_pad), the host functions reproduce every recorded epoch from the recorded seed: the drawn
overlaps, steps_per_epoch, and each batch as its (volume, corner, key) sequence.  Constructor validation needs no device."""
import json
import random

import numpy as np
import pytest

import make_golden_generator as mg
from oracle import data_step as ds


def brute_flags(volumes, cand, P, with_truth):
    """add_data's two tests (generator.py:202-207) per candidate: bit 0 = not np.all(data == 0), bit 1 = not np.all(truth == 0)"""
    flags = np.zeros(len(cand), np.uint8)
    for n, (v, cx, cy, cz) in enumerate(cand):
        vol, truth = volumes[v]
        f = int(not np.all(ds.crop_zero_pad(vol, (cx, cy, cz), P) == 0))
        if with_truth:
            f |= int(not np.all(ds.crop_zero_pad(truth, (cx, cy, cz), P) == 0)) << 1
        flags[n] = f
    return flags


def _cases(golden):
    g = golden("generator")
    for i in range(len(mg.generator_cases())):
        yield g, "case%d" % i, json.loads(str(g["case%d/config" % i]))


def _key_row(key):
    return [-1] * 6 if key is None else [key[0][0], key[0][1], key[1], key[2], key[3], key[4]]


def test_epoch_order_reproduces_the_reference_generator(golden):
    from nas_3d_unet_amd import generator as G
    volumes = mg.generator_volumes()
    boxes = [v.shape[1:] for v, _ in volumes]
    n_cases = 0
    for g, k, cfg in _cases(golden):
        kw = cfg["kwargs"]
        P, B, po = kw["patch_shape"], kw["batch_size"], kw["patch_overlap"]
        with_truth = cfg["truth"]
        skip = kw.get("skip_health", True) and with_truth
        rng = random.Random(cfg["seed"])
        overlaps = [G.draw_overlap(po, rng)]                         # Generator.__init__ -> epoch_init
        for e in range(cfg["epochs"]):
            cand = G.candidate_table(boxes, kw["indices_list"], P, overlaps[-1], kw.get("both_ps", False))
            flags = brute_flags(volumes, cand, P, with_truth)
            kept = int(G.kept_mask(flags, skip).sum())
            assert -(-kept // B) == int(g[k + "/spe"][e]), (cfg["name"], e)
            rows = []
            for b, batch in enumerate(G.epoch_order(flags, B, rng, skip, kw.get("shuffle_index_list", True), kw.get("permute", False))):
                assert 1 <= len(batch) <= B
                rows += [[b, *cand[i].tolist(), *_key_row(key)] for i, key in batch]
            assert len(rows) == kept
            np.testing.assert_array_equal(np.asarray(rows, np.int32).reshape(-1, 11), g[k + "/epoch%d/rows" % e], err_msg=cfg["name"])
            if po:
                overlaps.append(G.draw_overlap(po, rng))             # the end of epoch(): epoch_init again
        rec = [None if o < 0 else int(o) for o in g[k + "/overlap"]]
        assert overlaps == rec[:len(overlaps)] and all(o == rec[-1] for o in rec[len(overlaps):]), (cfg["name"], overlaps, rec)
        n_cases += 1
    assert n_cases == len(mg.generator_cases())


def test_the_fixture_exercises_both_filters(golden):
    """some candidate of the recorded configurations is dropped as empty, some as healthy, and batches end short"""
    from nas_3d_unet_amd import generator as G
    volumes = mg.generator_volumes()
    boxes = [v.shape[1:] for v, _ in volumes]
    cand = G.candidate_table(boxes, [0, 1, 2, 3], 8, None)
    flags = brute_flags(volumes, cand, 8, True)
    assert (flags == 0).any() and (flags == 1).any() and (flags == 3).any()
    remainders = 0
    for g, k, cfg in _cases(golden):
        rows = g[k + "/epoch0/rows"]
        remainders += int(len(rows) % cfg["kwargs"]["batch_size"] != 0)
    assert remainders >= 2


def test_permutation_keys_keep_the_reference_set_order():
    """augment.py:95-100 draws from list(set(...)), not from the sorted list datastep.random_permutation_key uses"""
    from nas_3d_unet_amd import datastep, generator as G
    assert G.KEYS == list(datastep.generate_permutation_keys()) and len(G.KEYS) == 48
    assert G.KEYS != sorted(G.KEYS)


class _NoVolumes:
    """stands in for a VolumeSet where validation must fail before any volume is touched"""

    def box(self, i):
        raise AssertionError("touched a volume")

    def __len__(self):
        raise AssertionError("touched the set")


class _TopDraw:
    """an rng whose randint always draws the largest overlap the configuration allows"""

    def randint(self, a, b):
        return b


def test_constructor_validation_without_a_device():
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd._lib import N3DError
    with pytest.raises(NotImplementedError):
        G.Generator([0], _NoVolumes(), 8, augment=True)
    with pytest.raises(N3DError):
        G.Generator([0], _NoVolumes(), 8, labels=[1, 2])
    with pytest.raises(N3DError):
        G.Generator([0], _NoVolumes(), (8, 8, 10))
    with pytest.raises(N3DError):
        G.Generator([0], _NoVolumes(), 8, batch_size=65)
    # the reference's search configuration (patch 64, patch_overlap 64) can draw overlap 64: its np.mgrid divides by zero
    with pytest.raises(N3DError, match="divides by zero"):
        G.Generator([0], _NoVolumes(), 64, patch_overlap=64, rng=_TopDraw())
    with pytest.raises(N3DError):
        G.Generator([0], _NoVolumes(), 8, patch_overlap=9, rng=_TopDraw())
    with pytest.raises(N3DError):
        G.VolumeSet("cpu")                      # no CPU fallback


def test_overlap_draws_follow_the_reference():
    """generator.py:127: None and 0 draw nothing (0 still selects the fixed-overlap strategy); a positive int draws randint(0, n)"""
    from nas_3d_unet_amd import generator as G
    rng = random.Random(3)
    state = rng.getstate()
    assert G.draw_overlap(None, rng) is None and G.draw_overlap(0, rng) == 0 and rng.getstate() == state
    ref = random.Random(3)
    assert [G.draw_overlap(5, rng) for _ in range(20)] == [ref.randint(0, 5) for _ in range(20)]
    box = [(30, 30, 30)]
    fixed, auto = G.candidate_table(box, [0], 8, 0), G.candidate_table(box, [0], 8, None)
    assert tuple(fixed[0, 1:]) == (11, 11, 11) and tuple(auto[-1, 1:]) == (11, 11, 11) and not np.array_equal(fixed, auto)
