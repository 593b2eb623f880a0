"""CPU: the rotation / linear interpolation / intensity options of the generator (nas_3d_unet_amd.generator: rotation_matrix,
warp_transform, draw_warp, epoch_order(warp=...), the Generator's new arguments) and the numpy statement of the device rule of
n3d_patch_gather_warp (tests/_warp_ref.py) against scipy.ndimage.affine_transform's recorded answers (tests/golden/warp.npz, written
by make_golden_warp.py).  No scipy and no device here."""
import inspect
import random

import numpy as np
import pytest
import torch

import _augment_ref as ar
import _warp_ref as wr
import make_golden_augment as mga
import make_golden_generator as mg
import make_golden_warp as mgw
from test_generator_host import _NoVolumes, brute_flags


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def test_helper_equals_scipy_on_the_fixture(golden):
    """order 0 and the labels with ==; order 1 to one float32 step (the two fp64 results differ by some 1e-13: scipy multiplies the
    sample by the three weights in turn, the rule multiplies the weights first), at most 1 voxel in 1000 differing at all"""
    recs = wr.records(golden("warp"))
    names = [c["name"] for c, *_ in recs]
    assert sum(n.startswith("rotation_") for n in names) >= 4 and sum(n.startswith("rotated_") for n in names) >= 6
    assert sum(n.startswith("zoom_") for n in names) >= 8 and names.count("quarter_turn") >= 3 and names.count("threshold") >= 3
    differ = total = interpolated = 0
    for cfg, k, x0, x1, y in recs:
        P = cfg["P"]
        data, truth = mgw.warp_inputs(P)
        h0, h1, hy = wr.warp_patch(data, cfg["mode"], k, 0), wr.warp_patch(data, cfg["mode"], k, 1), wr.warp_patch(truth, cfg["mode"], k, 0)
        assert h0.dtype == np.float32 and h1.dtype == np.float32 and hy.dtype == np.uint8
        assert np.array_equal(h0, x0) and np.array_equal(hy, y), cfg["name"]
        assert wr.one_step(h1, x1).all(), cfg["name"]
        differ += int((h1 != x1).sum())
        total += h1.size
        interpolated += int((x1 != np.round(x1)).sum())
        if cfg["name"] == "quarter_turn":                # every coordinate an integer: a permutation of the input, nothing lost
            assert np.array_equal(h1, h0) and np.array_equal(np.sort(h0[0].reshape(-1)), np.arange(1, P ** 3 + 1))
    assert differ * 1000 <= total and interpolated > total // 4


def test_the_fixture_separates_the_two_summation_orders(golden):
    """the matrix rule adds the products in axis order and the offset last: on the `order` cases the offset-first sum picks another
    voxel (or another inside / outside answer) somewhere, and scipy's recorded answer is the axis-order one"""
    recs = [r for r in wr.records(golden("warp")) if r[0]["name"] == "order"]
    assert len(recs) >= 2
    for cfg, k, x0, _, _ in recs:
        P = cfg["P"]
        j = [g.astype(np.float64) for g in np.meshgrid(*[np.arange(P)] * 3, indexing="ij")]
        other = np.stack([((k[9 + a] + k[3 * a] * j[0]) + k[3 * a + 1] * j[1]) + k[3 * a + 2] * j[2] for a in range(3)])
        c = wr.coordinates(P, 1, k)
        ok = np.all((0 <= c) & (c <= P - 1), axis=0)
        ok2 = np.all((0 <= other) & (other <= P - 1), axis=0)
        src = np.where(ok, ((np.floor(c[0] + 0.5) * P + np.floor(c[1] + 0.5)) * P + np.floor(c[2] + 0.5)) + 1, 0)
        src2 = np.where(ok2, ((np.floor(other[0] + 0.5) * P + np.floor(other[1] + 0.5)) * P + np.floor(other[2] + 0.5)) + 1, 0)
        assert np.array_equal(src, x0[0]) and not np.array_equal(src2, x0[0])


def test_host_functions_equal_their_restatements():
    from nas_3d_unet_amd import generator as G
    rs = np.random.RandomState(17)
    for n in range(40):
        angles = rs.uniform(-30, 30, 3) if n else np.zeros(3)
        R = G.rotation_matrix(angles)
        assert R.dtype == np.float64 and np.array_equal(_bits(R), _bits(wr.rotation_matrix(angles)))
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(R) - 1) < 1e-15
        P = int(rs.randint(5, 13))
        A, b = (rs.normal(1, 0.25, 3), rs.normal(0, 1, 3)) if n % 3 else (np.ones(3), np.zeros(3))
        M, off = G.warp_transform(A, b, R, P)
        M2, off2 = wr.warp_transform(A, b, R, P)
        assert np.array_equal(_bits(M), _bits(M2)) and np.array_equal(_bits(off), _bits(off2))
    # no angle: the identity, exactly; the centre (P - 1) / 2 is a fixed point of a rotation alone
    assert np.array_equal(G.rotation_matrix((0, 0, 0)), np.eye(3))
    M, off = G.warp_transform(np.ones(3), np.zeros(3), np.eye(3), 9)
    assert np.array_equal(M, np.eye(3)) and np.array_equal(off, np.zeros(3))
    M, off = G.warp_transform(np.ones(3), np.zeros(3), G.rotation_matrix((10, -20, 5)), 9)
    assert np.allclose(M @ np.full(3, 4.0) + off, 4.0, atol=1e-14)
    # a quarter turn about axis 2 maps output axis 0 onto -axis 1
    assert np.allclose(G.rotation_matrix((0, 0, 90)), [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-16)


class _Recorder:
    """an np.random-like object that notes the calls made on it"""

    def __init__(self, seed):
        self.rs, self.calls = np.random.RandomState(seed), []

    def __getattr__(self, name):
        fn = getattr(self.rs, name)

        def call(*a):
            self.calls.append((name,) + tuple(np.asarray(x).tolist() if isinstance(x, np.ndarray) else x for x in a))
            return fn(*a)
        return call


def test_draw_warp_makes_the_stated_calls_in_order():
    from nas_3d_unet_amd import generator as G
    a, b = _Recorder(23), np.random.RandomState(23)
    angles, gain, bias = G.draw_warp(a, 15, 0.1, 0.2, 4)
    assert a.calls == [("uniform", -15.0, 15.0, 3), ("uniform", 0.9, 1.1, 4), ("normal", 0, 0.2, 4)]
    assert np.array_equal(_bits(angles), _bits(b.uniform(-15, 15, 3))) and np.array_equal(_bits(gain), _bits(b.uniform(0.9, 1.1, 4)))
    assert np.array_equal(_bits(bias), _bits(b.normal(0, 0.2, 4)))
    # per-axis maxima; an option that is None draws nothing
    a, b = _Recorder(24), np.random.RandomState(24)
    angles, gain, bias = G.draw_warp(a, (10.0, 0.0, 5.0), None, 0.3, 2)
    assert [c[0] for c in a.calls] == ["uniform", "normal"] and gain is None and angles[1] == 0.0
    assert np.array_equal(_bits(angles), _bits(b.uniform([-10.0, -0.0, -5.0], [10.0, 0.0, 5.0], 3)))
    assert np.array_equal(_bits(bias), _bits(b.normal(0, 0.3, 2)))
    a = _Recorder(25)
    assert G.draw_warp(a, None, None, None, 4) == (None, None, None) and a.calls == []
    a, b = _Recorder(26), np.random.RandomState(26)
    assert G.draw_warp(a, None, 0.25, None, 3)[1].shape == (3,) and a.calls == [("uniform", 0.75, 1.25, 3)]


class _HostVolumes:
    """a volume set on the host that answers the generator's questions and records the batches it is asked for"""

    def __init__(self, volumes, with_warp=True):
        self.vols = volumes
        self.channels, self.has_truth = volumes[0][0].shape[0], True
        self.batches = []
        if not with_warp:
            self.patch_batch = self._patch_batch_without_warp

    def __len__(self):
        return len(self.vols)

    def box(self, i):
        return self.vols[i][0].shape[1:]

    def qualify_table(self, table, patch):
        return torch.from_numpy(brute_flags(self.vols, table, patch, True))

    def fits(self, out, B, patch, target_dtype):
        return False

    def patch_batch(self, refs, patch, inclusive_label=False, target_dtype=torch.float32, out=None, augment=None, warp=None):
        self.batches.append((refs, augment, warp))
        return len(self.batches), None

    def _patch_batch_without_warp(self, refs, patch, inclusive_label=False, target_dtype=torch.float32, out=None, augment=None):
        self.batches.append((refs, augment, None))
        return len(self.batches), None


def _rows_of(cand_batches, epoch):
    rows, scales = [], []
    for b, (refs, augs, _) in enumerate(cand_batches):
        for (v, corner, key), (A, sh, identity, axes) in zip(refs, augs):
            k = [-1] * 6 if key is None else [key[0][0], key[0][1], key[1], key[2], key[3], key[4]]
            rows.append([epoch, b, int(v), *[int(c) for c in corner], *k, *[int(a in (axes or [])) for a in range(3)]])
    return np.asarray(rows, np.int32).reshape(-1, 15)


def test_with_the_new_options_at_their_defaults_nothing_changes(golden):
    """a generator record of augment.npz replayed: the same draws from both random sources in the same order, three-element batch
    entries, and patch_batch called without a warp -- through epoch_order and through the Generator"""
    from nas_3d_unet_amd import generator as G
    cfg, rows, scales, _, _ = ar.generator_records(golden("augment"))[0]
    kw = cfg["kwargs"]
    assert kw["augment"] and kw["permute"] and cfg["epochs"] == 2
    volumes = mg.generator_volumes()
    for with_warp in (True, False):                      # a stand-in without `warp` still serves a generator that does not need it
        s = _HostVolumes(volumes, with_warp)
        np_rng = _Recorder(cfg["np_seed"])
        gen = G.Generator(volumes=s, labels=[1, 2, 4], rng=random.Random(cfg["seed"]), np_rng=np_rng, affine=mga.AFFINES[cfg["affine"]], **kw)
        assert not gen.warped
        for e in range(cfg["epochs"]):
            s.batches = []
            assert [x for x, _ in gen.epoch()] == list(range(1, cfg["spe"][e] + 1))
            assert all(w is None for _, _, w in s.batches)
            np.testing.assert_array_equal(_rows_of(s.batches, e), rows[rows[:, 0] == e])
        assert {c[0] for c in np_rng.calls} == {"normal", "choice"} and len(np_rng.calls) == 4 * len(rows)
    flags = np.array([1, 3, 3, 0, 3], np.uint8)
    plain = list(G.epoch_order(flags, 2, random.Random(3), True, True, True, augment=(np.random.RandomState(4), 0.25, True)))
    same = list(G.epoch_order(flags, 2, random.Random(3), True, True, True, augment=(np.random.RandomState(4), 0.25, True), warp=None))
    assert all(len(e) == 3 for b in plain for e in b) and repr(plain) == repr(same)


def test_epoch_order_with_a_warp_draws_after_the_augmentation_and_before_the_key():
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd._lib import N3DError
    flags = np.array([3, 1, 3, 3, 0, 3, 3], np.uint8)
    np_rng, twin, rng, rng2 = _Recorder(31), np.random.RandomState(31), random.Random(8), random.Random(8)
    batches = list(G.epoch_order(flags, 2, rng, True, True, True, augment=(np_rng, 0.25, True), warp=(np_rng, 15, 0.1, None, 4)))
    assert [len(b) for b in batches] == [2, 2, 1]
    per_patch = ["normal", "choice", "choice", "choice", "uniform", "uniform"]
    assert [c[0] for c in np_rng.calls] == per_patch * 5
    order = list(range(len(flags)))
    rng2.shuffle(order)
    kept = [i for i in reversed(order) if flags[i] == 3]
    for (i, key, (scale, axes), (angles, gain, bias)), want_i in zip([e for b in batches for e in b], kept):
        assert i == want_i
        assert np.array_equal(_bits(scale), _bits(twin.normal(1, 0.25, 3))) and axes == [a for a in range(3) if twin.choice([True, False])]
        assert np.array_equal(_bits(angles), _bits(twin.uniform(-15, 15, 3))) and np.array_equal(_bits(gain), _bits(twin.uniform(0.9, 1.1, 4)))
        assert bias is None and key == rng2.choice(G.KEYS)
    with pytest.raises(N3DError, match="augment"):
        next(G.epoch_order(flags, 2, rng, warp=(np_rng, 15, None, None, 4)))


def test_generator_hands_the_composed_transforms_to_patch_batch():
    """the Generator with every new option set, on a host stand-in: per kept patch the warp entry is (warp_transform of the scale
    map and the drawn rotation, order 1, gain, bias), next to the augment entry it made before"""
    from nas_3d_unet_amd import generator as G
    volumes = mg.generator_volumes()
    s = _HostVolumes(volumes)
    kw = dict(indices_list=[3, 0], patch_shape=8, patch_overlap=3, batch_size=2, permute=True, augment=True, labels=[1, 2, 4],
              affine=mga.BRATS_AFFINE, augment_rotation=(15, 10, 5), augment_interpolation="linear", augment_intensity_scale=0.1,
              augment_intensity_shift=0.2)
    gen = G.Generator(volumes=s, rng=random.Random(35), np_rng=np.random.RandomState(131), **kw)
    assert gen.warped
    rng, twin = random.Random(35), np.random.RandomState(131)
    assert G.draw_overlap(3, rng) == gen.overlap
    order = list(G.epoch_order(gen.flags, 2, rng, True, True, True, augment=(twin, 0.25, True), warp=(twin, (15, 10, 5), 0.1, 0.2, 4)))
    spe, kept = gen.steps_per_epoch, gen.n_patches
    assert len(list(gen.epoch())) == spe == len(order) == len(s.batches)
    n = 0
    for (refs, augs, warps), batch in zip(s.batches, order):
        assert len(refs) == len(batch) == len(augs) == len(warps)
        for (v, corner, key), aug, (matrix, order1, gain, bias), (i, key2, (scale, axes), (angles, g2, b2)) in zip(refs, augs, warps, batch):
            A, b, identity = G.resample_transform(G.check_affine(mga.BRATS_AFFINE), 8, scale)
            M, off = wr.warp_transform(A, b, wr.rotation_matrix(angles), 8)
            assert key == key2 and aug[3] == axes and order1 == 1 and np.all(np.abs(angles) <= (15, 10, 5))
            assert np.array_equal(_bits(matrix[0]), _bits(M)) and np.array_equal(_bits(matrix[1]), _bits(off))
            assert np.array_equal(_bits(gain), _bits(g2)) and np.array_equal(_bits(bias), _bits(b2)) and gain.shape == (4,)
            n += 1
    assert n == kept and n >= 4
    # interpolation alone: a warp entry per patch with no matrix and no intensity, and no further draw
    s2, rec = _HostVolumes(volumes), _Recorder(131)
    kw2 = {k: v for k, v in kw.items() if k not in ("augment_rotation", "augment_intensity_scale", "augment_intensity_shift")}
    gen2 = G.Generator(volumes=s2, rng=random.Random(35), np_rng=rec, **kw2)
    list(gen2.epoch())
    assert all(w == (None, 1, None, None) for _, _, ws in s2.batches for w in ws) and {c[0] for c in rec.calls} == {"normal", "choice"}


def test_warp_constructor_validation_without_a_device():
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd._lib import N3DError
    aff = mga.BRATS_AFFINE
    options = (dict(augment_rotation=15), dict(augment_interpolation="linear"), dict(augment_intensity_scale=0.1),
               dict(augment_intensity_shift=0.1))
    for opt in options:
        # no silent no-op without augment, and the cap of 16, both before any volume is touched or any draw made
        with pytest.raises(N3DError, match="augment=True"):
            G.Generator([0], _NoVolumes(), 8, **opt)
        with pytest.raises(N3DError, match="N3D_PATCH_WARP_MAX_BATCH"):
            G.Generator([0], _NoVolumes(), 8, augment=True, affine=aff, batch_size=17, **opt)
        # a stand-in whose patch_batch takes `augment` but no `warp`
        np_rng = _Recorder(1)
        with pytest.raises(NotImplementedError, match="warp"):
            G.Generator([0], _HostVolumes(mg.generator_volumes(), with_warp=False), 8, augment=True, affine=aff, np_rng=np_rng, **opt)
        assert np_rng.calls == []
    assert "warp" in inspect.signature(G.VolumeSet.patch_batch).parameters and G.WARP_MAX_BATCH == 16
    with pytest.raises(N3DError, match="interpolation"):
        G.Generator([0], _NoVolumes(), 8, augment=True, affine=aff, augment_interpolation="cubic")
    with pytest.raises(N3DError, match="augment_rotation"):
        G.Generator([0], _NoVolumes(), 8, augment=True, affine=aff, augment_rotation=(1, 2))
    with pytest.raises(N3DError, match="augment_intensity_shift"):
        G.Generator([0], _NoVolumes(), 8, augment=True, affine=aff, augment_intensity_shift=-1.0)
    # batch_size 17..32 stays legal for the reference's augmentation alone (the volumes are touched only after the checks)
    with pytest.raises(NotImplementedError, match="patch_batch"):
        G.Generator([0], _NoVolumes(), 8, augment=True, affine=aff, batch_size=32)
    # intensity on a set with more than 4 channels
    wide = _HostVolumes([(np.ones((5, 9, 9, 9), np.float32), np.ones((1, 9, 9, 9), np.uint8))])
    for opt in options[2:]:
        with pytest.raises(N3DError, match="at most 4 channels"):
            G.Generator([0], wide, 8, augment=True, affine=aff, **opt)
    assert G.Generator([0], wide, 8, augment=True, affine=aff, augment_rotation=5, augment_interpolation="linear").warped


def test_the_abi_declares_the_export_and_the_descriptor_fits_the_kernel_arguments():
    import ctypes as C
    import os
    import re
    from nas_3d_unet_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "n3d.h")).read()
    assert re.search(r"\bn3d_patch_gather_warp\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "n3d_patch_gather_warp" in _lib.PROTOTYPES
    cap = int(re.search(r"#define N3D_PATCH_WARP_MAX_BATCH (\d+)", hdr).group(1))
    assert cap == 16 and C.sizeof(_lib.WarpDesc) == 192 and _lib.WarpDesc.k.offset % 8 == 0
    assert cap * C.sizeof(_lib.WarpDesc) + 64 <= 4096
