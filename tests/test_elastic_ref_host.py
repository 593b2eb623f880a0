"""CPU: the numpy statement of n3d_patch_gather_elastic's rule (tests/_elastic_ref.py) against tests/golden/elastic.npz -- scipy's
map_coordinates on float64, recorded -- and against an independent evaluation of the field (scipy.interpolate.BSpline); the field's
properties; the host side of nas_3d_unet_amd.elastic: the validation, the folding bound, the draws and their order in epoch_order;
the descriptor's layout."""
import os
import random
import re

import numpy as np
import pytest

import _elastic_ref as er
import _warp_ref as wr
import make_golden_elastic as mge
from test_appearance_ref_host import _Recording

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def test_the_fixture_holds_the_stated_cases_and_a_field_that_does_something(golden):
    """the cases the generator lists, and on each: in every case with amp >= 1.5 and cells <= 4 at least 20 % of the voxels take
    another nearest source voxel than without the field; in every case fewer than 50 % of the voxels have no source"""
    recs = er.records(golden("elastic"))
    have = {(c["P"], c["cells"], c["lock"], tuple(c["amp"])) for c, *_ in recs}
    assert have >= {(8, 1, 0, (1.5,) * 3), (12, 2, 0, (2.0,) * 3), (12, 3, 2, (1.5,) * 3), (16, 4, 3, (1.8,) * 3), (16, 8, 0, (0.9,) * 3),
                    (12, 2, 0, (2.0, 0.0, 1.0))}
    assert {c["mode"] for c, *_ in recs} == {0, 1} and any(any(c["flips"]) for c, *_ in recs) and any(any(c["corner"]) for c, *_ in recs)
    checked = 0
    for c, k, *_ in recs:
        P = c["P"]
        c0, c1 = er.coordinates(P, c["mode"], k), er.coordinates(P, c["mode"], k, er.case_elastic(c))
        ok0, ok1 = (np.all((0.0 <= x) & (x <= P - 1.0), axis=0) for x in (c0, c1))
        moved = np.mean(np.any(np.floor(c0 + 0.5) != np.floor(c1 + 0.5), axis=0) | (ok0 != ok1))
        assert np.mean(~ok1) < 0.5, c["name"]
        if min(c["amp"]) >= 1.5 and c["cells"] <= 4:
            assert moved >= 0.2, (c["name"], moved)
            checked += 1
    assert checked >= 5


def test_restatement_equals_scipys_recorded_answers(golden):
    """order 0 data and the labels with ==, order 1 within one float32 step (the warp fixture's bound); no voxel is excluded"""
    for c, k, x0, x1, y in er.records(golden("elastic")):
        data, truth = mge.case_inputs(c)
        el, flips = er.case_elastic(c), c["flips"]
        assert np.array_equal(er.elastic_patch(data, c["mode"], k, el, 0, flips), x0), c["name"]
        assert np.array_equal(er.elastic_patch(truth, c["mode"], k, el, 0, flips), y), c["name"]
        h1 = er.elastic_patch(data, c["mode"], k, el, 1, flips)
        assert h1.dtype == np.float32 and wr.one_step(h1, x1).all(), c["name"]
        # and the field is what makes the answer: without it the patch is another one
        assert not np.array_equal(er.elastic_patch(data, c["mode"], k, None, 0, flips), x0), c["name"]


def _bspline_field(P, cells, lock, key, amp):
    """the same field by scipy.interpolate.BSpline: a tensor product of cubic splines on the uniform knots -3 .. cells + 3"""
    from scipy.interpolate import BSpline
    D = er.lattice(cells, lock, key)
    t = np.arange(-3, cells + 4).astype(np.float64)
    s = np.arange(P).astype(np.float64) * er.inv_h(cells, P)
    amp = np.broadcast_to(np.asarray(amp, np.float64), (3,))
    out = []
    for a in range(3):
        v = D[a]
        for _ in range(3):                                  # evaluate along the leading axis, then rotate it to the back
            v = np.moveaxis(BSpline(t, v, 3)(s), 0, -1)
        out.append(amp[a] * v)
    return np.stack(out)


def test_field_equals_an_independent_bspline_evaluation(golden):
    """bound 128 * eps * amp: at most 64 non-negative weights summing to 1 on values within [-1, 1], each term and each add rounded
    once, on either side"""
    cases = [er.case_elastic(c) + (c["P"],) for c, *_ in er.records(golden("elastic"))]
    cases += [(5, 1, (7, 9), 2.0, 33), (7, 0, (1, 2), (0.5, 1.0, 1.5), 26), (8, 3, (3, 4), 1.0, 50)]     # P - 1 = 49: (P - 1) * inv_h != n
    worst = 0.0
    for cells, lock, key, amp, P in cases:
        f = er.field(P, cells, lock, key, amp)
        g = _bspline_field(P, cells, lock, key, amp)
        a3 = np.broadcast_to(np.asarray(amp, np.float64), (3,))[:, None, None, None]
        assert (np.abs(f - g) <= 128 * EPS * a3).all(), (cells, lock, P)
        assert (np.abs(f) <= a3).all()                                           # the convex hull
        worst = max(worst, float(np.abs(f - g).max()))
        if max(np.ravel(amp)) > 0 and cells + 3 - 2 * lock >= 1:
            assert np.abs(f).max() > 0
    print("largest |field - BSpline| %.3g" % worst)


def test_lattice_values_lock_and_weights():
    key = (0xA4093822, 0x299F31D0)
    for cells, lock in ((1, 0), (1, 1), (4, 2), (4, 3), (8, 3), (5, 3)):
        G = cells + 3
        D = er.lattice(cells, lock, key)
        assert D.shape == (3, G, G, G) and (D >= -1).all() and (D < 1).all()
        inner = D[:, lock:G - lock, lock:G - lock, lock:G - lock]
        assert inner.size == 3 * (G - 2 * lock) ** 3 and (inner != 0).all()
        assert np.count_nonzero(D) == inner.size and not np.signbit(D[D == 0]).any()
        # the counter is (l, 1, 0, 0): word a of lattice point l
        l = ((G - lock - 1) * G + lock) * G + lock
        w = er.ap.philox4x32_10((l, 1, 0, 0), key)
        assert D[1, G - lock - 1, lock, lock] == 2.0 * (w[1] / 2.0 ** 32) - 1.0
    f = np.concatenate((np.linspace(0, 1, 1001), np.random.default_rng(3).uniform(0, 1, 5000)))
    b = er.weights(f)
    assert (b >= 0).all() and (np.abs(((b[0] + b[1]) + b[2]) + b[3] - 1.0) <= 4 * EPS).all()
    assert er.weights(0.0).tolist() == [er.SIXTH, 4.0 * er.SIXTH, er.SIXTH, 0.0] and er.weights(1.0)[0] == 0.0
    for P in (2, 8, 12, 16, 25, 50, 64, 128):
        for cells in range(1, 9):
            cell, bw = er.cells_and_weights(P, cells)
            assert cell.min() == 0 and cell.max() == cells - 1 and (np.diff(cell) >= 0).all()
            assert (bw > -1e-40).all() and (np.abs(bw.sum(axis=0) - 1.0) <= 4 * EPS).all()


def test_lock_3_holds_the_faces_and_zero_amp_changes_nothing(golden):
    key = (11, 12)
    for P, cells in ((16, 4), (12, 5), (9, 8), (25, 7)):
        f = er.field(P, cells, 3, key, 1.0)
        face = np.zeros((P, P, P), bool)
        face[[0, -1]] = face[:, [0, -1]] = face[:, :, [0, -1]] = True
        assert np.abs(f).max() > 0.01 and (f[:, face] == 0).all() and (f[:, ~face] != 0).any()
    for c, k, *_ in er.records(golden("elastic")):
        data, truth = mge.case_inputs(c)
        P, el = c["P"], er.case_elastic(c)
        zero = el[:3] + (0.0,)
        for order in (0, 1):
            plain = er.elastic_patch(data, c["mode"], k, None, order, c["flips"])
            assert np.array_equal(plain.view(np.uint32), er.elastic_patch(data, c["mode"], k, zero, order, c["flips"]).view(np.uint32))
            assert np.array_equal(plain, wr.warp_patch(data, c["mode"], k, order, c["flips"]))
            if c["lock"] == 3:
                face = np.zeros((P, P, P), bool)
                face[[0, -1]] = face[:, [0, -1]] = face[:, :, [0, -1]] = True
                moved = er.elastic_patch(data, c["mode"], k, el, order, c["flips"])
                assert np.array_equal(moved[:, face], plain[:, face]) and not np.array_equal(moved, plain)


def test_elastic_validation_and_the_folding_bound():
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.elastic import Elastic
    for kw in (dict(cells=0), dict(cells=9), dict(cells=2.0), dict(lock=-1), dict(lock=4), dict(cells=1, lock=2), dict(cells=2, lock=3),
               dict(p=-0.1), dict(p=1.5), dict(p=float("nan")), dict(displacement=-1.0), dict(displacement=float("inf")),
               dict(displacement=(1.0, 2.0)), dict(displacement=(1.0, float("nan"), 1.0)), dict(displacement="much")):
        with pytest.raises(N3DError):
            Elastic(**kw)
    e = Elastic()
    assert (e.cells, e.lock, e.p) == (4, 2, 0.2) and len(e.amp) == 3
    e = Elastic(cells=3, displacement=(2.0, 0.0, 1.0), p=1, lock=2)
    assert e.amp == (2.0, 0.0, 1.0) and e.entry(None) is None and e.entry((5, 6)) == (3, 2, (5, 6), (2.0, 0.0, 1.0))
    # the map does not fold for displacement < (P - 1) / (2 * cells): P = 13 gives exactly 2.0, which is refused; P = 14 passes
    e.check(14)
    with pytest.raises(N3DError, match=r"\(13 - 1\) / \(2 \* 3\) = 2"):
        e.check(13)
    Elastic(cells=1, displacement=1.5, lock=0).check(8)
    with pytest.raises(N3DError, match="fold"):
        Elastic(cells=8, displacement=1.0, lock=0).check(16)
    Elastic(cells=8, displacement=0.9, lock=0).check(16)
    # below the bound the restated field's slope stays below 1 along every axis: j + delta_a(j) is increasing in j_a
    for cells, amp, P in ((1, 3.4, 8), (4, 1.8, 16), (8, 0.9, 16)):
        Elastic(cells=cells, displacement=amp, lock=0).check(P)
        f = er.field(P, cells, 0, (21, 22), amp)
        assert all((np.diff(f[a], axis=a) > -1.0).all() for a in range(3))


def test_draw_makes_the_stated_calls():
    from nas_3d_unet_amd.elastic import Elastic
    e = Elastic(cells=2, displacement=1.0, p=0.5, lock=0)
    r = _Recording(1, uniforms=[0.49])
    key = e.draw(r)
    assert r.calls == [("uniform",), ("randint", 0, 2 ** 32, 2, np.uint32)]
    assert isinstance(key, tuple) and len(key) == 2 and all(isinstance(k, int) and 0 <= k < 2 ** 32 for k in key)
    r = _Recording(1, uniforms=[0.5])                          # a value equal to p is not active: no key is drawn
    assert e.draw(r) is None and r.calls == [("uniform",)]
    assert Elastic(p=0).draw(_Recording(2)) is None and Elastic(p=1).draw(_Recording(2)) is not None


def test_epoch_order_is_todays_without_the_keyword_and_inserts_the_draws_with_it():
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.appearance import Appearance
    from nas_3d_unet_amd.elastic import Elastic
    flags = np.array([3, 1, 3, 0, 3, 3, 2, 3, 3], np.uint8)
    warp = (15, 0.1, 0.1, 4)

    def order(np_rng, **kw):
        return list(G.epoch_order(flags, 2, random.Random(5), True, True, True, augment=(np_rng, 0.25, True), **kw))

    a = Appearance(contrast=(0.7, 1.3), p_contrast=1.0)
    r0, r1 = _Recording(9), _Recording(9)
    base = order(r0, warp=(r0,) + warp, appearance=(r0, a, 4))
    same = order(r1, warp=(r1,) + warp, appearance=(r1, a, 4), elastic=None)
    assert repr(base) == repr(same) and r0.calls == r1.calls and all(len(e) == 5 for b in base for e in b)
    per_patch = ["normal", "choice", "choice", "choice", "uniform", "uniform", "normal"]
    # with it: after draw_warp's calls and before Appearance.draw's; the element sits before the appearance one
    e = Elastic(cells=2, displacement=1.0, p=1.0, lock=0)
    r2 = _Recording(9)
    got = order(r2, warp=(r2,) + warp, appearance=(r2, a, 4), elastic=(r2, e))
    assert [[x[:2] for x in b] for b in got] == [[x[:2] for x in b] for b in base]
    assert all(len(x) == 6 and isinstance(x[4], tuple) and len(x[4]) == 2 and list(x[5]) == ["contrast"] for b in got for x in b)
    assert [c[0] for c in r2.calls] == (per_patch + ["uniform", "randint", "uniform", "uniform"]) * 6
    assert r2.calls[7:11] == [("uniform",), ("randint", 0, 2 ** 32, 2, np.uint32), ("uniform",), ("uniform", 0.7, 1.3, 4)]
    # a patch that is not deformed draws no key and carries None
    r3 = _Recording(9)
    got = order(r3, warp=(r3,) + warp, elastic=(r3, Elastic(p=0.0)))
    assert all(len(x) == 5 and x[4] is None for b in got for x in b)
    assert [c[0] for c in r3.calls] == (per_patch + ["uniform"]) * 6
    # without warp the draws follow draw_augment's
    r4 = _Recording(9)
    got = order(r4, elastic=(r4, e), appearance=(r4, a, 2))
    assert all(len(x) == 5 and len(x[3]) == 2 and x[4]["contrast"].shape == (2,) for b in got for x in b)
    assert [c[0] for c in r4.calls] == (["normal", "choice", "choice", "choice", "uniform", "randint", "uniform", "uniform"]) * 6
    with pytest.raises(N3DError, match="needs augment"):
        list(G.epoch_order(flags, 2, random.Random(5), elastic=(r4, e)))


def test_abi_surface_and_descriptor_layout():
    import ctypes as C
    import inspect
    from nas_3d_unet_amd import _lib, elastic, generator
    hdr = open(os.path.join(ROOT, "include", "n3d.h")).read()
    assert "n3d_patch_gather_elastic" in _lib.PROTOTYPES
    assert re.search(r"#define N3D_PATCH_ELASTIC_MAX_BATCH 8\b", hdr) and re.search(r"#define N3D_PATCH_ELASTIC_MAX_CELLS 8\b", hdr)
    assert elastic.MAX_BATCH == generator.ELASTIC_MAX_BATCH == 8 and elastic.MAX_CELLS == er.MAX_CELLS == 8
    E = _lib.ElasticDesc
    assert C.sizeof(_lib.WarpDesc) == 192 and C.sizeof(E) == 248 and 8 * C.sizeof(E) + 64 <= 4096 < 16 * C.sizeof(E) + 160
    assert [(n, getattr(E, n).offset) for n, _ in E._fields_] == [("w", 0), ("elastic", 192), ("cells", 196), ("lock", 200), ("key", 204),
                                                                 ("pad_", 212), ("amp", 216), ("inv_h", 240)]
    assert hasattr(_lib.load(), "n3d_patch_gather_elastic")
    assert "elastic" in inspect.signature(generator.VolumeSet.patch_batch).parameters
    assert inspect.signature(generator.Generator.__init__).parameters["augment_elastic"].default is None
