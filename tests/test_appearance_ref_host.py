"""CPU: the numpy statement of n3d_patch_appearance's rule (tests/_appearance_ref.py) against tests/golden/appearance.npz -- scipy's
gaussian_filter and plain numpy on float64, recorded -- and the host side of nas_3d_unet_amd.appearance: the draws and their order,
the validation, the blur weights, and epoch_order with and without the new keyword."""
import json
import os
import random
import re

import numpy as np
import pytest

import _appearance_ref as ap
import make_golden_appearance as mga

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_known_answers():
    kat = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for counter, key, want in kat:
        assert " ".join("%08x" % w for w in ap.philox4x32_10(counter, key)) == want
    # the vectorised form the helper's noise uses is the same function
    key = (0xA4093822, 0x299F31D0)
    words = ap.philox_voxels(300, key)
    for v in (0, 1, 77, 299):
        assert tuple(int(w[v]) for w in words) == ap.philox4x32_10((v, 0, 0, 0), key)


def test_helper_equals_the_fixture(golden):
    g = golden("appearance")
    cases = json.loads(str(g["config"]))["cases"]
    assert [c["P"] for c in cases] == [7, 12, 16, 20] and {c["Cv"] for c in cases} == {1, 3, 4}
    tol = {"noise": float(g["tol/noise"]), "gamma": float(g["tol/gamma"])}
    assert 0 <= tol["noise"] <= 2 and 0 <= tol["gamma"] <= 2
    for case in cases:
        x = mga.case_input(case)
        mask = ap.entry_mask(x)
        rw = [ap.blur_weights(s) for s in case["blur"]]
        helper = {"noise": ap.noise(x, mask, *case["noise"]), "blur": ap.blur(x, mask, [r for r, _ in rw], [w for _, w in rw]),
                  "contrast": ap.contrast(x, mask, case["contrast"]), "gamma": ap.gamma(x, mask, case["gamma"])}
        for stage, y in helper.items():
            fix = g["%s/%s" % (case["name"], stage)]
            assert y.dtype == np.float32 and (y[~mask] == 0).all() and not np.array_equal(y, x)
            if stage in tol:
                assert mga.channel_steps(y, fix) <= tol[stage], (case["name"], stage)
            else:
                assert (np.abs(y.astype(np.float64) - fix) <= np.spacing(np.abs(fix))).all(), (case["name"], stage)
        # chained, the stages see what the earlier ones left and the mask of the entry
        draw = dict(noise=tuple(case["noise"]), blur=case["blur"], contrast=case["contrast"], gamma=case["gamma"])
        y = ap.apply_draw(x, draw)
        assert np.isfinite(y).all() and (y[~mask] == 0).all()
        assert np.array_equal(y, ap.gamma(ap.contrast(helper_blur_after_noise(x, mask, case, rw), mask, case["contrast"]), mask, case["gamma"]))


def helper_blur_after_noise(x, mask, case, rw):
    return ap.blur(ap.noise(x, mask, *case["noise"]), mask, [r for r, _ in rw], [w for _, w in rw])


def test_blur_weights_are_scipys_and_the_fold_is_a_sum():
    from nas_3d_unet_amd import appearance as A
    for sigma in (0.12, 0.3, 0.5, 1.0, 1.3, 1.5, 1.62):
        r, w = A.blur_weights(sigma)
        r2, w2 = ap.blur_weights(sigma)
        assert r == r2 == int(4 * sigma + 0.5) <= A.MAX_RADIUS and np.array_equal(w, w2) and len(w) == r + 1
        assert abs(w[0] + 2 * w[1:].sum() - 1) < 1e-15
    rs = np.random.RandomState(3)
    a = rs.uniform(-1, 1, 5000)
    assert abs(ap.fixed_sum(a, np.ones(5000, bool)) - a.sum()) < 1e-11 and ap.fold([]) == 0.0
    assert ap.fixed_sum(np.arange(3000.0), np.arange(3000) % 2 == 0) == np.arange(0, 3000, 2).sum()


class _Recording:
    def __init__(self, seed, uniforms=None):
        self.rs, self.calls, self.uniforms = np.random.RandomState(seed), [], list(uniforms or [])

    def uniform(self, *a):
        self.calls.append(("uniform",) + a)
        if not a and self.uniforms:
            return self.uniforms.pop(0)
        return self.rs.uniform(*a)

    def randint(self, *a, **kw):
        self.calls.append(("randint",) + a + (kw.get("dtype"),))
        return self.rs.randint(*a, **kw)

    def normal(self, *a):
        self.calls.append(("normal",) + a)
        return self.rs.normal(*a)

    def choice(self, a):
        self.calls.append(("choice",))
        return self.rs.choice(a)


def test_draw_makes_the_stated_calls_in_the_stated_order():
    from nas_3d_unet_amd.appearance import Appearance
    a = Appearance(noise=0.5, blur=(0.5, 1.5), contrast=(0.65, 1.5), gamma=(0.7, 1.5))
    r = _Recording(1, uniforms=[0.05, 0.1, 0.1, 0.2])                 # all four active (p = 0.1, 0.2, 0.15, 0.3)
    d = a.draw(r, 3)
    assert r.calls == [("uniform",), ("uniform", 0, 0.5), ("randint", 0, 2 ** 32, 2, np.uint32), ("uniform",), ("uniform", 0.5, 1.5, 3),
                       ("uniform",), ("uniform", 0.65, 1.5, 3), ("uniform",), ("uniform", 0.7, 1.5, 3)]
    assert list(d) == ["noise", "blur", "contrast", "gamma"] and 0 <= d["noise"][0] <= 0.5 and len(d["noise"][1]) == 2
    assert all(d[k].shape == (3,) and d[k].dtype == np.float64 for k in ("blur", "contrast", "gamma"))
    r = _Recording(1, uniforms=[0.1, 0.2, 0.15, 0.3])                 # a value equal to p is not active: nothing else is drawn
    assert a.draw(r, 4) == {} and r.calls == [("uniform",)] * 4
    r = _Recording(1, uniforms=[0.9, 0.0])                            # options left None draw nothing at all
    d = Appearance(blur=(0.4, 0.4), gamma=(1.0, 1.2), p_gamma=1.0).draw(r, 2)
    assert r.calls == [("uniform",), ("uniform",), ("uniform", 1.0, 1.2, 2)] and list(d) == ["gamma"]
    assert Appearance().draw(_Recording(1), 4) == {}


def test_validation():
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.appearance import Appearance
    for kw in (dict(noise=-1.0), dict(noise=float("nan")), dict(noise=(1, 2)), dict(blur=1.0), dict(blur=(1.0, 0.5)), dict(blur=(-0.1, 0.5)),
               dict(blur=(0.5, 1.625)), dict(blur=(0.5, float("inf"))), dict(contrast=(1.5, 0.65)), dict(contrast=(0.5, float("nan"))),
               dict(gamma=(-1, 1)), dict(gamma=(1, 2, 3)), dict(p_noise=1.5), dict(p_gamma=-0.1)):
        with pytest.raises(N3DError):
            Appearance(**kw)
    a = Appearance(noise=0.0, blur=(0.0, 1.62), contrast=(1.0, 1.0), gamma=(0.0, 3.0), p_noise=0, p_blur=1)
    assert a.blur == (0.0, 1.62)
    with pytest.raises(N3DError, match="one value per channel"):
        Appearance.descriptors([dict(contrast=np.ones(3))], 4)
    d = Appearance.descriptors([None, dict(noise=(1.5, (7, 2 ** 32 - 1)), blur=np.array([0.5, 1.5]))], 2)
    assert (d[0].noise, d[0].blur, d[0].contrast, d[0].gamma) == (0, 0, 0, 0)
    assert (d[1].noise, d[1].blur, d[1].contrast, d[1].gamma) == (1, 1, 0, 0) and d[1].sigma == 1.5 and list(d[1].key) == [7, 2 ** 32 - 1]
    assert list(d[1].radius)[:2] == [2, 6] and list(d[1].weights[1]) == list(ap.blur_weights(1.5)[1])


def test_abi_surface_and_descriptor_layout():
    import ctypes as C
    from nas_3d_unet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "n3d.h")).read()
    assert "n3d_patch_appearance" in _lib.PROTOTYPES and "n3d_patch_appearance_scratch" in _lib.PROTOTYPES
    assert re.search(r"#define N3D_APPEAR_MAX_BATCH 16\b", hdr) and re.search(r"#define N3D_APPEAR_MAX_RADIUS 6\b", hdr)
    assert C.sizeof(_lib.AppearDesc) == 16 + 8 + 8 + 16 + 4 * 7 * 8 + 32 + 32 and _lib.AppearDesc.weights.offset == 48
    lib = _lib.load()
    assert lib.n3d_patch_appearance_scratch(2, 4, 64) >= 2 * 64 ** 3 * (1 + 16) and lib.n3d_patch_appearance_scratch(17, 4, 64) == 0
    assert lib.n3d_patch_appearance_scratch(1, 5, 8) == 0 and lib.n3d_patch_appearance_scratch(1, 1, 0) == 0


def test_epoch_order_is_todays_without_the_keyword_and_inserts_the_draws_with_it():
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.appearance import Appearance
    flags = np.array([3, 1, 3, 0, 3, 3, 2, 3, 3], np.uint8)
    warp = (15, 0.1, 0.1, 4)

    def order(np_rng, **kw):
        return list(G.epoch_order(flags, 2, random.Random(5), True, True, True, augment=(np_rng, 0.25, True), **kw))

    r0, r1 = _Recording(9), _Recording(9)
    base = order(r0, warp=(r0,) + warp)
    same = order(r1, warp=(r1,) + warp, appearance=None)
    assert repr(base) == repr(same) and r0.calls == r1.calls and all(len(e) == 4 for b in base for e in b)
    per_patch = [("normal", 1, 0.25, 3)] + [("choice",)] * 3 + [("uniform", -15.0, 15.0, 3), ("uniform", 0.9, 1.1, 4), ("normal", 0, 0.1, 4)]
    assert [c[:1] for c in r0.calls] == [c[:1] for c in per_patch] * 6
    # with it: the same entries up to the inserted draws, which come after draw_warp's calls of the same patch
    a = Appearance(contrast=(0.7, 1.3), p_contrast=1.0)
    r2 = _Recording(9)
    got = order(r2, warp=(r2,) + warp, appearance=(r2, a, 4))
    assert [[e[:2] for e in b] for b in got] == [[e[:2] for e in b] for b in base]
    assert all(len(e) == 5 and list(e[4]) == ["contrast"] and e[4]["contrast"].shape == (4,) for b in got for e in b)
    assert [c[0] for c in r2.calls] == ([c[0] for c in per_patch] + ["uniform", "uniform"]) * 6
    assert r2.calls[7:9] == [("uniform",), ("uniform", 0.7, 1.3, 4)]
    # without warp the draws follow draw_augment's
    r3 = _Recording(9)
    got = order(r3, appearance=(r3, a, 2))
    assert all(len(e) == 4 and e[3]["contrast"].shape == (2,) for b in got for e in b)
    assert [c[0] for c in r3.calls] == (["normal", "choice", "choice", "choice", "uniform", "uniform"]) * 6
    with pytest.raises(N3DError, match="needs augment"):
        list(G.epoch_order(flags, 2, random.Random(5), appearance=(r3, a, 4)))
