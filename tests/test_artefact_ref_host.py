"""CPU: the numpy statement of n3d_patch_artefact's rule (tests/_artefact_ref.py) against outside authorities -- torch's fp64
interpolate (nearest-exact, trilinear) for the low-resolution stage, TorchIO's coordinate rule restated with np.arange / np.meshgrid
and numpy's polyval3d for the bias field (TorchIO and batchgenerators themselves are not installed: never run here) -- and the host
side of nas_3d_unet_amd.artefact: the draws and their order, the validation, and epoch_order with and without the new keyword."""
import os
import random
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _artefact_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def test_nearest_index_is_torchs_nearest_exact_on_fp64_for_every_pair():
    """fp64 torch is the authority: its fp32 kernel forms the index in fp32 and differs from exact arithmetic for some pairs"""
    pairs = 0
    for P in range(2, 257):
        src = torch.arange(P, dtype=torch.float64).view(1, 1, P)
        for n in range(1, P + 1):
            want = F.interpolate(src, size=n, mode="nearest-exact").view(-1).numpy().astype(np.int64)
            assert np.array_equal(ar.nearest_index(P, n), want), (P, n)
            pairs += 1
    assert pairs == 32895


def _torch_lowres(xc, n):
    P = xc.shape[0]
    t = torch.from_numpy(np.asarray(xc, np.float64)).view(1, 1, P, P, P)
    down = F.interpolate(t, size=(n, n, n), mode="nearest-exact")
    return F.interpolate(down, size=(P, P, P), mode="trilinear", align_corners=False).view(P, P, P).numpy()


@pytest.mark.parametrize("P", (8, 12, 16, 21))
def test_composed_lowres_is_nearest_exact_then_trilinear(P):
    """the composed eight-tap statement against torch's two resamplings on fp64, every n, under the summation-order bound
    8 eps64 max|x| (5.33e-15 on these values in +-3).  Worst |statement - torch| over all n: P = 8: 0, P = 12: 1.78e-15, P = 16: 0,
    P = 21: 4.44e-15; the power-of-two extents are exact because every weight there is a dyadic fraction.  The bound holds only
    because the rule's source coordinate is ONE fused multiply-add, as torch evaluates it: with the product and the difference
    rounded separately the coordinate errs by an ulp of n and the same comparison gives 3.11e-15 at P = 12 and 6.44e-15 at
    P = 21 (2.6e-14 at P = 50)."""
    x = ar.make_data(40 + P, (P, P, P))
    assert (x == 0).mean() > 0.3 and np.abs(x).max() <= 3
    bound = 8 * EPS * float(np.abs(x).max())
    worst = 0.0
    for n in range(1, P + 1):
        err = float(np.abs(ar.lowres_channel(x, n) - _torch_lowres(x, n)).max())
        worst = max(worst, err)
    print("P = %d: worst |statement - torch| = %.3g (bound %.3g)" % (P, worst, bound))
    assert worst <= bound


def test_lowres_at_full_extent_is_the_identity_bit_for_bit():
    for P in (2, 8, 21):
        x = ar.make_data(7 + P, (2, P, P, P))
        mask = ar.entry_mask(x)
        a0, a1, l1 = ar.axis_taps(P, P)
        assert np.array_equal(a0, np.arange(P)) and not l1.any()
        assert np.array_equal(ar.lowres_channel(x[0], P).astype(np.float32).view(np.uint32), x[0].view(np.uint32))
        y = ar.lowres(x, mask, [P, P - 1])
        assert np.array_equal(y[0].view(np.uint32), x[0].view(np.uint32)) and not np.array_equal(y[1], x[1])
        assert (y[~mask] == 0).all()                                   # the background stays zero, though zeros are taps
    # n = 1: every masked voxel becomes the one voxel nearest-exact keeps
    x = ar.make_data(3, (1, 8, 8, 8))
    x[0, 4, 4, 4] = 1.5
    y = ar.lowres(x, ar.entry_mask(x), [1])
    assert ar.nearest_index(8, 1)[0] == 4 and (y[ar.entry_mask(x)] == np.float32(1.5)).all()


def _torchio_coords(P):
    """TorchIO's RandomBiasField coordinates of a P^3 image, restated: ranges = arange(-P / 2, P / 2) + 0.5, a meshgrid of them,
    each mesh divided by its maximum (its meshgrid is "xy" and the map is transposed back: "ij" here)"""
    half = P / 2
    r = np.arange(-half, half) + 0.5
    meshes = np.asarray(np.meshgrid(r, r, r, indexing="ij"))
    for mesh in meshes:
        if mesh.max() > 0:
            mesh /= mesh.max()
    return meshes


@pytest.mark.parametrize("P", (2, 7, 8, 12, 21))
def test_bias_coordinates_and_field_are_torchios(P):
    X = ar.bias_coords(P)
    mx, my, mz = _torchio_coords(P)
    assert mx.shape == (P, P, P)
    assert np.array_equal(mx, np.broadcast_to(X[:, None, None], mx.shape)) and np.array_equal(my, np.broadcast_to(X[None, :, None], my.shape))
    assert np.array_equal(mz, np.broadcast_to(X[None, None, :], mz.shape)) and X[0] == -1 and X[-1] == 1
    key = (0xA4093822, 0x299F31D0)
    for order in range(ar.MAX_ORDER + 1):
        terms = ar.bias_terms(order)
        assert len(terms) == (order + 1) * (order + 2) * (order + 3) // 6 and terms[0] == (0, 0, 0)
        coefs = ar.bias_coefs(key, 1, order, 0.5)
        # TorchIO's own loop: coefficient * x^a * y^b * z^c, summed in the same nesting
        tio = np.zeros((P, P, P))
        i = 0
        for a in range(order + 1):
            for b in range(order + 1 - a):
                for c in range(order + 1 - (a + b)):
                    tio += coefs[i] * mx ** a * my ** b * mz ** c
                    i += 1
        # ... and numpy's polynomial evaluation of the coefficient tensor
        cube = np.zeros((order + 1,) * 3)
        for t, (a, b, c) in enumerate(terms):
            cube[a, b, c] = coefs[t]
        pv = np.polynomial.polynomial.polyval3d(mx, my, mz, cube)
        poly = ar.bias_poly(P, coefs, order)
        # |monomial| <= 1.  A term takes at most 2 order + 3 roundings (the powers, two products, the coefficient) and the sum one
        # per term, so an evaluation errs by at most (terms + 2 order + 3) eps sum|coef| and two of them differ by twice that
        bound = 2 * (len(terms) + 2 * order + 3) * EPS * float(np.abs(coefs).sum())
        assert np.abs(poly - tio).max() <= bound and np.abs(poly - pv).max() <= bound
        field = np.exp(poly)
        assert (np.abs(field - np.exp(pv)) <= (1.001 * bound + 2 * EPS) * field).all()      # an exp is good to an eps
    assert len(ar.bias_terms(3)) == 20


def test_bias_coefficients_are_uniform_in_the_range_and_differ_by_channel_and_key():
    k1, k2 = (1, 2), (1, 3)
    for rng in (0.0, 0.25, 0.5):
        c = np.concatenate([ar.bias_coefs(k, ch, 3, rng) for k in (k1, k2) for ch in range(4)])
        assert ((c >= -rng) & (c < rng)).all() or (rng == 0 and not c.any())
    many = np.concatenate([ar.bias_coefs((s, 77), ch, 3, 1.0) for s in range(50) for ch in range(4)])
    assert abs(many.mean()) < 0.05 and abs(many.std() - 3 ** -0.5) < 0.03 and many.min() < -0.99 and many.max() > 0.99
    # the stated counter: word 1 is 3, word 2 the channel
    w0 = ar.philox4x32_10((5, 3, 2, 0), k1)[0]
    assert ar.bias_coefs(k1, 2, 3, 0.5)[5] == (np.float64(w0) * 2.0 ** -32 * 2.0 - 1.0) * 0.5
    x = np.full((2, 8, 8, 8), 2.0, np.float32)
    mask = ar.entry_mask(x)
    a, b = ar.bias(x, mask, k1, [3, 3], [0.5, 0.5]), ar.bias(x, mask, k2, [3, 3], [0.5, 0.5])
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[0], b[0]) and (a > 0).all()
    assert np.array_equal(ar.bias(x, mask, k1, [0, 0], [0.0, 0.0]).view(np.uint32), x.view(np.uint32))


class _Recording:
    def __init__(self, seed, uniforms=None, sized=None):
        self.rs, self.calls, self.uniforms, self.sized = np.random.RandomState(seed), [], list(uniforms or []), list(sized or [])

    def uniform(self, *a, size=None):
        self.calls.append(("uniform",) + a + ((("size", size),) if size is not None else ()))
        if not a and size is None and self.uniforms:
            return self.uniforms.pop(0)
        if not a and size is not None and self.sized:
            return np.asarray(self.sized.pop(0), np.float64)
        return self.rs.uniform(*a) if size is None else self.rs.uniform(*a, size=size)

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
    from nas_3d_unet_amd.artefact import Artefact
    a = Artefact(lowres=(0.5, 1.0), bias=0.5, dropout=0.3, p_bias=0.15, p_dropout=0.1)
    r = _Recording(1, uniforms=[0.2, 0.1, 0.05], sized=[[0.4, 0.5, 0.9], [0.1, 0.3, 0.7]])      # all three active
    d = a.draw(r, 3)
    assert r.calls == [("uniform",), ("uniform", ("size", 3)), ("uniform", 0.5, 1.0, 3), ("uniform",), ("randint", 0, 2 ** 32, 2, np.uint32),
                       ("uniform",), ("uniform", ("size", 3))]
    assert list(d) == ["lowres", "bias", "dropout"]
    # a value equal to p_lowres_channel does not select the channel; an unselected channel has scale 1
    assert d["lowres"].dtype == np.float64 and 0.5 <= d["lowres"][0] <= 1.0 and list(d["lowres"][1:]) == [1.0, 1.0]
    assert d["bias"][:2] == (0.5, 3) and len(d["bias"][2]) == 2 and all(isinstance(k, int) for k in d["bias"][2])
    assert d["dropout"].dtype == bool and list(d["dropout"]) == [True, False, False]
    r = _Recording(1, uniforms=[0.25, 0.15, 0.1])                     # a value equal to p is not active: nothing else is drawn
    assert a.draw(r, 4) == {} and r.calls == [("uniform",)] * 3
    r = _Recording(1, uniforms=[0.0])                                 # options left None draw nothing at all
    d = Artefact(bias=0.2, bias_order=2, p_bias=1.0).draw(r, 2)
    assert r.calls == [("uniform",), ("randint", 0, 2 ** 32, 2, np.uint32)] and list(d) == ["bias"] and d["bias"][:2] == (0.2, 2)
    assert Artefact().draw(_Recording(1), 4) == {}


def test_dropout_never_drops_every_channel():
    from nas_3d_unet_amd.artefact import Artefact
    a = Artefact(dropout=1.0, p_dropout=1.0)
    for seed in range(20):
        r = _Recording(seed)
        d = a.draw(r, 4)
        assert r.calls == [("uniform",), ("uniform", ("size", 4)), ("randint", 0, 4, None)]
        assert d["dropout"].sum() == 3                                # exactly one channel is kept
    kept = {int(np.flatnonzero(~a.draw(_Recording(s), 4)["dropout"])[0]) for s in range(40)}
    assert kept == {0, 1, 2, 3}
    r = _Recording(3, uniforms=[0.0], sized=[[0.9, 0.1, 0.9, 0.1]])   # not all fell: no further draw
    d = Artefact(dropout=0.5, p_dropout=1.0).draw(r, 4)
    assert list(d["dropout"]) == [False, True, False, True] and len(r.calls) == 2


def test_validation():
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.artefact import Artefact, extent
    for kw in (dict(lowres=0.5), dict(lowres=(0.0, 1.0)), dict(lowres=(0.8, 0.5)), dict(lowres=(0.5, 1.1)), dict(lowres=(0.5, float("nan"))),
               dict(lowres=(0.1, 0.2, 0.3)), dict(bias=-0.1), dict(bias=float("inf")), dict(bias=(0.1, 0.2)), dict(bias_order=4),
               dict(bias_order=-1), dict(bias_order=1.5), dict(bias_order=True), dict(dropout=1.5), dict(dropout=-0.1),
               dict(dropout=float("nan")), dict(p_lowres=1.5), dict(p_lowres_channel=-0.1), dict(p_bias=2), dict(p_dropout=float("nan"))):
        with pytest.raises(N3DError):
            Artefact(**kw)
    a = Artefact(lowres=(0.5, 1.0), bias=0.0, bias_order=0, dropout=0.0, p_lowres=0, p_bias=1)
    assert a.lowres == (0.5, 1.0) and a.bias == 0.0 and a.bias_order == 0
    # Python's round, to even on a tie, and never below 1
    assert [extent(8, s) for s in (1.0, 0.5, 0.0625, 0.01, 0.3125, 0.4375)] == [8, 4, 1, 1, 2, 4] and extent(12, 0.7) == ar.extent(12, 0.7) == 8
    for bad in ([dict(lowres=np.ones(3))], [dict(lowres=np.array([1.0, float("nan"), 1.0, 1.0]))], [dict(dropout=np.zeros(3, bool))],
                [dict(dropout=np.ones(4, bool))]):
        with pytest.raises(N3DError):
            Artefact.descriptors(bad, 4, 8)
    t = Artefact.descriptors([None, dict(lowres=np.array([0.5, 1.0]), bias=(0.25, 2, (7, 2 ** 32 - 1)), dropout=np.array([False, True]))], 2, 12)
    assert list(t.stages) == [0, 0, 0, 1, 1, 1] and list(t.n) == [0] * 4 + [6, 12, 0, 0] and list(t.order)[4:] == [2, 2, 0, 0]
    assert list(t.range)[4:] == [0.25, 0.25, 0.0, 0.0] and list(t.key) == [0, 0, 7, 2 ** 32 - 1] and list(t.drop)[4:] == [0, 1, 0, 0]


def test_abi_surface():
    from nas_3d_unet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "n3d.h")).read()
    assert "n3d_patch_artefact" in _lib.PROTOTYPES and "n3d_patch_artefact_scratch" in _lib.PROTOTYPES
    assert re.search(r"#define N3D_ARTEFACT_MAX_ORDER 3\b", hdr)
    lib = _lib.load()
    assert lib.n3d_patch_artefact_scratch(2, 4, 64) >= 2 * 64 ** 3 * (1 + 16) and lib.n3d_patch_artefact_scratch(17, 4, 64) == 0
    assert lib.n3d_patch_artefact_scratch(1, 5, 8) == 0 and lib.n3d_patch_artefact_scratch(1, 1, 1) == 0
    assert lib.n3d_patch_artefact_scratch(1, 1, 257) == 0 and lib.n3d_patch_artefact_scratch(16, 4, 2) > 0


def test_epoch_order_is_todays_without_the_keyword_and_appends_the_draws_with_it():
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.appearance import Appearance
    from nas_3d_unet_amd.artefact import Artefact
    flags = np.array([3, 1, 3, 0, 3, 3, 2, 3, 3], np.uint8)
    warp = (15, 0.1, 0.1, 4)
    app = Appearance(contrast=(0.7, 1.3), p_contrast=1.0)

    def order(np_rng, **kw):
        return list(G.epoch_order(flags, 2, random.Random(5), True, True, True, augment=(np_rng, 0.25, True), **kw))

    r0, r1 = _Recording(9), _Recording(9)
    base = order(r0, warp=(r0,) + warp, appearance=(r0, app, 4))
    same = order(r1, warp=(r1,) + warp, appearance=(r1, app, 4), artefact=None)
    assert repr(base) == repr(same) and r0.calls == r1.calls and all(len(e) == 5 for b in base for e in b)
    per_patch = ["normal", "choice", "choice", "choice", "uniform", "uniform", "normal", "uniform", "uniform"]
    assert [c[0] for c in r0.calls] == per_patch * 6
    # with it: the same entries, one element more at the very end, drawn after Appearance.draw's calls of the same patch
    art = Artefact(bias=0.5, dropout=0.5, p_bias=1.0, p_dropout=1.0)
    r2 = _Recording(9)
    got = order(r2, warp=(r2,) + warp, appearance=(r2, app, 4), artefact=(r2, art, 4))
    assert [[e[:2] for e in b] for b in got] == [[e[:2] for e in b] for b in base]
    assert all(len(e) == 6 and list(e[4]) == ["contrast"] and list(e[5]) == ["bias", "dropout"] and e[5]["dropout"].shape == (4,) for b in got for e in b)
    # uniform() + randint (bias), uniform() + uniform(size=) (dropout), and a randint more where every channel fell
    tail = ["uniform", "randint", "uniform", "uniform"]
    calls = [c[0] for c in r2.calls]
    at = 0
    for b in got:
        for e in b:
            n = len(per_patch) + len(tail)
            assert calls[at:at + n] == per_patch + tail
            at += n
            if e[5]["dropout"].sum() == 3 and calls[at:at + 1] == ["randint"]:
                at += 1
    assert at == len(calls)
    # without appearance (and without warp) the draws follow draw_augment's
    r3 = _Recording(9)
    got = order(r3, artefact=(r3, art, 2))
    assert all(len(e) == 4 and e[3]["dropout"].shape == (2,) for b in got for e in b)
    assert [c[0] for c in r3.calls[:8]] == ["normal", "choice", "choice", "choice"] + tail
    with pytest.raises(N3DError, match="needs augment"):
        list(G.epoch_order(flags, 2, random.Random(5), artefact=(r3, art, 4)))
