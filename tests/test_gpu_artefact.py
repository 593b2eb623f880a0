"""GPU: simulated low resolution, the bias field and modality dropout on a gathered batch (n3d_patch_artefact;
nas_3d_unet_amd.artefact, Generator(augment_artefact=...)).  Low resolution and dropout equal the numpy statement of the rule
(tests/_artefact_ref.py) with == on the bits; the bias field equals it within 2 float32 steps of the channel's largest output
magnitude (the device's fp64 exp may differ from libm's in the last place, and such a difference can flip the one rounding to
float32) -- the bound the appearance noise and gamma stages carry for the same reason, never one taken from the kernel's output.
Shapes: B = 3, Cv = 4 at pitch 4 with P = 8 (one 1024-voxel chunk, half filled) and P = 16 (four chunks) -- the 16-byte path --
and B = 2, Cv = 3 at pitch 4 with P = 12 (ragged last chunk) -- the 4-byte path, whose fourth lane is padding.  About 40 % of
every patch is exact zeros and one patch of every batch has no draw."""
import random

import numpy as np
import pytest
import torch

import _artefact_ref as ar

pytestmark = pytest.mark.gpu

SHAPES = {"b3c4p8": (3, 4, 8), "b3c4p16": (3, 4, 16), "b2c3p12": (2, 3, 12)}
LD = 4
PAD = 7.0
KEYS = ((0xA4093822, 0x299F31D0), (5, 6), (2 ** 32 - 1, 0))
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _data(name):
    if name not in _cache:
        B, Cv, P = SHAPES[name]
        x = ar.make_data(11 + P, (B, Cv, P, P, P))
        assert 0.3 < (x == 0).mean() < 0.5
        _cache[name] = x
    return _cache[name]


def _run(x, draws):
    """the batch on a pitch-LD NDHWC buffer whose pad lanes hold PAD, through Artefact.apply"""
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd.artefact import Artefact
    B, Cv, P = x.shape[:3]
    wide = torch.full((B, P, P, P, LD), PAD, device="cuda")
    wide[..., :Cv] = torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, 1, -1))).cuda()
    view = wide.permute(0, 4, 1, 2, 3)[:, :Cv]
    assert K._pitch_of(view) == LD and (Cv == 4) == (view.data_ptr() % 16 == 0 and Cv == LD)
    a = _cache.setdefault("artefact", Artefact())
    assert a.apply(view, draws) is view
    out = view.cpu().numpy()
    assert bool((wide[..., Cv:] == PAD).all())                          # the lanes between Cv and ld keep their bits
    return out


def _scales(P, n):
    """scales that Artefact.descriptors turns into exactly the extents n"""
    s = np.array([k / P for k in n], np.float64)
    assert [ar.extent(P, v) for v in s] == list(n)
    return s


def _assert_within(got, want, tol, what):
    """within tol float32 steps of the largest magnitude of each (patch, channel) of `want`"""
    for b in range(want.shape[0]):
        for c in range(want.shape[1]):
            scale = np.abs(want[b, c]).max()
            if scale == 0:
                assert not got[b, c].any(), (what, b, c)
                continue
            worst = float(ar.steps(got[b, c], want[b, c], scale).max())
            assert worst <= tol, "%s: patch %d channel %d is %.2f steps off (bound %.2f)" % (what, b, c, worst, tol)


def _draws(name, lowres=None, bias=None, dropout=None):
    """patch 1 has no draw; the others get what is given, a list per stage with one item per active patch in order (B = 2 has one
    active patch and uses the first item only)"""
    B = SHAPES[name][0]
    out, at = [], 0
    for b in range(B):
        if b == 1:
            out.append(None)
            continue
        d = {}
        if lowres is not None:
            d["lowres"] = lowres[at]
        if bias is not None:
            d["bias"] = bias[at]
        if dropout is not None:
            d["dropout"] = dropout[at]
        out.append(d)
        at += 1
    return out


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_lowres_equals_the_statement_bit_for_bit(name):
    x = _data(name)
    B, Cv, P = SHAPES[name]
    extents = [1, 2, P - 1, P]
    for k, n in enumerate(extents):
        # patch 0: a different extent per channel, starting at n; patch 2 (B = 3): n for every channel
        mixed = [extents[(k + c) % 4] for c in range(Cv)]
        draws = _draws(name, lowres=[_scales(P, mixed), _scales(P, [n] * Cv)])
        want = ar.apply_batch(x, draws)
        got = _run(x, draws)
        assert np.array_equal(_bits(got), _bits(want)), n
        assert np.array_equal(_bits(got)[x == 0], _bits(x)[x == 0])                             # the background is 0.0f bit for bit
        assert np.array_equal(_bits(got[1]), _bits(x[1]))                                       # the patch without a draw
        for c in range(Cv):
            assert np.array_equal(_bits(got[0, c]), _bits(x[0, c])) == (mixed[c] == P)          # n == P: the channel is untouched
        if B == 3:
            assert np.array_equal(_bits(got[2]), _bits(x[2])) == (n == P)
        assert np.array_equal(_bits(_run(x, draws)), _bits(got))                                # two runs, the same bits


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_dropout_zeroes_whole_channels_and_nothing_else(name):
    x = _data(name)
    B, Cv, P = SHAPES[name]
    drop = [np.arange(Cv) != 0, np.arange(Cv) == 1]
    draws = _draws(name, dropout=drop)
    got = _run(x, draws)
    assert np.array_equal(_bits(got), _bits(ar.apply_batch(x, draws)))
    assert not got[0, 1:].any() and x[0, 1].any() and np.array_equal(_bits(got[0, 0]), _bits(x[0, 0]))
    if B == 3:
        assert not got[2, 1].any() and all(np.array_equal(_bits(got[2, c]), _bits(x[2, c])) for c in range(Cv) if c != 1)
    assert np.array_equal(_bits(got[1]), _bits(x[1]))
    # flags without work (no channel falls, every extent is P) and a list of None: nothing changes
    idle = _draws(name, lowres=[_scales(P, [P] * Cv)] * 2, dropout=[np.zeros(Cv, bool)] * 2)
    assert np.array_equal(_bits(_run(x, idle)), _bits(x)) and np.array_equal(_bits(_run(x, [None] * B)), _bits(x))
    assert np.array_equal(_bits(_run(x, [{} for _ in range(B)])), _bits(x))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_bias_field_is_within_two_steps_of_the_statement(name):
    x = _data(name)
    B, Cv, P = SHAPES[name]
    for order in (0, 1, 2, 3):
        draws = _draws(name, bias=[(0.5, order, KEYS[0]), (0.25, order, KEYS[order % 2 + 1])])
        want = ar.apply_batch(x, draws)
        got = _run(x, draws)
        assert np.isfinite(got).all() and not np.array_equal(got[0], x[0])
        assert np.array_equal(_bits(got)[x == 0], _bits(x)[x == 0]) and np.array_equal(_bits(got[1]), _bits(x[1]))
        _assert_within(got, want, 2, "bias order %d" % order)
        assert np.array_equal(_bits(_run(x, draws)), _bits(got))
    # order 0 with range 0: exp(0) = 1, the input bit for bit
    got = _run(x, _draws(name, bias=[(0.0, 0, KEYS[0]), (0.0, 0, KEYS[1])]))
    assert np.array_equal(_bits(got), _bits(x))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_all_three_stages_run_in_the_stated_order(name):
    x = _data(name)
    B, Cv, P = SHAPES[name]
    draws = _draws(name, lowres=[_scales(P, [P // 2, P, 3, P - 1][:Cv]), _scales(P, [P, 2, P // 2 + 1, 1][:Cv])],
                   bias=[(0.5, 3, KEYS[0]), (0.3, 2, KEYS[2])], dropout=[np.arange(Cv) == 0, np.arange(Cv) == Cv - 1])
    want = ar.apply_batch(x, draws)
    # the statement chains the stages on the mask of the entry: low resolution, then the bias field on its output, then dropout
    d = draws[0]
    mask = ar.entry_mask(x[0])
    by_hand = ar.dropout(ar.bias(ar.lowres(x[0], mask, [ar.extent(P, s) for s in d["lowres"]]), mask, KEYS[0], [3] * Cv, [0.5] * Cv), d["dropout"])
    assert np.array_equal(_bits(by_hand), _bits(want[0]))
    got = _run(x, draws)
    assert np.isfinite(got).all() and np.array_equal(_bits(got)[x == 0], _bits(x)[x == 0]) and np.array_equal(_bits(got[1]), _bits(x[1]))
    assert not got[0, 0].any() and (B < 3 or not got[2, Cv - 1].any())
    _assert_within(got, want, 2, "all three stages")
    assert np.array_equal(_bits(_run(x, draws)), _bits(got))                                    # two runs, the same bits


def test_bad_arguments_return_an_error_and_launch_nothing():
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.artefact import Artefact, ArtefactTable
    lib = _lib.load()
    P = 8
    x = torch.from_numpy(ar.make_data(3, (17, P, P, P, 8))).cuda()          # room for B = 17 and Cv = 5 at pitch 8
    before = x.clone()
    scratch = torch.empty(int(lib.n3d_patch_artefact_scratch(16, 4, P)) * 2, dtype=torch.uint8, device="cuda")

    def call(t, B, Cv, p=P, ws=scratch):
        return lib.n3d_patch_artefact(K.ptr(x), 8, B, Cv, p, *t.args(), K.ptr(ws) if ws is not None else None, ws.numel() if ws is not None else 0,
                                      K.stream_ptr())

    def table(B, lowres=None, bias=None, dropout=None):
        t = ArtefactTable(B)
        for b in range(B):
            if lowres is not None:
                t.stages[3 * b] = 1
                t.n[4 * b:4 * b + 4] = lowres
            if bias is not None:
                t.stages[3 * b + 1] = 1
                t.order[4 * b:4 * b + 4], t.range[4 * b:4 * b + 4] = bias
                t.key[2 * b], t.key[2 * b + 1] = 3, 4
            if dropout is not None:
                t.stages[3 * b + 2] = 1
                t.drop[4 * b:4 * b + 4] = dropout
        return t

    inf, nan = float("inf"), float("nan")
    assert lib.n3d_patch_artefact_scratch(17, 4, P) == 0 and lib.n3d_patch_artefact_scratch(2, 5, P) == 0 and lib.n3d_patch_artefact_scratch(2, 4, 1) == 0
    for t, B, Cv, p, word in ((table(17, lowres=[4] * 4), 17, 4, P, b"N3D_APPEAR_MAX_BATCH"),
                              (table(2, lowres=[4] * 4), 2, 5, P, b"Cv"),
                              (table(2, lowres=[4, 0, 4, 4]), 2, 4, P, b"extent"),
                              (table(2, lowres=[4, 4, P + 1, 4]), 2, 4, P, b"extent"),
                              (table(2, bias=([3, 4, 3, 3], [0.5] * 4)), 2, 4, P, b"N3D_ARTEFACT_MAX_ORDER"),
                              (table(2, bias=([3] * 4, [0.5, inf, 0.5, 0.5])), 2, 4, P, b"range"),
                              (table(2, bias=([3] * 4, [0.5, 0.5, nan, 0.5])), 2, 4, P, b"range"),
                              (table(2, bias=([3] * 4, [0.5, 0.5, 0.5, -0.1])), 2, 4, P, b"range"),
                              (table(2, lowres=[1] * 4), 2, 4, 1, b"2 <= P")):
        assert call(t, B, Cv, p) == -1 and word in lib.n3d_last_error(), lib.n3d_last_error()
    for kw in (dict(lowres=[4] * 4), dict(bias=([3] * 4, [0.5] * 4)), dict(dropout=[0, 1, 0, 0])):
        assert call(table(2, **kw), 2, 4, P, scratch[:64]) == -1 and b"scratch" in lib.n3d_last_error()
    assert call(table(2), 2, 4, P, None) == 0                           # no flag set: nothing to do, the scratch is not looked at
    assert call(table(2, lowres=[P] * 4, dropout=[0] * 4), 2, 4, P, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, before)                                       # nothing was launched
    assert call(table(16, lowres=[4, 8, 2, 1]), 16, 4) == 0
    torch.cuda.synchronize()
    assert not torch.equal(x[:16, ..., 0], before[:16, ..., 0]) and torch.equal(x[:16, ..., 1], before[:16, ..., 1])
    assert torch.equal(x[16], before[16]) and torch.equal(x[..., 4:], before[..., 4:])
    # the Python surface
    a = Artefact()
    ok = K.empty_ndhwc(2, 4, P, P, P, torch.device("cuda", 0), torch.float32)
    d = [dict(dropout=np.arange(4) == 2), None]
    for bad, word in ((ok.cpu(), "device"), (ok.double(), "fp32"), (torch.zeros((2, 4, P, P, P), device="cuda"), "NDHWC"), (ok[0], "5-D")):
        with pytest.raises(N3DError, match=word):
            a.apply(bad, d)
    with pytest.raises(N3DError, match="one draw"):
        a.apply(ok, d[:1])
    with pytest.raises(N3DError, match="extent"):
        a.apply(ok, [dict(lowres=np.full(4, 1.5)), None])


def _tiny_set():
    from nas_3d_unet_amd import generator as G
    s = G.VolumeSet()
    rs = np.random.RandomState(21)
    for dims in ((14, 12, 13), (12, 15, 12)):
        v = ar.make_data(int(rs.randint(1000)), (4,) + dims)
        t = rs.choice(np.array([0, 1, 2, 4], np.uint8), size=dims, p=(0.4, 0.2, 0.2, 0.2))
        s.add(v, t)
    return s


class _Recorder:
    """an np.random.RandomState that notes every call's result and whether Artefact.draw made it"""

    def __init__(self, seed):
        self.rs, self.log, self.inside = np.random.RandomState(seed), [], False

    def __getattr__(self, name):
        fn = getattr(self.rs, name)

        def call(*a, **kw):
            out = fn(*a, **kw)
            self.log.append((self.inside, name, out))
            return out
        return call


class _Replay:
    """replays a recorder's calls, leaving out the ones Artefact.draw made"""

    def __init__(self, log):
        self.log = [(name, out) for inside, name, out in log if not inside]

    def __getattr__(self, name):
        def call(*a, **kw):
            n, out = self.log.pop(0)
            assert n == name, (n, name)
            return out
        return call


@pytest.mark.parametrize("with_appearance", (False, True), ids=("alone", "after-appearance"))
def test_generator_with_artefact_is_the_gather_and_apply_by_hand(with_appearance):
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd.appearance import Appearance
    from nas_3d_unet_amd.artefact import Artefact

    class Noting(Artefact):
        def draw(self, np_rng, Cv):
            np_rng.inside = True
            d = super().draw(np_rng, Cv)
            np_rng.inside = False
            self.drawn.append(d)
            return d

    s = _tiny_set()
    P = 8
    kw = dict(indices_list=[1, 0], volumes=s, patch_shape=P, patch_overlap=3, batch_size=3, labels=[1, 2, 4], permute=True, augment=True)
    if with_appearance:
        kw["augment_appearance"] = Appearance(contrast=(0.7, 1.3), p_contrast=1.0)       # contrast equals its statement bit for bit
    a = Noting(lowres=(0.3, 1.0), bias=0.5, dropout=0.4, p_lowres=0.7, p_lowres_channel=0.6, p_bias=0.6, p_dropout=0.6)
    a.drawn = []
    rec = _Recorder(141)
    with_it = [(x.clone(), t.clone()) for x, t in G.Generator(rng=random.Random(41), np_rng=rec, augment_artefact=a, **kw).epoch()]
    without = [(x.clone(), t.clone()) for x, t in G.Generator(rng=random.Random(41), np_rng=_Replay(rec.log), **kw).epoch()]
    assert len(with_it) == len(without) >= 2 and sum(len(x) for x, _ in without) == len(a.drawn) >= 6
    assert {k for d in a.drawn for k in d} == {"lowres", "bias", "dropout"}
    at, changed = 0, 0
    for (x1, t1), (x0, t0) in zip(with_it, without):
        draws = a.drawn[at:at + len(x0)]
        at += len(x0)
        assert torch.equal(t1, t0)                                     # the truth is never touched
        x0n, x1n = x0.cpu().numpy(), x1.cpu().numpy()
        by_hand = Artefact().apply(x0.clone(memory_format=torch.preserve_format), draws)
        assert torch.equal(x1, by_hand)                                # the gather and Artefact.apply by hand, bit for bit
        _assert_within(x1n, ar.apply_batch(x0n, draws), 2, "generator batch")
        assert np.array_equal(_bits(x1n)[x0n == 0], _bits(x0n)[x0n == 0])
        changed += int(not np.array_equal(x1n, x0n))
    assert changed >= 2


def test_generator_without_the_option_makes_the_calls_and_bits_it_made(monkeypatch):
    """left None, the generator calls the library exactly as before and yields the same bits and draws as a generator that was never
    given the keyword; the option needs augment=True and at most 16 patches of at most 4 channels"""
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.artefact import Artefact
    s = _tiny_set()
    kw = dict(indices_list=[1, 0], volumes=s, patch_shape=8, batch_size=3, labels=[1, 2, 4], permute=True, augment=True)
    lib = _lib.load()
    calls = []
    for name in _lib.PROTOTYPES:
        if name.startswith("n3d_patch_"):
            monkeypatch.setattr(lib, name, (lambda fn, n: lambda *a: (calls.append(n), fn(*a))[1])(getattr(lib, name), name))
    runs, states = [], []
    for extra in ({}, {"augment_artefact": None}):
        np_rng = np.random.RandomState(8)
        gen = G.Generator(rng=random.Random(7), np_rng=np_rng, **kw, **extra)
        del calls[:]
        batches = [(x.clone(), t.clone()) for x, t in gen.epoch()]
        assert calls == ["n3d_patch_gather_aug"] * len(batches) and len(batches) == gen.steps_per_epoch >= 2
        runs.append(batches)
        states.append(np_rng.uniform())
    assert all(torch.equal(xa, xb) and torch.equal(ta, tb) for (xa, ta), (xb, tb) in zip(*runs)) and states[0] == states[1]
    always = Artefact(dropout=0.5, p_dropout=1.0, lowres=(0.4, 0.6), p_lowres=1.0, p_lowres_channel=1.0)
    mk = lambda: G.Generator(rng=random.Random(7), np_rng=np.random.RandomState(8), augment_artefact=always, **kw)
    gen = mk()                                                                                  # qualifies its candidates once
    del calls[:]
    n = len(list(gen.epoch()))
    launching = [c for c in calls if c != "n3d_patch_artefact_scratch"]                        # a size query launches nothing
    assert launching == ["n3d_patch_gather_aug", "n3d_patch_artefact"] * n
    # a batch that goes into the caller's buffers is transformed there
    bufs = (K.empty_ndhwc(3, 4, 8, 8, 8, s.device, torch.float32), torch.empty((3, 3, 8, 8, 8), device=s.device))
    fresh = [(x.clone(), t.clone()) for x, t in mk().epoch()]
    in_place = 0
    for (x, t), (fx, ft) in zip(mk().epoch(out=bufs), fresh):
        in_place += int(x is bufs[0] and t is bufs[1])
        assert torch.equal(x, fx) and torch.equal(t, ft)
    assert in_place >= 2
    with pytest.raises(N3DError, match="augment=True"):
        G.Generator(**dict(kw, augment=False, augment_artefact=Artefact(bias=0.5)))
    with pytest.raises(N3DError, match="N3D_APPEAR_MAX_BATCH"):
        G.Generator(**dict(kw, batch_size=17, augment_artefact=Artefact(bias=0.5)))
    with pytest.raises(N3DError, match="artefact.Artefact"):
        G.Generator(**dict(kw, augment_artefact=object()))
    with pytest.raises(N3DError, match="N3D_APPEAR_MAX_PATCH"):
        G.Generator(**dict(kw, patch_shape=1, augment_artefact=Artefact(bias=0.5)))
