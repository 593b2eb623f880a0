"""GPU: Gaussian noise, Gaussian blur, contrast and gamma on the brain voxels of a gathered batch (n3d_patch_appearance;
nas_3d_unet_amd.appearance, Generator(augment_appearance=...)).  Blur and contrast equal the numpy statement of the rule
(tests/_appearance_ref.py) with == on the bits and scipy's / numpy's recorded fp64 answers (tests/golden/appearance.npz) to one float32
step; noise and gamma equal the recorded answers within the fixture's tol/* plus 2 float32 steps of the channel's largest magnitude
(the device's fp64 log, sincos and pow may differ from libm's in the last place, and each such difference can flip one of the at most
two roundings to float32 on the way) -- a bound that comes from the fixture, never from the kernel's output.  Shapes: P = 7 with
radius 6 (reflection at both ends of every line), 12 (ragged against the 8-wide tile), 16 and 20 (full tiles; 20^3 = 8 chunks of the
statistics, the last ragged), B = 1, 5, 16, Cv = 1, 3, 4, channel pitch Cv and 8."""
import json
import random

import numpy as np
import pytest
import torch

import _appearance_ref as ap
import make_golden_appearance as mga
import make_golden_augment as mgaug
import make_golden_generator as mg

pytestmark = pytest.mark.gpu

STAGES = ("noise", "blur", "contrast", "gamma")
BATCH = {"p7": 5, "p12": 16, "p16": 1, "p20": 5}
PAD = 7.0
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _device_batch(x, ld):
    """x (B, Cv, P, P, P) float32 -> (the logical view on a pitched NDHWC buffer whose pad lanes hold PAD, the buffer)"""
    B, Cv, P = x.shape[:3]
    wide = torch.full((B, P, P, P, ld), PAD, device="cuda")
    wide[..., :Cv] = torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, 1, -1))).cuda()
    return wide.permute(0, 4, 1, 2, 3)[:, :Cv], wide


def _run(x, draws, ld):
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd.appearance import Appearance
    view, wide = _device_batch(x, ld)
    assert K._pitch_of(view) == ld
    a = _cache.setdefault("appearance", Appearance())
    assert a.apply(view, draws) is view
    out = view.cpu().numpy()
    assert bool((wide[..., x.shape[1]:] == PAD).all())                  # the pad lanes between Cv and ld keep their bits
    return out


def _case_batch(case):
    """the fixture case as patch 0 of a batch, the others from further seeds with their own parameters; patch 1 (if any) has no draw"""
    key = ("batch", case["name"])
    if key not in _cache:
        B, Cv, P = BATCH[case["name"]], case["Cv"], case["P"]
        rs = np.random.RandomState(1000 + case["seed"])
        x = np.stack([mga.case_input(case)] + [ap.make_data(100 * case["seed"] + b, (Cv, P, P, P)) for b in range(1, B)])
        draws = [dict(noise=tuple(case["noise"]), blur=np.array(case["blur"]), contrast=np.array(case["contrast"]), gamma=np.array(case["gamma"]))]
        for b in range(1, B):
            draws.append(None if b == 1 else dict(
                noise=(float(rs.uniform(0, 10)), tuple(int(k) for k in rs.randint(0, 2 ** 32, 2, dtype=np.uint32))),
                blur=rs.uniform(0.1, min(1.6, (P + 0.4) / 4), Cv), contrast=rs.uniform(0.65, 1.5, Cv), gamma=rs.uniform(0.7, 1.5, Cv)))
        want = {s: ap.apply_batch(x, [None if d is None else {s: d[s]} for d in draws]) for s in STAGES}
        want["all"] = ap.apply_batch(x, draws)
        _cache[key] = (x, draws, want)
    return _cache[key]


def _assert_within(got, want, tol, what):
    """within tol float32 steps of the largest magnitude of each (patch, channel) of `want`"""
    for b in range(want.shape[0]):
        for c in range(want.shape[1]):
            scale = np.abs(want[b, c]).max()
            if scale == 0:
                assert not got[b, c].any(), (what, b, c)
                continue
            worst = float(ap.steps(got[b, c], want[b, c], scale).max())
            assert worst <= tol, "%s: patch %d channel %d is %.2f steps off (bound %.2f)" % (what, b, c, worst, tol)


def _cases(g):
    return json.loads(str(g["config"]))["cases"]


@pytest.mark.parametrize("wide", (False, True), ids=("ld=Cv", "ld=8"))
@pytest.mark.parametrize("name", ("p7", "p12", "p16", "p20"))
def test_each_stage_and_all_four_equal_the_helper_and_the_fixture(golden, name, wide):
    g = golden("appearance")
    case = [c for c in _cases(g) if c["name"] == name][0]
    x, draws, want = _case_batch(case)
    B, Cv = x.shape[:2]
    ld = 8 if wide else Cv
    tol = {"noise": float(g["tol/noise"]) + 2, "gamma": float(g["tol/gamma"]) + 2}
    assert B in (1, 5, 16) and all(ap.blur_weights(s)[0] <= case["P"] for d in draws if d for s in d["blur"])
    if name == "p7":
        assert [ap.blur_weights(s)[0] for s in case["blur"]] == [6, 6, 0, 4]
    for stage in STAGES:
        got = _run(x, [None if d is None else {stage: d[stage]} for d in draws], ld)
        fix = g["%s/%s" % (name, stage)]
        assert np.isfinite(got).all()
        assert np.array_equal(_bits(got)[x == 0], _bits(x)[x == 0]) and not (x == 0).all()      # the background is 0.0f bit for bit
        if B > 1:
            assert np.array_equal(_bits(got[1]), _bits(x[1]))                                   # the patch without a draw keeps its bits
        assert not np.array_equal(got[0], x[0])
        if stage in ("blur", "contrast"):
            assert np.array_equal(_bits(got), _bits(want[stage])), stage
            assert (np.abs(got[0].astype(np.float64) - fix) <= np.spacing(np.abs(fix))).all(), stage
        else:
            _assert_within(got[:1], fix[None], tol[stage], "%s against the fixture" % stage)
            _assert_within(got, want[stage], tol[stage], "%s against the helper" % stage)
    got = _run(x, draws, ld)
    assert np.isfinite(got).all() and np.array_equal(_bits(got)[x == 0], _bits(x)[x == 0])
    _assert_within(got, want["all"], max(tol.values()), "all four stages")
    assert np.array_equal(_bits(_run(x, draws, ld)), _bits(got))                                # two runs, the same bits
    # descriptors with every flag clear, and a list of None: nothing changes
    assert np.array_equal(_bits(_run(x, [{} for _ in draws], ld)), _bits(x))
    assert np.array_equal(_bits(_run(x, [None] * B, ld)), _bits(x))


def test_degenerate_channels_follow_the_rule_without_nan():
    """channel 0 without a masked voxel, channel 1 with one (hi - lo = 0, sd = 0), channel 2 constant, channel 3 ordinary"""
    P = 9
    x = np.zeros((2, 4, P, P, P), np.float32)
    x[:, 1, 4, 5, 2] = 37.5
    x[:, 2] = np.where(ap.make_data(5, (P, P, P)) != 0, np.float32(21.25), 0)
    x[:, 3] = ap.make_data(6, (P, P, P))
    draw = dict(noise=(3.0, (5, 6)), blur=np.array([1.0, 0.6, 1.5, 0.9]), contrast=np.array([1.3, 0.7, 1.4, 1.2]), gamma=np.array([0.8, 1.4, 0.7, 1.2]))
    for stage in STAGES + ("all",):
        draws = [draw if stage == "all" else {stage: draw[stage]}, None]
        want = ap.apply_batch(x, draws)
        got = _run(x, draws, 4)
        assert np.isfinite(got).all() and np.isfinite(want).all(), stage
        assert np.array_equal(_bits(got)[x == 0], _bits(x)[x == 0]) and np.array_equal(_bits(got[1]), _bits(x[1]))
        if stage in ("blur", "contrast"):
            assert np.array_equal(_bits(got), _bits(want)), stage
        else:
            _assert_within(got, want, 2, stage)
    # the literal values: contrast leaves a single voxel and a constant channel as they are; gamma maps them to m
    for stage in ("contrast", "gamma"):
        got = _run(x, [{stage: draw[stage]}, None], 4)
        assert got[0, 1, 4, 5, 2] == np.float32(37.5) and np.array_equal(got[0, 2], x[0, 2]), stage


def test_bad_arguments_return_an_error_and_launch_nothing():
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd._lib import AppearDesc, N3DError
    from nas_3d_unet_amd.appearance import Appearance
    lib = _lib.load()
    P = 8
    x = torch.from_numpy(ap.make_data(3, (17, P, P, P, 8))).cuda()          # room for B = 17 and Cv = 5 at pitch 8
    before = x.clone()
    scratch = torch.empty(max(int(lib.n3d_patch_appearance_scratch(16, 4, P)), 8) * 2, dtype=torch.uint8, device="cuda")

    def call(descs, B, Cv, p=P, ws=scratch):
        return lib.n3d_patch_appearance(K.ptr(x), 8, B, Cv, p, descs, K.ptr(ws), ws.numel() if ws is not None else 0, K.stream_ptr())

    def descs_of(n, **kw):
        d = (AppearDesc * n)()
        for k, v in kw.items():
            for i in range(n):
                if isinstance(v, (list, tuple)):
                    for c, vc in enumerate(v):
                        getattr(d[i], k)[c] = vc
                else:
                    setattr(d[i], k, v)
        return d

    w = [0.2] * 4
    assert lib.n3d_patch_appearance_scratch(17, 4, P) == 0 and lib.n3d_patch_appearance_scratch(2, 5, P) == 0
    for descs, B, Cv, p, word in ((descs_of(17, contrast=1, factor=[1.2] * 4), 17, 4, P, b"N3D_APPEAR_MAX_BATCH"),
                                  (descs_of(2, contrast=1, factor=[1.2] * 4), 2, 5, P, b"Cv"),
                                  (descs_of(2, blur=1, radius=[1, 7, 1, 1]), 2, 4, P, b"N3D_APPEAR_MAX_RADIUS"),
                                  (descs_of(2, blur=1, radius=[1, 1, 5, 1]), 2, 4, 4, b"exceeds the patch"),
                                  (descs_of(2, noise=1, sigma=float("nan")), 2, 4, P, b"sigma"),
                                  (descs_of(2, contrast=1, factor=[1.0, float("inf"), 1.0, 1.0]), 2, 4, P, b"finite"),
                                  (descs_of(2, gamma=1, gamma_c=[1.0, 1.0, -1.0, 1.0]), 2, 4, P, b"gamma")):
        assert call(descs, B, Cv, p) == -1 and word in lib.n3d_last_error(), lib.n3d_last_error()
    assert call(descs_of(2, contrast=1, factor=[1.2] * 4), 2, 4, P, scratch[:64]) == -1 and b"scratch" in lib.n3d_last_error()
    assert call(descs_of(2), 2, 4, P, None) == 0                       # no flag set: nothing to do, the scratch is not looked at
    torch.cuda.synchronize()
    assert torch.equal(x, before)                                     # nothing was launched
    assert call(descs_of(16, contrast=1, factor=[1.2] * 4), 16, 4) == 0
    torch.cuda.synchronize()
    assert not torch.equal(x[:16, ..., :4], before[:16, ..., :4]) and torch.equal(x[16], before[16]) and torch.equal(x[..., 4:], before[..., 4:])
    # the Python surface
    a = Appearance()
    ok = K.empty_ndhwc(2, 4, P, P, P, torch.device("cuda", 0), torch.float32)
    d = [dict(contrast=np.full(4, 1.2)), None]
    for bad, word in ((ok.cpu(), "device"), (ok.double(), "fp32"), (torch.zeros((2, 4, P, P, P), device="cuda"), "NDHWC"), (ok[0], "5-D")):
        with pytest.raises(N3DError, match=word):
            a.apply(bad, d)
    with pytest.raises(N3DError, match="one draw"):
        a.apply(ok, d[:1])
    with pytest.raises(N3DError, match="N3D_APPEAR_MAX_RADIUS"):
        a.apply(ok, [dict(blur=np.full(4, 1.7)), None])


class _Recorder:
    """an np.random.RandomState that notes every call's result and whether Appearance.draw made it"""

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
    """replays a recorder's calls, leaving out the ones Appearance.draw made"""

    def __init__(self, log):
        self.log = [(name, out) for inside, name, out in log if not inside]

    def __getattr__(self, name):
        def call(*a, **kw):
            n, out = self.log.pop(0)
            assert n == name, (n, name)
            return out
        return call


@pytest.mark.parametrize("warped", (False, True), ids=("scale-flip", "rotation-linear-intensity"))
def test_generator_with_appearance_equals_the_helper_on_the_batches_without_it(golden, warped):
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd.appearance import Appearance

    class Noting(Appearance):
        drawn = []

        def draw(self, np_rng, Cv):
            np_rng.inside = True
            d = super().draw(np_rng, Cv)
            np_rng.inside = False
            self.drawn.append(d)
            return d

    g = golden("appearance")
    s = G.VolumeSet()
    for v, t in mg.generator_volumes():
        s.add(v, t)
    P = 8
    kw = dict(indices_list=[3, 0, 1], volumes=s, patch_shape=P, patch_overlap=3, batch_size=3, labels=[1, 2, 4], permute=True, augment=True,
              affine=mgaug.BRATS_AFFINE)
    if warped:
        kw.update(augment_rotation=15, augment_interpolation="linear", augment_intensity_scale=0.1, augment_intensity_shift=0.1)
    a = Noting(noise=2.0, blur=(0.3, 1.5), contrast=(0.65, 1.5), gamma=(0.7, 1.5), p_noise=0.5, p_blur=0.7, p_contrast=0.5, p_gamma=0.6)
    a.drawn = []
    rec = _Recorder(141)
    with_it = [(x.cpu().numpy(), t.cpu().numpy()) for x, t in G.Generator(rng=random.Random(41), np_rng=rec, augment_appearance=a, **kw).epoch()]
    without = [(x.cpu().numpy(), t.cpu().numpy()) for x, t in G.Generator(rng=random.Random(41), np_rng=_Replay(rec.log), **kw).epoch()]
    assert len(with_it) == len(without) >= 2 and sum(len(x) for x, _ in without) == len(a.drawn) >= 6
    assert {k for d in a.drawn for k in d} == set(STAGES)
    tol = max(float(g["tol/noise"]), float(g["tol/gamma"])) + 2
    at, changed = 0, 0
    for (x1, t1), (x0, t0) in zip(with_it, without):
        draws = a.drawn[at:at + len(x0)]
        at += len(x0)
        assert np.array_equal(t1, t0)                                  # the truth is never touched
        _assert_within(x1, ap.apply_batch(x0, draws), tol, "generator batch")
        assert np.array_equal(_bits(x1)[x0 == 0], _bits(x0)[x0 == 0])
        changed += int(not np.array_equal(x1, x0))
    assert changed >= 2


def test_generator_without_the_option_makes_the_calls_and_bits_it_made(monkeypatch):
    """left None, the generator calls the library exactly as before -- one gather per batch and nothing else -- and yields the same bits
    as a generator that was never given the keyword; the option needs augment=True and at most 16 patches of at most 4 channels"""
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd import generator as G
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.appearance import Appearance
    s = G.VolumeSet()
    for v, t in mg.generator_volumes():
        s.add(v, t)
    kw = dict(indices_list=[3, 0, 1], volumes=s, patch_shape=8, batch_size=3, labels=[1, 2, 4], permute=True, augment=True, affine=mgaug.BRATS_AFFINE)
    lib = _lib.load()
    calls = []
    for name in _lib.PROTOTYPES:
        if name.startswith("n3d_patch_"):
            monkeypatch.setattr(lib, name, (lambda fn, n: lambda *a: (calls.append(n), fn(*a))[1])(getattr(lib, name), name))
    runs = []
    for extra in ({}, {"augment_appearance": None}):
        gen = G.Generator(rng=random.Random(7), np_rng=np.random.RandomState(8), **kw, **extra)
        del calls[:]
        batches = [(x.clone(), t.clone()) for x, t in gen.epoch()]
        assert calls == ["n3d_patch_gather_aug"] * len(batches) and len(batches) == gen.steps_per_epoch >= 2
        runs.append(batches)
    assert all(torch.equal(xa, xb) and torch.equal(ta, tb) for (xa, ta), (xb, tb) in zip(*runs))
    gen = G.Generator(rng=random.Random(7), np_rng=np.random.RandomState(8), augment_appearance=Appearance(contrast=(0.7, 1.3), p_contrast=1.0), **kw)
    del calls[:]
    n = len(list(gen.epoch()))
    launching = [c for c in calls if c != "n3d_patch_appearance_scratch"]                      # a size query launches nothing
    assert launching == ["n3d_patch_gather_aug", "n3d_patch_appearance"] * n
    # a batch that goes into the caller's buffers is transformed there
    from nas_3d_unet_amd import kernels as K
    bufs = (K.empty_ndhwc(3, 4, 8, 8, 8, s.device, torch.float32), torch.empty((3, 3, 8, 8, 8), device=s.device))
    mk = lambda: G.Generator(rng=random.Random(7), np_rng=np.random.RandomState(8), augment_appearance=Appearance(contrast=(0.7, 1.3), p_contrast=1.0), **kw)
    fresh = [(x.clone(), t.clone()) for x, t in mk().epoch()]
    in_place = 0
    for (x, t), (fx, ft) in zip(mk().epoch(out=bufs), fresh):
        in_place += int(x is bufs[0] and t is bufs[1])
        assert torch.equal(x, fx) and torch.equal(t, ft)
    assert in_place >= 2
    with pytest.raises(N3DError, match="augment=True"):
        G.Generator(**dict(kw, augment=False, augment_appearance=Appearance(noise=1.0)))
    with pytest.raises(N3DError, match="N3D_APPEAR_MAX_BATCH"):
        G.Generator(**dict(kw, batch_size=17, augment_appearance=Appearance(noise=1.0)))
    with pytest.raises(N3DError, match="appearance.Appearance"):
        G.Generator(**dict(kw, augment_appearance=object()))
