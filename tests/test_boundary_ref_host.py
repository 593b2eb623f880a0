"""CPU: the numpy statement of the signed distance transform (tests/_boundary_ref.py) against scipy's recorded squared distances
(tests/golden/boundary.npz, written by tests/golden/make_golden_boundary.py), with `==` throughout, and the fp64 statement of the
boundary loss against autograd.  The GPU tests hold the kernels to this fixture and to these statements."""
import os

import numpy as np
import pytest
import torch

import _boundary_ref as br
import _loss_ref as lr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boundary.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _maps():
    return [(name, b, c, cases[b * shape[1] + c]) for name, (shape, cases) in br.SHAPES.items() for b in range(shape[0]) for c in range(shape[1])]


def test_the_fixture_holds_every_case(golden):
    want = {"empty", "full", "voxel_interior", "voxel_corner", "two_blobs", "speckle_50", "speckle_02", "nested_wt", "nested_tc", "nested_et",
            "full_but_one"}
    assert {m[3] for m in _maps()} == want
    for name, (shape, _) in br.SHAPES.items():
        t = golden[name + ".t"]
        assert t.shape == shape and t.dtype == np.uint8 and set(np.unique(t)) <= {0, 1}
        assert golden[name + ".phi"].dtype == np.float32 and golden[name + ".d2fg"].dtype == np.int32
    wt, tc, et = (golden["box.t"][0, c].astype(bool) for c in range(3))
    assert et.sum() > 0 and (et <= tc).all() and (tc <= wt).all() and et.sum() < tc.sum() < wt.sum() < wt.size


@pytest.mark.parametrize("name,b,c,case", _maps())
def test_squared_distances_equal_scipys(golden, name, b, c, case):
    t = golden[name + ".t"][b, c]
    assert np.array_equal(t, br.fixture_targets(name)[b, c])
    d2fg, d2bg = br.squared_distances(t)
    assert np.array_equal(d2fg, golden[name + ".d2fg"][b, c])
    assert np.array_equal(d2bg, golden[name + ".d2bg"][b, c])
    # a voxel is at distance 0 from its own kind, and the fields are INF exactly when the map holds no such voxel
    assert ((d2fg == 0) == (t != 0)).all() and ((d2bg == 0) == (t == 0)).all()
    assert (d2fg == br.INF).all() == (not t.any()) and (d2fg == br.INF).any() == (not t.any())
    assert (d2bg == br.INF).all() == bool(t.all()) and (d2bg == br.INF).any() == bool(t.all())


@pytest.mark.parametrize("name,b,c,case", _maps())
def test_phi_is_the_rule_on_the_exact_distances(golden, name, b, c, case):
    t = golden[name + ".t"][b, c] != 0
    d2fg, d2bg = (golden[name + k][b, c].astype(np.int64) for k in (".d2fg", ".d2bg"))
    phi = br.signed_distance(golden[name + ".t"][b:b + 1, c:c + 1])[0, 0]
    want = np.zeros(t.shape, np.float32)
    if t.any() and not t.all():
        want = np.where(t, np.float32(-(np.sqrt(d2bg.astype(np.float64)) - 1.0)), np.float32(np.sqrt(d2fg.astype(np.float64))))
    elif case == "full":
        assert t.all()
    else:
        assert case == "empty" and not t.any()
    assert phi.dtype == np.float32 and np.array_equal(phi, want) and np.array_equal(phi, golden[name + ".phi"][b, c])
    if case in ("empty", "full"):
        assert not phi.any()
    else:
        # signs: positive on the background, at most 0 on the foreground (0 on its rim, where the nearest background voxel is a neighbour)
        assert (phi[~t] >= 1).all() and (phi[t] <= 0).all()


def test_float_and_byte_targets_give_the_same_map(golden):
    t = golden["box.t"]
    assert np.array_equal(br.signed_distance(t), br.signed_distance(t.astype(np.float32)))


# ---- the statements behind tests/test_gpu_sdt_extents.py ---------------------------------------------------------------------------
ODD = (65, 33, 40)
NEW_CASES = br.CORNERS + br.FACES + ("ramp", "comb", "speckle_98")


@pytest.mark.parametrize("name", list(br.SHAPES))
def test_chunked_equals_unchunked_on_the_fixture_shapes(golden, name):
    for t in golden[name + ".t"].reshape((-1,) + br.SHAPES[name][0][2:]):
        L = max(t.shape)
        for got, want in zip(br.squared_distances_chunked(t, 3 * 8 * L * L), br.squared_distances(t)):      # slabs of three lines
            assert got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("case", ["speckle_50", "two_blobs", "ramp", "empty"])
def test_chunked_equals_unchunked_on_odd_extents(case):
    t = br.make_case(case, ODD, 5)
    for max_bytes in (8 * 65 * 65, 1 << 20, 1 << 30):      # one line of the longest axis at a time; some; all at once
        for got, want in zip(br.squared_distances_chunked(t, max_bytes), br.squared_distances(t)):
            assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        br.squared_distances_chunked(t, 8 * 65 * 65 - 1)


@pytest.mark.parametrize("k", [1, 7, 64])
@pytest.mark.parametrize("name", ["sparse_fg", "sparse_bg"])
@pytest.mark.parametrize("shape", [(16, 16, 16), (8, 12, 20)])
def test_the_points_statement_equals_the_separable_one(shape, name, k):
    t, phi = br.sparse_case(name, shape, k, 40 + k)
    few = t if name == "sparse_fg" else 1 - t
    assert int(few.sum()) == k and t.dtype == np.uint8
    pts = [tuple(p) for p in np.argwhere(few)]
    d2 = br.squared_distances(t)
    assert np.array_equal(br.squared_distances_from_points(shape, pts, max_bytes=4096), d2[0 if name == "sparse_fg" else 1])
    assert np.array_equal(phi.view(np.uint32), br.phi_rule(t, *d2).view(np.uint32))
    assert (br.squared_distances_from_points(shape, []) == br.INF).all()


def test_the_new_named_cases_are_what_they_say():
    for k in range(8):
        t = br.make_case("corner_%d" % k, ODD, 0)
        assert t.sum() == 1 and t[tuple(s - 1 if (k >> a) & 1 else 0 for a, s in enumerate(ODD))] == 1
    for a in range(3):
        t = br.make_case("face_%d" % a, ODD, 0)
        assert t.sum() == t.size // ODD[a] and np.take(t, 0, axis=a).all()
        assert br.squared_distances(t)[0].max() == (ODD[a] - 1) ** 2
    t = br.make_case("ramp", ODD, 0)
    assert t[0, 0, 0] == 1 and t[-1, -1, -1] == 0 and t[10, 20, 15] == 1 and t[10, 20, 16] == 0      # 46 = (65 + 33 + 40) // 3
    t = br.make_case("comb", ODD, 0)
    assert [i for i in range(65) if t[i].all()] == list(range(0, 65, 7)) and t.sum() == 10 * 33 * 40
    t = br.make_case("speckle_98", ODD, 0)
    assert 0.975 < t.mean() < 0.985


@pytest.mark.parametrize("case", NEW_CASES)
def test_new_cases_equal_kervadecs_rule_on_scipy(case):
    """phi_rule of the separable statement == one_hot2dist on scipy's own float64 distances, rounded once to float32"""
    edt = pytest.importorskip("scipy.ndimage").distance_transform_edt
    t = br.make_case(case, ODD, 11)
    m = t != 0
    assert m.any() and not m.all()
    phi = br.phi_rule(t, *br.squared_distances_chunked(t))
    one_hot2dist = edt(~m) * ~m - (edt(m) - 1) * m
    assert phi.dtype == np.float32 and np.array_equal(phi, one_hot2dist.astype(np.float32))


@pytest.mark.parametrize("spec", [lr.SPECS[2], lr.SPECS[3]])
def test_closed_form_gradient_is_autograds(spec):
    rng = np.random.default_rng(3)
    shape = (2, 3, 5, 6, 7)
    z = torch.from_numpy(rng.standard_normal(shape)).double().requires_grad_(True)
    tn = br.tumour_targets(2, shape[2:], 4)
    t, phi = torch.from_numpy(tn).double(), torch.from_numpy(br.signed_distance(tn)).double()
    w = 0.37
    loss = br.torch_loss(z, t, phi, spec, w)
    loss.backward()
    c = br.closed_form(z, t, phi, spec, w)
    assert abs(c.loss - float(loss.detach())) <= 1e-12 and abs(c.base + c.bnd - c.loss) <= 1e-15
    assert float((c.dz - z.grad).abs().max()) <= 1e-12
    assert c.kphi == float(np.float32(w)) / z.numel() and c.sums.shape == (2, 3, 5)
    # the boundary term alone: its gradient with respect to p is k_phi phi
    p = torch.sigmoid(z.detach())
    c0 = br.closed_form(z, t, phi, spec, 0.0)
    assert c0.bnd == 0.0 and c0.loss == c0.base
    assert float(((c.dz - c0.dz) - c.kphi * phi * p * (1 - p)).abs().max()) <= 1e-15
