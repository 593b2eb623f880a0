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
