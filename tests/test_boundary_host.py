"""CPU: loss.BoundaryLoss without a device -- argument validation, the module-call error, the bindings of the new entry points."""
import ctypes as C

import pytest
import torch

from nas_3d_unet_amd import _lib
from nas_3d_unet_amd._lib import N3DError
from nas_3d_unet_amd.loss import BoundaryLoss, TverskyBCELoss, WeightedDiceLoss, signed_distance


def test_arguments():
    b = BoundaryLoss()
    assert isinstance(b.base, WeightedDiceLoss) and b.weight == 0.01
    tv = TverskyBCELoss(0.3, 0.7, 0.75, 0.5)
    b = BoundaryLoss(tv, 0.0)
    assert b.base is tv and b.spec is tv and b.weight == 0.0 and b.smooth == tv.smooth
    for bad in (-0.01, float("nan")):
        with pytest.raises(ValueError, match="weight >= 0"):
            BoundaryLoss(tv, bad)
        with pytest.raises(ValueError, match="weight >= 0"):
            b.set_weight(bad)
    for bad in (torch.nn.MSELoss(), BoundaryLoss(), "dice"):
        with pytest.raises(TypeError, match="base must be"):
            BoundaryLoss(bad)
    b.set_weight(0.25)      # before the device scalar exists: kept for its creation
    assert b.weight == 0.25 and b._wdev is None


def test_the_dice_base_is_stated_as_its_tversky_equivalent():
    """WeightedDiceLoss(smooth=s) is alpha = beta = 0.5, gamma = 1, smooth = s / 2 (loss.TverskyBCELoss), which is what the head forms"""
    sp = BoundaryLoss(WeightedDiceLoss(smooth=1e-4)).spec
    assert (sp.alpha, sp.beta, sp.gamma, sp.bce_weight, sp.smooth) == (0.5, 0.5, 1.0, 0.0, 5e-5)


def test_the_loss_is_no_part_of_a_state_dict():
    b = BoundaryLoss(TverskyBCELoss(), 0.5)
    assert len(b.state_dict()) == 0 and not list(b.parameters()) and not list(b.buffers())


def test_called_on_probabilities_it_names_the_routes():
    p = torch.rand(1, 3, 4, 4, 4)
    with pytest.raises(N3DError, match=r"Trainer\(loss=\.\.\.\) or forward_loss"):
        BoundaryLoss()(p, (p > 0.5).float())


def test_signed_distance_has_no_cpu_fallback():
    with pytest.raises(N3DError, match="no CPU fallback"):
        signed_distance(torch.zeros(1, 3, 4, 4, 4))
    with pytest.raises(N3DError, match="no CPU fallback"):
        BoundaryLoss.signed_distance(torch.zeros(1, 3, 4, 4, 4, dtype=torch.uint8))


def test_check_loss_head_refuses_other_heads():
    """a five-channel head and a head the fused kernel does not take: the reasons are raised without a device"""
    from nas_3d_unet_amd import head as H, prim_ops
    mk = lambda ci, co, k=1: torch.nn.Sequential(prim_ops.ConvOps(ci, co, kernel_size=k, ops_order="weight"), torch.nn.Sigmoid())
    H.check_loss_head(mk(12, 3), BoundaryLoss())
    with pytest.raises(N3DError, match="three-channel head"):
        H.check_loss_head(mk(12, 5), BoundaryLoss())
    with pytest.raises(N3DError, match="three-channel head"):
        H.check_loss_head(mk(12, 4), BoundaryLoss())
    with pytest.raises(N3DError, match="not one it takes"):
        H.check_loss_head(mk(12, 3, k=3), BoundaryLoss())
    with pytest.raises(N3DError, match="not one it takes"):
        H.check_loss_head(mk(10, 3), BoundaryLoss())


def test_prototypes():
    P = _lib.PROTOTYPES
    for name in ("n3d_target_sdt_workspace_bytes", "n3d_target_sdt", "n3d_head_bnd_fwd", "n3d_head_bnd_bwd"):
        assert name in P, name
    assert P["n3d_target_sdt_workspace_bytes"] == (C.c_size_t, [C.c_int] * 5)
    assert P["n3d_target_sdt"][0] is C.c_int and len(P["n3d_target_sdt"][1]) == 17
    # n3d_head_loss_fwd / _bwd plus (phi, three strides) -- and the device weight in the forward
    lf, lb = P["n3d_head_loss_fwd"][1], P["n3d_head_loss_bwd"][1]
    phi = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64]
    assert P["n3d_head_bnd_fwd"][1] == lf[:11] + phi + [C.c_void_p] + lf[11:]
    assert P["n3d_head_bnd_bwd"][1] == lb[:5] + phi + lb[5:]
