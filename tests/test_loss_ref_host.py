"""CPU: the fp64 reference of loss.TverskyBCELoss (tests/_loss_ref.py) -- the closed-form gradient the head kernels implement against
torch autograd of the literal formula, the Dice special case against the oracle's loss, the u == 0 convention -- and the module's
constructor validation."""
import numpy as np
import pytest
import torch

import _loss_ref as lr
from oracle import ref_path as orc


def _data(seed=0, shape=(2, 3, 5, 6, 7)):
    """random logits and {0, 1} targets; class 1 of sample 0 has an EMPTY target"""
    rng = np.random.default_rng(seed)
    z = torch.from_numpy(rng.standard_normal(shape) * 2.0)
    t = torch.from_numpy((rng.uniform(0, 1, shape) < 0.3).astype(np.float64))
    t[0, 1] = 0
    return z, t


@pytest.mark.parametrize("spec", lr.SPECS)
def test_closed_form_matches_autograd_of_the_literal_formula(spec):
    z, t = _data()
    zq = z.clone().requires_grad_(True)
    loss = lr.torch_loss(zq, t, spec)
    loss.backward()
    loss = loss.detach()
    c = lr.closed_form(z, t, spec)
    assert abs(float(c.loss) - float(loss)) <= 1e-12 * abs(float(loss))
    assert float((c.dz - zq.grad).abs().max()) <= 1e-12 * float(zq.grad.abs().max())
    assert float(c.sums[0, 1, 2]) == 0.0        # the empty target
    assert torch.isfinite(c.dz).all()


def test_tversky_half_half_is_the_reference_dice_loss():
    z, t = _data(1)
    s = 1e-6
    c = lr.closed_form(z, t, lr.Spec(0.5, 0.5, 1.0, 0.0, s / 2))
    ref = orc.dice_loss(torch.sigmoid(z), t, s)
    assert abs(float(c.loss) - float(ref)) <= 1e-14
    pq = torch.sigmoid(z).requires_grad_(True)
    orc.dice_loss(pq, t, s).backward()
    lp, dp = lr.closed_form_probs(torch.sigmoid(z), t, lr.Spec(0.5, 0.5, 1.0, 0.0, s / 2))
    assert abs(float(lp) - float(ref)) <= 1e-14
    assert float((dp - pq.grad).abs().max()) <= 1e-12 * float(pq.grad.abs().max())


@pytest.mark.parametrize("gamma", [0.75, 1.0, 2.0])
def test_an_empty_pair_contributes_nothing_and_has_no_nan(gamma):
    """P = A = T = 0 (p == 0 exactly: sigmoid(-800) underflows in fp64): u = 0, no loss contribution, a zero gradient, for every gamma --
    in the closed form and in autograd of the masked literal formula"""
    z, t = _data(2)
    z[1, 2] = -800.0
    t[1, 2] = 0
    spec = lr.Spec(0.3, 0.7, gamma, 0.0)
    c = lr.closed_form(z, t, spec)
    assert float(c.sums[1, 2, :3].abs().sum()) == 0.0
    assert float(c.u[1, 2]) == 0.0 and float(c.k2[1, 2]) == 0.0 and float(c.k0[1, 2]) == 0.0
    assert float(c.dz[1, 2].abs().max()) == 0.0
    assert torch.isfinite(c.dz).all() and np.isfinite(float(c.loss))
    others = [(b, k) for b in range(2) for k in range(3) if (b, k) != (1, 2)]
    assert abs(float(c.loss) - sum(float(c.u[b, k]) ** gamma for b, k in others) / 6) <= 1e-15
    zq = z.clone().requires_grad_(True)
    lr.torch_loss(zq, t, spec).backward()
    assert torch.isfinite(zq.grad).all() and float(zq.grad[1, 2].abs().max()) == 0.0


def test_constructor_validation():
    from nas_3d_unet_amd.loss import TverskyBCELoss
    ok = TverskyBCELoss(0.3, 0.7, 0.75, 0.5)
    assert (ok.alpha, ok.beta, ok.gamma, ok.bce_weight, ok.smooth) == (0.3, 0.7, 0.75, 0.5, 1e-6)
    TverskyBCELoss(0.0, 1.0)
    for kw in (dict(alpha=-0.1), dict(beta=-1.0), dict(alpha=0.0, beta=0.0), dict(gamma=0.0), dict(gamma=-1.0), dict(bce_weight=-0.5),
               dict(smooth=0.0), dict(smooth=-1e-6), dict(alpha=float("nan"))):
        with pytest.raises(ValueError):
            TverskyBCELoss(**kw)


def test_trainers_refuse_a_cross_entropy_term_the_head_cannot_form():
    """bce_weight > 0 needs the fused three-channel head: a trainer on another head raises at construction, with the reason
    (construction only: no kernel runs on the CPU)"""
    from nas_3d_unet_amd import nas, searched
    from nas_3d_unet_amd._lib import N3DError
    from nas_3d_unet_amd.loss import TverskyBCELoss, WeightedDiceLoss
    from nas_3d_unet_amd.train import SearchTrainer, Trainer
    gene = searched.Genotype(down=[("down_conv", 0), ("down_dil_conv", 1), ("down_conv", 1), ("conv", 2), ("dil_conv", 2), ("conv", 3)],
                             up=[("conv", 0), ("up_conv", 1), ("up_conv", 1), ("dil_conv", 2), ("conv", 3), ("up_dil_conv", 1)])
    with pytest.raises(N3DError, match="three-channel"):
        Trainer(searched.SearchedNet(4, 4, 2, 2, 3, True, gene), graph=False, loss=TverskyBCELoss(bce_weight=0.5))
    with pytest.raises(N3DError, match="three-channel"):
        SearchTrainer(nas.ShellNet(4, 4, 4, 2, 3, False, True), graph=False, loss=TverskyBCELoss(bce_weight=0.5))
    with pytest.raises(TypeError):
        Trainer(searched.SearchedNet(4, 4, 3, 2, 3, True, gene), graph=False, loss=torch.nn.BCELoss())
    # the Tversky / focal term alone works on every head the Dice mode takes, and the default stays the Dice loss
    assert isinstance(Trainer(searched.SearchedNet(4, 4, 2, 2, 3, True, gene), graph=False, loss=TverskyBCELoss(0.3, 0.7)).loss_fn, TverskyBCELoss)
    assert isinstance(Trainer(searched.SearchedNet(4, 4, 3, 2, 3, True, gene), graph=False).loss_fn, WeightedDiceLoss)
    tr = Trainer(searched.SearchedNet(4, 4, 3, 2, 3, True, gene), graph=False, loss=TverskyBCELoss(0.3, 0.7, 0.75, 0.5))
    assert tr._direct_ok()
