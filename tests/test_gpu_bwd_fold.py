"""GPU: a node's GroupNorm-epilogue backward rebuilt inside its data-gradient pair launch (n3d_gn_bwd_conv_data2,
conv_gemm16_gnpair_kernel) on the levels with at most 64 voxels per sample.

The launch must give what n3d_affine_act_bwd_small + n3d_conv_bwd_data2 give on the same operands, bit for bit: both d(raw), the
norms' parameter gradients, the conv-bias gradients and both input gradients.  Shapes: the node shapes of the 4 x 64^3 step (C = 64 at
4^3 and 2^3, C = 32 at 4^3) in every gather form their data gradients take (stride 1 with dilation 1 / 2, the forward-type stride-2
gather of a transposed conv's gradient whose tiles span two samples, the stride-2 gradient with parity lanes), B = 1 and 3 at 2^3
(a partly valid last tile, samples padded to whole waves).  Then the shapes the launch declines, and the trainers' schedule switch
kernels.GN_BWD_FOLD: same loss and parameters bit for bit with the switch on and off, and one n3d_affine_act_bwd_small call less per
folded node."""
import os
import sys

import pytest
import torch

from test_gpu_nets import build_net
from test_gpu_side import _batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, C, G, extent of d(raw), [(input extent, stride, dilation, transposed)] * 2): the conv of job i produced raw of term i
SHAPES = {
    "c64_4_s1_convT": (2, 64, 4, 4, [(4, 1, 1, False), (4, 2, 1, True)]),       # the transposed conv's gradient: 4^3 -> 2^3, two samples per tile
    "c64_4_d2_d1": (2, 64, 4, 4, [(4, 1, 2, False), (4, 1, 1, False)]),
    "c64_2_s1_s2": (2, 64, 4, 2, [(2, 1, 1, False), (4, 2, 1, False)]),         # stride-2 gradient 2^3 -> 4^3: den == 2, parity lanes
    "c32_4_s2_d1_d2": (2, 32, 2, 4, [(8, 2, 1, False), (8, 2, 2, False)]),      # 256 workgroups
    "c64_2_b1": (1, 64, 4, 2, [(2, 1, 1, False), (4, 2, 1, False)]),            # half a tile of rows
    "c64_2_b3": (3, 64, 4, 2, [(2, 1, 1, False), (4, 2, 1, False)]),            # a partly valid last tile
}


class _Node:
    """operands of one node backward: two terms on raws of one shape, the node gradient, the two convs' weights and input-gradient targets"""

    def __init__(self, B, Cc, G, e, convs, extras, seed=0, cin=None):
        from nas_3d_unet_amd import _lib, kernels as K
        self.K, self.G, self.B, self.C = K, G, B, Cc
        gen = torch.Generator(device="cuda").manual_seed(1000 + seed)
        rn = lambda *s: torch.randn(s, device="cuda", generator=gen)
        N = e * e * e
        self.dout = K.as_view(rn(B, e, e, e, Cc).permute(0, 4, 1, 2, 3))
        self.relu = [True, not extras]
        self.terms0, self.calls0 = [], []
        for k, (ei, stride, dil, transposed) in enumerate(convs):
            raw = K.as_view(rn(B, e, e, e, Cc).permute(0, 4, 1, 2, 3))
            gamma = torch.nn.Parameter(rn(Cc) * 0.5 + 1.0)
            beta = torch.nn.Parameter(rn(Cc) * 0.2)        # GroupNorm output around 0: about half of a * raw + b lies under the ReLU threshold
            with torch.no_grad():
                gamma[5] = 0.0
                beta[5] = -1.0                                 # channel 5: a = 0, b = -1 -- a ReLU mask that is zero everywhere
            st, rows = K.channel_stats(raw)
            a, b, mr, sumraw = K.gn_coeffs(st, rows, gamma, beta, B, Cc, G, N, 1e-5)[:4]
            cb = torch.nn.Parameter(torch.zeros(Cc, device="cuda")) if extras else None      # conv bias in front of the norm, fed from sumraw
            self.terms0.append(dict(raw=raw, a=a, b=b, mr=mr, sumraw=sumraw, gamma=gamma, beta=beta, wptr=None, relu=self.relu[k], conv_bias=cb))
            ci = cin if cin is not None else Cc
            if transposed:      # the gradient of a transposed conv y[i side] = convT(x[o side]): dy on the i side, dx on the o side
                assert ei == e
                g = K.conv_geom(B, e, e, e, Cc, ci, 3, stride, dil, dil)
                ed = g.Do
            else:
                g = K.conv_geom(B, ei, ei, ei, ci, Cc, 3, stride, dil, dil)
                assert (g.Do, g.Ho, g.Wo) == (e, e, e)
                ed = ei
            w = rn(Cc, ci, 3, 3, 3) * 0.1 if not transposed else rn(ci, Cc, 3, 3, 3) * 0.1
            dx0 = rn(B, ed, ed, ed, ci)
            x = rn(B, ed, ed, ed, ci)                        # the conv's input, ReLU mask source of its gradient
            acc = extras and k == 0
            mask = extras and k == 1 and not transposed
            self.calls0.append((g, w, dx0, _lib.ACCUMULATE if acc else 0, K.as_view(x.permute(0, 4, 1, 2, 3)) if mask else None, transposed))

    def operands(self, flags=0):
        K = self.K
        terms = [dict(t, draw=K.as_view(torch.full_like(t["raw"].t, 7.0))) for t in self.terms0]
        calls = [(g, t["draw"], w, K.as_view(dx0.clone().permute(0, 4, 1, 2, 3)), fl | flags, mask, None, tr)
                 for t, (g, w, dx0, fl, mask, tr) in zip(terms, self.calls0)]
        return terms, calls

    @staticmethod
    def tensors(terms, calls, outs):
        res = [t["draw"].t for t in terms] + [c[3].t for c in calls]
        for o in outs:
            res += [x for x in o if x is not None]
        return res


def _node(name, extras, **kw):
    B, Cc, G, e, convs = SHAPES[name]
    return _Node(B, Cc, G, e, convs, extras, seed=sorted(SHAPES).index(name) * 2 + int(extras), **kw)


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "extras"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fused_launch_equals_the_two_launches_bit_for_bit(name, extras):
    """extras: term 1 without ReLU, a conv bias fed from sumraw on both terms, N3D_ACCUMULATE on the first input gradient, a ReLU mask
    source on the second (where its conv is not transposed)"""
    from nas_3d_unet_amd import kernels as K
    nd = _node(name, extras)
    terms, calls = nd.operands()
    outs = K.affine_act_bwd_small(nd.dout, terms, nd.G)
    K.conv_bwd_data2(calls)
    ref = nd.tensors(terms, calls, outs)
    terms2, calls2 = nd.operands()
    fold = K.GnBwdFold(nd.dout, terms2, nd.G, calls2)
    assert fold.ok, "n3d_gn_bwd_conv_data2_ok declined %s" % name
    got = nd.tensors(terms2, calls2, fold.launch())
    torch.cuda.synchronize()
    assert len(got) == len(ref) == 4 + (6 if extras else 4)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.isfinite(b).all()
        assert torch.equal(a, b), "%s: output %d differs, max |d| = %.3e" % (name, i, float((a - b).abs().max()))
    assert not torch.equal(ref[0], torch.full_like(ref[0], 7.0))


def _declined(nd, flags=0):
    from nas_3d_unet_amd import kernels as K
    terms, calls = nd.operands(flags)
    fold = K.GnBwdFold(nd.dout, terms, nd.G, calls)
    assert hasattr(fold, "args") and not fold.ok
    before = [x.clone() for x in nd.tensors(terms, calls, fold.outs)]
    with pytest.raises(K.N3DError, match=r"\(-2\)"):      # N3D_ERR_UNSUPPORTED
        fold.launch()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(nd.tensors(terms, calls, fold.outs), before)), "a declined call wrote something"


def test_declined_shapes_touch_nothing():
    """the query says 0 and the entry point returns N3D_ERR_UNSUPPORTED with every output untouched: 8^3 at B = 2, 16 channels in two groups
    of 8, the bf16 matrix flag, a pair on the 4-way K-split plan (128 input channels at 8^3: 512 tiles)"""
    from nas_3d_unet_amd import _lib
    _declined(_Node(2, 64, 4, 8, [(8, 1, 1, False), (8, 1, 2, False)], False))
    _declined(_Node(2, 16, 2, 4, [(4, 1, 1, False), (4, 1, 2, False)], False))
    _declined(_node("c64_4_d2_d1", False), flags=_lib.MM_BF16)
    _declined(_Node(2, 64, 4, 4, [(8, 2, 1, False), (8, 2, 2, False)], False, cin=128))


def _steps(side, fold, x, t, record=False):
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd.train import Trainer
    prev, K.GN_BWD_FOLD = K.GN_BWD_FOLD, fold
    try:
        torch.manual_seed(5)
        net, _ = build_net("searched", "G_CONV", 4)
        tr = Trainer(net, graph=True, side_wgrad="force" if side else False)
        calls = None
        if record:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            from kernel_table import Recorder
            with Recorder() as rec:
                losses = [tr.step(x, t).clone()]
            calls = [n for n, _ in rec.calls]
        else:
            losses = [tr.step(x, t).clone()]
        losses += [tr.step(x, t).clone() for _ in range(2)]
        torch.cuda.synchronize()
        if side:
            tr.check_sync()
            assert tr.sync_timeouts() == 0 and tr._use_side
        return losses, tr.fp.flat.clone(), calls
    finally:
        K.GN_BWD_FOLD = prev


@pytest.mark.parametrize("side", [True, False], ids=["side-stream", "single-stream"])
def test_trainer_computes_the_same_bits_with_the_switch_on_and_off(side):
    """SearchedNet / G_CONV, batch 2, 4 x 64^3, three steps from the captured graphs.  In the side-stream schedule every folded node
    issues one n3d_affine_act_bwd_small call less (the calls recorded while the first step is captured); the single-stream schedule
    keeps its two launches per node (epilogue backward, then data and weight gradients of both convs in one)."""
    x, t = _batch(71, size=64)
    l1, p1, c1 = _steps(side, True, x, t, record=True)
    l0, p0, c0 = _steps(side, False, x, t, record=True)
    assert all(torch.equal(a, b) for a, b in zip(l1, l0))
    assert torch.equal(p1, p0)
    small = lambda c: sum(1 for n in c if n == "n3d_affine_act_bwd_small")
    fused = lambda c: sum(1 for n in c if n == "n3d_gn_bwd_conv_data2")
    print("n3d_affine_act_bwd_small calls: switch on %d, off %d; fused launches %d" % (small(c1), small(c0), fused(c1)))
    assert fused(c0) == 0
    assert small(c0) - small(c1) == fused(c1)
    assert (fused(c1) > 0) == side
