"""Per-launch A/B of the node backward on the levels with <= 64 voxels per sample (4 x 64^3 step: up-cell 0, down-cells 3 and 2):
n3d_affine_act_bwd_small + n3d_conv_bwd_data2 back to back against the one launch n3d_gn_bwd_conv_data2, pre-packed weights, HIP-graph
replay + HIP events (conv_ab.timed: 40 dependent repetitions per replay).  One line per shape class: us of the two launches, us of the
fused one, the difference.  The schedule keeps the fold for a shape class only where the fused launch is the faster one.
N3D_LIB=<another libn3d.so> times another build."""
import os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch
from nas_3d_unet_amd import kernels as K, _lib
from conv_ab import timed

dev = torch.device("cuda", 0)
# conv forms: (input extent relative to d(raw)'s extent e, stride, dilation, transposed)
S1D1, S1D2 = (1, 1, 1, False), (1, 1, 2, False)
S2D1, S2D2 = (2, 2, 1, False), (2, 2, 2, False)      # stride-2 convs: gradient from e^3 to (2e)^3
UP = (1, 2, 1, True)                                 # transposed conv: gradient from e^3 to (e/2)^3
CASES = [("up0   C=64 4^3", 64, 4, 4, [(S1D1, S1D2), (S1D1, UP), (UP, UP)]),
         ("down3 C=64 2^3", 64, 4, 2, [(S1D1, S1D2), (S1D1, S2D1), (S2D1, S2D2)]),
         ("down2 C=32 4^3", 32, 2, 4, [(S1D1, S1D2), (S1D1, S2D1), (S2D1, S2D2)])]


def name(f):
    return "convT" if f[3] else "s%dd%d" % (f[1], f[2])


def case(label, Cc, G, e, forms, B=2):
    rn = lambda *s: torch.randn(s, device=dev)
    dout = K.as_view(rn(B, e, e, e, Cc).permute(0, 4, 1, 2, 3))
    terms, calls = [], []
    for (rel, stride, dil, tr) in forms:
        raw = K.as_view(rn(B, e, e, e, Cc).permute(0, 4, 1, 2, 3))
        gamma, beta = torch.nn.Parameter(rn(Cc) * 0.5 + 1.0), torch.nn.Parameter(rn(Cc) * 0.2)
        st, rows = K.channel_stats(raw)
        a, b, mr, sumraw = K.gn_coeffs(st, rows, gamma, beta, B, Cc, G, e ** 3, 1e-5)[:4]
        draw = K.like(raw)
        terms.append(dict(raw=raw, a=a, b=b, mr=mr, sumraw=sumraw, gamma=gamma, beta=beta, wptr=None, relu=True, conv_bias=None, draw=draw))
        if tr:
            g = K.conv_geom(B, e, e, e, Cc, Cc, 3, stride, dil, dil)
            ed = g.Do
        else:
            g = K.conv_geom(B, e * rel, e * rel, e * rel, Cc, Cc, 3, stride, dil, dil)
            ed = e * rel
        w = rn(Cc, Cc, 3, 3, 3) * 0.1
        dx = K.as_view(rn(B, ed, ed, ed, Cc).permute(0, 4, 1, 2, 3))
        calls.append((g, draw, w, dx, 0, None, None, tr))
    ctx = K.StepContext(dev)
    with K.step_context(ctx):
        K.affine_act_bwd_small(dout, terms, G)
        K.conv_bwd_data2(calls)
        ctx.freeze()
        ctx.pack_all()

        def two():
            K.affine_act_bwd_small(dout, terms, G)
            K.conv_bwd_data2(calls)
        t2 = timed(two)
        t1s = timed(lambda: K.affine_act_bwd_small(dout, terms, G))
        fold = K.GnBwdFold(dout, terms, G, calls)
        if not fold.ok:
            print("%s %s + %s: two launches %6.2f us; the fused launch declines" % (label, name(forms[0]), name(forms[1]), t2), flush=True)
            return
        t1 = timed(fold.launch)
    print("%s %-6s+ %-6s: small %5.2f us, small + pair %6.2f us, fused %6.2f us, saved %+5.2f us" %
          (label, name(forms[0]), name(forms[1]), t1s, t2, t1, t2 - t1), flush=True)


if __name__ == "__main__":
    print("lib:", _lib.LIB_PATH)
    torch.manual_seed(3)
    for label, Cc, G, e, pairs in CASES:
        for forms in pairs:
            case(label, Cc, G, e, forms)
