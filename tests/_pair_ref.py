"""fp64 torch-CPU restatement of the two-term GroupNorm epilogues (n3d_affine_act_gn2 and its family, include/n3d.h "node-level pair
epilogues"), the case table of test_gpu_pair_reference.py with the route every case is meant to reach, and a Python restatement of the
row mapping (ew_map, csrc/n3d_common.h) those routes follow from.  Shared by test_pair_ref_host.py (CPU) and the GPU test.

The pair is two _epilogue_ref.term_reference calls:
  node mode         y  = [prev +] w0 * act0(GN0(raw0)) + w1 * act1(GN1(raw1));          both terms run backward under the same dout
  two-output mode   y0 = [prev0 +] w0 * act0(GN0(raw0)),  y1 = w1 * act1(GN1(raw1));   term 1 runs backward under dout1
(the two preprocess ops of a cell, cell.py:47-50; N3D_ACCUMULATE reaches `out` only, `out1` is overwritten).

A term's reference is computed once per (term, ReLU, output gradient) with weight 1 and scaled by the weight afterwards: y, d(raw),
dgamma, dbeta and dbias_conv are linear in w; z, the reduction sums, dalpha = <dout, z> and the saved forward coefficients do not depend on
it (test_pair_ref_host.py checks the scaled form against autograd with the weight as a leaf)."""
import collections

import numpy as np

import _epilogue_ref as R

W0, W1 = 0.37, 0.81        # the device scalars behind the two `wptr`s (w0 != w1)

# ------------------------------------------------------------------------------------------ the row mapping, restated
EwMap = collections.namedtuple("EwMap", "cpb vpb iters vpc rows")


def cdiv(a, b):
    return -(-a // b)


def ew_map(N, C):
    """csrc/n3d_common.h ew_map: C / 4 channel quads per voxel, 256 / cpb voxels per block-iteration; at most 1024 rows per sample;
    one iteration up to 8 block-iterations per sample, two up to 256, else at least four (sixteen where C / 4 is no power of two)"""
    cpb = max(C // 4, 1)
    vpb = max(256 // cpb, 1)
    nit = cdiv(N, vpb)
    it = cdiv(nit, 1024)
    mi = 16 if cpb & (cpb - 1) else 4
    if nit <= 8:
        mi = 1
    elif nit <= 256 and mi > 2:
        mi = 2
    if it < mi:
        it = max(nit, 1) if nit < mi else mi
    vpc = vpb * it
    return EwMap(cpb, vpb, it, vpc, cdiv(N, vpc))


def pair_shape_ok(C, G):
    """elementwise.hip pair_shape_ok, G already the number of groups"""
    return 4 <= C <= 64 and C & (C - 1) == 0 and G >= 1 and C % G == 0 and C // G <= 16


def small_mode(B, N, C, G):
    """elementwise.hip n3d_bwd_small_mode: 1 = one workgroup per group (B * roundup(N * cg / 4, 64) <= 2048 quads), 2 = one per (group,
    sample) (B = 2..4, roundup(N * cg / 4, 64) <= 2048), 0 = not taken (always with padded channels)"""
    if G < 0 or not pair_shape_ok(C, G) or not 1 <= B <= 4 or not 1 <= N <= 4096:
        return 0
    per_b = cdiv(N * (C // G // 4), 64) * 64
    if B * per_b <= 2048:
        return 1
    return 2 if B >= 2 and per_b <= 2048 else 0


FUSED_MAX_ROWS = 64     # n3d_fused_max_rows() today; the tests read the library's value and compare
GNF_MAXB = 4            # samples the fused backward's parameter-gradient wave takes


def routes(c, fused_max_rows=FUSED_MAX_ROWS):
    """what kernels.py and the library do with a case: (rows, iters, ragged, fused, small)
    fused: n3d_affine_act_gn2 / n3d_affine_act_bwd_apply_gn2 take it (else n3d_gn_coeffs2 + n3d_affine_act2 and n3d_gn_bwd_coeffs2 +
    n3d_affine_act_bwd_apply2); ragged: the last block of a sample is partial; small: n3d_bwd_small_mode"""
    N = int(np.prod(c.shape))
    m = ew_map(N, c.C)
    fused = pair_shape_ok(c.C, R.n_groups(c.G)) and m.rows <= fused_max_rows and c.B <= GNF_MAXB
    ragged = N % m.rows != 0 or (N // m.rows) % m.vpb != 0
    return m.rows, m.iters, ragged, fused, small_mode(c.B, N, c.C, c.G)


# ------------------------------------------------------------------------------------------ cases
Pair = collections.namedtuple("Pair", "C shape B G rows iters ragged fused small variants note")
# A variant is one forward + backward of the pair with these options:
#   relu = (term 0, term 1); w = which terms carry a device weight scalar (W0 / W1); two = two-output mode (out1, dout1); acc =
#   N3D_ACCUMULATE in the forward; dalpha = both terms' weight gradients requested (never taken by the one-launch backward: the wrapper
#   must route such a call to the two-launch forms); bias = dbias_conv of both terms (dropped where G < 0: include/n3d.h forbids it)
Variant = collections.namedtuple("Variant", "relu w two acc dalpha bias")
VARIANTS = {
    "node": Variant((True, False), (True, True), False, False, False, True),
    "node_acc": Variant((False, True), (False, True), False, True, True, True),           # only w1
    "two": Variant((False, False), (True, True), True, False, False, True),
    "two_acc": Variant((True, True), (True, True), True, True, True, False),
    # the remaining ReLU pairs and the lone w1 without dalpha, for the cases the one-launch backward takes
    "node_w1": Variant((False, True), (False, True), False, True, False, True),
    "two_tt": Variant((True, True), (True, True), True, True, False, True),
}
ALL = ("node", "node_acc", "two", "two_acc")
SMALL = ALL + ("node_w1", "two_tt")
# rows / iters / ragged / fused / small: what today's row mapping gives (asserted against the library on the CPU and again on the GPU, so
# that a retuning reads "route moved, pick a new shape").  P6 and P9 cut their samples into whole blocks; the ragged last block of the
# separate-coefficient route is P8's, P10's and P11's.  P9 and P11 run two variants (their fp64 reference is most of their time).
PAIR_CASES = {
    "P1": Pair(4, (8, 8, 16), 2, 1, 4, 1, False, True, 1, SMALL, "fused, 1 iteration; one-launch mode 1 with 2 quads per thread"),
    "P2": Pair(16, (6, 10, 14), 3, 1, 7, 2, True, True, 0, ALL, "fused, 2 iterations, ragged; the GNF_MAXB leader with one slot off"),
    "P3": Pair(64, (4, 4, 6), 4, 4, 6, 1, False, True, 1, SMALL, "fused, four groups, B = 4 (leader full); one-launch mode 1"),
    "P4": Pair(32, (8, 8, 8), 2, 2, 8, 2, False, True, 2, SMALL, "one-launch mode 2 (one workgroup per group and sample)"),
    "P5": Pair(8, (6, 10, 14), 2, -6, 7, 1, True, True, 0, ALL, "padded channels on the fused route"),
    "P6": Pair(4, (32, 32, 33), 2, 1, 66, 2, False, False, 0, ALL, "66 rows > 64: separate coefficients, gn_bwd_coeffs_kernel<2>"),
    "P7": Pair(8, (4, 8, 8), 5, 1, 2, 1, False, False, 0, ALL, "2 rows but B = 5: separate coefficients, gn_bwd_coeffs_kernel<GNB_BP>"),
    "P8": Pair(64, (14, 18, 22), 2, 4, 87, 4, True, False, 0, ALL, "iters == 4, ragged, separate coefficients"),
    "P9": Pair(64, (40, 40, 41), 1, 4, 820, 5, False, False, 0, ("node_acc", "two"), "iters == 5: the beyond-four loops, last group partial"),
    "P10": Pair(8, (6, 10, 14), 5, -6, 7, 1, True, False, 0, ALL, "padded channels on the separate-coefficient route"),
    # at iters == 5 only the first slot of the second group of four is live, so a mix-up BETWEEN the slots of that group cannot show in
    # P9; N = 82720 has iters == 6 (two live slots, two dead) and a ragged last block
    "P11": Pair(64, (40, 44, 47), 1, 4, 862, 6, True, False, 0, ("node_acc", "two"), "iters == 6: two live slots in the beyond-four loops, ragged"),
    # P1, P3 and P4 all hold two quads per thread in the one-launch kernel (more than 1024 quads per workgroup); these two hold one
    "P12": Pair(8, (4, 8, 8), 2, 1, 2, 1, False, True, 1, SMALL, "one-launch mode 1 with 1 quad per thread (P7's shape at B = 2)"),
    "P13": Pair(16, (4, 8, 8), 3, 1, 4, 1, False, True, 2, SMALL, "one-launch mode 2 with 1 quad per thread, three samples"),
}
LARGE_CASES = ("P9", "P11")
BF16_CASES = ("P1", "P2", "P6", "P8")

_inputs = {}        # one case at a time (P9 and P11 hold 17 and 21 MB per tensor)
_terms = {}


def pair_inputs(cid):
    """raw / gamma / beta of both terms (margin_inputs on both: either may carry a ReLU), the two output gradients, previous contents"""
    if cid in _inputs:
        return _inputs[cid]
    _inputs.clear()
    _terms.clear()
    c = PAIR_CASES[cid]
    rng = np.random.default_rng(6000 + list(PAIR_CASES).index(cid))
    real = R.real_channels(c.C, c.G)
    terms = []
    for _ in range(2):
        gamma, beta = R.draw_gamma_beta(rng, c.C, real)
        raw, zmin, passes = R.margin_inputs(R.draw_tensor(rng, c.B, c.C, c.shape, real, 1.5, 0.3), c.G, gamma, beta)
        terms.append(dict(raw=raw, gamma=gamma, beta=beta, zmin=zmin, passes=passes))
    # (padded channels of the output gradients and of the previous node content are zero, as in a padded net)
    inp = dict(terms=terms, dout=R.draw_tensor(rng, c.B, c.C, c.shape, real), dout1=R.draw_tensor(rng, c.B, c.C, c.shape, real),
               prev=R.draw_tensor(rng, c.B, c.C, c.shape, real), prev1=R.draw_tensor(rng, c.B, c.C, c.shape, real))
    _inputs[cid] = inp
    return inp


def scale_term(ref, w):
    """the weight-1 reference of a term under the weight w (None = 1): what is linear in w is scaled, the rest is shared"""
    s = R.w64(w)
    out = dict(ref)
    for k in ("y", "draw", "dgamma", "dbeta", "dbias_conv"):
        out[k] = ref[k] * s
    return out


def pair_term(cid, k, relu, w, own_dout=False):
    """fp64 reference of term k of a case under weight w and the output gradient dout (own_dout: dout1); cached per case.  With padded
    channels `draw` is the padded twin's (twin_draw: the group's coupling term on the padded channels), after checking that it is
    GroupNorm(1, real)'s on the real ones."""
    c, inp = PAIR_CASES[cid], pair_inputs(cid)
    key = (cid, k, bool(relu), bool(own_dout))
    ref = _terms.get(key)
    if ref is None:
        t = inp["terms"][k]
        d = inp["dout1"] if own_dout else inp["dout"]
        ref = R.term_reference(t["raw"], t["gamma"], t["beta"], c.G, relu, None, d)
        if c.G < 0:
            real = R.real_channels(c.C, c.G)
            twin = R.twin_draw(t["raw"], t["gamma"], t["beta"], c.G, relu, None, d)
            err = np.abs(twin[:, :real] - ref["draw"][:, :real]).max()
            assert err <= 1e-9 * np.abs(ref["draw"]).max(), "the twin formula against GroupNorm(1, real): %.3e" % err
            ref["draw"] = twin
        _terms[key] = ref
    return scale_term(ref, w)


def variant_weights(v):
    return (W0 if v.w[0] else None, W1 if v.w[1] else None)


def pair_reference(cid, v):
    """(out, out1 | None, [term 0, term 1]) of a variant in fp64"""
    inp = pair_inputs(cid)
    w = variant_weights(v)
    t0 = pair_term(cid, 0, v.relu[0], w[0], False)
    t1 = pair_term(cid, 1, v.relu[1], w[1], v.two)
    prev = inp["prev"].astype(np.float64) if v.acc else 0.0
    if v.two:
        return t0["y"] + prev, t1["y"], [t0, t1]          # out1 is overwritten whatever the flags say
    return (t0["y"] + t1["y"]) + prev, None, [t0, t1]
