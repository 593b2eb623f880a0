"""The small pointwise conv kernel (conv_point_kernel: the fp32 1x1x1 convs with channel counts and pitches that are multiples of 4 which
neither the MFMA family nor the 1x1x1 streaming kernel takes) against
  * the generic gather path the same call takes under N3D_NO_POINTWISE: outputs and statistics rows BIT FOR BIT (torch.equal) --
    the kernel performs the gather kernel's fp32 operations in its order;
  * an fp64 torch-CPU conv of the same inputs, with the conv tolerances of DESIGN.md section 2 (forward 2e-5 max|ref|, data gradient
    5e-5 max|ref|);
and the two-job entry points (n3d_conv_fwd2 / n3d_conv_bwd_data2) against their two single calls, bit for bit.  Which path a call
took is read from n3d_conv_pointwise_counts.  B = 2; volumes of 288 voxels (4 x 6 x 12: two voxel blocks, the second ragged);
strided cases 8 x 6 x 12 -> 4 x 3 x 6 for the forward and the reverse for the data gradient."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import assert_close

pytestmark = pytest.mark.gpu

B = 2
GEOMS = [(24, 16, 1), (48, 8, 1), (12, 16, 2), (24, 32, 2), (20, 12, 1), (16, 24, 1)]   # (Ci, Co, stride)


def in_shape(stride):
    return (4, 6, 12) if stride == 1 else (8, 6, 12)


def out_shape(stride):
    return tuple((d - 1) // stride + 1 for d in in_shape(stride))


def _mk(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(ci, co, stride):
    """seeded inputs of one geometry and their fp64 torch-CPU results (computed once, shared, never written)"""
    seed = 1000 * ci + 10 * co + stride
    c = dict(x=_mk((B, ci) + in_shape(stride), seed), w=_mk((co, ci, 1, 1, 1), seed + 1, 1.0 / np.sqrt(ci)), b=_mk((co,), seed + 2, 0.1),
             gate=np.abs(_mk((B, ci), seed + 3)) + 0.5, dy=_mk((B, co) + out_shape(stride), seed + 4), base=_mk((B, ci) + in_shape(stride), seed + 5))
    x64, w64 = torch.from_numpy(c["x"]).double(), torch.from_numpy(c["w"]).double()
    c["y_plain"] = F.conv3d(x64, w64, None, stride=stride)
    u = F.relu(x64) * torch.from_numpy(c["gate"]).double()[:, :, None, None, None]
    c["y_extras"] = F.conv3d(u, w64, torch.from_numpy(c["b"]).double(), stride=stride)
    xg = x64.clone().requires_grad_(True)
    (F.conv3d(xg, w64, None, stride=stride) * torch.from_numpy(c["dy"]).double()).sum().backward()
    c["dx_plain"] = xg.grad
    # ACCUMULATE + ReLU mask of the conv input + output gate: dx = base + gate * [x > 0] * (W^T dy)
    c["dx_extras"] = (torch.from_numpy(c["base"]).double()
                      + xg.grad * (x64 > 0) * torch.from_numpy(c["gate"]).double()[:, :, None, None, None])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def geom(K, ci, co, stride):
    d, h, w = in_shape(stride)
    return K.conv_geom(B, d, h, w, ci, co, 1, stride, 1, 0)


def view(K, a, wide=0):
    """an NDHWC view of the array on the GPU; wide: as a channel slice of a buffer with `wide` more channels (pitch > channels)"""
    dev = torch.device("cuda")
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if not wide:
        return K.as_view(t)
    buf = K.empty_ndhwc(a.shape[0], a.shape[1] + wide, *a.shape[2:], dev, torch.float32)
    buf.fill_(7.0)
    sl = buf[:, 4:4 + a.shape[1]]
    sl.copy_(t)
    v = K.as_view(sl)
    assert v.ld == a.shape[1] + wide and v.t.data_ptr() == sl.data_ptr()
    v.t._wide = buf       # the whole buffer, for the check that nothing outside the slice was written
    return v


def empty_view(K, shape, wide=0):
    return view(K, np.zeros(shape, np.float32), wide)


def counted(K, fn):
    """run fn, return (pointwise launches, jobs) it added"""
    l0, j0 = K.conv_pointwise_counts()
    fn()
    l1, j1 = K.conv_pointwise_counts()
    return l1 - l0, j1 - j0


def run_fwd(K, ci, co, stride, mode, flags):
    c = case(ci, co, stride)
    g = geom(K, ci, co, stride)
    dev = torch.device("cuda")
    wide = 8 if mode == "sliced" else 0
    x, y = view(K, c["x"], wide), empty_view(K, (B, co) + out_shape(stride), wide)
    w = torch.from_numpy(c["w"]).to(dev)
    stats = None
    if mode == "extras":
        rows = K.conv_stats_rows(g, False)
        assert rows == -(-int(np.prod(out_shape(stride))) // 256)
        stats = torch.zeros((B, rows, co, 2), dtype=torch.float64, device=dev)
        bias, gate = torch.from_numpy(c["b"]).to(dev), torch.from_numpy(c["gate"]).to(dev)
        K.conv_fwd(g, x, w, bias, y, K.RELU_IN | flags, gate, stats, False)
    else:
        K.conv_fwd(g, x, w, None, y, flags, None, None, False)
    torch.cuda.synchronize()
    return y, stats


@pytest.mark.parametrize("mode", ["plain", "extras", "sliced"])
@pytest.mark.parametrize("ci,co,stride", GEOMS)
def test_forward(ci, co, stride, mode):
    from nas_3d_unet_amd import kernels as K
    c = case(ci, co, stride)
    res = {}
    n_new = counted(K, lambda: res.setdefault("new", run_fwd(K, ci, co, stride, mode, 0)))
    n_old = counted(K, lambda: res.setdefault("old", run_fwd(K, ci, co, stride, mode, K.NO_POINTWISE)))
    assert n_new == (1, 1), "the pointwise kernel did not take an eligible call: %s" % (n_new,)
    assert n_old == (0, 0), "N3D_NO_POINTWISE did not send the call down the gather path: %s" % (n_old,)
    (y, st), (y0, st0) = res["new"], res["old"]
    assert torch.equal(y.t, y0.t), "forward differs from the gather path"
    ref = c["y_extras"] if mode == "extras" else c["y_plain"]
    assert_close(y.t.double(), ref, 2e-5, "y")
    if mode == "sliced":
        full = y.t._wide
        assert float(full[:, :4].min()) == 7.0 and float(full[:, 4 + co:].max()) == 7.0, "wrote outside its channel slice"
    if st is not None:
        assert torch.equal(st, st0), "statistics rows differ from the gather path"
        tot = st.sum(dim=1).cpu().numpy()
        assert_close(tot[..., 0], ref.sum(dim=(2, 3, 4)).numpy(), 1e-5, "stats sum")
        assert_close(tot[..., 1], (ref * ref).sum(dim=(2, 3, 4)).numpy(), 1e-5, "stats sumsq")


def run_bwd(K, ci, co, stride, mode, flags):
    c = case(ci, co, stride)
    g = geom(K, ci, co, stride)
    dev = torch.device("cuda")
    dy, w = view(K, c["dy"]), torch.from_numpy(c["w"]).to(dev)
    if mode == "extras":
        dx = view(K, c["base"])
        K.conv_bwd_data(g, dy, w, dx, K.ACCUMULATE | flags, view(K, c["x"]), torch.from_numpy(c["gate"]).to(dev), False)
    else:
        dx = view(K, np.full((B, ci) + in_shape(stride), 3.0, np.float32))     # stale content: must be overwritten, unreached voxels by 0
        K.conv_bwd_data(g, dy, w, dx, flags, None, None, False)
    torch.cuda.synchronize()
    return dx


def unreached(stride):
    """mask over the input volume of the voxels no output voxel of a stride-2 pointwise conv reads"""
    d, h, w = in_shape(stride)
    m = np.ones((d, h, w), bool)
    m[::stride, ::stride, ::stride] = False
    return torch.from_numpy(m)


@pytest.mark.parametrize("mode", ["plain", "extras"])
@pytest.mark.parametrize("ci,co,stride", GEOMS)
def test_data_gradient(ci, co, stride, mode):
    from nas_3d_unet_amd import kernels as K
    c = case(ci, co, stride)
    res = {}
    n_new = counted(K, lambda: res.setdefault("new", run_bwd(K, ci, co, stride, mode, 0)))
    n_old = counted(K, lambda: res.setdefault("old", run_bwd(K, ci, co, stride, mode, K.NO_POINTWISE)))
    assert n_new == (1, 1), "the pointwise kernel did not take an eligible call: %s" % (n_new,)
    assert n_old == (0, 0), "N3D_NO_POINTWISE did not send the call down the gather path: %s" % (n_old,)
    dx, dx0 = res["new"], res["old"]
    assert torch.equal(dx.t, dx0.t), "data gradient differs from the gather path"
    assert_close(dx.t.double(), c["dx_extras"] if mode == "extras" else c["dx_plain"], 5e-5, "dx")
    if stride == 2:
        m = unreached(stride)
        got = dx.t.cpu()[:, :, m]
        if mode == "plain":
            assert int((got.view(torch.int32) & 0x7fffffff).max()) == 0, "an unreached voxel is not 0"
        else:
            assert torch.equal(got, torch.from_numpy(c["base"])[:, :, m]), "accumulate changed an unreached voxel"


def fwd_call(K, ci, co, stride, flags, extras, dev):
    c = case(ci, co, stride)
    g = geom(K, ci, co, stride)
    y = empty_view(K, (B, co) + out_shape(stride))
    stats = torch.zeros((B, K.conv_stats_rows(g, False), co, 2), dtype=torch.float64, device=dev) if extras else None
    bias = torch.from_numpy(c["b"]).to(dev) if extras else None
    gate = torch.from_numpy(c["gate"]).to(dev) if extras else None
    return (g, view(K, c["x"]), torch.from_numpy(c["w"]).to(dev), bias, y, (K.RELU_IN if extras else 0) | flags, gate, stats, False)


# (job 0, job 1, extras of job 0 / 1): a cell's preprocess pair, a pair that differs in everything, the same geometry twice
FWD_PAIRS = [((12, 16, 2), (24, 16, 1), True, True), ((48, 8, 1), (24, 32, 2), False, True), ((20, 12, 1), (20, 12, 1), True, False)]


@pytest.mark.parametrize("j0,j1,e0,e1", FWD_PAIRS)
def test_forward_pair_is_one_launch_and_bit_identical(j0, j1, e0, e1):
    from nas_3d_unet_amd import kernels as K
    dev = torch.device("cuda")
    pair = [fwd_call(K, *j0, 0, e0, dev), fwd_call(K, *j1, 0, e1, dev)]
    assert counted(K, lambda: K.conv_fwd2(pair)) == (1, 2), "two eligible forward convs did not share one pointwise launch"
    single = [fwd_call(K, *j0, 0, e0, dev), fwd_call(K, *j1, 0, e1, dev)]
    old = [fwd_call(K, *j0, K.NO_POINTWISE, e0, dev), fwd_call(K, *j1, K.NO_POINTWISE, e1, dev)]
    for call in single + old:
        K.conv_fwd(*call)
    assert counted(K, lambda: K.conv_fwd2([fwd_call(K, *j0, K.NO_POINTWISE, e0, dev), fwd_call(K, *j1, K.NO_POINTWISE, e1, dev)])) == (0, 0)
    torch.cuda.synchronize()
    for k, (geo, ex) in enumerate(((j0, e0), (j1, e1))):
        assert torch.equal(pair[k][4].t, single[k][4].t), "job %d of the pair differs from its single launch" % k
        assert torch.equal(pair[k][4].t, old[k][4].t), "job %d of the pair differs from the gather path" % k
        if ex:
            assert torch.equal(pair[k][7], single[k][7]) and torch.equal(pair[k][7], old[k][7]), "statistics rows of job %d differ" % k
        assert_close(pair[k][4].t.double(), case(*geo)["y_extras" if ex else "y_plain"], 2e-5, "y of job %d" % k)


def test_forward_pair_with_one_ineligible_job():
    """a 3x3x3 conv beside an eligible pointwise conv: two launches, the eligible one on the pointwise kernel"""
    from nas_3d_unet_amd import kernels as K
    dev = torch.device("cuda")
    x3, w3 = _mk((B, 4, 4, 6, 12), 77), _mk((4, 4, 3, 3, 3), 78, 0.1)
    g3 = K.conv_geom(B, 4, 6, 12, 4, 4, 3, 1, 1, 1)

    def k3_call():
        return (g3, view(K, x3), torch.from_numpy(w3).to(dev), None, empty_view(K, (B, 4, 4, 6, 12)), 0, None, None, False)

    for order in (0, 1):
        pair = [fwd_call(K, 24, 16, 1, 0, True, dev), k3_call()]
        single = [fwd_call(K, 24, 16, 1, 0, True, dev), k3_call()]
        if order:
            pair.reverse(), single.reverse()
        assert counted(K, lambda: K.conv_fwd2(pair)) == (1, 1)
        for call in single:
            K.conv_fwd(*call)
        torch.cuda.synchronize()
        for k in range(2):
            assert torch.equal(pair[k][4].t, single[k][4].t), "call %d differs from its single launch" % k
    y3 = F.conv3d(torch.from_numpy(x3).double(), torch.from_numpy(w3).double(), None, padding=1)
    assert_close(pair[0][4].t.double(), y3, 2e-5, "3x3x3 y")


def bwd_call(K, ci, co, stride, flags, extras, dev, dx=None):
    c = case(ci, co, stride)
    g = geom(K, ci, co, stride)
    if dx is None:
        dx = view(K, c["base"]) if extras else view(K, np.full((B, ci) + in_shape(stride), 3.0, np.float32))
    relu_src = view(K, c["x"]) if extras else None
    gate = torch.from_numpy(c["gate"]).to(dev) if extras else None
    return (g, view(K, c["dy"]), torch.from_numpy(c["w"]).to(dev), dx, (K.ACCUMULATE if extras else 0) | flags, relu_src, gate, False)


# the backward pairs of the benchmarked cells (neighbours with distinct targets), and a pair that differs in everything
BWD_PAIRS = [((24, 16, 1), (12, 16, 2), True, True), ((24, 32, 2), (48, 8, 1), False, True), ((16, 24, 1), (20, 12, 1), False, False)]


@pytest.mark.parametrize("j0,j1,e0,e1", BWD_PAIRS)
def test_data_gradient_pair_is_one_launch_and_bit_identical(j0, j1, e0, e1):
    from nas_3d_unet_amd import kernels as K
    dev = torch.device("cuda")
    pair = [bwd_call(K, *j0, 0, e0, dev), bwd_call(K, *j1, 0, e1, dev)]
    assert counted(K, lambda: K.conv_bwd_data2(pair)) == (1, 2), "two eligible data gradients did not share one pointwise launch"
    single = [bwd_call(K, *j0, 0, e0, dev), bwd_call(K, *j1, 0, e1, dev)]
    old = [bwd_call(K, *j0, K.NO_POINTWISE, e0, dev), bwd_call(K, *j1, K.NO_POINTWISE, e1, dev)]
    for call in single + old:
        K.conv_bwd_data(*call)
    torch.cuda.synchronize()
    for k, (geo, ex) in enumerate(((j0, e0), (j1, e1))):
        assert torch.equal(pair[k][3].t, single[k][3].t), "job %d of the pair differs from its single launch" % k
        assert torch.equal(pair[k][3].t, old[k][3].t), "job %d of the pair differs from the gather path" % k
        assert_close(pair[k][3].t.double(), case(*geo)["dx_extras" if ex else "dx_plain"], 5e-5, "dx of job %d" % k)


def test_data_gradient_pair_with_one_ineligible_job_and_with_a_shared_target():
    from nas_3d_unet_amd import kernels as K
    dev = torch.device("cuda")
    # a 3x3x3 data gradient beside an eligible pointwise one: two launches, the eligible one on the pointwise kernel
    dy3, w3 = _mk((B, 4, 4, 6, 12), 87), _mk((4, 4, 3, 3, 3), 88, 0.1)
    g3 = K.conv_geom(B, 4, 6, 12, 4, 4, 3, 1, 1, 1)

    def k3_call():
        return (g3, view(K, dy3), torch.from_numpy(w3).to(dev), empty_view(K, (B, 4, 4, 6, 12)), 0, None, None, False)

    pair = [k3_call(), bwd_call(K, 24, 16, 1, 0, True, dev)]
    single = [k3_call(), bwd_call(K, 24, 16, 1, 0, True, dev)]
    assert counted(K, lambda: K.conv_bwd_data2(pair)) == (1, 1)
    for call in single:
        K.conv_bwd_data(*call)
    torch.cuda.synchronize()
    for k in range(2):
        assert torch.equal(pair[k][3].t, single[k][3].t), "call %d differs from its single launch" % k
    # both accumulate into ONE target: they must run one after the other, in order (two launches)
    c = case(24, 16, 1)
    outs = []
    for fold in (True, False):
        dx = view(K, c["base"])
        calls = [bwd_call(K, 24, 16, 1, 0, True, dev, dx), bwd_call(K, 24, 16, 1, 0, True, dev, dx)]
        if fold:
            assert counted(K, lambda: K.conv_bwd_data2(calls)) == (2, 2)
        else:
            for call in calls:
                K.conv_bwd_data(*call)
        outs.append(dx)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].t, outs[1].t), "a shared target was not accumulated in call order"
    g = c["dx_extras"] - torch.from_numpy(c["base"]).double()
    assert_close(outs[0].t.double(), torch.from_numpy(c["base"]).double() + 2 * g, 5e-5, "dx accumulated twice")


def _raw_fwd_call(K, call, ws, nbytes):
    from nas_3d_unet_amd._lib import ConvFwdCall
    import ctypes as C
    g, x, w, bias, y, flags, gate, stats, _ = call
    return ConvFwdCall(C.pointer(g), 0, flags, x.p.value, x.ld, w.data_ptr(), bias.data_ptr() if bias is not None else None, y.p.value, y.ld,
                       gate.data_ptr() if gate is not None else None, stats.data_ptr() if stats is not None else None, ws.data_ptr(), nbytes)


def _raw_bwd_call(K, call, ws, nbytes):
    from nas_3d_unet_amd._lib import ConvBwdCall
    import ctypes as C
    g, dy, w, dx, flags, relu_src, gate, _ = call
    return ConvBwdCall(C.pointer(g), 0, flags, 0, 0, None, 0, dy.p.value, dy.ld, w.data_ptr(), dx.p.value, dx.ld,
                       relu_src.p.value if relu_src is not None else None, relu_src.ld if relu_src is not None else 0,
                       gate.data_ptr() if gate is not None else None, ws.data_ptr(), nbytes, None, None, None, None, 0, None)


def _workspace(K, geoms, dev):
    from nas_3d_unet_amd import _lib
    import ctypes as C
    n = max(int(_lib.load().n3d_conv_workspace_bytes(C.byref(g))) for g in geoms)
    return torch.empty(n, dtype=torch.uint8, device=dev), n


@pytest.mark.parametrize("overlap", ["same", "offset"])
def test_pairs_that_share_one_workspace_are_not_folded(overlap):
    """A C-ABI caller may hand both calls of a pair ONE scratch buffer (weights not N3D_PREPACKED): each call packs its weights into it
    as it runs, so the two must run one after the other -- two pointwise launches, results of the single calls bit for bit.  `offset`:
    the second workspace starts inside the first one's packed weights."""
    from nas_3d_unet_amd import kernels as K, _lib
    import ctypes as C
    dev = torch.device("cuda")
    lib = _lib.load()
    j0, j1 = (24, 16, 1), (12, 16, 2)
    off = 0 if overlap == "same" else 256
    # forward
    pair = [fwd_call(K, *j0, 0, True, dev), fwd_call(K, *j1, 0, True, dev)]
    single = [fwd_call(K, *j0, 0, True, dev), fwd_call(K, *j1, 0, True, dev)]
    ws, n = _workspace(K, [pair[0][0], pair[1][0]], dev)
    big = torch.empty(n + off, dtype=torch.uint8, device=dev)
    c0, c1 = _raw_fwd_call(K, pair[0], big, n), _raw_fwd_call(K, pair[1], big[off:], n)
    assert counted(K, lambda: _lib.check(lib.n3d_conv_fwd2(C.byref(c0), C.byref(c1), K.stream_ptr()), "n3d_conv_fwd2")) == (2, 2)
    for call in single:
        K.conv_fwd(*call)
    torch.cuda.synchronize()
    for k, geo in enumerate((j0, j1)):
        assert torch.equal(pair[k][4].t, single[k][4].t), "forward call %d computed with the other call's weights" % k
        assert torch.equal(pair[k][7], single[k][7]), "statistics rows of call %d differ" % k
        assert_close(pair[k][4].t.double(), case(*geo)["y_extras"], 2e-5, "y of call %d" % k)
    # distinct workspaces, same raw entry: folded
    ws1, _ = _workspace(K, [pair[1][0]], dev)
    d0, d1 = _raw_fwd_call(K, pair[0], ws, n), _raw_fwd_call(K, pair[1], ws1, ws1.numel())
    assert counted(K, lambda: _lib.check(lib.n3d_conv_fwd2(C.byref(d0), C.byref(d1), K.stream_ptr()), "n3d_conv_fwd2")) == (1, 2)
    # data gradient
    pair = [bwd_call(K, *j0, 0, True, dev), bwd_call(K, *j1, 0, True, dev)]
    single = [bwd_call(K, *j0, 0, True, dev), bwd_call(K, *j1, 0, True, dev)]
    b0, b1 = _raw_bwd_call(K, pair[0], big, n), _raw_bwd_call(K, pair[1], big[off:], n)
    assert counted(K, lambda: _lib.check(lib.n3d_conv_bwd_data2(C.byref(b0), C.byref(b1), K.stream_ptr()), "n3d_conv_bwd_data2")) == (2, 2)
    for call in single:
        K.conv_bwd_data(*call)
    torch.cuda.synchronize()
    for k, geo in enumerate((j0, j1)):
        assert torch.equal(pair[k][3].t, single[k][3].t), "data gradient %d computed with the other call's weights" % k
        assert_close(pair[k][3].t.double(), case(*geo)["dx_extras"], 5e-5, "dx of call %d" % k)


def test_pair_with_a_failing_call_launches_nothing_it_should_not():
    """a workspace too small for its packed weights is an error return: call 0 failing launches nothing; call 1 failing leaves call 0
    done, as on the sequential path"""
    from nas_3d_unet_amd import kernels as K, _lib
    import ctypes as C
    dev = torch.device("cuda")
    lib = _lib.load()
    j0, j1 = (24, 16, 1), (20, 12, 1)
    good = [fwd_call(K, *j0, 0, False, dev), fwd_call(K, *j1, 0, False, dev)]
    ws0, n0 = _workspace(K, [good[0][0]], dev)
    ws1, n1 = _workspace(K, [good[1][0]], dev)
    for bad in (0, 1):
        calls = [fwd_call(K, *j0, 0, False, dev), fwd_call(K, *j1, 0, False, dev)]
        for c in calls:
            c[4].t.fill_(5.0)
        c0 = _raw_fwd_call(K, calls[0], ws0, 16 if bad == 0 else n0)
        c1 = _raw_fwd_call(K, calls[1], ws1, 16 if bad == 1 else n1)
        before = K.conv_pointwise_counts()
        assert lib.n3d_conv_fwd2(C.byref(c0), C.byref(c1), K.stream_ptr()) == -4      # N3D_ERR_WORKSPACE
        after = K.conv_pointwise_counts()
        torch.cuda.synchronize()
        if bad == 0:
            assert after == before and float(calls[0][4].t.min()) == 5.0 and float(calls[1][4].t.min()) == 5.0
        else:
            assert (after[0] - before[0], after[1] - before[1]) == (1, 1) and float(calls[1][4].t.min()) == 5.0
            assert_close(calls[0][4].t.double(), case(*j0)["y_plain"], 2e-5, "y of the call in front of the failing one")
