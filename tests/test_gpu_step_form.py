"""The kernels in the form a training step runs them (kernels.step_context), against fp64 references (tests/_step_form_ref.py):
A. n3d_wgrad_finalize_batch on hand-built jobs -- every reduction branch, the launch split after 80 jobs, the overflow of the
   workgroup -> job map and single jobs larger than the map;
B. the conv family with batch-packed weights (N3D_PREPACKED) and deferred weight-gradient slabs (at the end of the file: it uses
   part C's helpers);
C. the stem's recompute kernels n3d_conv_k1_norm_*.
`pytest -s` prints, after the module, the worst observed error of every quantity as a fraction of its bound and what each conv row
reached.  Bounds come from the summation model (A) and from the caps of the standalone tests (B, C), never from these figures.

On an MI355X (49 tests, 5 to 6.5 s), worst error / bound: A dw 0.63 (tile), 0.50 (direct), 0.066 (many-chunk), dbias 0.49; B y 0.048,
dx 0.017, dw 0.0093, db 0.057, statistics 0.038, bf16-stored y / dx 0.78 / 0.65 (the bound is the rounding of the store itself), dw on
bf16 storage 0.0077; C y 0.0075, bf16-stored y 0.92, statistics 0.016, reduce columns 0.023, apply dW 0.0018, chain y 0.011, chain
dW / dgamma / dbeta / dbias 0.002.  Every step-form result was bit-identical to its standalone call.

Value-only mutations of the kernels, each run once against this file (all eight fail) and against test_gpu_conv.py + test_gpu_train.py:
  tail loop of the many-chunk path dropped       A (4 batch tests), B (4 rows), C (K2 - K5, chains K2 / K4)   | conv: caught
  `c < nchunks` mask of final_direct dropped     A, B (192-64 k1, 12-3 k1, 4-4 bf16)                          | conv: caught
  tile path's bias sum from chunk 1              A, B (8 rows)                                                | conv: caught
  pack: `flip ? 26 - k : k` -> `k`               B (4-4 8x8x64, 4-4 8x16x16 bf16)                             | train only (9 tests)
  k1n_bwd: fmaxf on z dropped                    C test_k1_norm_kernels_against_fp64 (all 13)                 | NOT caught
  k1n_bwd: Bv dropped from d(raw)                C kernels (13) and chains (6)                                | NOT caught
  normalise pass ignores oshift                  C kernels (13), pitched, chains (6)                          | train only (5 tests)
  27-tap tile path's `c < nchunks` mask dropped  A (3 batch tests), B (8 rows)                                | conv: caught
The standalone conv tests do reach the reduction branches through their own one-job calls; what they cannot see is the batch: job
order, the launch split, the map, jobs larger than it, and the stem's backward kernels."""
import ctypes as C

import numpy as np
import pytest
import torch

import _step_form_ref as R
from _util import assert_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
_WORST = {}      # quantity -> (worst observed error / its bound or cap, where): reported after the module, never used to set a bound
_SEEN = {}       # part B case id -> (forward layout, data-gradient layout, job shape)


def _note(what, ratio, where):
    if ratio > _WORST.get(what, (-1.0, ""))[0]:
        _WORST[what] = (float(ratio), where)


@pytest.fixture(scope="module", autouse=True)
def _report():
    """after the module: worst observed error of every quantity as a fraction of its bound or cap, and what part B's cases reached"""
    yield
    for k in sorted(_WORST):
        print("\nworst %-22s %.3e of its bound (%s)" % (k, _WORST[k][0], _WORST[k][1]), end="")
    for k, (lf, ld, job) in _SEEN.items():
        print("\ncase %-34s pack layout fwd %2d dgrad %2d, job (nchunks, ntiles, ci_t, co_t, taps) = %s" % (k, lf, ld, job), end="")
    print()


# ------------------------------------------------------------------------------------------ A. n3d_wgrad_finalize_batch
def _align(n, a=64):
    return (n + a - 1) // a * a


class _FinalBatch:
    """device inputs of a list of R.FinalSpec: one arena of random slabs (generated on the device, copied back once for the reference)
    and, per run, one sentinel-filled output arena with a guard in front of and behind every dw / dbias"""

    def __init__(self, specs, seed):
        self.specs = specs
        self.in_off, n = [], 0
        for s in specs:
            ns, nb = R.final_slab_floats(s)
            po = n
            n += _align(max(s.nchunks, 1) * ns)
            bo = n
            n += _align(max(s.nchunks, 1) * nb)
            self.in_off.append((po, bo))
        gen = torch.Generator(device=DEV).manual_seed(seed)
        self.slabs = torch.randn(n, device=DEV, generator=gen)
        self.out_off, m = [], R.GUARD
        for s in specs:
            wo = m
            m += _align(s.Co * s.Ci * s.taps) + R.GUARD
            do = m
            m += _align(s.Co) + R.GUARD
            self.out_off.append((wo, do))
        self.out_floats = m
        self._host = None

    def host_slabs(self):
        if self._host is None:
            self._host = self.slabs.cpu().numpy()
        return self._host

    def jobs(self, out):
        from nas_3d_unet_amd._lib import FinalJob
        arr = (FinalJob * len(self.specs))()
        for i, s in enumerate(self.specs):
            (po, bo), (wo, do) = self.in_off[i], self.out_off[i]
            arr[i] = FinalJob(self.slabs.data_ptr() + 4 * po, self.slabs.data_ptr() + 4 * bo if s.has_pb else None,
                              out.data_ptr() + 4 * wo if s.has_dw else None, out.data_ptr() + 4 * do if s.has_pb else None,
                              s.nchunks, R.final_ntiles(s), s.tci, s.tco, s.ci_t, s.co_t, s.Co, s.Ci, s.taps, 0)
        return arr

    def run(self, one_call=True):
        """-> the output arena on the host"""
        from nas_3d_unet_amd import kernels as K
        from nas_3d_unet_amd import _lib
        out = torch.full((self.out_floats,), float(R.SENTINEL), device=DEV)
        arr = self.jobs(out)
        fn = _lib.load().n3d_wgrad_finalize_batch
        if one_call:
            _lib.check(fn(arr, len(self.specs), K.stream_ptr()), "n3d_wgrad_finalize_batch")
        else:
            for i in range(len(self.specs)):
                _lib.check(fn(C.byref(arr[i]), 1, K.stream_ptr()), "n3d_wgrad_finalize_batch")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def check(self, got, tag):
        """every element within its summation bound of the fp64 sum; everything outside the jobs' extents still the sentinel"""
        host = self.host_slabs()
        written = np.zeros(self.out_floats, dtype=bool)
        for i, s in enumerate(self.specs):
            if s.nchunks == 0:
                continue
            (po, bo), (wo, do) = self.in_off[i], self.out_off[i]
            ns, nb = R.final_slab_floats(s)
            part = host[po:po + s.nchunks * ns].reshape(s.nchunks, ns)
            pb = host[bo:bo + s.nchunks * nb].reshape(s.nchunks, nb) if s.has_pb else None
            dw, dwa, db, dba = R.final_reference(s, part, pb)
            if s.has_dw:
                n = s.Co * s.Ci * s.taps
                g = got[wo:wo + n].reshape(s.Co, s.Ci, s.taps).astype(np.float64)
                ratio = np.abs(g - dw) / R.final_bound(s, dwa)
                _note("A dw %s" % R.final_path(s), ratio.max(), s.name)
                assert ratio.max() <= 1.0, "%s %s (%s): dw off by %.3g of its bound at %s" % (
                    tag, s.name, R.final_path(s), ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))
                written[wo:wo + n] = True
            if s.has_pb:
                g = got[do:do + s.Co].astype(np.float64)
                ratio = np.abs(g - db) / R.final_bound(s, dba)
                _note("A dbias %s" % R.final_path(s), ratio.max(), s.name)
                assert ratio.max() <= 1.0, "%s %s (%s): dbias off by %.3g of its bound at %d" % (tag, s.name, R.final_path(s), ratio.max(), ratio.argmax())
                written[do:do + s.Co] = True
        stray = np.flatnonzero((got.view(np.uint32) != R.SENTINEL.view(np.uint32)) & ~written)
        assert stray.size == 0, "%s: %d floats outside the jobs' (Co, Ci, taps) / (Co) extents were written, first at arena offset %d" % (
            tag, stray.size, stray[0])


@pytest.fixture(scope="module")
def final_main():
    b = _FinalBatch(R.final_main_jobs(), 101)
    return b, b.run(one_call=True)


def test_final_batch_every_branch(final_main):
    """(i) all branches and variants in ONE call, shuffled"""
    b, got = final_main
    paths = {R.final_path(s) for s in b.specs}
    assert paths == {"none", "tile", "direct4", "direct16", "many64", "many16", "many8", "many4"}
    assert R.final_launch_plan(b.specs) == [(0, len(b.specs))]
    b.check(got, "one call")


def test_final_single_calls_bit_identical(final_main):
    """(ii) the same jobs one call each: the order of summation is fixed, so the results are those of the batch bit for bit"""
    b, got = final_main
    single = b.run(one_call=False)
    assert np.array_equal(single.view(np.uint32), got.view(np.uint32))


def test_final_more_jobs_than_a_launch_holds():
    """(iii) 200 jobs in one call: three launches"""
    b = _FinalBatch(R.final_many_small_jobs(200), 102)
    assert [m for _, m in R.final_launch_plan(b.specs)] == [80, 80, 40]
    got = b.run()
    b.check(got, "200 jobs")
    assert np.array_equal(b.run(one_call=False).view(np.uint32), got.view(np.uint32))


def test_final_map_overflow():
    """(iv) the workgroup -> job map fills up before the job table does"""
    b = _FinalBatch(R.final_map_overflow_jobs(), 103)
    plan = R.final_launch_plan(b.specs)
    assert len(b.specs) < R.N_FINAL_JOBS and len(plan) >= 3 and all(m < R.N_FINAL_JOBS for _, m in plan)
    got = b.run()
    b.check(got, "map overflow")
    assert np.array_equal(b.run(one_call=False).view(np.uint32), got.view(np.uint32))


def test_final_job_larger_than_the_map():
    """(v) single jobs of more than 8192 workgroups (every map entry names them), tile path and many-chunk path, between ordinary jobs"""
    b = _FinalBatch(R.final_giant_jobs(), 104)
    big = {s.name: R.final_blocks(s) for s in b.specs if R.final_blocks(s) > R.MAP_UNITS * R.MAP_GROUP}
    assert set(big) == {"g_tile", "g_many"}
    assert R.final_path(b.specs[1]) == "tile" and R.final_path(b.specs[3]) == "many8"
    assert [m for _, m in R.final_launch_plan(b.specs)] == [1, 1, 1, 1, 1]
    got = b.run()
    b.check(got, "giant jobs")


# ------------------------------------------------------------------------------------------ C. the stem's recompute kernels
CAP_STATS, CAP_Y, CAP_DW = 1e-5, 2e-5, 1e-4      # the caps of test_conv_family; bf16-stored y: half a bf16 ulp of the largest value
BF16_ULP = 2.0 ** -8


def _close(got, ref, cap, what, where):
    """_util.assert_close (max |err| / max |ref| <= cap), with the observed ratio noted"""
    if isinstance(got, torch.Tensor):
        got = got.detach().double().cpu().numpy()
    ref = np.asarray(ref)
    got = got.reshape(ref.shape)
    _note(what, np.abs(got - ref).max() / max(1e-30, np.abs(ref).max()) / cap, where)
    assert_close(got, ref, cap, "%s %s" % (where, what))


def _act(a, c, bf16):
    """(B, C, N) host array -> dense NDHWC View in the given storage type"""
    from nas_3d_unet_amd import kernels as K
    t = K.empty_ndhwc(c.B, a.shape[1], *c.shape, DEV, torch.bfloat16 if bf16 else torch.float32)
    t.copy_(torch.from_numpy(a).to(DEV).view(c.B, a.shape[1], *c.shape))
    return K.as_view(t)


def _act5(a, dt):
    """(B, C, D, H, W) host array -> dense NDHWC View of storage type dt"""
    from nas_3d_unet_amd import kernels as K
    t = K.empty_ndhwc(*a.shape, DEV, dt)
    t.copy_(torch.from_numpy(a).to(DEV))
    return K.as_view(t)


def _flat(v, c):
    """View -> (B, C, N) fp64 host array"""
    return v.t.double().cpu().numpy().reshape(c.B, v.C, -1)


class _K1Dev:
    def __init__(self, cid, mix):
        from nas_3d_unet_amd import kernels as K
        self.inp = inp = R.k1_inputs(cid, mix)
        self.c = c = inp["case"]
        self.x16, self.d16 = mix.startswith("bf16"), mix.endswith("bf16")
        self.g = K.conv_geom(c.B, *c.shape, c.Ci, c.Co, 1, 1, 1, 0)
        assert K.conv_k1_norm_ok(self.g)
        self.x, self.dout = _act(inp["x"], c, self.x16), _act(inp["dout"], c, self.d16)
        assert self.x.ld == c.Ci and self.dout.ld == c.Co
        dv = lambda k: torch.from_numpy(inp[k]).to(DEV)
        self.w, self.bias = dv("w").view(c.Co, c.Ci, 1, 1, 1), dv("bias")
        self.a, self.b, self.A, self.Bc, self.Cc = (dv(k) for k in ("a", "b", "A", "Bc", "Cc"))
        self.where = "%s %s" % (cid, mix)

    def new_y(self):
        from nas_3d_unet_amd import kernels as K
        c = self.c
        return K.as_view(K.empty_ndhwc(c.B, c.Co, *c.shape, DEV, torch.bfloat16 if self.d16 else torch.float32))

    def stats(self, bias):
        from nas_3d_unet_amd import kernels as K
        from nas_3d_unet_amd import _lib
        c = self.c
        rows = K.conv_stats_rows(self.g, False, _lib.SRC_BF16 if self.x16 else 0)
        st = torch.full((c.B, rows, c.Co, 2), float("nan"), dtype=torch.float64, device=DEV)
        K.conv_k1_norm_fwd(self.g, self.x, self.w, bias, None, None, None, st)
        return st, rows


def _k1_params():
    return [(cid, mix) for cid in R.K1_CASES for mix in (R.K1_MIXES if cid in R.K1_BF16_CASES else R.K1_MIXES[:1])]


@pytest.mark.parametrize("cid,mix", _k1_params())
def test_k1_norm_kernels_against_fp64(cid, mix):
    """statistics pass, normalise pass, bwd_reduce and bwd_apply_wgrad (without / with ReLU) of n3d_conv_k1_norm_*, without / with a
    conv bias, on random coefficients; every voxel is compared (the inputs keep a margin to every ReLU threshold by construction)"""
    from nas_3d_unet_amd import kernels as K
    d = _K1Dev(cid, mix)
    c, g, where = d.c, d.g, d.where
    assert int(K._lib.load().n3d_conv_k1_norm_rows(C.byref(g))) == -(-d.inp["N"] // R.k1_chunk(d.inp["N"]))
    for bias in (None, d.bias):
        ref = R.k1_reference(d.inp, bias is not None)
        tag = where + (" bias" if bias is not None else " nobias")
        st, _ = d.stats(bias)
        st = st.sum(dim=1).cpu().numpy()
        _close(st[..., 0], ref["stats"][..., 0], CAP_STATS, "C stats sum", tag)
        _close(st[..., 1], ref["stats"][..., 1], CAP_STATS, "C stats sumsq", tag)
        y = d.new_y()
        K.conv_k1_norm_fwd(g, d.x, d.w, bias, y, d.a, d.b, None)
        _close(_flat(y, c), ref["y"], BF16_ULP if d.d16 else CAP_Y, "C y bf16" if d.d16 else "C y", tag)
        # the same pass in trainer form: the weight packed by n3d_pack_batch, N3D_PREPACKED
        ctx = K.StepContext(torch.device(DEV))
        with K.step_context(ctx):
            ctx.slot(d.w, g, False, 0)
        ctx.freeze()
        assert ctx.njobs == 1
        ctx.pack_all()
        y2 = d.new_y()
        with K.step_context(ctx):
            K.conv_k1_norm_fwd(g, d.x, d.w, bias, y2, d.a, d.b, None)
        assert torch.equal(y2.t, y.t), tag + ": normalise pass with batch-packed weights differs from the standalone call"
        for relu in (False, True):
            rt = tag + (" relu" if relu else "")
            sums, rows = K.conv_k1_norm_bwd_reduce(g, d.x, d.w, bias, d.dout, d.a, d.b, relu)
            s = sums.sum(dim=1).cpu().numpy()
            for k, name in enumerate(("sum g", "sum g raw", "sum dout z")):
                _close(s[..., k], ref["sums", relu][..., k], CAP_STATS, "C reduce " + name, rt)
            dw = torch.full((c.Co, c.Ci, 1, 1, 1), float(R.SENTINEL), device=DEV)
            K.conv_k1_norm_bwd_apply_wgrad(g, d.x, d.w, bias, d.dout, d.a, d.b, d.A, d.Bc, d.Cc, dw, relu)
            _close(dw, ref["dw", relu], CAP_DW, "C apply dW", rt)
            # trainer form: slabs left in the workspace, reduced by StepContext.flush_final
            dw2 = torch.full_like(dw, float(R.SENTINEL))
            ctx = K.StepContext(torch.device(DEV))
            with K.step_context(ctx):
                K.conv_k1_norm_bwd_apply_wgrad(g, d.x, d.w, bias, d.dout, d.a, d.b, d.A, d.Bc, d.Cc, dw2, relu)
                assert len(ctx.final) == 1 and ctx.final[0].nchunks == rows * c.B
                assert torch.equal(dw2, torch.full_like(dw2, float(R.SENTINEL))), "deferred: dW must not be written before flush_final"
            ctx.flush_final()
            assert torch.equal(dw2, dw), rt + ": deferred dW differs from the standalone call"


def test_k1_norm_pitched_output_keeps_the_other_channels():
    """K2's normalise pass into a 12-channel view of a 16-channel tensor (pitch 16: the per-voxel store path, not the flat one)"""
    from nas_3d_unet_amd import kernels as K
    d = _K1Dev("K2", "f32->f32")
    c = d.c
    base = K.empty_ndhwc(c.B, 16, *c.shape, DEV, torch.float32)
    base.fill_(float(R.SENTINEL))
    y = K.as_view(base[:, :12])
    assert y.ld == 16 and y.C == 12 and y.t.data_ptr() == base.data_ptr()
    K.conv_k1_norm_fwd(d.g, d.x, d.w, d.bias, y, d.a, d.b, None)
    ref = R.k1_reference(d.inp, True)
    _close(_flat(y, c), ref["y"], CAP_Y, "C y pitched", "K2 pitch 16")
    rest = base[:, 12:]
    assert torch.equal(rest, torch.full_like(rest, float(R.SENTINEL))), "channels 12..15 of the pitched tensor were overwritten"


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("cid", R.K1_CHAIN_CASES)
def test_k1_norm_chain_against_group_norm_autograd(cid, with_bias):
    """statistics -> gn_coeffs -> normalise -> bwd_reduce -> gn_bwd_coeffs -> apply_wgrad as programs._seg_*_recompute chains them,
    against fp64 autograd of GroupNorm(conv1x1(x))"""
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd import programs
    d = _K1Dev(cid, "f32->f32")
    c, g, N = d.c, d.g, d.inp["N"]
    G = programs.group_count(c.Co)
    ref = R.k1_chain_reference(d.inp, with_bias, G)
    gamma, beta = torch.from_numpy(d.inp["gamma"]).to(DEV), torch.from_numpy(d.inp["beta"]).to(DEV)
    bias = torch.nn.Parameter(d.bias.clone()) if with_bias else None
    where = "%s chain%s" % (cid, " bias" if with_bias else "")
    st, rows = d.stats(bias)
    a, b, mr, sumraw = K.gn_coeffs(st, rows, gamma, beta, c.B, c.Co, G, N, 1e-5)
    y = d.new_y()
    K.conv_k1_norm_fwd(g, d.x, d.w, bias, y, a, b, None)
    _close(_flat(y, c), ref["y"], CAP_Y, "C chain y", where)
    sums, rrows = K.conv_k1_norm_bwd_reduce(g, d.x, d.w, bias, d.dout, a, b)
    dgamma, dbeta, A, Bc, Cc, dcb = K.gn_bwd_coeffs(sums, rrows, gamma, mr, None, c.B, c.Co, G, N, None, beta, sumraw, bias)
    dw = torch.full((c.Co, c.Ci, 1, 1, 1), float(R.SENTINEL), device=DEV)
    K.conv_k1_norm_bwd_apply_wgrad(g, d.x, d.w, bias, d.dout, a, b, A, Bc, Cc, dw)
    _close(dw, ref["dw"], CAP_DW, "C chain dW", where)
    _close(dgamma, ref["dgamma"], CAP_DW, "C chain dgamma", where)
    _close(dbeta, ref["dbeta"], CAP_DW, "C chain dbeta", where)
    if with_bias:
        _close(dcb, ref["dbias"], CAP_DW, "C chain dbias", where)


# ------------------------------------------------------------------------------------------ B. the conv family in trainer form
CAP_DX = 5e-5                                  # with CAP_Y, CAP_DW, CAP_STATS: the caps of test_conv_family
CAP_DW_BF16 = 2e-5                             # test_conv_family_bf16_storage


def _conv_geom(c):
    from nas_3d_unet_amd import kernels as K
    pad = R.conv_padding(c.k, c.stride, c.dil)
    if c.transposed:
        return K.conv_geom(c.B, *R.conv_out_shape(c), c.cout, c.cin, c.k, c.stride, c.dil, pad, c.depthwise)
    return K.conv_geom(c.B, *c.shape, c.cin, c.cout, c.k, c.stride, c.dil, pad, c.depthwise)


def _conv_flags(c):
    from nas_3d_unet_amd import _lib
    return (_lib.SRC_BF16 | _lib.DST_BF16) if c.bf16 else 0


def _pack_info(c, data_grad):
    from nas_3d_unet_amd import _lib
    lay, cdp, fl = C.c_int32(), C.c_int32(), C.c_int64()
    g = _conv_geom(c)
    _lib.check(_lib.load().n3d_conv_pack_info(C.byref(g), 1 if data_grad else 0, _conv_flags(c), C.byref(lay), C.byref(cdp), C.byref(fl)), "n3d_conv_pack_info")
    return lay.value, cdp.value, fl.value


@pytest.fixture(scope="module")
def conv_params():
    """device weight and bias of every row of the table (a StepContext keys its slots by the weight's address)"""
    return [tuple(torch.from_numpy(a).to(DEV) for a in R.conv_weights(i)) for i in range(len(R.CONV_CASES))]


def _step_context_with_every_conv(conv_params):
    """a StepContext holding the forward and the data-gradient slot of EVERY conv of the table, packed by one n3d_pack_batch"""
    from nas_3d_unet_amd import kernels as K
    ctx = K.StepContext(torch.device(DEV))
    with K.step_context(ctx):
        for c, (w, _) in zip(R.CONV_CASES, conv_params):
            g = _conv_geom(c)
            ctx.slot(w, g, c.transposed, _conv_flags(c))            # as conv_fwd asks for it
            ctx.slot(w, g, not c.transposed, _conv_flags(c))        # as conv_bwd_data does
    ctx.freeze()
    ctx.pack_all()
    return ctx


def _job_shape(job):
    return (job.nchunks, job.ntiles, job.ci_t, job.co_t, job.taps)


@pytest.mark.parametrize("i", range(len(R.CONV_CASES)), ids=[R.conv_case_id(c) for c in R.CONV_CASES])
def test_conv_family_in_trainer_form(i, conv_params):
    """forward, data gradient and weight gradients (bias gradient with / without, combined backward, queued launch) under a
    StepContext -- weights packed by the batch, slabs reduced by flush_final -- against the references of the standalone tests, and
    bit for bit against the standalone calls: packing only moves values and the reduction is the same fixed-order kernel"""
    from nas_3d_unet_amd import kernels as K
    c = R.CONV_CASES[i]
    ref = R.conv_reference(i)
    where = R.conv_case_id(c)
    g, (w, b) = _conv_geom(c), conv_params[i]
    dt = torch.bfloat16 if c.bf16 else torch.float32
    x, dy = _act5(ref["x"], dt), _act5(ref["dy"], dt)
    oshape, T = ref["y"].shape, c.transposed
    new_y = lambda: K.as_view(K.empty_ndhwc(*oshape, DEV, dt))
    new_dx = lambda: K.as_view(K.empty_ndhwc(c.B, c.cin, *c.shape, DEV, dt))
    sent = lambda t: torch.full_like(t, float(R.SENTINEL))
    want_db = not (c.bf16 and T)               # as the standalone tests call it
    want_stats = not c.bf16 and not c.depthwise
    rows = K.conv_stats_rows(g, T, 0, x, new_y()) if want_stats else 0

    def forward_and_data():
        y, dx = new_y(), new_dx()
        stats = torch.zeros((c.B, max(rows, 1), oshape[1], 2), dtype=torch.float64, device=DEV) if rows > 0 else None
        K.conv_fwd(g, x, w, b, y, 0, None, stats, T)
        K.conv_bwd_data(g, dy, w, dx, 0, None, None, T)
        return dict(y=y.t, dx=dx.t, stats=stats)

    def weight_grads():
        dw1, db1, dw2 = sent(w), sent(b), sent(w)
        K.conv_bwd_weight(g, x, dy, dw1, db1 if want_db else None, 0, None, T)
        K.conv_bwd_weight(g, x, dy, dw2, None, 0, None, T)
        return dict(dw=dw1, db=db1 if want_db else None, dw_nobias=dw2)

    def both():
        dx3, dw3, db3 = new_dx(), sent(w), sent(b)
        K.conv_bwd_both(g, x, dy, w, dx3, dw3, None if T else db3, 0, None, None, 0, None, T)
        return dict(dx_both=dx3.t, dw_both=dw3, db_both=None if T else db3)

    has_both = not c.bf16 and not c.depthwise          # (conv_bwd_both is an fp32 call; the depthwise family has no combined form)
    alone = {**forward_and_data(), **weight_grads(), **(both() if has_both else {})}
    # ---- trainer form
    ctx = _step_context_with_every_conv(conv_params)
    lay_f, lay_d = _pack_info(c, T)[0], _pack_info(c, not T)[0]
    with K.step_context(ctx):
        if not c.depthwise:         # the calls below really take the batch-packed slots
            assert ctx.slot(w, g, T, _conv_flags(c)) is not None and ctx.slot(w, g, not T, _conv_flags(c)) is not None
        step = forward_and_data()
        step.update(weight_grads())
        jobs = [_job_shape(j) for j in ctx.final]
        if has_both:
            step.update(both())
    ctx.flush_final()
    _SEEN[where] = (lay_f, lay_d, jobs[0] if jobs else "not deferred")
    path = R.final_path_of(jobs[0][0], *jobs[0][2:]) if jobs else None
    assert (lay_f, lay_d, path) == R.CONV_REACHES[where], "%s: the kernel selection moved, see _step_form_ref.CONV_REACHES" % where
    # ---- queued weight-gradient launches (the side-stream schedule): flush_final launches the queue, then reduces
    ctx.defer_wgrad = True
    with K.step_context(ctx):
        queued = weight_grads()
        assert len(ctx.wq) == 2
        if ctx.wq:
            assert torch.equal(queued["dw"], sent(w)), "a queued weight gradient ran before flush_final"
    ctx.flush_final()
    torch.cuda.synchronize()
    # ---- against the CPU reference
    bf = c.bf16
    for res, tag in ((alone, "standalone"), (step, "step"), (queued, "queued")):
        if "y" in res:
            _close(res["y"], ref["y"], BF16_ULP if bf else CAP_Y, "B y" + (" bf16" if bf else ""), where + " " + tag)
            _close(res["dx"], ref["dx"], BF16_ULP if bf else CAP_DX, "B dx" + (" bf16" if bf else ""), where + " " + tag)
            if res["stats"] is not None and oshape[1] % 4 == 0:
                st, yd = res["stats"].sum(dim=1).cpu().numpy(), ref["y"].astype(np.float64)
                _close(st[..., 0], yd.sum(axis=(2, 3, 4)), CAP_STATS, "B stats sum", where + " " + tag)
                _close(st[..., 1], (yd * yd).sum(axis=(2, 3, 4)), CAP_STATS, "B stats sumsq", where + " " + tag)
        cap_dw = CAP_DW_BF16 if bf else CAP_DW
        _close(res["dw"], ref["dw"], cap_dw, "B dw" + (" bf16" if bf else ""), where + " " + tag)
        _close(res["dw_nobias"], ref["dw"], cap_dw, "B dw" + (" bf16" if bf else ""), where + " " + tag + " no dbias")
        if res["db"] is not None:
            _close(res["db"], ref["db"], CAP_DW, "B db", where + " " + tag)
        if "dw_both" in res:
            _close(res["dx_both"], ref["dx"], CAP_DX, "B dx", where + " " + tag + " both")
            _close(res["dw_both"], ref["dw"], CAP_DW, "B dw", where + " " + tag + " both")
            if res["db_both"] is not None:
                _close(res["db_both"], ref["db"], CAP_DW, "B db", where + " " + tag + " both")
    # ---- bit for bit against the standalone calls
    for k, v in alone.items():
        if v is None:
            continue
        assert torch.equal(step[k], v), "%s: %s under the step context differs from the standalone call" % (where, k)
        if k in queued:
            assert torch.equal(queued[k], v), "%s: %s from the queued launch differs from the standalone call" % (where, k)


def test_conv_table_reaches_every_pack_layout():
    """layouts 0 generic, 1 gemm16, 2 vox64, 3 vox_up, 4 / 5 their bfloat16 forms; -1: the depthwise kernels read native weights"""
    seen = set()
    for c in R.CONV_CASES:
        lays = (_pack_info(c, c.transposed)[0], _pack_info(c, not c.transposed)[0])
        assert lays == R.CONV_REACHES[R.conv_case_id(c)][:2], R.conv_case_id(c)
        seen |= set(lays)
    assert seen == {-1, 0, 1, 2, 3, 4, 5}
    # the deferred weight gradients of the table reach the tile path, the direct path and two widths of the many-chunk path
    assert {v[2] for v in R.CONV_REACHES.values()} == {"tile", "direct16", "many64", "many16"}


def test_pack_batch_more_jobs_than_a_launch_holds(conv_params):
    """n3d_pack_batch with more than 160 jobs in one call and a workgroup -> job map that overflows on the way (the large 3x3x3 and
    1x1x1 weights repeated): every slot bit-equal to the slot the same job gets when packed alone"""
    from nas_3d_unet_amd import kernels as K
    from nas_3d_unet_amd import _lib
    from nas_3d_unet_amd._lib import PackJob
    base = []
    for c, (w, _) in zip(R.CONV_CASES, conv_params):
        if c.depthwise:
            continue
        for dg in (False, True):
            lay, cdp, fl = _pack_info(c, dg)
            base.append((w, c.cout if not c.transposed else c.cin, c.cin if not c.transposed else c.cout, c.k ** 3, int(dg), lay, cdp, fl))
    big = sorted(base, key=lambda j: -R.pack_blocks(*j[1:7]))[:6]
    jobs = base * 2 + big * 18 + base * 3
    blocks = [R.pack_blocks(*j[1:7]) for j in jobs]
    plan = R.pack_launch_plan(blocks)
    assert len(jobs) > R.N_PACK_JOBS and any(why == "map" for _, why in plan) and any(why == "table" for _, why in plan), plan
    offs, n = [], R.GUARD
    for j in jobs:
        offs.append(n)
        n += _align(j[7]) + R.GUARD
    fn = _lib.load().n3d_pack_batch

    def run(one_call):
        buf = torch.full((n,), float(R.SENTINEL), device=DEV)
        arr = (PackJob * len(jobs))()
        for k, (w, Co, Ci, taps, dg, lay, cdp, fl) in enumerate(jobs):
            arr[k] = PackJob(w.data_ptr(), buf.data_ptr() + 4 * offs[k], Co, Ci, taps, dg, lay, cdp)
        if one_call:
            _lib.check(fn(arr, len(jobs), K.stream_ptr()), "n3d_pack_batch")
        else:
            for k in range(len(jobs)):
                _lib.check(fn(C.byref(arr[k]), 1, K.stream_ptr()), "n3d_pack_batch")
        torch.cuda.synchronize()
        return buf.cpu().numpy().view(np.uint32)

    batch, single = run(True), run(False)
    for k, j in enumerate(jobs):
        lo, hi = offs[k], offs[k] + j[7]
        assert np.array_equal(batch[lo:hi], single[lo:hi]), "pack job %d (Co %d, Ci %d, taps %d, data_grad %d, layout %d) differs from packing it alone" % ((k,) + j[1:6])
        assert (batch[hi:hi + R.GUARD] == R.SENTINEL.view(np.uint32)).all(), "pack job %d wrote behind its slot" % k
    assert np.array_equal(batch, single)
    # a packed slot holds exactly the weight's values (layouts 0 - 3: fp32, moved and zero-padded, never changed)
    for k in (0, 1):
        w, Co, Ci, taps, dg, lay, cdp, fl = jobs[k]
        if lay <= 3:
            slot = np.sort(batch[offs[k]:offs[k] + fl])
            src = np.sort(np.concatenate([w.cpu().numpy().view(np.uint32).ravel(), np.zeros(fl - w.numel(), np.uint32)]))
            assert np.array_equal(slot, src)
