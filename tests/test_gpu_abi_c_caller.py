"""GPU: libn3d.so driven from plain C through include/n3d.h -- tests/abi/n3d_abi_caller.c, compiled here and run ONCE.

Why.  Every other GPU test reaches the library through ctypes with buffers that torch allocated (512-byte alignment, pooled slack
behind every tensor) on torch's current stream.  A C host follows the header's "Conventions" block literally: hipMalloc, streams of
its own, the documented layouts.  The program includes only <hip/hip_runtime_api.h>, n3d.h and libc, is compiled as C11 (no
-pedantic: HIP's own headers are not pedantic-clean) and linked with -ln3d -lamdhip64; its references are naive fp64 loops written
from the header's text.  Every output lies inside a larger hipMalloc allocation with sentinel floats in front of it, behind it and
in the foreign channels of its pitch (pitch = C + 8, the slice 4 channels in, 64 floats off the allocation's start); inputs carry a
large sentinel in their foreign channels.  All work runs on two streams the program created.

Checks (one output line each, `name status max_err scale`; a parametrised test per line, so a failure names its check):
  query.* / refuse.*   version, device, workspace and row queries; four refusals whose argument check precedes every launch
                       (read in csrc: run_fwd_call / check_geom, n3d_affine_act_bwd_apply_gn2, check_head): NULL operands and
                       k = 2 for n3d_conv_fwd, B = 5 for n3d_affine_act_bwd_apply_gn2, byte targets with Co = 2 for n3d_head_fwd --
                       documented status, a message naming the entry point, outputs untouched.
  conv*                exact integer data (|x| <= 3, |w| <= 2, |bias| <= 4, |dy| <= 2; the program asserts its worst-case sums
                       < 2^24), so the result equals the fp64 reference bit for bit: 3x3x3 4->4 at (1, 8x8x16) with bias
                       (INTEGRATION.md's example, shrunk: the one-plane-tile kernel), 16->16 at (2, 4^3) (MFMA K-split), 1x1x1
                       12->8 at (2, 8^3) (LDS-weight pointwise kernel), stride-2 4->12 at (2, 8x8x12) (gather kernel),
                       n3d_convT_fwd 8->8 from (2, 4x4x6).  The statistics rows, summed over rows, equal the exact per-sample
                       sums of y and y^2 (the buffer is pre-filled with a sentinel, not zeros).  n3d_conv_bwd_both on the first
                       two: dx, dw, dbias exact.
  chain.*              conv -> statistics -> n3d_gn_coeffs -> n3d_affine_act(N3D_RELU | N3D_ACCUMULATE) onto a non-zero base,
                       against fp64 GroupNorm + ReLU at TOL_FWD = 2e-5 (max|err| / max|ref| over every element).
  graph.*              the same three calls between n3d_stream_capture_begin / _end, n3d_graph_launch twice (outputs reset by
                       stream copies in between): bit-identical to the eager run.
  adam.*               three n3d_adam_step on 8192 + 5 elements, every buffer 4 bytes off a 16-byte boundary, lr from a device
                       float, ticketed device step counter; tolerance = 4 x the error of a plain fp32 C restatement of the
                       recurrence against the fp64 one + 2^-23 max|ref| (test_gpu_optim._tol's rule), measured by the program.
  patch_* / stitch.*   n3d_patch_batch (identity key; permutation + flips with the corner partly outside on all axes; float and
                       byte targets; pitched x_out) and n3d_stitch + n3d_tumor_labels on two overlapping patches, bit for bit.
  handoff.*            the two C snippets of INTEGRATION.md section 3 as written: signal / wait / signal / wait over two
                       streams with finite max_polls, then n3d_adam_step_guarded with a word from n3d_host_word_alloc: no
                       time-out, the step words as the text says, host word 0, update applied = adam's first step bit for bit.

Found when written: the second snippet of INTEGRATION.md passed `&sync[4]` as `acked` -- the word the first snippet uses as its
hand-off flag.  After a step that flag holds 1 while the time-out count `sync[1]` holds 0, and the guard of the update withholds it
whenever the two words differ (adam_kernel, include/n3d.h "Guarded update"): a host that pasted both snippets would never have
updated a weight.  The text now gives `acked` a word of its own (`sync[6]`), and this program runs it that way.  The library itself
needed no change: every check passed on unchanged code, with hipMalloc buffers, foreign pitches and the program's own streams, and the
three calls of the chain were capturable as documented.

Figures of the first run on an MI355X.  The child's wall time was 0.38 s (0.26 - 0.27 s in later runs) and the whole file, compile
included, takes about 3 s; TIME_LIMIT_S = max(10 x 0.38 s, 60 s) = 60 s.  Every conv, statistics, patch, stitch and label line printed
max_err 0.  chain: a 1.9e-9 at scale 4.7e-2, b 1.3e-8 at 0.42, (mean, rstd) 7.9e-10 at 1.0, output 2.6e-7 at 4.97 (5.3e-8 relative,
bound 2e-5); both graph replays bit-identical.  adam after three steps, with the fp32 restatement's own error and the bound the
program derives from it: param 1.385e-7 (fp32 1.521e-7, bound 8.450e-7, scale 1.98), exp_avg 1.602e-8 (1.874e-8, 9.702e-8, 0.185),
exp_avg_sq 1.281e-10 (1.638e-10, 8.401e-10, 1.55e-3).  The HIP runtime writes one line, "rocdevice.cpp .. Unknown Event Type", to the
child's stderr after the last check, while the program frees its host word and destroys its streams; the exit status is 0, and
stderr is kept apart from the lines that are parsed.

Mutation evidence (VALUE mutations only, none changes an address; each applied alone to a scratch copy of csrc/, the library rebuilt
and handed to this file through N3D_LIB):
  A conv_gather_kernel: the taps with kw == 2 contribute nothing (`ok && kw != 2` in both tap loops)
        -> conv3s2_4to12.fwd / .stats and convT3s2_8to8.fwd / .stats fail (max_err 58 and 59 at scale 110 / 83); 44 pass.
  B adam_kernel: bias correction 2 with the power step + 1 (`pow(b2, step + 1)`)
        -> adam.param fails (7.9e-3 against the bound 8.5e-7); handoff.guarded_adam still passes, as it must: it compares the
           guarded call with the library's own first step.
  C gn_coeffs_body: the unbiased variance (`* n / (n - 1)`, n = 4096)
        -> chain.gn_a (5.8e-6 at 4.7e-2 = 1.2e-4 relative) and chain.affine_act (4.4e-4 at 4.97) fail; chain.gn_mean_rstd does
           not see it (rstd moves by 1.2e-4 of 0.05, and the pair is judged at the scale of the mean).
  D stitch_kernel: the mean divided by count + 1
        -> stitch.mean (0.5) and stitch.labels (67 voxels) fail.
In each run test_c_caller_ran_to_the_end fails as well (exit status 1).
Not shown: an out-of-bounds write of a kernel (that would be an address mutation; the sentinels are there for it), a refusal that
comes after a launch (every refusal here was read in csrc to sit in front of one), a capture invalidated by a synchronising call
(the program reports it as graph.capture FAIL and goes on; no entry point of the chain does it).
"""
import os
import shutil
import subprocess
import time

import pytest

from nas_3d_unet_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "abi", "n3d_abi_caller.c")
TIME_LIMIT_S = 60       # a cap against a hang, not a performance number

CHECKS = (
    ["query." + n for n in ("device_ok", "version", "workspace_bytes", "conv_stats_rows", "stats_rows", "job_tables")]
    + ["refuse." + n for n in ("conv_fwd_null", "conv_fwd_k2", "apply_gn2_B5", "head_fwd_u8_co2", "outputs_untouched")]
    + ["chain." + n for n in ("conv", "stats", "gn_a", "gn_b", "gn_mean_rstd", "affine_act")]
    + ["graph." + n for n in ("capture", "replay0", "replay1")]
    + ["%s.%s" % (c, n) for c in ("conv3_4to4", "conv3_16to16") for n in ("fwd", "stats", "bwd_dx", "bwd_dw", "bwd_dbias")]
    + ["%s.%s" % (c, n) for c in ("conv1_12to8", "conv3s2_4to12", "convT3s2_8to8") for n in ("fwd", "stats")]
    + ["adam." + n for n in ("param", "exp_avg", "exp_avg_sq", "step_counter")]
    + ["patch_f32.x", "patch_f32.t", "patch_u8.x", "patch_u8.t", "stitch.mean", "stitch.labels", "handoff.words", "handoff.guarded_adam"]
)


def _compiler_and_rocm():
    rocm = os.environ.get("ROCM_PATH") or "/opt/rocm"
    for cand in (os.path.join(rocm, "lib", "llvm", "bin", "clang"), shutil.which("cc")):
        if cand and os.path.exists(cand):
            return cand, rocm
    pytest.fail("no C compiler: neither $ROCM_PATH/lib/llvm/bin/clang nor cc exists")


def compile_line(out_path):
    """the compile line INTEGRATION.md section 3 gives"""
    cc, rocm = _compiler_and_rocm()
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    return [cc, "-std=c11", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
            "-I" + os.path.join(ROOT, "include"), SOURCE, "-o", out_path, "-L" + libdir, "-ln3d", "-L" + os.path.join(rocm, "lib"),
            "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(rocm, "lib")]


@pytest.fixture(scope="module")
def caller(tmp_path_factory):
    """(exit status, {check: (status, max_err, scale)}, whole output): the program compiled and run once, as a child process"""
    _lib.require_device()
    exe = str(tmp_path_factory.mktemp("abi_caller") / "n3d_abi_caller")
    r = subprocess.run(compile_line(exe), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout
    t0 = time.time()
    try:
        # (stderr apart: the HIP runtime logs there, and only the program's own lines are parsed)
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=TIME_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        pytest.exit("the C caller hung (killed after %d s), no further test is started:\n%s" % (TIME_LIMIT_S, e.stdout), returncode=3)
    wall = time.time() - t0
    print("n3d_abi_caller: exit status %d, %.2f s wall\n%s\nstderr:\n%s" % (r.returncode, wall, r.stdout, r.stderr))
    if r.returncode < 0 or r.returncode in (3, 124, 134, 137, 139):
        pytest.exit("the C caller ended with status %d (GPU fault or abort), no further test is started:\n%s" % (r.returncode, r.stdout),
                    returncode=3)
    lines = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if not w or w[0] == "#":
            continue
        assert len(w) == 4 and w[0] not in lines, "unexpected output line %r" % line
        lines[w[0]] = (w[1], float(w[2]), float(w[3]))
    return r.returncode, lines, r.stdout


@pytest.mark.parametrize("check", CHECKS)
def test_c_caller(check, caller):
    _, lines, out = caller
    assert check in lines, "the program printed no line for %s:\n%s" % (check, out)
    status, err, scale = lines[check]
    assert status == "ok", "%s: %s, max error %g at scale %g\n%s" % (check, status, err, scale, out)


def test_c_caller_ran_to_the_end(caller):
    status, lines, out = caller
    assert "# done" in out and status == 0, out
    assert set(lines) == set(CHECKS), sorted(set(lines) ^ set(CHECKS))
