/*
 * n3d_abi_caller.c -- a plain-C11 host of libn3d.so, written from include/n3d.h alone.
 *
 * What a C integrator has: the header, hipMalloc, streams of its own.  Nothing here comes from torch: every buffer is a hipMalloc
 * allocation, every launch goes to a stream this program created, every reference is a naive fp64 loop over the layouts the header
 * documents (NDHWC addressing with a voxel pitch, torch-native weight layouts, double[B][rows][C][nv] statistics rows).
 *
 * Output: one line per check, `name status max_err scale` (status ok / FAIL); lines starting with '#' are remarks.
 * Every output tensor sits inside a larger allocation: SENT_OUT in front of it, behind it and in the foreign channels of its
 * pitch; a check fails when one of those comes back changed.  Inputs carry SENT_IN in their foreign channels.
 * After a HIP error the program prints what it has, launches nothing more and exits with status 3.
 *
 * Build (tests/test_gpu_abi_c_caller.py does exactly this):
 *   $ROCM_PATH/lib/llvm/bin/clang -std=c11 -O1 -Wall -Werror -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -Iinclude \
 *       tests/abi/n3d_abi_caller.c -o n3d_abi_caller -Lnas_3d_unet_amd -ln3d -L$ROCM_PATH/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/nas_3d_unet_amd -Wl,-rpath,$ROCM_PATH/lib
 * `n3d_abi_caller --host-only` runs the checks that need no device (queries and refusals with host-only arguments).
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "n3d.h"

#define SENT_IN 28672.0f
#define SENT_OUT (-12288.0f)
#define TOL_FWD 2e-5

static hipStream_t S;          /* the program's main stream */
static hipStream_t S2;         /* its side stream */
static int g_failed;

static void report(const char* name, int ok, double err, double scale) {
  printf("%s %s %.3e %.3e\n", name, ok ? "ok" : "FAIL", err, scale);
  fflush(stdout);
  if (!ok) g_failed = 1;
}

static void die_hip(hipError_t e, const char* what) {
  printf("# HIP error, nothing more is launched: %s: %s\n", what, hipGetErrorString(e));
  fflush(stdout);
  exit(3);
}
#define HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) die_hip(e_, #call); } while (0)
/* a libn3d status other than N3D_OK fails the check `name` and leaves the case */
#define N3(name, call) do { int rc_ = (call); if (rc_ != N3D_OK) { printf("# %s: status %d: %s\n", #call, rc_, n3d_last_error()); \
                                                                     report(name, 0, NAN, 0.0); return; } } while (0)

static void* dmalloc(size_t bytes) { void* p = NULL; HIP(hipMalloc(&p, bytes ? bytes : 4)); return p; }
static void up(void* dst, const void* src, size_t bytes) { HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, S)); HIP(hipStreamSynchronize(S)); }
static void down(void* dst, const void* src, size_t bytes) { HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S)); HIP(hipStreamSynchronize(S)); }
static void* xmalloc(size_t bytes) { void* p = malloc(bytes ? bytes : 1); if (!p) { printf("# out of host memory\n"); exit(2); } return p; }

static uint32_t g_rng = 12345u;
static int irand(int lo, int hi) {            /* integer in [lo, hi] */
  g_rng = g_rng * 1664525u + 1013904223u;
  return lo + (int)((g_rng >> 8) % (uint32_t)(hi - lo + 1));
}

/* ---- a pitched NDHWC tensor (or, with nvox = 1, a plain vector) inside a guarded allocation -------------------------------------
 * element (v, c) at front + v * ld + coff + c;  front = 64 floats (a non-zero offset that keeps 16-byte alignment), 4 foreign
 * channels on each side of the slice, 64 floats behind. */
typedef struct { size_t nvox; int C, ld, coff; size_t front, total; float* h; float* d; float fill; } T;

static T t_make(size_t nvox, int C, float fill) {
  T t;
  t.nvox = nvox; t.C = C; t.coff = 4; t.ld = C + 8; t.front = 64; t.total = 64 + nvox * (size_t)t.ld + 64; t.fill = fill;
  t.h = (float*)xmalloc(t.total * sizeof(float));
  for (size_t i = 0; i < t.total; ++i) t.h[i] = fill;
  t.d = (float*)dmalloc(t.total * sizeof(float));
  return t;
}
static float* t_at(T* t, size_t v, int c) { return &t->h[t->front + v * (size_t)t->ld + (size_t)t->coff + (size_t)c]; }
static float* t_dev(const T* t) { return t->d + t->front + t->coff; }
static void t_up(const T* t) { up(t->d, t->h, t->total * sizeof(float)); }
static void t_set(T* t, const double* dense) {      /* dense [nvox][C] */
  for (size_t v = 0; v < t->nvox; ++v) for (int c = 0; c < t->C; ++c) *t_at(t, v, c) = (float)dense[v * (size_t)t->C + (size_t)c];
}
/* slice against ref (dense [nvox][C]), everything else against the fill, bit for bit.  tol = 0: exact; else max|err| <= tol * max|ref|
 * (abs_tol > 0: an absolute bound instead).  got (optional) receives the downloaded allocation. */
static int t_compare(const T* t, const double* ref, double tol, double abs_tol, double* err_out, double* scale_out, float* got_out) {
  float* got = got_out ? got_out : (float*)xmalloc(t->total * sizeof(float));
  down(got, t->d, t->total * sizeof(float));
  double err = 0.0, scale = 0.0;
  size_t bad_sent = 0;
  uint32_t fill_bits, bits;
  memcpy(&fill_bits, &t->fill, 4);
  for (size_t i = 0; i < t->total; ++i) {
    int in_slice = 0;
    size_t v = 0; int c = 0;
    if (i >= t->front && i < t->front + t->nvox * (size_t)t->ld) {
      v = (i - t->front) / (size_t)t->ld; c = (int)((i - t->front) % (size_t)t->ld) - t->coff;
      in_slice = c >= 0 && c < t->C;
    }
    if (in_slice) {
      const double r = ref[v * (size_t)t->C + (size_t)c], e = fabs((double)got[i] - r);
      if (!(e <= err)) err = e;       /* a NaN sticks */
      if (fabs(r) > scale) scale = fabs(r);
    } else {
      memcpy(&bits, &got[i], 4);
      if (bits != fill_bits) ++bad_sent;
    }
  }
  if (bad_sent) printf("# %zu sentinel floats changed\n", bad_sent);
  if (!got_out) free(got);
  *err_out = err; *scale_out = scale;
  if (bad_sent) return 0;
  if (abs_tol > 0.0) return err <= abs_tol;
  return tol == 0.0 ? err == 0.0 : err <= tol * scale;
}
static void t_check(const char* name, const T* t, const double* ref, double tol) {
  double err, scale;
  const int ok = t_compare(t, ref, tol, 0.0, &err, &scale, NULL);
  report(name, ok, err, scale);
}
static int t_untouched(const T* t) {      /* the whole allocation still holds its host image? */
  float* got = (float*)xmalloc(t->total * sizeof(float));
  down(got, t->d, t->total * sizeof(float));
  const int same = memcmp(got, t->h, t->total * sizeof(float)) == 0;
  free(got);
  return same;
}

/* ---- guarded double / byte buffers ------------------------------------------------------------------------------------------- */
#define DGUARD 16
static double* dbl_make(size_t n, double fill, double** host) {      /* returns the device base; payload at base + DGUARD */
  double* h = (double*)xmalloc((n + 2 * DGUARD) * sizeof(double));
  for (size_t i = 0; i < n + 2 * DGUARD; ++i) h[i] = fill;
  double* d = (double*)dmalloc((n + 2 * DGUARD) * sizeof(double));
  up(d, h, (n + 2 * DGUARD) * sizeof(double));
  *host = h;
  return d;
}
static int dbl_guards_ok(const double* got, size_t n, double fill) {
  for (size_t i = 0; i < DGUARD; ++i) if (memcmp(&got[i], &fill, 8) != 0 || memcmp(&got[DGUARD + n + i], &fill, 8) != 0) return 0;
  return 1;
}

/* ---- fp64 references of the conv family ------------------------------------------------------------------------------------------
 * One walk over (b, o, tap, ci, co) with i = o * stride - pad + tap * dil on every axis (torch Conv3d semantics, n3d_conv_geom):
 *   mode 0  forward             Y[b, o, co] += X[b, i, ci] * W[co][ci][tap]          X on the i side, Y on the o side
 *   mode 1  transposed / dgrad  Y[b, i, ci] += X[b, o, co] * W[co][ci][tap]          X on the o side, Y on the i side
 *   mode 2  weight gradient     Y[co][ci][tap] += X[b, i, ci] * D[b, o, co]
 * W is (Cout, Cin, k, k, k) of a Conv3d and (Cin, Cout, k, k, k) of a ConvTranspose3d whose Cin sits on the o side: the same
 * [g->Co][g->Ci][tap] indexing both times. */
static void ref_conv(const n3d_conv_geom* g, int mode, const double* X, const double* W, const double* D, double* Y) {
  const int k = g->k, taps = k * k * k;
  for (int b = 0; b < g->B; ++b)
    for (int od = 0; od < g->Do; ++od) for (int oh = 0; oh < g->Ho; ++oh) for (int ow = 0; ow < g->Wo; ++ow)
      for (int kd = 0; kd < k; ++kd) for (int kh = 0; kh < k; ++kh) for (int kw = 0; kw < k; ++kw) {
        const int id = od * g->stride - g->pad + kd * g->dil, ih = oh * g->stride - g->pad + kh * g->dil, iw = ow * g->stride - g->pad + kw * g->dil;
        if (id < 0 || id >= g->Di || ih < 0 || ih >= g->Hi || iw < 0 || iw >= g->Wi) continue;
        const size_t o = (((size_t)b * g->Do + od) * g->Ho + oh) * g->Wo + ow, i = (((size_t)b * g->Di + id) * g->Hi + ih) * g->Wi + iw;
        const int tap = (kd * k + kh) * k + kw;
        for (int co = 0; co < g->Co; ++co) for (int ci = 0; ci < g->Ci; ++ci) {
          const size_t wi = ((size_t)co * g->Ci + ci) * taps + tap;
          if (mode == 0) Y[o * g->Co + co] += X[i * g->Ci + ci] * W[wi];
          else if (mode == 1) Y[i * g->Ci + ci] += X[o * g->Co + co] * W[wi];
          else Y[wi] += X[i * g->Ci + ci] * D[o * g->Co + co];
        }
      }
}

static int odim(int i, int k, int stride, int dil, int pad) { return (i + 2 * pad - dil * (k - 1) - 1) / stride + 1; }

static double* rand_dense(size_t n, int lo, int hi) {
  double* p = (double*)xmalloc(n * sizeof(double));
  for (size_t i = 0; i < n; ++i) p[i] = (double)irand(lo, hi);
  return p;
}
static double* zeros(size_t n) { double* p = (double*)xmalloc(n * sizeof(double)); for (size_t i = 0; i < n; ++i) p[i] = 0.0; return p; }

/* statistics rows double[B][rows][C][2] against the exact per-sample sums of ref [B][nvox][C] */
static void check_stats(const char* name, const double* d_base, int B, int rows, int C, size_t nvox, const double* ref) {
  const size_t n = (size_t)B * rows * C * 2;
  double* got = (double*)xmalloc((n + 2 * DGUARD) * sizeof(double));
  down(got, d_base, (n + 2 * DGUARD) * sizeof(double));
  const double fill = -7777.0;
  int ok = dbl_guards_ok(got, n, fill);
  if (!ok) printf("# guards of the statistics buffer changed\n");
  double err = 0.0, scale = 0.0;
  for (int b = 0; b < B; ++b) for (int c = 0; c < C; ++c) {
    double s1 = 0.0, s2 = 0.0, r1 = 0.0, r2 = 0.0;
    for (int r = 0; r < rows; ++r) { s1 += got[DGUARD + (((size_t)b * rows + r) * C + c) * 2]; s2 += got[DGUARD + (((size_t)b * rows + r) * C + c) * 2 + 1]; }
    for (size_t v = 0; v < nvox; ++v) { const double y = ref[((size_t)b * nvox + v) * C + c]; r1 += y; r2 += y * y; }
    const double e = fmax(fabs(s1 - r1), fabs(s2 - r2));
    if (!(e <= err)) err = e;
    scale = fmax(scale, fmax(fabs(r1), fabs(r2)));
  }
  free(got);
  report(name, ok && err == 0.0, err, scale);
}

/* ---- case b: one convolution on channel slices, exact integer data ---------------------------------------------------------- */
static void conv_case(const char* name, int Ci, int Co, int k, int stride, int B, int D, int H, int W, int transposed, int with_bwd) {
  char nm[96];
  n3d_conv_geom g;
  memset(&g, 0, sizeof g);
  g.B = B; g.Ci = Ci; g.Co = Co; g.k = k; g.stride = stride; g.dil = 1; g.pad = k == 3 ? 1 : 0; g.depthwise = 0;
  if (transposed) { g.Di = D * stride; g.Hi = H * stride; g.Wi = W * stride; }    /* (D, H, W) is the input = the o side; the i side is the doubled grid */
  else { g.Di = D; g.Hi = H; g.Wi = W; }
  g.Do = odim(g.Di, k, stride, 1, g.pad); g.Ho = odim(g.Hi, k, stride, 1, g.pad); g.Wo = odim(g.Wi, k, stride, 1, g.pad);
  const int taps = k * k * k;
  const size_t ni = (size_t)g.Di * g.Hi * g.Wi, no = (size_t)g.Do * g.Ho * g.Wo;
  const size_t nin = transposed ? no : ni, nout = transposed ? ni : no;       /* voxels per sample of the call's input / output */
  const int cin = transposed ? Co : Ci, cout = transposed ? Ci : Co;
  snprintf(nm, sizeof nm, "%s.fwd", name);
  /* |x| <= 3, |w| <= 2, |bias| <= 4, |dy| <= 2: every sum below is an integer under 2^24, so fp32 holds it whatever the order */
  const double worst_fwd = (double)cin * taps * 3 * 2 + 4, worst_dx = (double)cout * taps * 2 * 2, worst_dw = (double)B * (double)no * 3 * 2;
  if (!(worst_fwd < 16777216.0 && worst_dx < 16777216.0 && worst_dw < 16777216.0)) { printf("# %s: the integer budget does not hold\n", name); report(nm, 0, NAN, 0.0); return; }

  double* x = rand_dense((size_t)B * nin * cin, -3, 3);
  double* w = rand_dense((size_t)Co * Ci * taps, -2, 2);
  double* bias = rand_dense((size_t)cout, -4, 4);
  double* yref = zeros((size_t)B * nout * cout);
  for (size_t v = 0; v < (size_t)B * nout; ++v) for (int c = 0; c < cout; ++c) yref[v * cout + c] = bias[c];
  ref_conv(&g, transposed ? 1 : 0, x, w, NULL, yref);

  T tx = t_make((size_t)B * nin, cin, SENT_IN), ty = t_make((size_t)B * nout, cout, SENT_OUT);
  T tw = t_make(1, Co * Ci * taps, SENT_IN), tb = t_make(1, cout, SENT_IN);
  t_set(&tx, x); t_set(&tw, w); t_set(&tb, bias);
  t_up(&tx); t_up(&ty); t_up(&tw); t_up(&tb);
  const size_t ws_bytes = n3d_conv_workspace_bytes(&g);
  void* ws = dmalloc(ws_bytes > 256 ? ws_bytes : 256);
  const int rows = n3d_conv_stats_rows(&g, transposed, 0);
  if (rows <= 0) { printf("# %s: n3d_conv_stats_rows = %d\n", name, rows); report(nm, 0, NAN, 0.0); return; }
  double* hstats;
  const size_t nstats = (size_t)B * rows * cout * 2;
  double* dstats = dbl_make(nstats, -7777.0, &hstats);
  if (transposed) N3(nm, n3d_convT_fwd(&g, t_dev(&tx), tx.ld, t_dev(&tw), t_dev(&tb), t_dev(&ty), ty.ld, 0, NULL, dstats + DGUARD, ws, ws_bytes, S));
  else N3(nm, n3d_conv_fwd(&g, t_dev(&tx), tx.ld, t_dev(&tw), t_dev(&tb), t_dev(&ty), ty.ld, 0, NULL, dstats + DGUARD, ws, ws_bytes, S));
  HIP(hipStreamSynchronize(S));
  t_check(nm, &ty, yref, 0.0);
  snprintf(nm, sizeof nm, "%s.stats", name);
  check_stats(nm, dstats, B, rows, cout, nout, yref);
  if (!t_untouched(&tx) || !t_untouched(&tw) || !t_untouched(&tb)) { snprintf(nm, sizeof nm, "%s.inputs_untouched", name); report(nm, 0, NAN, 0.0); }

  if (with_bwd) {        /* n3d_conv_bwd_both: dx on the i side, dw native, dbias */
    double* dy = rand_dense((size_t)B * no * Co, -2, 2);
    double* dxref = zeros((size_t)B * ni * Ci);
    double* dwref = zeros((size_t)Co * Ci * taps);
    double* dbref = zeros((size_t)Co);
    ref_conv(&g, 1, dy, w, NULL, dxref);
    ref_conv(&g, 2, x, NULL, dy, dwref);
    for (size_t v = 0; v < (size_t)B * no; ++v) for (int c = 0; c < Co; ++c) dbref[c] += dy[v * Co + c];
    T tdy = t_make((size_t)B * no, Co, SENT_IN), tdx = t_make((size_t)B * ni, Ci, SENT_OUT);
    T tdw = t_make(1, Co * Ci * taps, SENT_OUT), tdb = t_make(1, Co, SENT_OUT);
    t_set(&tdy, dy);
    t_up(&tdy); t_up(&tdx); t_up(&tdw); t_up(&tdb);
    void* ws_d = dmalloc(ws_bytes > 256 ? ws_bytes : 256);
    void* ws_w = dmalloc(ws_bytes > 256 ? ws_bytes : 256);
    snprintf(nm, sizeof nm, "%s.bwd_dx", name);
    N3(nm, n3d_conv_bwd_both(&g, t_dev(&tx), tx.ld, t_dev(&tdy), tdy.ld, t_dev(&tw), t_dev(&tdx), tdx.ld, 0, NULL, 0, NULL, ws_d, ws_bytes,
                             t_dev(&tdw), t_dev(&tdb), 0, NULL, ws_w, ws_bytes, NULL, S));
    HIP(hipStreamSynchronize(S));
    t_check(nm, &tdx, dxref, 0.0);
    snprintf(nm, sizeof nm, "%s.bwd_dw", name);
    t_check(nm, &tdw, dwref, 0.0);
    snprintf(nm, sizeof nm, "%s.bwd_dbias", name);
    t_check(nm, &tdb, dbref, 0.0);
  }
}

/* ---- cases b(i) + c + g: INTEGRATION.md's conv -> statistics -> n3d_gn_coeffs -> n3d_affine_act chain ------------------------- */
typedef struct {
  n3d_conv_geom g;
  T x, w, bias, y, gamma, beta, a, b, mr, out;
  double* dstats; size_t nstats; int rows;
  void* ws; size_t ws_bytes;
  size_t nvox;
} Chain;
#define CHAIN_EPS 1e-5f

static int chain_enqueue(Chain* c, hipStream_t s) {
  const n3d_conv_geom* g = &c->g;
  int rc = n3d_conv_fwd(g, t_dev(&c->x), c->x.ld, t_dev(&c->w), t_dev(&c->bias), t_dev(&c->y), c->y.ld, 0, NULL, c->dstats + DGUARD, c->ws, c->ws_bytes, s);
  if (rc) return rc;
  rc = n3d_gn_coeffs(c->dstats + DGUARD, c->rows, t_dev(&c->gamma), t_dev(&c->beta), g->B, g->Co, 1, (int64_t)c->nvox, CHAIN_EPS, t_dev(&c->a), t_dev(&c->b),
                     t_dev(&c->mr), NULL, s);
  if (rc) return rc;
  return n3d_affine_act(t_dev(&c->y), c->y.ld, t_dev(&c->a), t_dev(&c->b), NULL, t_dev(&c->out), c->out.ld, g->B, (int64_t)c->nvox, g->Co,
                        N3D_RELU | N3D_ACCUMULATE, s);
}

static void chain_case(void) {
  Chain c;
  memset(&c, 0, sizeof c);
  const int B = 1, Ci = 4, Co = 4, D = 8, H = 8, W = 16, taps = 27;
  c.g.B = B; c.g.Di = c.g.Do = D; c.g.Hi = c.g.Ho = H; c.g.Wi = c.g.Wo = W; c.g.Ci = Ci; c.g.Co = Co; c.g.k = 3; c.g.stride = 1; c.g.dil = 1; c.g.pad = 1;
  c.nvox = (size_t)D * H * W;
  const size_t nall = (size_t)B * c.nvox;
  double* x = rand_dense(nall * Ci, -3, 3);
  double* w = rand_dense((size_t)Co * Ci * taps, -2, 2);
  double* bias = rand_dense(Co, -4, 4);
  double* gamma = (double*)xmalloc(Co * sizeof(double));
  double* beta = (double*)xmalloc(Co * sizeof(double));
  for (int i = 0; i < Co; ++i) { gamma[i] = 0.5 + 0.25 * i; beta[i] = -0.375 + 0.25 * i; }
  double* base = (double*)xmalloc(nall * Co * sizeof(double));
  for (size_t i = 0; i < nall * Co; ++i) base[i] = (double)irand(-8, 8) * 0.125;
  double* yref = zeros(nall * Co);
  for (size_t v = 0; v < nall; ++v) for (int k = 0; k < Co; ++k) yref[v * Co + k] = bias[k];
  ref_conv(&c.g, 0, x, w, NULL, yref);
  /* fp64 GroupNorm(1, C) + ReLU on top of the base: one group per sample over nvox * C elements, biased variance */
  double* oref = (double*)xmalloc(nall * Co * sizeof(double));
  double* aref = (double*)xmalloc((size_t)B * Co * sizeof(double));
  double* bref = (double*)xmalloc((size_t)B * Co * sizeof(double));
  double* mrref = (double*)xmalloc((size_t)B * 2 * sizeof(double));
  for (int b = 0; b < B; ++b) {
    double s1 = 0.0, s2 = 0.0;
    const double cnt = (double)c.nvox * Co;
    for (size_t i = 0; i < c.nvox * Co; ++i) { const double y = yref[(size_t)b * c.nvox * Co + i]; s1 += y; s2 += y * y; }
    const double mean = s1 / cnt, var = s2 / cnt - mean * mean, rstd = 1.0 / sqrt(var + (double)CHAIN_EPS);
    mrref[b * 2] = mean; mrref[b * 2 + 1] = rstd;
    for (int k = 0; k < Co; ++k) { aref[b * Co + k] = gamma[k] * rstd; bref[b * Co + k] = beta[k] - mean * rstd * gamma[k]; }
    for (size_t v = 0; v < c.nvox; ++v) for (int k = 0; k < Co; ++k) {
      const size_t i = ((size_t)b * c.nvox + v) * Co + k;
      const double z = (yref[i] - mean) * rstd * gamma[k] + beta[k];
      oref[i] = base[i] + (z > 0.0 ? z : 0.0);
    }
  }
  c.x = t_make(nall, Ci, SENT_IN); c.w = t_make(1, Co * Ci * taps, SENT_IN); c.bias = t_make(1, Co, SENT_IN);
  c.gamma = t_make(1, Co, SENT_IN); c.beta = t_make(1, Co, SENT_IN);
  c.y = t_make(nall, Co, SENT_OUT); c.out = t_make(nall, Co, SENT_OUT);
  c.a = t_make(1, B * Co, SENT_OUT); c.b = t_make(1, B * Co, SENT_OUT); c.mr = t_make(1, B * 2, SENT_OUT);
  t_set(&c.x, x); t_set(&c.w, w); t_set(&c.bias, bias); t_set(&c.gamma, gamma); t_set(&c.beta, beta); t_set(&c.out, base);
  t_up(&c.x); t_up(&c.w); t_up(&c.bias); t_up(&c.gamma); t_up(&c.beta); t_up(&c.y); t_up(&c.out); t_up(&c.a); t_up(&c.b); t_up(&c.mr);
  c.ws_bytes = n3d_conv_workspace_bytes(&c.g);
  c.ws = dmalloc(c.ws_bytes > 256 ? c.ws_bytes : 256);
  c.rows = n3d_conv_stats_rows(&c.g, 0, 0);
  if (c.rows <= 0) { printf("# chain: n3d_conv_stats_rows = %d\n", c.rows); report("chain.conv", 0, NAN, 0.0); return; }
  double* hstats;
  c.nstats = (size_t)B * c.rows * Co * 2;
  c.dstats = dbl_make(c.nstats, -7777.0, &hstats);

  N3("chain.conv", chain_enqueue(&c, S));
  HIP(hipStreamSynchronize(S));
  t_check("chain.conv", &c.y, yref, 0.0);
  check_stats("chain.stats", c.dstats, B, c.rows, Co, c.nvox, yref);
  t_check("chain.gn_a", &c.a, aref, TOL_FWD);
  t_check("chain.gn_b", &c.b, bref, TOL_FWD);
  t_check("chain.gn_mean_rstd", &c.mr, mrref, TOL_FWD);
  float* eager_out = (float*)xmalloc(c.out.total * sizeof(float));
  float* eager_y = (float*)xmalloc(c.y.total * sizeof(float));
  double err, scale;
  const int ok = t_compare(&c.out, oref, TOL_FWD, 0.0, &err, &scale, eager_out);
  report("chain.affine_act", ok, err, scale);
  down(eager_y, c.y.d, c.y.total * sizeof(float));

  /* case g: the same three calls captured into a graph and replayed twice; y, the coefficients and the statistics are reset to
   * their sentinel images and `out` to its base before every replay, by copies on the stream, outside the graph */
  void* graph = NULL;
  N3("graph.capture", n3d_stream_capture_begin(S));
  const int rc_chain = chain_enqueue(&c, S);
  const int rc_end = n3d_stream_capture_end(S, &graph);
  if (rc_chain != N3D_OK || rc_end != N3D_OK || !graph) {
    printf("# capture: chain status %d, end status %d: %s\n", rc_chain, rc_end, n3d_last_error());
    report("graph.capture", 0, NAN, 0.0);
    return;
  }
  report("graph.capture", 1, 0.0, 0.0);
  float* got = (float*)xmalloc(c.out.total * sizeof(float));
  for (int rep = 0; rep < 2; ++rep) {
    char nm[64];
    HIP(hipMemcpyAsync(c.out.d, c.out.h, c.out.total * sizeof(float), hipMemcpyHostToDevice, S));
    HIP(hipMemcpyAsync(c.y.d, c.y.h, c.y.total * sizeof(float), hipMemcpyHostToDevice, S));
    HIP(hipMemcpyAsync(c.a.d, c.a.h, c.a.total * sizeof(float), hipMemcpyHostToDevice, S));
    HIP(hipMemcpyAsync(c.b.d, c.b.h, c.b.total * sizeof(float), hipMemcpyHostToDevice, S));
    HIP(hipMemcpyAsync(c.dstats, hstats, (c.nstats + 2 * DGUARD) * sizeof(double), hipMemcpyHostToDevice, S));
    HIP(hipStreamSynchronize(S));
    snprintf(nm, sizeof nm, "graph.replay%d", rep);
    N3(nm, n3d_graph_launch(graph, S));
    HIP(hipStreamSynchronize(S));
    down(got, c.out.d, c.out.total * sizeof(float));
    int same = memcmp(got, eager_out, c.out.total * sizeof(float)) == 0;
    down(got, c.y.d, c.y.total * sizeof(float));       /* y.total == out.total: same shape */
    same = same && memcmp(got, eager_y, c.y.total * sizeof(float)) == 0;
    report(nm, same, same ? 0.0 : NAN, scale);
  }
  (void)n3d_graph_destroy(graph);
}

/* ---- case d: n3d_adam_step, three steps; case f: the guarded form behind the stream hand-off of INTEGRATION.md ------------------- */
#define ADAM_N (8192 + 5)
typedef struct { float lr, b1, b2, eps, wd, gs; } AdamHp;
static const AdamHp HP = {1e-2f, 0.9f, 0.999f, 1e-8f, 0.f, 1.f};      /* the values of INTEGRATION.md's snippet */

static void adam_ref64(double* p, double* m, double* v, const double* g, size_t n, int t) {
  const double b1 = (double)HP.b1, b2 = (double)HP.b2, lr = (double)HP.lr, eps = (double)HP.eps;
  const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
  for (size_t i = 0; i < n; ++i) {
    double gi = g[i] * (double)HP.gs;
    if (HP.wd != 0.f) gi += (double)HP.wd * p[i];
    m[i] = b1 * m[i] + (1.0 - b1) * gi;
    v[i] = b2 * v[i] + (1.0 - b2) * gi * gi;
    p[i] -= lr / bc1 * (m[i] / (sqrt(v[i]) / sqrt(bc2) + eps));
  }
}
static void adam_ref32(float* p, float* m, float* v, const float* g, size_t n, int t) {      /* the same recurrence, every operation in fp32 */
  const float bc1 = 1.f - powf(HP.b1, (float)t), bc2 = 1.f - powf(HP.b2, (float)t);
  for (size_t i = 0; i < n; ++i) {
    float gi = g[i] * HP.gs;
    if (HP.wd != 0.f) gi += HP.wd * p[i];
    m[i] = HP.b1 * m[i] + (1.f - HP.b1) * gi;
    v[i] = HP.b2 * v[i] + (1.f - HP.b2) * gi * gi;
    p[i] -= HP.lr / bc1 * (m[i] / (sqrtf(v[i]) / sqrtf(bc2) + HP.eps));
  }
}
/* n floats one float (4 bytes) off a 16-byte boundary, 64 sentinel floats on each side */
typedef struct { float* d; float* h; size_t n, total; } Off;
static Off off_make(size_t n, const float* init) {
  Off o;
  o.n = n; o.total = 64 + 1 + n + 64;
  o.h = (float*)xmalloc(o.total * sizeof(float));
  for (size_t i = 0; i < o.total; ++i) o.h[i] = SENT_OUT;
  for (size_t i = 0; i < n; ++i) o.h[65 + i] = init ? init[i] : 0.f;
  o.d = (float*)dmalloc(o.total * sizeof(float));
  up(o.d, o.h, o.total * sizeof(float));
  return o;
}
static float* off_dev(const Off* o) { return o->d + 65; }
static int off_check(const Off* o, const double* ref, double tol_abs, double* err_out, double* scale_out, float* keep) {
  float* got = (float*)xmalloc(o->total * sizeof(float));
  down(got, o->d, o->total * sizeof(float));
  const float s = SENT_OUT;
  int ok = 1;
  for (size_t i = 0; i < 65; ++i) if (memcmp(&got[i], &s, 4) != 0) ok = 0;
  for (size_t i = 65 + o->n; i < o->total; ++i) if (memcmp(&got[i], &s, 4) != 0) ok = 0;
  if (!ok) printf("# sentinel floats around an optimiser buffer changed\n");
  double err = 0.0, scale = 0.0;
  for (size_t i = 0; i < o->n; ++i) {
    const double e = fabs((double)got[65 + i] - ref[i]);
    if (!(e <= err)) err = e;
    if (fabs(ref[i]) > scale) scale = fabs(ref[i]);
  }
  if (keep) memcpy(keep, got + 65, o->n * sizeof(float));
  free(got);
  *err_out = err; *scale_out = scale;
  return ok && err <= tol_abs;
}

static float g_adam_p0[ADAM_N], g_adam_g0[ADAM_N], g_adam_first[3][ADAM_N];      /* initial state and the device's first step (p, m, v) */
static int g_adam_have_first;

static void adam_case(void) {
  const size_t n = ADAM_N;
  static float g[3][ADAM_N], p32[ADAM_N], m32[ADAM_N], v32[ADAM_N];
  static double gd[ADAM_N], p64[ADAM_N], m64[ADAM_N], v64[ADAM_N];
  for (size_t i = 0; i < n; ++i) {
    g_adam_p0[i] = (float)irand(-2000, 2000) * (1.0f / 1024.0f);
    for (int s = 0; s < 3; ++s) g[s][i] = (float)irand(-3000, 3000) * (1.0f / 4096.0f);
    g_adam_g0[i] = g[0][i];
    p32[i] = g_adam_p0[i]; p64[i] = (double)g_adam_p0[i]; m32[i] = v32[i] = 0.f; m64[i] = v64[i] = 0.0;
  }
  Off P = off_make(n, g_adam_p0), M = off_make(n, NULL), V = off_make(n, NULL), G = off_make(n, g[0]);
  float lr_host = HP.lr;
  float* lr_dev = (float*)dmalloc(4);
  int32_t* step = (int32_t*)dmalloc(8);        /* int32[2]: steps taken, ticket counter (inc_step == 2) */
  int32_t step_host[2] = {0, 0};
  up(lr_dev, &lr_host, 4);
  up(step, step_host, 8);
  for (int s = 0; s < 3; ++s) {
    if (s > 0) { memcpy(G.h + 65, g[s], n * sizeof(float)); up(G.d, G.h, G.total * sizeof(float)); }
    /* the immediate learning rate is a decoy: lr_ptr wins */
    N3("adam.param", n3d_adam_step(off_dev(&P), off_dev(&G), off_dev(&M), off_dev(&V), (int64_t)n, 123.f, lr_dev, HP.b1, HP.b2, HP.eps, HP.wd, HP.gs,
                                   step, 2, S));
    HIP(hipStreamSynchronize(S));
    for (size_t i = 0; i < n; ++i) gd[i] = (double)g[s][i];
    adam_ref64(p64, m64, v64, gd, n, s + 1);
    adam_ref32(p32, m32, v32, g[s], n, s + 1);
    if (s == 0) {
      double e, sc;
      (void)off_check(&P, p64, INFINITY, &e, &sc, g_adam_first[0]);
      (void)off_check(&M, m64, INFINITY, &e, &sc, g_adam_first[1]);
      (void)off_check(&V, v64, INFINITY, &e, &sc, g_adam_first[2]);
      g_adam_have_first = 1;
    }
  }
  /* tolerance, the suite's rule for the optimisers: 4 x the error of the fp32 restatement against the fp64 recurrence + 2^-23 max|ref| */
  const Off* bufs[3] = {&P, &M, &V};
  const double* r64[3] = {p64, m64, v64};
  const float* r32[3] = {p32, m32, v32};
  const char* names[3] = {"adam.param", "adam.exp_avg", "adam.exp_avg_sq"};
  for (int k = 0; k < 3; ++k) {
    double e32 = 0.0, scale = 0.0, err, sc;
    for (size_t i = 0; i < n; ++i) { e32 = fmax(e32, fabs((double)r32[k][i] - r64[k][i])); scale = fmax(scale, fabs(r64[k][i])); }
    const double tol = 4.0 * e32 + ldexp(1.0, -23) * scale;
    const int ok = off_check(bufs[k], r64[k], tol, &err, &sc, NULL);
    printf("# %s: fp32 restatement error %.3e, tolerance %.3e\n", names[k], e32, tol);
    report(names[k], ok, err, sc);
  }
  down(step_host, step, 8);
  report("adam.step_counter", step_host[0] == 3 && step_host[1] == 0, fabs((double)step_host[0] - 3.0) + fabs((double)step_host[1]), 3.0);
}

static void handoff_case(void) {
  /* INTEGRATION.md section 3, first snippet, as written: two streams `main`, `side`; sync = device uint32_t[8], sync[0] = sync[2] = 1 */
  hipStream_t main_ = S, side = S2;
  uint32_t init[8] = {1, 0, 1, 0, 0, 0, 0, 0}, got[8];
  uint32_t* sync = (uint32_t*)dmalloc(sizeof init);
  up(sync, init, sizeof init);
  N3("handoff.words", n3d_sync_signal(&sync[4], &sync[0], /*bump*/ 0, main_));
  N3("handoff.words", n3d_sync_wait(&sync[4], &sync[2], /*timeouts*/ &sync[1], /*bump*/ 0, /*max_polls*/ 5000000, side));
  N3("handoff.words", n3d_sync_signal(&sync[5], &sync[2], 1, side));
  N3("handoff.words", n3d_sync_wait(&sync[5], &sync[0], &sync[1], 1, 5000000, main_));
  HIP(hipStreamSynchronize(side));
  HIP(hipStreamSynchronize(main_));
  down(got, sync, sizeof got);
  /* no time-out; both step counters bumped once; each flag holds the step its signal published */
  const int ok = got[1] == 0 && got[0] == 2 && got[2] == 2 && got[4] == 1 && got[5] == 1 && got[3] == 0 && got[6] == 0 && got[7] == 0;
  if (!ok) printf("# sync words: %u %u %u %u %u %u %u %u\n", got[0], got[1], got[2], got[3], got[4], got[5], got[6], got[7]);
  report("handoff.words", ok, (double)got[1], 1.0);

  /* second snippet: the guarded update; acked is a device word of its own (sync[6]), equal to the time-out count (both 0) */
  if (!g_adam_have_first) { report("handoff.guarded_adam", 0, NAN, 0.0); return; }
  const size_t n = ADAM_N;
  Off P = off_make(n, g_adam_p0), M = off_make(n, NULL), V = off_make(n, NULL), G = off_make(n, g_adam_g0);
  float lr_host = HP.lr, loss_host = 0.25f;
  float* lr_dev = (float*)dmalloc(4);
  float* loss_dev = (float*)dmalloc(4);
  int32_t* step = (int32_t*)dmalloc(8);
  int32_t step_host[2] = {0, 0};
  void* host_word = NULL;
  up(lr_dev, &lr_host, 4); up(loss_dev, &loss_host, 4); up(step, step_host, 8);
  N3("handoff.guarded_adam", n3d_host_word_alloc(&host_word));
  N3("handoff.guarded_adam", n3d_adam_step_guarded(off_dev(&P), off_dev(&G), off_dev(&M), off_dev(&V), (int64_t)n, HP.lr, lr_dev, 0.9f, 0.999f, 1e-8f, 0.f, 1.f,
                                                   step, /*inc_step*/ 2, /*timeouts*/ &sync[1], /*acked*/ &sync[6], /*peer_flag*/ NULL,
                                                   /*loss*/ loss_dev, host_word, main_));
  HIP(hipStreamSynchronize(main_));
  const uint32_t word = *(volatile uint32_t*)host_word;
  static float back[3][ADAM_N];
  static double ref[ADAM_N];
  double err = 0.0, scale = 0.0, e, sc;
  int same = 1;
  const Off* bufs[3] = {&P, &M, &V};
  for (int k = 0; k < 3; ++k) {
    for (size_t i = 0; i < n; ++i) ref[i] = (double)g_adam_first[k][i];
    same = off_check(bufs[k], ref, 0.0, &e, &sc, back[k]) && same;      /* bit for bit case d's first step */
    err = fmax(err, e); scale = fmax(scale, sc);
  }
  down(&loss_host, loss_dev, 4); down(step_host, step, 8);
  const int ok2 = same && word == 0 && loss_host == 0.25f && step_host[0] == 1 && step_host[1] == 0;
  if (!ok2) printf("# guarded adam: host word %u, loss %g, step words %d %d\n", word, (double)loss_host, step_host[0], step_host[1]);
  report("handoff.guarded_adam", ok2, err, scale);
  (void)n3d_host_word_free(host_word);
}

/* ---- case e: index work, bit for bit --------------------------------------------------------------------------------------------- */
static void patch_case(void) {
  enum { Cv = 2, X = 6, Y = 7, Z = 5, P = 4, B = 2, P3 = P * P * P };
  static float vol[Cv][X][Y][Z];
  static uint8_t truth[X][Y][Z];
  static const uint8_t label_of[4] = {0, 1, 2, 4};
  for (int c = 0; c < Cv; ++c) for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) for (int z = 0; z < Z; ++z) vol[c][x][y][z] = (float)(1000 * (c + 1) + 100 * x + 10 * y + z);
  for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) for (int z = 0; z < Z; ++z) truth[x][y][z] = label_of[irand(0, 3)];
  /* patch 0: the identity key inside the volume; patch 1: permutation + flips, its corner partly outside on every axis */
  const n3d_patch_desc descs[B] = {{{1, 2, 0}, {0, 1, 2}, {0, 0, 0}}, {{-1, 5, 3}, {2, 0, 1}, {1, 0, 1}}};
  static double xref[B * P3 * Cv];
  static uint8_t lab[B][P3];
  for (int b = 0; b < B; ++b) for (int i0 = 0; i0 < P; ++i0) for (int i1 = 0; i1 < P; ++i1) for (int i2 = 0; i2 < P; ++i2) {
    const int i[3] = {i0, i1, i2};
    int q[3], inside = 1;
    const int dims[3] = {X, Y, Z};
    for (int a = 0; a < 3; ++a) {
      const int s = descs[b].flip[a] ? P - 1 - i[descs[b].perm[a]] : i[descs[b].perm[a]];
      q[a] = descs[b].corner[a] + s;
      if (q[a] < 0 || q[a] >= dims[a]) inside = 0;
    }
    const int v = (i0 * P + i1) * P + i2;
    for (int c = 0; c < Cv; ++c) xref[((size_t)b * P3 + v) * Cv + c] = inside ? (double)vol[c][q[0]][q[1]][q[2]] : 0.0;
    lab[b][v] = inside ? truth[q[0]][q[1]][q[2]] : 0;
  }
  float* dvol = (float*)dmalloc(sizeof vol);
  uint8_t* dtruth = (uint8_t*)dmalloc(sizeof truth);
  up(dvol, vol, sizeof vol); up(dtruth, truth, sizeof truth);
  for (int pass = 0; pass < 2; ++pass) {
    const int u8 = pass == 1, inclusive = pass == 1;
    const char* nx = u8 ? "patch_u8.x" : "patch_f32.x";
    const char* nt = u8 ? "patch_u8.t" : "patch_f32.t";
    static double tref[B * 3 * P3];
    for (int b = 0; b < B; ++b) for (int v = 0; v < P3; ++v) {
      const int l = lab[b][v];
      /* N3D_PATCH_INCLUSIVE: (TC, "WT" with the reference's quirk = labels {1, 2}, ET); otherwise (label 1, label 2, label 4) */
      const int ch[3] = {inclusive ? (l == 1 || l == 4) : l == 1, inclusive ? (l == 1 || l == 2) : l == 2, l == 4};
      for (int k = 0; k < 3; ++k) tref[((size_t)b * 3 + k) * P3 + v] = (double)ch[k];
    }
    T tx = t_make((size_t)B * P3, Cv, SENT_OUT);
    t_up(&tx);
    if (!u8) {
      T tt = t_make(1, B * 3 * P3, SENT_OUT);
      t_up(&tt);
      N3(nx, n3d_patch_batch(dvol, Cv, dtruth, X, Y, Z, descs, B, P, 0, t_dev(&tx), tx.ld, t_dev(&tt), S));
      HIP(hipStreamSynchronize(S));
      t_check(nx, &tx, xref, 0.0);
      t_check(nt, &tt, tref, 0.0);
    } else {
      enum { NT = B * 3 * P3, GUARD = 64 };
      static uint8_t ht[NT + 2 * GUARD], got[NT + 2 * GUARD];
      memset(ht, 0xAB, sizeof ht);
      uint8_t* dt = (uint8_t*)dmalloc(sizeof ht);
      up(dt, ht, sizeof ht);
      N3(nx, n3d_patch_batch(dvol, Cv, dtruth, X, Y, Z, descs, B, P, N3D_PATCH_INCLUSIVE | N3D_PATCH_T_U8, t_dev(&tx), tx.ld, dt + GUARD, S));
      HIP(hipStreamSynchronize(S));
      t_check(nx, &tx, xref, 0.0);
      down(got, dt, sizeof got);
      int ok = 1, wrong = 0;
      for (int i = 0; i < GUARD; ++i) if (got[i] != 0xAB || got[GUARD + NT + i] != 0xAB) ok = 0;
      for (int i = 0; i < NT; ++i) if ((double)got[GUARD + i] != tref[i]) ++wrong;
      report(nt, ok && wrong == 0, (double)wrong, 1.0);
    }
  }
}

static void stitch_case(void) {
  enum { C = 3, P = 4, B = 2, X = 6, Y = 5, Z = 4, FX = 8, FY = 6, FZ = 5, OX = 1, OY = 1, OZ = 0, P3 = P * P * P, NF = FX * FY * FZ };
  const int32_t corners[B][3] = {{0, 0, 0}, {2, 1, -1}};        /* overlap on a 2 x 3 x 3 block; the second hangs over the low z border */
  /* patches as the net leaves them: pitched NDHWC, element (b, c, v) at b * sb + c * sc + v * sv */
  T tp = t_make((size_t)B * P3, C, SENT_IN);
  static double pv[B][C][P3];
  for (int b = 0; b < B; ++b) for (int c = 0; c < C; ++c) for (int v = 0; v < P3; ++v) {
    pv[b][c][v] = (double)irand(0, 8) * 0.125;
    *t_at(&tp, (size_t)b * P3 + v, c) = (float)pv[b][c][v];
  }
  t_up(&tp);
  int32_t* dcorners = (int32_t*)dmalloc(sizeof corners);
  up(dcorners, corners, sizeof corners);
  const double fill = -7.0;
  static double ref[C * NF];
  for (int i = 0; i < C * NF; ++i) ref[i] = fill;
  for (int x = 0; x < X; ++x) for (int y = 0; y < Y; ++y) for (int z = 0; z < Z; ++z) for (int c = 0; c < C; ++c) {
    double sum = 0.0; int cnt = 0;
    for (int b = 0; b < B; ++b) {        /* list order, fp64 */
      const int lx = x - corners[b][0], ly = y - corners[b][1], lz = z - corners[b][2];
      if (lx < 0 || lx >= P || ly < 0 || ly >= P || lz < 0 || lz >= P) continue;
      sum += pv[b][c][(lx * P + ly) * P + lz];
      ++cnt;
    }
    ref[((c * FX + x + OX) * FY + y + OY) * FZ + z + OZ] = cnt ? sum / (double)cnt : 0.0;
  }
  double* hout;
  double* dout = dbl_make((size_t)C * NF, fill, &hout);
  N3("stitch.mean", n3d_stitch(t_dev(&tp), (int64_t)P3 * tp.ld, 1, tp.ld, C, P, dcorners, B, X, Y, Z, dout + DGUARD, FX, FY, FZ, OX, OY, OZ, S));
  HIP(hipStreamSynchronize(S));
  static double got[C * NF + 2 * DGUARD];
  down(got, dout, sizeof got);
  int ok = dbl_guards_ok(got, (size_t)C * NF, fill);
  double err = 0.0;
  for (int i = 0; i < C * NF; ++i) { const double e = fabs(got[DGUARD + i] - ref[i]); if (!(e <= err)) err = e; }
  report("stitch.mean", ok && err == 0.0, err, 1.0);

  /* n3d_tumor_labels on the stitched image (3, NF), inclusive channels TC / WT / ET: nested regions, so ET wins, then TC, then WT.
   * the means are multiples of 1/16 and the fill is negative: nothing sits on the threshold */
  const double thr = 0.46875 + 1.0 / 64.0;
  enum { GUARD = 64 };
  static uint8_t hl[NF + 2 * GUARD], gl[NF + 2 * GUARD];
  memset(hl, 0xAB, sizeof hl);
  uint8_t* dl = (uint8_t*)dmalloc(sizeof hl);
  up(dl, hl, sizeof hl);
  N3("stitch.labels", n3d_tumor_labels(dout + DGUARD, NF, thr, 1, dl + GUARD, S));
  HIP(hipStreamSynchronize(S));
  down(gl, dl, sizeof gl);
  int wrong = 0;
  ok = 1;
  for (int i = 0; i < GUARD; ++i) if (gl[i] != 0xAB || gl[GUARD + NF + i] != 0xAB) ok = 0;
  for (int i = 0; i < NF; ++i) {
    const int tc = ref[i] >= thr, wt = ref[NF + i] >= thr, et = ref[2 * NF + i] >= thr;
    const int want = et ? 4 : tc ? 1 : wt ? 2 : 0;
    if (gl[GUARD + i] != want) ++wrong;
  }
  report("stitch.labels", ok && wrong == 0, (double)wrong, 1.0);
}

/* ---- case a: queries and refusals --------------------------------------------------------------------------------------------------- */
static void refusal(const char* name, int rc, int want, const char* entry, int outputs_untouched) {
  const char* msg = n3d_last_error();
  const int ok = rc == want && msg && msg[0] && strstr(msg, entry) != NULL && outputs_untouched;
  if (!ok) printf("# %s: status %d (want %d), message \"%s\" (want it to name %s), outputs untouched %d\n", name, rc, want, msg ? msg : "", entry, outputs_untouched);
  report(name, ok, 0.0, 0.0);
}

static void query_case(int have_device) {
  n3d_conv_geom g = {2, 8, 8, 16, 4, 8, 8, 16, 4, 3, 1, 1, 1, 0};
  report("query.version", n3d_version() >= 1, 0.0, 0.0);
  report("query.workspace_bytes", n3d_conv_workspace_bytes(&g) > 0, 0.0, 0.0);
  report("query.conv_stats_rows", n3d_conv_stats_rows(&g, 0, 0) > 0, 0.0, 0.0);
  report("query.stats_rows", n3d_stats_rows(4096, 16) > 0 && n3d_fused_max_rows() > 0 && n3d_head_rows(4096) > 0 && n3d_dice_rows(4096) > 0, 0.0, 0.0);
  report("query.job_tables", n3d_selftest_job_tables() > 0, 0.0, 0.0);
  /* refusals whose argument check sits in front of every launch (csrc: check_geom / N3D_CHECK_ARG at the top of run_fwd_call,
   * n3d_affine_act_bwd_apply_gn2, check_head).  Without a device the pointers are host dummies that are never dereferenced. */
  static float dummy[64];
  T ty, tdraw;
  memset(&ty, 0, sizeof ty); memset(&tdraw, 0, sizeof tdraw);
  float *y = dummy, *draw = dummy, *x = dummy;
  if (have_device) {
    ty = t_make(64, 4, SENT_OUT); tdraw = t_make(64, 16, SENT_OUT);
    t_up(&ty); t_up(&tdraw);
    y = t_dev(&ty); draw = t_dev(&tdraw); x = (float*)dmalloc(4096);
  }
  int rc = n3d_conv_fwd(&g, NULL, 12, NULL, NULL, y, 12, 0, NULL, NULL, NULL, 0, have_device ? (void*)S : NULL);
  refusal("refuse.conv_fwd_null", rc, N3D_ERR_INVALID, "conv_fwd", 1);
  n3d_conv_geom g2 = g;
  g2.k = 2;
  rc = n3d_conv_fwd(&g2, x, 12, x, x, y, 12, 0, NULL, NULL, x, 4096, have_device ? (void*)S : NULL);
  refusal("refuse.conv_fwd_k2", rc, N3D_ERR_UNSUPPORTED, "conv_fwd", 1);
  n3d_gn_bwd_term t0, t1;
  memset(&t0, 0, sizeof t0);
  t0.rows = 1; t0.draw = draw; t0.drld = 24;
  t1 = t0;
  rc = n3d_affine_act_bwd_apply_gn2(x, 16, NULL, 0, &t0, &t1, /*B*/ 5, /*N*/ 8, /*C*/ 16, /*G*/ 1, have_device ? (void*)S : NULL);
  refusal("refuse.apply_gn2_B5", rc, N3D_ERR_UNSUPPORTED, "affine_act_bwd_apply_gn2", 1);
  n3d_head h;
  memset(&h, 0, sizeof h);
  h.x = x; h.xld = 4; h.x_dtype = N3D_F32; h.B = 1; h.Ci = 4; h.Co = 2; h.N = 64; h.w = x; h.bias = x; h.t_dtype = N3D_U8;
  rc = n3d_head_fwd(&h, y, 64 * 12, 1, 12, NULL, NULL, 0, 0, 0, 1.f, NULL, NULL, NULL, have_device ? (void*)S : NULL);
  refusal("refuse.head_fwd_u8_co2", rc, N3D_ERR_UNSUPPORTED, "head_fwd", 1);
  if (have_device) {
    HIP(hipStreamSynchronize(S));
    report("refuse.outputs_untouched", t_untouched(&ty) && t_untouched(&tdraw), 0.0, 0.0);
  }
}

int main(int argc, char** argv) {
  const int host_only = argc > 1 && strcmp(argv[1], "--host-only") == 0;
  if (host_only) {
    query_case(0);
    return g_failed ? 1 : 0;
  }
  const int dev_ok = n3d_device_ok();
  report("query.device_ok", dev_ok == 1, 0.0, 0.0);
  if (dev_ok != 1) { printf("# %s\n", n3d_last_error()); return 1; }
  HIP(hipStreamCreateWithFlags(&S, hipStreamNonBlocking));
  HIP(hipStreamCreateWithFlags(&S2, hipStreamNonBlocking));
  query_case(1);
  chain_case();                                                     /* b(i) forward + c + g */
  conv_case("conv3_4to4", 4, 4, 3, 1, 1, 8, 8, 16, 0, 1);           /* b(i) again, with its backward */
  conv_case("conv3_16to16", 16, 16, 3, 1, 2, 4, 4, 4, 0, 1);
  conv_case("conv1_12to8", 12, 8, 1, 1, 2, 8, 8, 8, 0, 0);
  conv_case("conv3s2_4to12", 4, 12, 3, 2, 2, 8, 8, 12, 0, 0);
  conv_case("convT3s2_8to8", 8, 8, 3, 2, 2, 4, 4, 6, 1, 0);
  adam_case();
  patch_case();
  stitch_case();
  handoff_case();
  HIP(hipStreamSynchronize(S));
  HIP(hipStreamSynchronize(S2));
  HIP(hipStreamDestroy(S2));
  HIP(hipStreamDestroy(S));
  printf("# done\n");
  return g_failed ? 1 : 0;
}
