// Acquisition artefacts of a gathered batch, in place (artefact.Artefact, Generator(augment_artefact=...)):
// n3d_patch_artefact -- simulated low resolution, a multiplicative bias field and modality dropout on a pitched NDHWC batch.
// include/n3d.h states the rule operation by operation; every fp64 product, sum and quotient below is one separately rounded
// operation in the association written there, so this file is compiled with contraction off (Makefile); the one fused
// multiply-add the rule has, the low-resolution source coordinate, is an explicit fma().
// Shape: one mask launch (launch_brain_mask, shared with appearance.hip), then per stage that some patch of the batch asks for
//   low resolution  2 launches  a thread per masked voxel: the channel's per-axis taps (a0, a1, l1) from a table the workgroup
//                               builds in LDS, the eight taps of a channel loaded together, the rounded result to scratch; then
//                               the masked voxels land back in x (the taps read x: the result must not depend on who wrote first)
//   bias + dropout  1 launch    the channel's at most 20 coefficients from Philox4x32-10 into LDS, then a thread per voxel: the 20
//                               monomials once, a polynomial and an exp per channel; a dropped channel is stored as 0.0f
// No atomics and no host sync: two runs give the same bits.
#include "n3d_common.h"

namespace n3d {

constexpr int AR_B = N3D_APPEAR_MAX_BATCH;
constexpr int AR_P = N3D_APPEAR_MAX_PATCH;
constexpr int AR_CHUNK = 1024;     // voxels per workgroup: 256 threads x 4
constexpr int AR_TERMS = 20;       // the terms of an order-3 field

// the launch-argument blocks (a stage's parameters travel by value in its kernel's arguments); chan / drop: bit 4 b + c
struct ArLow { uint16_t n[AR_B][4]; uint64_t chan; };
struct ArBias { double range[AR_B][4]; uint32_t k0[AR_B], k1[AR_B]; uint8_t order[AR_B][4]; uint32_t active; uint64_t drop; };

// a workgroup's voxels: chunk * 1024 + t + 256 i, i = 0 .. 3
#define AR_EACH_VOXEL(v, i) _Pragma("unroll") for (int i = 0; i < 4; ++i) for (uint32_t v = blockIdx.x * AR_CHUNK + threadIdx.x + 256 * i; v < P3; v = P3)

// ---- low resolution.  One axis of one channel at output index o: the two low-resolution samples around it as the indices of the
// voxels they were taken from, and the weight of the second
struct alignas(16) ArTap { double l1; int32_t a0, a1; };      // one 16-byte LDS read

__device__ __forceinline__ int nearest_exact(int i, int n, int P) {
  const int a = ((2 * i + 1) * P) / (2 * n);
  return a < P - 1 ? a : P - 1;
}

// grid (chunks of a patch, B).  The table is the same for the three axes (cubic patches): 4 channels x P entries.  The taps of a
// channel differ from the next one's (n[c] does), so they are 4-byte loads whatever the pitch; all eight of a channel are issued
// before the first is used.  Only what the landing launch reads is computed: a voxel none of whose active channels is masked is
// skipped whole (outside the brain that is every channel at once), a channel outside the mask inside its voxel.  out: [B][P^3][4]
// fp32, 16-byte stores.
__global__ __launch_bounds__(256) void artefact_lowres_kernel(const float* __restrict__ x, int64_t ld, int Cv, int P, FastDiv fP, FastDiv fPP, uint32_t P3,
                                                              const uint8_t* __restrict__ mask, float* __restrict__ out, const ArLow a) {
  __shared__ ArTap tab[4][AR_P];
  const int b = blockIdx.y;
  const int chan = (int)(a.chan >> (4 * b)) & 15;
  if (!chan) return;
  const int o = threadIdx.x;
  if (o < P) {
    N3D_EACH_CHANNEL(c, Cv) {
      if ((chan >> c) & 1) {
        const int n = a.n[b][c];
        double src = fma((double)n / (double)P, (double)o + 0.5, -0.5);      // fused whatever the contraction flag says: the rule's one fma
        src = src > 0.0 ? src : 0.0;
        int i0 = (int)src;
        i0 = i0 < n - 1 ? i0 : n - 1;
        const int i1 = i0 + (i0 < n - 1);
        ArTap t;
        t.l1 = src - (double)i0;
        t.a0 = nearest_exact(i0, n, P);
        t.a1 = nearest_exact(i1, n, P);
        tab[c][o] = t;
      }
    }
  }
  __syncthreads();
  const float* xb = x + (int64_t)b * P3 * ld;
  AR_EACH_VOXEL(v, it) {
    const int m = mask[(int64_t)b * P3 + v] & chan;
    if (!m) continue;
    uint32_t i, r, j, k;
    fPP.divmod(v, i, r);
    fP.divmod(r, j, k);
    float y[4] = {0.f, 0.f, 0.f, 0.f};
    N3D_EACH_CHANNEL(c, Cv) {
      if ((m >> c) & 1) {
        const ArTap ti = tab[c][i], tj = tab[c][j], tk = tab[c][k];
        const int ai[2] = {ti.a0, ti.a1}, aj[2] = {tj.a0, tj.a1}, ak[2] = {tk.a0, tk.a1};
        const double li[2] = {1.0 - ti.l1, ti.l1}, lj[2] = {1.0 - tj.l1, tj.l1}, lk[2] = {1.0 - tk.l1, tk.l1};
        float f[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] = xb[(int64_t)((ai[q >> 2] * P + aj[(q >> 1) & 1]) * P + ak[q & 1]) * ld + c];
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) acc = acc + ((li[q >> 2] * lj[(q >> 1) & 1]) * lk[q & 1]) * (double)f[q];
        y[c] = (float)acc;
      }
    }
    st4(out + ((int64_t)b * P3 + v) * 4, make_float4(y[0], y[1], y[2], y[3]));
  }
}

template <bool V4>
__global__ __launch_bounds__(256) void artefact_land_kernel(float* __restrict__ x, int64_t ld, int Cv, uint32_t P3, const uint8_t* __restrict__ mask,
                                                            const float* __restrict__ src, uint64_t chan) {
  const int b = blockIdx.y;
  const int act = (int)(chan >> (4 * b)) & 15;
  if (!act) return;
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= P3) return;
  const int m = mask[(int64_t)b * P3 + v] & act;
  if (!m) return;
  float* p = x + ((int64_t)b * P3 + v) * ld;
  float f[4];
  ld_vox<V4>(p, Cv, f);
  const float4 q = ld4(src + ((int64_t)b * P3 + v) * 4);
  const float y[4] = {q.x, q.y, q.z, q.w};
  N3D_EACH_CHANNEL(c, Cv) {
    if ((m >> c) & 1) f[c] = y[c];
  }
  st_vox<V4>(p, Cv, m, f);
}

// ---- bias field and dropout.  The terms (pa, pb, pc) of an order-3 field in the rule's nesting are slots 0 .. 19; a field of a
// lower order has the slots of degree <= order, in the same sequence, and a term's index t (its Philox counter) is its rank among
// them.  A slot outside the channel's order holds the coefficient 0.0: adding 0.0 * monomial leaves the sum's bits alone (the sum
// starts at +0.0 and so is never -0.0), which makes the per-voxel loop the same straight line for every order.
#define AR_EACH_TERM(s, pa, pb, pc)                                        \
  _Pragma("unroll") for (int pa = 0, s = 0; pa <= 3; ++pa)                 \
  _Pragma("unroll") for (int pb = 0; pb <= 3 - pa; ++pb)                   \
  _Pragma("unroll") for (int pc = 0; pc <= 3 - pa - pb; ++pc, ++s)

template <bool V4>
__global__ __launch_bounds__(256) void artefact_bias_kernel(float* __restrict__ x, int64_t ld, int Cv, int P, FastDiv fP, FastDiv fPP, uint32_t P3,
                                                            const uint8_t* __restrict__ mask, const ArBias a) {
  __shared__ double coef[4][AR_TERMS];
  const int b = blockIdx.y;
  const int drop = (int)(a.drop >> (4 * b)) & 15;
  const bool bias = (a.active >> b) & 1;
  if (!bias && !drop) return;
  if (bias) {
    const int t = threadIdx.x;
    if (t < AR_TERMS) {
      N3D_EACH_CHANNEL(c, Cv) {
        const int ord = a.order[b][c];
        int rank = 0, deg = 0;
        AR_EACH_TERM(s, pa, pb, pc) {
          rank += (s < t && pa + pb + pc <= ord);
          deg = s == t ? pa + pb + pc : deg;
        }
        double cf = 0.0;
        if (deg <= ord) {
          uint32_t w[4];
          philox4x32_10((uint32_t)rank, 3, (uint32_t)c, 0, a.k0[b], a.k1[b], w);
          cf = ((double)w[0] * 0x1p-32 * 2.0 - 1.0) * a.range[b][c];
        }
        coef[c][t] = cf;
      }
    }
    __syncthreads();
  }
  const double inv = (double)(P - 1);
  AR_EACH_VOXEL(v, it) {
    const int m = bias ? mask[(int64_t)b * P3 + v] : 0;
    const int wm = m | drop;
    if (!wm) continue;
    float* p = x + ((int64_t)b * P3 + v) * ld;
    float f[4];
    ld_vox<V4>(p, Cv, f);
    if (m) {
      uint32_t i, r, j, k;
      fPP.divmod(v, i, r);
      fP.divmod(r, j, k);
      double X[4], Y[4], Z[4];
      X[0] = Y[0] = Z[0] = 1.0;
      const double x1 = (double)(2 * (int)i - P + 1) / inv, y1 = (double)(2 * (int)j - P + 1) / inv, z1 = (double)(2 * (int)k - P + 1) / inv;
#pragma unroll
      for (int e = 1; e < 4; ++e) {
        X[e] = X[e - 1] * x1;
        Y[e] = Y[e - 1] * y1;
        Z[e] = Z[e - 1] * z1;
      }
      double poly[4] = {0.0, 0.0, 0.0, 0.0};
      AR_EACH_TERM(s, pa, pb, pc) {
        const double mono = (X[pa] * Y[pb]) * Z[pc];
        N3D_EACH_CHANNEL(c, Cv) poly[c] = poly[c] + coef[c][s] * mono;
      }
      N3D_EACH_CHANNEL(c, Cv) {
        if ((m >> c) & 1) f[c] = (float)((double)f[c] * exp(poly[c]));
      }
    }
    N3D_EACH_CHANNEL(c, Cv) {
      if ((drop >> c) & 1) f[c] = 0.f;
    }
    st_vox<V4>(p, Cv, wm, f);
  }
}

// scratch: the mask (a byte per voxel, bit c = channel c) and the low-resolution stage's output (fp32, [B][P^3][4])
struct ArLayout { size_t mask, low, total; };
static ArLayout ar_layout(int B, int P) {
  ArLayout l;
  const size_t P3 = (size_t)P * P * P;
  auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
  l.mask = 0;
  l.low = up((size_t)B * P3);
  l.total = l.low + up((size_t)B * P3 * 16);
  return l;
}

static inline bool fin(double v) { return v - v == 0.0; }

}  // namespace n3d

using namespace n3d;

extern "C" size_t n3d_patch_artefact_scratch(int B, int Cv, int P) {
  if (B < 1 || B > AR_B || Cv < 1 || Cv > 4 || P < 2 || P > AR_P) return 0;
  return ar_layout(B, P).total;
}

extern "C" int n3d_patch_artefact(void* x, int64_t ld, int B, int Cv, int P, const int32_t* stages, const int32_t* n, const int32_t* order,
                                  const double* range, const uint32_t* key, const int32_t* drop, void* scratch, size_t scratch_bytes, void* stream) {
  N3D_CHECK_ARG(x && stages, "patch_artefact: null batch or stage table");
  N3D_CHECK_ARG(B >= 1 && B <= AR_B, "patch_artefact: 1 <= B <= %d (N3D_APPEAR_MAX_BATCH), got %d", AR_B, B);
  N3D_CHECK_ARG(Cv >= 1 && Cv <= 4, "patch_artefact: 1 <= Cv <= 4, got %d", Cv);
  N3D_CHECK_ARG(P >= 2 && P <= AR_P && ld >= Cv, "patch_artefact: 2 <= P <= %d and ld >= Cv (P %d, ld %lld)", AR_P, P, (long long)ld);
  ArLow al;
  ArBias ab;
  memset(&al, 0, sizeof al);
  memset(&ab, 0, sizeof ab);
  for (int b = 0; b < B; ++b) {
    const int32_t* st = stages + 3 * b;
    if (st[0]) {
      N3D_CHECK_ARG(n, "patch_artefact: patch %d asks for low resolution and n is null", b);
      for (int c = 0; c < Cv; ++c) {
        const int nc = n[4 * b + c];
        N3D_CHECK_ARG(nc >= 1 && nc <= P, "patch_artefact: patch %d channel %d: low-resolution extent n = %d outside 1 .. P = %d", b, c, nc, P);
        al.n[b][c] = (uint16_t)nc;
        if (nc < P) al.chan |= (uint64_t)1 << (4 * b + c);      // n == P: the channel is untouched
      }
    }
    if (st[1]) {
      N3D_CHECK_ARG(order && range && key, "patch_artefact: patch %d asks for a bias field and order, range or key is null", b);
      ab.active |= 1u << b;
      ab.k0[b] = key[2 * b];
      ab.k1[b] = key[2 * b + 1];
      for (int c = 0; c < Cv; ++c) {
        const int oc = order[4 * b + c];
        const double rc = range[4 * b + c];
        N3D_CHECK_ARG(oc >= 0 && oc <= N3D_ARTEFACT_MAX_ORDER, "patch_artefact: patch %d channel %d: bias order %d outside 0 .. %d (N3D_ARTEFACT_MAX_ORDER)", b,
                      c, oc, N3D_ARTEFACT_MAX_ORDER);
        N3D_CHECK_ARG(fin(rc) && rc >= 0, "patch_artefact: patch %d channel %d: the bias range must be finite and non-negative", b, c);
        ab.order[b][c] = (uint8_t)oc;
        ab.range[b][c] = rc;
      }
    }
    if (st[2]) {
      N3D_CHECK_ARG(drop, "patch_artefact: patch %d asks for dropout and drop is null", b);
      for (int c = 0; c < Cv; ++c) {
        if (drop[4 * b + c]) ab.drop |= (uint64_t)1 << (4 * b + c);
      }
    }
  }
  if (!(al.chan | ab.active | ab.drop)) return N3D_OK;      // nothing to do: no launch, the scratch is not looked at
  const ArLayout L = ar_layout(B, P);
  N3D_CHECK_ARG(scratch && scratch_bytes >= L.total, "patch_artefact: scratch of %zu bytes, n3d_patch_artefact_scratch asks for %zu",
                scratch ? scratch_bytes : (size_t)0, L.total);
  N3D_CHECK_ARG(aligned16(scratch), "patch_artefact: scratch must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  float* xf = (float*)x;
  uint8_t* mask = (uint8_t*)scratch + L.mask;
  float* low = (float*)((char*)scratch + L.low);
  const uint32_t P3 = (uint32_t)P * P * P, nvox = (uint32_t)B * P3;
  const FastDiv fP((uint32_t)P), fPP((uint32_t)(P * P));
  const bool v4 = Cv == 4 && ld % 4 == 0 && aligned16(x);
#define AR_LAUNCH_V(kernel_, ...)                     \
  do {                                                \
    if (v4) N3D_LAUNCH(kernel_<true>, __VA_ARGS__);   \
    else N3D_LAUNCH(kernel_<false>, __VA_ARGS__);     \
  } while (0)
  const dim3 gv((unsigned)cdiv(P3, 256), (unsigned)B), gc((unsigned)cdiv(P3, AR_CHUNK), (unsigned)B);
  if (int rc = launch_brain_mask(xf, ld, Cv, nvox, mask, s)) return rc;      // appearance.hip
  if (al.chan) {
    N3D_LAUNCH(artefact_lowres_kernel, gc, dim3(256), 0, s, xf, ld, Cv, P, fP, fPP, P3, mask, low, al);
    N3D_LAUNCH_CHECK();
    AR_LAUNCH_V(artefact_land_kernel, gv, dim3(256), 0, s, xf, ld, Cv, P3, mask, low, al.chan);
    N3D_LAUNCH_CHECK();
  }
  if (ab.active | ab.drop) {
    AR_LAUNCH_V(artefact_bias_kernel, gc, dim3(256), 0, s, xf, ld, Cv, P, fP, fPP, P3, mask, ab);
    N3D_LAUNCH_CHECK();
  }
#undef AR_LAUNCH_V
  return N3D_OK;
}
