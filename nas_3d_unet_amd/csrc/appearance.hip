// Appearance augmentation of a gathered batch, in place (appearance.Appearance, Generator(augment_appearance=...)):
// n3d_patch_appearance -- Gaussian noise, Gaussian blur, contrast and gamma with retained statistics on the brain voxels of a
// pitched NDHWC batch.  include/n3d.h states the rule operation by operation; every fp64 product, sum and quotient below is one
// separately rounded operation in the association written there, so this file is compiled with contraction off (Makefile).
// Shape: one mask launch, then per stage that some patch of the batch asks for
//   noise      1 launch   a thread per voxel: Philox4x32-10 on the voxel's index, Box-Muller, all channels of the voxel
//   blur       2 launches a workgroup per 8^3 tile of one (patch, channel): the tile and its r-wide halo in LDS, three axis passes
//                         in fp64, the rounded result to scratch; then the masked voxels land back in x
//   contrast   2 launches partial statistics per 1024-voxel chunk to scratch; the apply launch sums them in index order
//   gamma      4 launches the same statistics; squared deviations + x' + its sums; its squared deviations; the apply launch
// No floating-point atomics and no host sync: a consumer launch re-sums the chunk partials of its patch in every workgroup, in
// the same fixed order (gather_partials, block_reduce below), so two runs give the same bits.
#include "n3d_common.h"

namespace n3d {

constexpr int AP_B = N3D_APPEAR_MAX_BATCH;
constexpr int AP_R = N3D_APPEAR_MAX_RADIUS;
constexpr int AP_CHUNK = 1024;     // voxels per workgroup of the statistics / apply launches: 256 threads x 4
constexpr int AP_TILE = 8;         // blur: output tile edge

// the launch-argument blocks (a stage's parameters travel by value in its kernels' arguments)
struct ApNoise { double sigma[AP_B]; uint32_t k0[AP_B], k1[AP_B]; uint32_t active; };
struct ApBlur {
  double w[AP_B][4][AP_R + 1];     // w[|k|]: the kernel is symmetric
  uint8_t r[AP_B][4];
  uint32_t active;
};
struct ApChan { double p[AP_B][4]; uint32_t active; };
// chunk partials in scratch, each [B][nchunk][4]
struct ApPart { double *S, *Q, *S2, *Q2; float *lo, *hi; int32_t* n; };

// a voxel's channels: ld_vox / st_vox (n3d_common.h)
template <bool V4>
__global__ __launch_bounds__(256) void appear_mask_kernel(const float* __restrict__ x, int64_t ld, int Cv, uint32_t nvox, uint8_t* __restrict__ mask) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nvox) return;
  float f[4];
  ld_vox<V4>(x + (int64_t)v * ld, Cv, f);
  int m = 0;
  N3D_EACH_CHANNEL(c, Cv) m |= nonzero_f32(f[c]) << c;
  mask[v] = (uint8_t)m;
}

int launch_brain_mask(const float* x, int64_t ld, int Cv, uint32_t nvox, uint8_t* mask, hipStream_t s) {
  if (Cv == 4 && ld % 4 == 0 && aligned16(x)) N3D_LAUNCH(appear_mask_kernel<true>, dim3((unsigned)cdiv(nvox, 256)), dim3(256), 0, s, x, ld, Cv, nvox, mask);
  else N3D_LAUNCH(appear_mask_kernel<false>, dim3((unsigned)cdiv(nvox, 256)), dim3(256), 0, s, x, ld, Cv, nvox, mask);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

// ---- noise (philox4x32_10: n3d_common.h)
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, double& za, double& zb) {
  const double u1 = ((double)wa + 1.0) * 0x1p-32, u2 = (double)wb * 0x1p-32;
  const double rho = sqrt(-2.0 * log(u1)), th = 6.283185307179586 * u2;
  za = rho * cos(th);
  zb = rho * sin(th);
}

template <bool V4>
__global__ __launch_bounds__(256) void appear_noise_kernel(float* __restrict__ x, int64_t ld, int Cv, uint32_t P3, const uint8_t* __restrict__ mask,
                                                           const ApNoise a) {
  const int b = blockIdx.y;
  if (!((a.active >> b) & 1)) return;
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= P3) return;
  const int m = mask[(int64_t)b * P3 + v];
  if (!m) return;
  uint32_t w[4];
  philox4x32_10(v, 0, 0, 0, a.k0[b], a.k1[b], w);
  double z[4] = {0, 0, 0, 0};
  box_muller(w[0], w[1], z[0], z[1]);
  if (Cv > 2) box_muller(w[2], w[3], z[2], z[3]);
  float* p = x + ((int64_t)b * P3 + v) * ld;
  const double s = a.sigma[b];
  float f[4];
  ld_vox<V4>(p, Cv, f);
  N3D_EACH_CHANNEL(c, Cv) {
    if ((m >> c) & 1) f[c] = (float)((double)f[c] + s * z[c]);
  }
  st_vox<V4>(p, Cv, m, f);
}

// ---- blur
__device__ __forceinline__ int reflect_clamp(int i, int P) {
  i = i < 0 ? -i - 1 : (i >= P ? 2 * P - 1 - i : i);      // scipy's "reflect": (d c b a | a b c d | d c b a); r <= P: once is enough
  return i < 0 ? 0 : (i >= P ? P - 1 : i);                 // only positions that no voxel inside the patch reads get clamped
}

// A tile of one (patch, channel) at radius R.  LDS: regA = the tile with its halo as fp32, E^3 (later the second pass' output, 64 E
// fp64); regB = the first pass' output, 8 E^2 fp64.  The halo positions hold the reflected voxels, so every pass is a plain window
// sum.  R is a template argument: with a run-time radius every tap is a dependent round trip (a scalar load of its weight, an LDS
// read, the add); unrolled, a thread's 2 R + 1 reads are in flight together and the weights sit in registers.
template <int R>
__device__ __forceinline__ void blur_tile(const float* __restrict__ xb, int64_t ld, int P, int o0, int o1, int o2, const double* __restrict__ wk,
                                          double* lds, uint32_t regA_bytes, float* __restrict__ ob) {
  constexpr int E = AP_TILE + 2 * R, EE = E * E, NIN = EE * E;
  float* in = reinterpret_cast<float*>(lds);
  double* p1 = lds;
  double* p0 = lds + regA_bytes / 8;
  const int t = threadIdx.x;
  double w[R + 1];
#pragma unroll
  for (int k = 0; k <= R; ++k) w[k] = wk[k];
  for (int base = t; base < NIN; base += 256 * 4) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = base + 256 * u < NIN ? base + 256 * u : 0;
      const int i0 = i / EE, i1 = (i - i0 * EE) / E, i2 = i - i0 * EE - i1 * E;
      const int g0 = reflect_clamp(o0 - R + i0, P), g1 = reflect_clamp(o1 - R + i1, P), g2 = reflect_clamp(o2 - R + i2, P);
      v[u] = xb[(((int64_t)g0 * P + g1) * P + g2) * ld];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (base + 256 * u < NIN) in[base + 256 * u] = v[u];
    }
  }
  __syncthreads();
  // axis 0: p0[o][i1][i2], o < 8; taps k = -R .. R in that order
  for (int i = t; i < AP_TILE * EE; i += 256) {
    const float* s = in + i;
    double acc = w[R] * (double)s[0];
#pragma unroll
    for (int k = -R + 1; k <= R; ++k) acc = acc + w[k < 0 ? -k : k] * (double)s[(k + R) * EE];
    p0[i] = acc;
  }
  __syncthreads();
  // axis 1: p1[o][p][i2], o, p < 8 (regA is free from here on)
  for (int i = t; i < AP_TILE * AP_TILE * E; i += 256) {
    const int op = i / E, i2 = i - op * E;
    const double* s = p0 + (op >> 3) * EE + (op & 7) * E + i2;
    double acc = w[R] * s[0];
#pragma unroll
    for (int k = -R + 1; k <= R; ++k) acc = acc + w[k < 0 ? -k : k] * s[(k + R) * E];
    p1[i] = acc;
  }
  __syncthreads();
  // axis 2: the tile's 512 voxels, two per thread
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = t + 256 * h, op = i >> 3, q = i & 7;
    const double* s = p1 + op * E + q;
    double acc = w[R] * s[0];
#pragma unroll
    for (int k = -R + 1; k <= R; ++k) acc = acc + w[k < 0 ? -k : k] * s[k + R];
    const int g0 = o0 + (op >> 3), g1 = o1 + (op & 7), g2 = o2 + q;
    if (g0 < P && g1 < P && g2 < P) ob[((int64_t)g0 * P + g1) * P + g2] = (float)acc;
  }
}

// grid (tiles of one channel, B * Cv); the radius is uniform over the workgroup
__global__ __launch_bounds__(256) void appear_blur_kernel(const float* __restrict__ x, int64_t ld, int Cv, int P, int nt, FastDiv fnt, FastDiv fntnt,
                                                          uint32_t regA_bytes, float* __restrict__ out, const ApBlur a) {
  extern __shared__ double ap_lds[];
  const int b = blockIdx.y / Cv, c = blockIdx.y - b * Cv;
  if (!((a.active >> b) & 1)) return;
  uint32_t t0, t1, t2, rem;
  fntnt.divmod(blockIdx.x, t0, rem);
  fnt.divmod(rem, t1, t2);
  const int o0 = (int)t0 * AP_TILE, o1 = (int)t1 * AP_TILE, o2 = (int)t2 * AP_TILE;
  const int64_t P3 = (int64_t)P * P * P;
  const float* xb = x + (int64_t)b * P3 * ld + c;
  float* ob = out + ((int64_t)b * Cv + c) * P3;
  const double* w = a.w[b][c];
  switch (a.r[b][c]) {
#define AP_BLUR_CASE(R_) case R_: blur_tile<R_>(xb, ld, P, o0, o1, o2, w, ap_lds, regA_bytes, ob); break;
    AP_BLUR_CASE(0) AP_BLUR_CASE(1) AP_BLUR_CASE(2) AP_BLUR_CASE(3) AP_BLUR_CASE(4) AP_BLUR_CASE(5) AP_BLUR_CASE(6)
#undef AP_BLUR_CASE
    default: break;
  }
}

template <bool V4>
__global__ __launch_bounds__(256) void appear_land_kernel(float* __restrict__ x, int64_t ld, int Cv, uint32_t P3, const uint8_t* __restrict__ mask,
                                                          const float* __restrict__ src, uint32_t active) {
  const int b = blockIdx.y;
  if (!((active >> b) & 1)) return;
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= P3) return;
  const int m = mask[(int64_t)b * P3 + v];
  if (!m) return;
  float* p = x + ((int64_t)b * P3 + v) * ld;
  float f[4];
  ld_vox<V4>(p, Cv, f);
  N3D_EACH_CHANNEL(c, Cv) {
    if ((m >> c) & 1) f[c] = src[((int64_t)b * Cv + c) * P3 + v];
  }
  st_vox<V4>(p, Cv, m, f);
}

// ---- fixed-order reductions.  block_reduce: thread t's four values v[c] over the 256 threads by folding halves -- a[t] = a[t] (op)
// a[t + s] for s = 128, 64, .., 1 -- the result in every thread.  For the sums this IS the stated order (include/n3d.h).
struct OpAdd { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct OpMin { __device__ __forceinline__ float operator()(float a, float b) const { return b < a ? b : a; } };
struct OpMax { __device__ __forceinline__ float operator()(float a, float b) const { return b > a ? b : a; } };

template <typename T, typename Op>
__device__ __forceinline__ void block_reduce(T (&v)[4], double* lds, Op op) {
  T* a = reinterpret_cast<T*>(lds);
  const int t = threadIdx.x;
  __syncthreads();                                 // the buffer may still be read by the reduction before this one
#pragma unroll
  for (int c = 0; c < 4; ++c) a[c * 256 + t] = v[c];
  __syncthreads();
  if (t < 128) {
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c * 256 + t] = op(a[c * 256 + t], a[c * 256 + t + 128]);
  }
  __syncthreads();
  if (t < 64) {                                    // the first wave: s = 64 from LDS, s = 32 .. 1 across its lanes (lane t + s is below 2 s)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      T x = op(a[c * 256 + t], a[c * 256 + t + 64]);
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) x = op(x, __shfl_down(x, s, 64));
      if (t == 0) a[c * 256] = x;
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = a[c * 256];
}

// the chunk partials p[b][0 .. nchunk)[c] of a patch: thread t adds those of index t, t + 256, .. in that order (from init); the fold
// is block_reduce on the result.  A kernel gathers all the quantities it needs first and reduces them afterwards, so the loads of
// one do not wait behind the barriers of another.
template <typename T, typename Op>
__device__ __forceinline__ void gather_partials(const T* __restrict__ p, int b, int nchunk, T init, T (&v)[4], Op op) {
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = init;
  for (int i = threadIdx.x; i < nchunk; i += 256) {
    const T* q = p + ((int64_t)b * nchunk + i) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = op(v[c], q[c]);
  }
}

template <typename T>
__device__ __forceinline__ void store_partial(T* __restrict__ p, int b, int nchunk, const T (&v)[4]) {
  if (threadIdx.x == 0) {
    T* q = p + ((int64_t)b * nchunk + blockIdx.x) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = v[c];
  }
}

#define AP_INF __builtin_inff()
// a workgroup's voxels: chunk * 1024 + t + 256 i, i = 0 .. 3
#define AP_EACH_VOXEL(v, i) _Pragma("unroll") for (int i = 0; i < 4; ++i) for (uint32_t v = blockIdx.x * AP_CHUNK + threadIdx.x + 256 * i; v < P3; v = P3)

// n, lo, hi, S of the masked voxels per chunk (contrast and gamma)
template <bool V4>
__global__ __launch_bounds__(256) void appear_stats_kernel(const float* __restrict__ x, int64_t ld, int Cv, uint32_t P3, const uint8_t* __restrict__ mask,
                                                           uint32_t active, ApPart part) {
  __shared__ double lds[4 * 256];
  const int b = blockIdx.y, nchunk = gridDim.x;
  if (!((active >> b) & 1)) return;
  double S[4] = {0, 0, 0, 0};
  float lo[4] = {AP_INF, AP_INF, AP_INF, AP_INF}, hi[4] = {-AP_INF, -AP_INF, -AP_INF, -AP_INF};
  int n[4] = {0, 0, 0, 0};
  AP_EACH_VOXEL(v, i) {
    const int m = mask[(int64_t)b * P3 + v];
    float fv[4];
    ld_vox<V4>(x + ((int64_t)b * P3 + v) * ld, Cv, fv);
    N3D_EACH_CHANNEL(c, Cv) {
      const bool on = (m >> c) & 1;
      const float f = fv[c];
      S[c] = S[c] + (on ? (double)f : 0.0);
      if (on) {
        lo[c] = f < lo[c] ? f : lo[c];
        hi[c] = f > hi[c] ? f : hi[c];
        n[c] += 1;
      }
    }
  }
  block_reduce(S, lds, OpAdd());
  block_reduce(lo, lds, OpMin());
  block_reduce(hi, lds, OpMax());
  block_reduce(n, lds, OpAdd());
  store_partial(part.S, b, nchunk, S);
  store_partial(part.lo, b, nchunk, lo);
  store_partial(part.hi, b, nchunk, hi);
  store_partial(part.n, b, nchunk, n);
}

struct ApStats { int n[4]; float lo[4], hi[4]; double m[4]; };
__device__ __forceinline__ void load_stats(const ApPart& part, int b, int nchunk, double* lds, ApStats& s) {
  double S[4];
  gather_partials(part.S, b, nchunk, 0.0, S, OpAdd());
  gather_partials(part.lo, b, nchunk, AP_INF, s.lo, OpMin());
  gather_partials(part.hi, b, nchunk, -AP_INF, s.hi, OpMax());
  gather_partials(part.n, b, nchunk, 0, s.n, OpAdd());
  block_reduce(S, lds, OpAdd());
  block_reduce(s.lo, lds, OpMin());
  block_reduce(s.hi, lds, OpMax());
  block_reduce(s.n, lds, OpAdd());
#pragma unroll
  for (int c = 0; c < 4; ++c) s.m[c] = s.n[c] > 0 ? S[c] / (double)s.n[c] : 0.0;
}

template <bool V4>
__global__ __launch_bounds__(256) void appear_contrast_kernel(float* __restrict__ x, int64_t ld, int Cv, uint32_t P3, const uint8_t* __restrict__ mask,
                                                              ApPart part, const ApChan a) {
  __shared__ double lds[4 * 256];
  const int b = blockIdx.y, nchunk = gridDim.x;
  if (!((a.active >> b) & 1)) return;
  ApStats s;
  load_stats(part, b, nchunk, lds, s);
  AP_EACH_VOXEL(v, i) {
    const int m = mask[(int64_t)b * P3 + v];
    float* p = x + ((int64_t)b * P3 + v) * ld;
    float f[4];
    ld_vox<V4>(p, Cv, f);
    N3D_EACH_CHANNEL(c, Cv) {
      if (((m >> c) & 1) && s.n[c] > 0) {
        const double y = ((double)f[c] - s.m[c]) * a.p[b][c] + s.m[c];
        f[c] = (float)fmin(fmax(y, (double)s.lo[c]), (double)s.hi[c]);
      }
    }
    st_vox<V4>(p, Cv, m, f);
  }
}

// gamma, second launch: Q = sum (x - m)^2, then x' in place and S2 = sum x'
template <bool V4>
__global__ __launch_bounds__(256) void appear_gamma_pow_kernel(float* __restrict__ x, int64_t ld, int Cv, uint32_t P3, const uint8_t* __restrict__ mask,
                                                               ApPart part, const ApChan a) {
  __shared__ double lds[4 * 256];
  const int b = blockIdx.y, nchunk = gridDim.x;
  if (!((a.active >> b) & 1)) return;
  ApStats s;
  load_stats(part, b, nchunk, lds, s);
  double Q[4] = {0, 0, 0, 0}, S2[4] = {0, 0, 0, 0};
  AP_EACH_VOXEL(v, i) {
    const int m = mask[(int64_t)b * P3 + v];
    float* p = x + ((int64_t)b * P3 + v) * ld;
    float f[4];
    ld_vox<V4>(p, Cv, f);
    N3D_EACH_CHANNEL(c, Cv) {
      const bool on = ((m >> c) & 1) && s.n[c] > 0;
      double q = 0.0, s2 = 0.0;
      if (on) {
        const double xv = (double)f[c], lo = (double)s.lo[c], range = (double)s.hi[c] - lo;
        const double d = xv - s.m[c];
        q = d * d;
        const float y = (float)(pow((xv - lo) / (range + 1e-7), a.p[b][c]) * range + lo);
        f[c] = y;
        s2 = (double)y;
      }
      Q[c] = Q[c] + q;
      S2[c] = S2[c] + s2;
    }
    st_vox<V4>(p, Cv, m, f);
  }
  block_reduce(Q, lds, OpAdd());
  block_reduce(S2, lds, OpAdd());
  store_partial(part.Q, b, nchunk, Q);
  store_partial(part.S2, b, nchunk, S2);
}

// gamma, third launch: Q2 = sum (x' - m')^2
template <bool V4>
__global__ __launch_bounds__(256) void appear_gamma_dev_kernel(const float* __restrict__ x, int64_t ld, int Cv, uint32_t P3,
                                                               const uint8_t* __restrict__ mask, uint32_t active, ApPart part) {
  __shared__ double lds[4 * 256];
  const int b = blockIdx.y, nchunk = gridDim.x;
  if (!((active >> b) & 1)) return;
  int n[4];
  double S2[4], Q2[4] = {0, 0, 0, 0};
  gather_partials(part.n, b, nchunk, 0, n, OpAdd());
  gather_partials(part.S2, b, nchunk, 0.0, S2, OpAdd());
  block_reduce(n, lds, OpAdd());
  block_reduce(S2, lds, OpAdd());
  AP_EACH_VOXEL(v, i) {
    const int m = mask[(int64_t)b * P3 + v];
    float f[4];
    ld_vox<V4>(x + ((int64_t)b * P3 + v) * ld, Cv, f);
    N3D_EACH_CHANNEL(c, Cv) {
      double q = 0.0;
      if (((m >> c) & 1) && n[c] > 0) {
        const double d = (double)f[c] - S2[c] / (double)n[c];
        q = d * d;
      }
      Q2[c] = Q2[c] + q;
    }
  }
  block_reduce(Q2, lds, OpAdd());
  store_partial(part.Q2, b, nchunk, Q2);
}

// gamma, fourth launch: back to the mean and deviation the channel had
template <bool V4>
__global__ __launch_bounds__(256) void appear_gamma_apply_kernel(float* __restrict__ x, int64_t ld, int Cv, uint32_t P3, const uint8_t* __restrict__ mask,
                                                                 uint32_t active, ApPart part) {
  __shared__ double lds[4 * 256];
  const int b = blockIdx.y, nchunk = gridDim.x;
  if (!((active >> b) & 1)) return;
  int n[4];
  double S[4], Q[4], S2[4], Q2[4];
  gather_partials(part.n, b, nchunk, 0, n, OpAdd());
  gather_partials(part.S, b, nchunk, 0.0, S, OpAdd());
  gather_partials(part.Q, b, nchunk, 0.0, Q, OpAdd());
  gather_partials(part.S2, b, nchunk, 0.0, S2, OpAdd());
  gather_partials(part.Q2, b, nchunk, 0.0, Q2, OpAdd());
  block_reduce(n, lds, OpAdd());
  block_reduce(S, lds, OpAdd());
  block_reduce(Q, lds, OpAdd());
  block_reduce(S2, lds, OpAdd());
  block_reduce(Q2, lds, OpAdd());
  double m[4], sd[4], m2[4], sd2[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double nn = n[c] > 0 ? (double)n[c] : 1.0;
    m[c] = S[c] / nn;
    sd[c] = sqrt(Q[c] / nn);
    m2[c] = S2[c] / nn;
    sd2[c] = sqrt(Q2[c] / nn);
  }
  AP_EACH_VOXEL(v, i) {
    const int mk = mask[(int64_t)b * P3 + v];
    float* p = x + ((int64_t)b * P3 + v) * ld;
    float f[4];
    ld_vox<V4>(p, Cv, f);
    N3D_EACH_CHANNEL(c, Cv) {
      if (((mk >> c) & 1) && n[c] > 0) f[c] = (float)(((double)f[c] - m2[c]) / (sd2[c] + 1e-8) * sd[c] + m[c]);
    }
    st_vox<V4>(p, Cv, mk, f);
  }
}

// scratch: the mask (a byte per voxel, bit c = channel c), the blur's output (fp32, [B][Cv][P^3]) and the chunk partials
struct ApLayout { size_t mask, blur, part, total; int nchunk; };
static ApLayout ap_layout(int B, int Cv, int P) {
  ApLayout l;
  const size_t P3 = (size_t)P * P * P;
  l.nchunk = (int)cdiv((int64_t)P3, AP_CHUNK);
  auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
  l.mask = 0;
  l.blur = up((size_t)B * P3);
  l.part = l.blur + up((size_t)B * Cv * P3 * 4);
  l.total = l.part + up((size_t)B * l.nchunk * 4 * (4 * 8 + 3 * 4));
  return l;
}

static inline bool fin(double v) { return v - v == 0.0; }

}  // namespace n3d

using namespace n3d;

extern "C" size_t n3d_patch_appearance_scratch(int B, int Cv, int P) {
  if (B < 1 || B > AP_B || Cv < 1 || Cv > 4 || P < 1 || P > N3D_APPEAR_MAX_PATCH) return 0;
  return ap_layout(B, Cv, P).total;
}

extern "C" int n3d_patch_appearance(void* x, int64_t ld, int B, int Cv, int P, const n3d_appear_desc* descs, void* scratch, size_t scratch_bytes,
                                    void* stream) {
  N3D_CHECK_ARG(x && descs, "patch_appearance: null batch or descriptors");
  N3D_CHECK_ARG(B >= 1 && B <= AP_B, "patch_appearance: 1 <= B <= %d (N3D_APPEAR_MAX_BATCH), got %d", AP_B, B);
  N3D_CHECK_ARG(Cv >= 1 && Cv <= 4, "patch_appearance: 1 <= Cv <= 4, got %d", Cv);
  N3D_CHECK_ARG(P >= 1 && P <= N3D_APPEAR_MAX_PATCH && ld >= Cv, "patch_appearance: 1 <= P <= %d and ld >= Cv (P %d, ld %lld)", N3D_APPEAR_MAX_PATCH,
                P, (long long)ld);
  ApNoise an;
  ApBlur ab;
  ApChan ac, ag;
  memset(&an, 0, sizeof an);
  memset(&ab, 0, sizeof ab);
  memset(&ac, 0, sizeof ac);
  memset(&ag, 0, sizeof ag);
  int rmax = 0;
  for (int b = 0; b < B; ++b) {
    const n3d_appear_desc& d = descs[b];
    if (d.noise) {
      N3D_CHECK_ARG(fin(d.sigma) && d.sigma >= 0, "patch_appearance: patch %d: the noise sigma must be finite and non-negative", b);
      an.active |= 1u << b;
      an.sigma[b] = d.sigma;
      an.k0[b] = d.key[0];
      an.k1[b] = d.key[1];
    }
    if (d.blur) {
      ab.active |= 1u << b;
      for (int c = 0; c < Cv; ++c) {
        const int r = d.radius[c];
        N3D_CHECK_ARG(r >= 0 && r <= AP_R, "patch_appearance: patch %d channel %d: blur radius %d outside 0 .. %d (N3D_APPEAR_MAX_RADIUS)", b, c, r, AP_R);
        N3D_CHECK_ARG(r <= P, "patch_appearance: patch %d channel %d: blur radius %d exceeds the patch edge %d (one reflection must suffice)", b, c, r, P);
        for (int k = 0; k <= r; ++k) {
          N3D_CHECK_ARG(fin(d.weights[c][k]), "patch_appearance: patch %d channel %d: blur weights must be finite", b, c);
          ab.w[b][c][k] = d.weights[c][k];
        }
        ab.r[b][c] = (uint8_t)r;
        rmax = r > rmax ? r : rmax;
      }
    }
    if (d.contrast) {
      ac.active |= 1u << b;
      for (int c = 0; c < Cv; ++c) {
        N3D_CHECK_ARG(fin(d.factor[c]), "patch_appearance: patch %d channel %d: the contrast factor must be finite", b, c);
        ac.p[b][c] = d.factor[c];
      }
    }
    if (d.gamma) {
      ag.active |= 1u << b;
      for (int c = 0; c < Cv; ++c) {
        N3D_CHECK_ARG(fin(d.gamma_c[c]) && d.gamma_c[c] >= 0, "patch_appearance: patch %d channel %d: gamma must be finite and non-negative", b, c);
        ag.p[b][c] = d.gamma_c[c];
      }
    }
  }
  if (!(an.active | ab.active | ac.active | ag.active)) return N3D_OK;      // nothing asked for: no launch, the scratch is not looked at
  const ApLayout L = ap_layout(B, Cv, P);
  N3D_CHECK_ARG(scratch && scratch_bytes >= L.total, "patch_appearance: scratch of %zu bytes, n3d_patch_appearance_scratch asks for %zu",
                scratch ? scratch_bytes : (size_t)0, L.total);
  N3D_CHECK_ARG((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "patch_appearance: scratch must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  float* xf = (float*)x;
  char* base = (char*)scratch;
  uint8_t* mask = (uint8_t*)(base + L.mask);
  float* blur = (float*)(base + L.blur);
  const size_t each = (size_t)B * L.nchunk * 4;
  ApPart part;
  part.S = (double*)(base + L.part);
  part.Q = part.S + each;
  part.S2 = part.Q + each;
  part.Q2 = part.S2 + each;
  part.lo = (float*)(part.Q2 + each);
  part.hi = part.lo + each;
  part.n = (int32_t*)(part.hi + each);
  const uint32_t P3 = (uint32_t)P * P * P, nvox = (uint32_t)B * P3;
  const bool v4 = Cv == 4 && ld % 4 == 0 && aligned16(x);
#define AP_LAUNCH_V(kernel_, ...)                     \
  do {                                                \
    if (v4) N3D_LAUNCH(kernel_<true>, __VA_ARGS__);   \
    else N3D_LAUNCH(kernel_<false>, __VA_ARGS__);     \
  } while (0)
  const dim3 gv((unsigned)cdiv(P3, 256), (unsigned)B), gc((unsigned)L.nchunk, (unsigned)B);
  if (int rc = launch_brain_mask(xf, ld, Cv, nvox, mask, s)) return rc;
  if (an.active) {
    AP_LAUNCH_V(appear_noise_kernel, gv, dim3(256), 0, s, xf, ld, Cv, P3, mask, an);
    N3D_LAUNCH_CHECK();
  }
  if (ab.active) {
    const uint32_t E = AP_TILE + 2 * rmax;
    const uint32_t regA = E * E * E * 4 > 64 * E * 8 ? E * E * E * 4 : 64 * E * 8, regB = AP_TILE * E * E * 8;      // E is even: regA % 8 == 0
    const int nt = (int)cdiv(P, AP_TILE);
    N3D_LAUNCH(appear_blur_kernel, dim3((unsigned)(nt * nt * nt), (unsigned)(B * Cv)), dim3(256), regA + regB, s, xf, ld, Cv, P, nt, FastDiv((uint32_t)nt),
               FastDiv((uint32_t)(nt * nt)), regA, blur, ab);
    N3D_LAUNCH_CHECK();
    AP_LAUNCH_V(appear_land_kernel, gv, dim3(256), 0, s, xf, ld, Cv, P3, mask, blur, ab.active);
    N3D_LAUNCH_CHECK();
  }
  if (ac.active) {
    AP_LAUNCH_V(appear_stats_kernel, gc, dim3(256), 0, s, xf, ld, Cv, P3, mask, ac.active, part);
    N3D_LAUNCH_CHECK();
    AP_LAUNCH_V(appear_contrast_kernel, gc, dim3(256), 0, s, xf, ld, Cv, P3, mask, part, ac);
    N3D_LAUNCH_CHECK();
  }
  if (ag.active) {
    AP_LAUNCH_V(appear_stats_kernel, gc, dim3(256), 0, s, xf, ld, Cv, P3, mask, ag.active, part);
    N3D_LAUNCH_CHECK();
    AP_LAUNCH_V(appear_gamma_pow_kernel, gc, dim3(256), 0, s, xf, ld, Cv, P3, mask, part, ag);
    N3D_LAUNCH_CHECK();
    AP_LAUNCH_V(appear_gamma_dev_kernel, gc, dim3(256), 0, s, xf, ld, Cv, P3, mask, ag.active, part);
    N3D_LAUNCH_CHECK();
    AP_LAUNCH_V(appear_gamma_apply_kernel, gc, dim3(256), 0, s, xf, ld, Cv, P3, mask, ag.active, part);
    N3D_LAUNCH_CHECK();
  }
#undef AP_LAUNCH_V
  return N3D_OK;
}
