// Raw scans to normalised brain-wise boxes (preprocess.py:77-144, create_h5:58-66): the dataset statistics over the nonzero
// voxels of every modality (cal_mean_std), and per subject the outline (cal_outline), the normalisation (normalize, with its
// write-back into the int16 array: the stored value is the fp64 result truncated toward zero) and the crop to the brain box.
// Raw data is int16 (Cm, X, Y, Z).  Counts, sums, extrema and outlines are integer work (exact, order-independent, integer
// atomics); the squared deviations are summed in fp64 in a fixed order (partial rows, no floating-point atomics); the normalised
// value is a chain of single-rounded fp64 operations, so this file is compiled without contraction: the pragma below states it,
// and because -ffp-contract=fast makes the backend fuse regardless of it, the Makefile also ends this file's flags with
// -ffp-contract=off.
// Next to the reference's rule stands a second one, chosen per call (further down): an exact histogram of each modality's counts,
// the percentile bounds, mean and std read from it, and z-scoring of the clipped counts fused with the same crop.
#include <cfloat>

#include "n3d_common.h"

#pragma clang fp contract(off)

namespace n3d {

// A modality's N = X * Y * Z voxels start at raw + c * N: 16-byte aligned only when c * N is a multiple of 8.  Every pass splits
// them into `head` voxels up to the first 16-byte boundary (0..7), `groups` aligned groups of eight and a tail of 0..7.
struct Span {
  int64_t head, groups, tail0;   // tail0: index of the first tail voxel
};
__host__ __device__ static inline Span span_of(const int16_t* p, int64_t N) {
  Span s;
  s.head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 1);
  if (s.head > N) s.head = N;
  s.groups = (N - s.head) >> 3;
  s.tail0 = s.head + s.groups * 8;
  return s;
}
// blocks along x for a pass over N voxels: a function of N alone (the fixed-order sums depend on it), 8 groups per thread, <= 1024
static inline int span_blocks(int64_t N) {
  const int64_t b = cdiv(N >> 3, 256 * 8);
  return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

__device__ __forceinline__ int16_t half_of(int w, int k) { return (int16_t)(k ? (w >> 16) : (w & 0xffff)); }

struct ScanAcc {
  uint32_t cnt;
  long long sum;
  int mn, mx, lo[3], hi[3];
  __device__ __forceinline__ void init() {
    cnt = 0; sum = 0; mn = INT32_MAX; mx = INT32_MIN;
    lo[0] = lo[1] = lo[2] = INT32_MAX;
    hi[0] = hi[1] = hi[2] = -1;
  }
  __device__ __forceinline__ void add(int v, int x, int y, int z) {
    ++cnt; sum += v;
    mn = min(mn, v); mx = max(mx, v);
    lo[0] = min(lo[0], x); lo[1] = min(lo[1], y); lo[2] = min(lo[2], z);
    hi[0] = max(hi[0], x); hi[1] = max(hi[1], y); hi[2] = max(hi[2], z);
  }
  __device__ __forceinline__ void merge(const ScanAcc& o) {
    cnt += o.cnt; sum += o.sum;
    mn = min(mn, o.mn); mx = max(mx, o.mx);
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], o.lo[a]); hi[a] = max(hi[a], o.hi[a]); }
  }
};

// grid (blocks, Cm).  Sixteen-byte loads of eight voxels; a group of zeros (the background) costs the load and one test.  The
// index of a group's first voxel is decoded once (FastDiv: N < 2^31) and stepped with carries.  Wave butterfly, LDS across the four
// waves, then ten integer atomics per workgroup that saw a nonzero voxel.
__global__ __launch_bounds__(256) void brain_scan_kernel(const int16_t* __restrict__ raw, int64_t N, int Y, int Z, FastDiv fY, FastDiv fZ,
                                                         unsigned long long* __restrict__ totals, int* __restrict__ rec) {
  const int c = blockIdx.y;
  const int16_t* p = raw + (int64_t)c * N;
  const Span sp = span_of(p, N);
  ScanAcc a;
  a.init();
  auto one = [&](int64_t i) {
    const int v = p[i];
    if (v != 0) {
      uint32_t q, z, x, y;
      fZ.divmod((uint32_t)i, q, z);
      fY.divmod(q, x, y);
      a.add(v, (int)x, (int)y, (int)z);
    }
  };
  const int4* body = reinterpret_cast<const int4*>(p + sp.head);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < sp.groups; g += (int64_t)gridDim.x * 256) {
    const int4 v = body[g];
    if ((v.x | v.y | v.z | v.w) == 0) continue;
    uint32_t q, z, x, y;
    fZ.divmod((uint32_t)(sp.head + g * 8), q, z);
    fY.divmod(q, x, y);
    const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int s = half_of(w[k >> 1], k & 1);
      if (s != 0) a.add(s, (int)x, (int)y, (int)z);
      if (++z == (uint32_t)Z) {
        z = 0;
        if (++y == (uint32_t)Y) { y = 0; ++x; }
      }
    }
  }
  if (blockIdx.x == 0) {
    if ((int64_t)threadIdx.x < sp.head) one(threadIdx.x);
    else if (threadIdx.x >= 64 && sp.tail0 + (threadIdx.x - 64) < N) one(sp.tail0 + (threadIdx.x - 64));
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    ScanAcc o;
    o.cnt = __shfl_xor(a.cnt, d, 64);
    o.sum = __shfl_xor(a.sum, d, 64);
    o.mn = __shfl_xor(a.mn, d, 64);
    o.mx = __shfl_xor(a.mx, d, 64);
#pragma unroll
    for (int k = 0; k < 3; ++k) { o.lo[k] = __shfl_xor(a.lo[k], d, 64); o.hi[k] = __shfl_xor(a.hi[k], d, 64); }
    a.merge(o);
  }
  __shared__ ScanAcc part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) a.merge(part[w]);
    if (a.cnt) {
      atomicAdd(totals + 2 * c, (unsigned long long)a.cnt);
      atomicAdd(totals + 2 * c + 1, (unsigned long long)a.sum);
      int* r = rec + N3D_BRAIN_REC_WORDS * c;
      atomicMin(r + 0, a.mn);
      atomicMax(r + 1, a.mx);
#pragma unroll
      for (int k = 0; k < 3; ++k) { atomicMin(r + 2 + k, a.lo[k]); atomicMax(r + 5 + k, a.hi[k]); }
    }
  }
}

// the same butterfly for one double: commutative adds in a fixed pattern, every lane ends with the same bits
__device__ __forceinline__ double wave_sum_fixed(double s) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d, 64);
  return s;
}
__device__ __forceinline__ double block_sum_fixed(double s, double* lds) {
  s = wave_sum_fixed(s);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// grid (rows, Cm): workgroup (r, c) writes its sum of (x - mean)^2 over the nonzero voxels it walks to partial[c * rows + r].
// A thread's terms are added in index order, the lanes, waves and (brain_sqdev_final_kernel) rows in a fixed pattern: the result
// depends on N, the launch shape and the 16-byte phase of the data, not on timing.
__global__ __launch_bounds__(256) void brain_sqdev_kernel(const int16_t* __restrict__ raw, int64_t N, const double* __restrict__ mean,
                                                          double* __restrict__ partial) {
  const int c = blockIdx.y;
  const int16_t* p = raw + (int64_t)c * N;
  const Span sp = span_of(p, N);
  const double m = mean[c];
  double s = 0.0;
  auto one = [&](int v) {
    if (v != 0) {
      const double d = (double)v - m;
      s += d * d;
    }
  };
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < sp.head) one(p[threadIdx.x]);
  const int4* body = reinterpret_cast<const int4*>(p + sp.head);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < sp.groups; g += (int64_t)gridDim.x * 256) {
    const int4 v = body[g];
    if ((v.x | v.y | v.z | v.w) == 0) continue;
    const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) one(half_of(w[k >> 1], k & 1));
  }
  if (blockIdx.x == 0 && threadIdx.x >= 64 && sp.tail0 + (threadIdx.x - 64) < N) one(p[sp.tail0 + (threadIdx.x - 64)]);
  __shared__ double lds[4];
  s = block_sum_fixed(s, lds);
  if (threadIdx.x == 0) partial[(int64_t)c * gridDim.x + blockIdx.x] = s;
}

// grid (Cm): the rows of one modality in a fixed order, added to the running total (plain add: launches on one stream are
// ordered, so subjects accumulate in the order they were enqueued)
__global__ __launch_bounds__(256) void brain_sqdev_final_kernel(const double* __restrict__ partial, int rows, double* __restrict__ acc) {
  const int c = blockIdx.x;
  double s = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) s += partial[(int64_t)c * rows + r];
  __shared__ double lds[4];
  s = block_sum_fixed(s, lds);
  if (threadIdx.x == 0) acc[c] += s;
}

struct CropGeom {
  int64_t N;         // X * Y * Z
  int Y, Z;
  int lo[3], b[3];   // box [lo, lo + b)
  FastDiv fby, fbz;
};

// grid (blocks, Cm + (truth ? 1 : 0)): plane c < Cm of the output box is modality c normalised, plane Cm the label crop.
//   z = (x - mean) / std;  q = (z - zmin) / (zmax - zmin);  v = (q + 0.1) * 100;  stored: (float)(int16)v   (x != 0; else 0)
// each operation rounded once in fp64 (contraction off above; fp64 division is correctly rounded).  zmin / zmax: z of the
// subject's smallest / largest nonzero raw value of the modality (rec, written by brain_scan_kernel); z is monotone in x.
__global__ __launch_bounds__(256) void brain_normalize_kernel(const int16_t* __restrict__ raw, int Cm, CropGeom g, const double* __restrict__ mean_std,
                                                              const int* __restrict__ rec, float* __restrict__ out,
                                                              const uint8_t* __restrict__ truth, uint8_t* __restrict__ truth_out) {
  const int c = blockIdx.y;
  const int64_t nb = (int64_t)g.b[0] * g.b[1] * g.b[2];
  double mean = 0.0, sd = 1.0, zmin = 0.0, range = 1.0;
  if (c < Cm) {
    mean = mean_std[2 * c];
    sd = mean_std[2 * c + 1];
    zmin = ((double)rec[N3D_BRAIN_REC_WORDS * c] - mean) / sd;
    range = ((double)rec[N3D_BRAIN_REC_WORDS * c + 1] - mean) / sd - zmin;
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (int64_t)gridDim.x * 256) {
    uint32_t q, k, ii, j;
    g.fbz.divmod((uint32_t)i, q, k);
    g.fby.divmod(q, ii, j);
    const int64_t src = ((int64_t)(g.lo[0] + (int)ii) * g.Y + (g.lo[1] + (int)j)) * g.Z + (g.lo[2] + (int)k);
    if (c == Cm) {
      truth_out[i] = truth[src];
      continue;
    }
    const int x = raw[(int64_t)c * g.N + src];
    float r = 0.f;
    if (x != 0) {
      const double z = ((double)x - mean) / sd;
      const double qn = (z - zmin) / range;
      const double v = (qn + 0.1) * 100.0;
      r = (float)(int16_t)(int)v;
    }
    out[(int64_t)c * nb + i] = r;
  }
}

// ---- the second scheme (include/n3d.h, "n3d_brain_hist .. n3d_brain_zscore"): per subject and modality, z-scoring over the brain
// voxels after clipping to two percentiles.  Every order statistic comes from an exact histogram of the modality's counts.

constexpr int kHistBins = N3D_BRAIN_HIST_BINS;
// LDS window of brain_hist_kernel: 8192 int32 bins = 32 KiB per workgroup, five workgroups in a CU's 160 KiB (the 256-thread
// workgroups of this kernel then sit at 20 of the 32 waves a CU takes).  BraTS counts of one modality span a few thousand values
// above the minimum, so the window takes nearly every voxel; what falls outside goes to global memory one atomic each.
constexpr int kHistWindow = 8192;
constexpr int kHistMaxBlocks = 128;   // per modality: each workgroup flushes its nonzero window bins once, so few, long-running workgroups

// grid (blocks, Cm).  hist: int32 [Cm][65536], bin v + 32768, ADDED to (the entry point zeroes it).  Reads as brain_scan_kernel
// does.  A nonzero voxel v with 0 <= v - min < kHistWindow (min: rec's minimum of the modality, read here) is one LDS atomic; any
// other one global atomic, so a wrong `min` costs time and never a count.  Integer adds only: the result does not depend on order.
__global__ __launch_bounds__(256) void brain_hist_kernel(const int16_t* __restrict__ raw, int64_t N, const int* __restrict__ rec,
                                                         int* __restrict__ hist) {
  const int c = blockIdx.y;
  const int16_t* p = raw + (int64_t)c * N;
  const Span sp = span_of(p, N);
  const int mn = rec[N3D_BRAIN_REC_WORDS * c];
  int* gh = hist + (int64_t)c * kHistBins;
  __shared__ int lh[kHistWindow];
  for (int i = threadIdx.x; i < kHistWindow; i += 256) lh[i] = 0;
  __syncthreads();
  auto one = [&](int v) {
    if (v != 0) {
      const uint32_t d = (uint32_t)v - (uint32_t)mn;
      if (d < (uint32_t)kHistWindow) atomicAdd(&lh[d], 1);
      else atomicAdd(gh + (v + 32768), 1);          // v is an int16: the bin is inside [0, 65536)
    }
  };
  if (blockIdx.x == 0) {
    if ((int64_t)threadIdx.x < sp.head) one(p[threadIdx.x]);
    else if (threadIdx.x >= 64 && sp.tail0 + (threadIdx.x - 64) < N) one(p[sp.tail0 + (threadIdx.x - 64)]);
  }
  const int4* body = reinterpret_cast<const int4*>(p + sp.head);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < sp.groups; g += (int64_t)gridDim.x * 256) {
    const int4 v = body[g];
    if ((v.x | v.y | v.z | v.w) == 0) continue;
    const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) one(half_of(w[k >> 1], k & 1));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kHistWindow; i += 256) {
    const int h = lh[i];
    const int64_t b = (int64_t)mn + 32768 + i;      // a bin that was counted is inside the histogram; the test keeps a stray `min` harmless
    if (h != 0 && b >= 0 && b < kHistBins) atomicAdd(gh + b, h);
  }
}

// one record of n3d_brain_robust: N3D_BRAIN_ROBUST_WORDS 8-byte words (include/n3d.h states the layout)
struct RobustRec {
  long long count, order[4], n_below, n_above, sum_in;
  double lower, upper, mean, std, ssd;
  long long reserved[3];
};
static_assert(sizeof(RobustRec) == 8 * N3D_BRAIN_ROBUST_WORDS, "RobustRec is the record of include/n3d.h");

constexpr int kRobustThreads = 1024;
constexpr int kRobustBins = kHistBins / kRobustThreads;   // 64 consecutive bins per thread

__device__ __forceinline__ long long wave_sum_ll(long long s) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d, 64);
  return s;
}

// numpy's linear percentile from the two order statistics around the virtual index and its fraction t
__device__ __forceinline__ double lerp_bound(long long a, long long b, double t) {
  const double A = (double)a, B = (double)b;
  const double d = B - A;
  return t >= 0.5 ? B - d * (1.0 - t) : A + d * t;
}

// grid (Cm), 1024 threads: thread t owns bins [64 t, 64 t + 64).  Integer work (prefix sums, order statistics, nL, nU, S_in) is
// exact.  Sum of squared deviations: thread t adds its interior bins' h * ((v - mean) * (v - mean)) in ascending v from 0.0, the
// 1024 partial sums are added in adjacent pairs (p[2i] + p[2i + 1], ten rounds), then (low term + that) + high term.
__global__ __launch_bounds__(kRobustThreads) void brain_robust_kernel(const int* __restrict__ hist, double lower, double upper,
                                                                       RobustRec* __restrict__ out) {
  const int c = blockIdx.x, t = threadIdx.x;
  const int4* hp = reinterpret_cast<const int4*>(hist + (int64_t)c * kHistBins + t * kRobustBins);
  __shared__ uint32_t scan[kRobustThreads];
  __shared__ long long order[4];
  __shared__ long long red[3][kRobustThreads / 64];
  __shared__ double part[kRobustThreads];
  auto bins = [&](auto&& f) {      // f(v, h) over this thread's nonzero bins in ascending v
    for (int j = 0; j < kRobustBins / 4; ++j) {
      const int4 q = hp[j];
      const int h[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (h[k] != 0) f(t * kRobustBins + j * 4 + k - 32768, h[k]);
    }
  };
  uint32_t local = 0;
  bins([&](int, int h) { local += (uint32_t)h; });
  scan[t] = local;
  __syncthreads();
  for (int d = 1; d < kRobustThreads; d <<= 1) {
    const uint32_t add = t >= d ? scan[t - d] : 0u;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const long long n = scan[kRobustThreads - 1];
  RobustRec r = {};
  r.count = n;
  if (n == 0) {                    // (uniform) nothing to rank: the caller refuses count < 2
    if (t == 0) out[c] = r;
    return;
  }
  long long idx[4];
  double frac[2];
  const double qs[2] = {lower, upper};
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const double vi = (double)(n - 1) * (qs[e] / 100.0);
    const double kf = floor(vi);
    frac[e] = vi - kf;
    const long long k = (long long)kf;
    idx[2 * e] = k;
    idx[2 * e + 1] = k + 1 < n - 1 ? k + 1 : n - 1;
  }
  long long cum = (long long)scan[t] - local;
  bins([&](int v, int h) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (idx[m] >= cum && idx[m] < cum + h) order[m] = v;
    cum += h;
  });
  __syncthreads();
#pragma unroll
  for (int m = 0; m < 4; ++m) r.order[m] = order[m];
  const double L = lerp_bound(r.order[0], r.order[1], frac[0]), U = lerp_bound(r.order[2], r.order[3], frac[1]);
  long long nb = 0, na = 0, s = 0;
  bins([&](int v, int h) {
    const double dv = (double)v;
    if (dv < L) nb += h;
    else if (dv > U) na += h;
    else s += (long long)h * v;
  });
  nb = wave_sum_ll(nb);
  na = wave_sum_ll(na);
  s = wave_sum_ll(s);
  if ((t & 63) == 0) { red[0][t >> 6] = nb; red[1][t >> 6] = na; red[2][t >> 6] = s; }
  __syncthreads();
  nb = na = s = 0;
  for (int w = 0; w < kRobustThreads / 64; ++w) { nb += red[0][w]; na += red[1][w]; s += red[2][w]; }
  const double dn = (double)n;
  const double mean = (((double)nb * L + (double)s) + (double)na * U) / dn;
  double acc = 0.0;
  bins([&](int v, int h) {
    const double dv = (double)v;
    if (dv >= L && dv <= U) {
      const double d = dv - mean;
      acc += (double)h * (d * d);
    }
  });
  part[t] = acc;
  __syncthreads();
  for (int d = 1; d < kRobustThreads; d <<= 1) {
    if ((t & (2 * d - 1)) == 0) part[t] += part[t + d];
    __syncthreads();
  }
  if (t == 0) {
    const double ssd = ((double)nb * ((L - mean) * (L - mean)) + part[0]) + (double)na * ((U - mean) * (U - mean));
    r.n_below = nb; r.n_above = na; r.sum_in = s;
    r.lower = L; r.upper = U; r.mean = mean; r.ssd = ssd;
    r.std = sqrt(ssd / dn);
    out[c] = r;
  }
}

// brain_normalize_kernel's geometry with the second rule: w = min(max(x, L), U);  stored (float)((w - mean) / std), FLT_MIN where
// that is zero (x != 0; else 0): the box stays nonzero exactly where raw is.  L, U, mean, std: the device record of the modality.
__global__ __launch_bounds__(256) void brain_zscore_kernel(const int16_t* __restrict__ raw, int Cm, CropGeom g, const RobustRec* __restrict__ rr,
                                                           float* __restrict__ out, const uint8_t* __restrict__ truth,
                                                           uint8_t* __restrict__ truth_out) {
  const int c = blockIdx.y;
  const int64_t nb = (int64_t)g.b[0] * g.b[1] * g.b[2];
  double L = 0.0, U = 0.0, mean = 0.0, sd = 1.0;
  if (c < Cm) { L = rr[c].lower; U = rr[c].upper; mean = rr[c].mean; sd = rr[c].std; }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (int64_t)gridDim.x * 256) {
    uint32_t q, k, ii, j;
    g.fbz.divmod((uint32_t)i, q, k);
    g.fby.divmod(q, ii, j);
    const int64_t src = ((int64_t)(g.lo[0] + (int)ii) * g.Y + (g.lo[1] + (int)j)) * g.Z + (g.lo[2] + (int)k);
    if (c == Cm) {
      truth_out[i] = truth[src];
      continue;
    }
    const int x = raw[(int64_t)c * g.N + src];
    float r = 0.f;
    if (x != 0) {
      const double dx = (double)x;
      const double w = dx < L ? L : (dx > U ? U : dx);
      r = (float)((w - mean) / sd);
      if (r == 0.f) r = FLT_MIN;
    }
    out[(int64_t)c * nb + i] = r;
  }
}

}  // namespace n3d

using namespace n3d;

static int check_raw(const int16_t* raw, int Cm, int X, int Y, int Z, const char* what) {
  N3D_CHECK_ARG(raw && Cm >= 1 && X > 0 && Y > 0 && Z > 0, "%s: bad args", what);
  N3D_CHECK_ARG((reinterpret_cast<uintptr_t>(raw) & 1) == 0, "%s: raw must be 2-byte aligned", what);
  N3D_CHECK_ARG((int64_t)X * Y * Z < (1ll << 31), "%s: X * Y * Z = %lld voxels: the index arithmetic needs X * Y * Z < 2^31", what,
                (long long)X * Y * Z);
  return N3D_OK;
}

extern "C" int n3d_brain_scan(const int16_t* raw, int Cm, int X, int Y, int Z, int64_t* totals, int32_t* rec, void* stream) {
  if (int e = check_raw(raw, Cm, X, Y, Z, "brain_scan")) return e;
  N3D_CHECK_ARG(totals && rec, "brain_scan: bad args");
  N3D_CHECK_ARG((reinterpret_cast<uintptr_t>(totals) & 7) == 0 && (reinterpret_cast<uintptr_t>(rec) & 3) == 0,
                "brain_scan: totals must be 8-byte and rec 4-byte aligned");
  const int64_t N = (int64_t)X * Y * Z;
  N3D_LAUNCH(brain_scan_kernel, dim3((unsigned)span_blocks(N), (unsigned)Cm), dim3(256), 0, (hipStream_t)stream, raw, N, Y, Z,
             FastDiv((uint32_t)Y), FastDiv((uint32_t)Z), reinterpret_cast<unsigned long long*>(totals), rec);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_brain_sqdev_rows(int64_t N) { return N > 0 ? span_blocks(N) : 0; }

extern "C" int n3d_brain_sqdev(const int16_t* raw, int Cm, int64_t N, const double* mean, double* ws, double* acc, void* stream) {
  N3D_CHECK_ARG(raw && mean && ws && acc && Cm >= 1 && N > 0, "brain_sqdev: bad args");
  N3D_CHECK_ARG((reinterpret_cast<uintptr_t>(raw) & 1) == 0, "brain_sqdev: raw must be 2-byte aligned");
  N3D_CHECK_ARG(((reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(acc)) & 7) == 0,
                "brain_sqdev: mean, ws and acc must be 8-byte aligned");
  const int rows = span_blocks(N);
  hipStream_t s = (hipStream_t)stream;
  N3D_LAUNCH(brain_sqdev_kernel, dim3((unsigned)rows, (unsigned)Cm), dim3(256), 0, s, raw, N, mean, ws);
  N3D_LAUNCH_CHECK();
  N3D_LAUNCH(brain_sqdev_final_kernel, dim3((unsigned)Cm), dim3(256), 0, s, ws, rows, acc);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

// the box [lo, hi) of a normalise + crop launch, checked against the image, and the launch's blocks along x
static int crop_geom(int X, int Y, int Z, const int32_t* lo, const int32_t* hi, const char* what, CropGeom& g, unsigned& blocks) {
  const int dims[3] = {X, Y, Z};
  g.N = (int64_t)X * Y * Z;
  g.Y = Y;
  g.Z = Z;
  for (int a = 0; a < 3; ++a) {
    N3D_CHECK_ARG(0 <= lo[a] && lo[a] < hi[a] && hi[a] <= dims[a], "%s: box [%d, %d) on axis %d is not inside the image (%d)", what, lo[a],
                  hi[a], a, dims[a]);
    g.lo[a] = lo[a];
    g.b[a] = hi[a] - lo[a];
  }
  g.fby = FastDiv((uint32_t)g.b[1]);
  g.fbz = FastDiv((uint32_t)g.b[2]);
  const int64_t b = cdiv((int64_t)g.b[0] * g.b[1] * g.b[2], 256 * 4);
  blocks = (unsigned)(b > 4096 ? 4096 : b);
  return N3D_OK;
}

extern "C" int n3d_brain_normalize(const int16_t* raw, int Cm, int X, int Y, int Z, const double* mean_std, const int32_t* rec,
                                   const int32_t* lo, const int32_t* hi, float* out, const uint8_t* truth, uint8_t* truth_out, void* stream) {
  if (int e = check_raw(raw, Cm, X, Y, Z, "brain_normalize")) return e;
  N3D_CHECK_ARG(mean_std && rec && lo && hi && out && (truth == nullptr) == (truth_out == nullptr), "brain_normalize: bad args");
  N3D_CHECK_ARG((reinterpret_cast<uintptr_t>(mean_std) & 7) == 0 && (reinterpret_cast<uintptr_t>(rec) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(out) & 3) == 0, "brain_normalize: mean_std must be 8-byte, rec and out 4-byte aligned");
  CropGeom g;
  unsigned blocks;
  if (int e = crop_geom(X, Y, Z, lo, hi, "brain_normalize", g, blocks)) return e;
  N3D_LAUNCH(brain_normalize_kernel, dim3(blocks, (unsigned)(Cm + (truth ? 1 : 0))), dim3(256), 0, (hipStream_t)stream, raw, Cm, g,
             mean_std, rec, out, truth, truth_out);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_brain_hist_window(void) { return kHistWindow; }

extern "C" int n3d_brain_hist(const int16_t* raw, int Cm, int X, int Y, int Z, const int32_t* rec, int32_t* hist, void* stream) {
  if (int e = check_raw(raw, Cm, X, Y, Z, "brain_hist")) return e;
  N3D_CHECK_ARG(rec && hist, "brain_hist: bad args");
  N3D_CHECK_ARG((reinterpret_cast<uintptr_t>(rec) & 3) == 0 && aligned16(hist), "brain_hist: rec must be 4-byte and hist 16-byte aligned");
  const int64_t N = (int64_t)X * Y * Z;
  n3d::entry_flush();      // (the memset is no kernel of ours: an armed entry signal goes out in front)
  hipError_t e = hipMemsetAsync(hist, 0, sizeof(int32_t) * (size_t)Cm * kHistBins, (hipStream_t)stream);
  if (e != hipSuccess) { set_error("brain_hist: hipMemsetAsync: %s", hipGetErrorString(e)); return N3D_ERR_HIP; }
  int64_t blocks = cdiv(N >> 3, 256 * 16);
  blocks = blocks < 1 ? 1 : (blocks > kHistMaxBlocks ? kHistMaxBlocks : blocks);
  N3D_LAUNCH(brain_hist_kernel, dim3((unsigned)blocks, (unsigned)Cm), dim3(256), 0, (hipStream_t)stream, raw, N, rec, hist);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_brain_robust(const int32_t* hist, int Cm, double lower, double upper, int64_t* out, void* stream) {
  N3D_CHECK_ARG(hist && out && Cm >= 1, "brain_robust: bad args");
  N3D_CHECK_ARG(aligned16(hist) && (reinterpret_cast<uintptr_t>(out) & 7) == 0, "brain_robust: hist must be 16-byte and out 8-byte aligned");
  N3D_CHECK_ARG(0.0 <= lower && lower < upper && upper <= 100.0, "brain_robust: percentiles %g, %g: needs 0 <= lower < upper <= 100", lower,
                upper);
  N3D_LAUNCH(brain_robust_kernel, dim3((unsigned)Cm), dim3(kRobustThreads), 0, (hipStream_t)stream, hist, lower, upper,
             reinterpret_cast<RobustRec*>(out));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_brain_zscore(const int16_t* raw, int Cm, int X, int Y, int Z, const int64_t* robust, const int32_t* lo, const int32_t* hi,
                                float* out, const uint8_t* truth, uint8_t* truth_out, void* stream) {
  if (int e = check_raw(raw, Cm, X, Y, Z, "brain_zscore")) return e;
  N3D_CHECK_ARG(robust && lo && hi && out && (truth == nullptr) == (truth_out == nullptr), "brain_zscore: bad args");
  N3D_CHECK_ARG((reinterpret_cast<uintptr_t>(robust) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                "brain_zscore: robust must be 8-byte and out 4-byte aligned");
  CropGeom g;
  unsigned blocks;
  if (int e = crop_geom(X, Y, Z, lo, hi, "brain_zscore", g, blocks)) return e;
  N3D_LAUNCH(brain_zscore_kernel, dim3(blocks, (unsigned)(Cm + (truth ? 1 : 0))), dim3(256), 0, (hipStream_t)stream, raw, Cm, g,
             reinterpret_cast<const RobustRec*>(robust), out, truth, truth_out);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}
