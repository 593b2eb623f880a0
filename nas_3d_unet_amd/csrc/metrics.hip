// Segmentation metrics (include/n3d.h, "Segmentation metrics"): a predicted label volume against the truth, per region WT / TC / ET:
// the TP / FP / FN counts, both surfaces, the exact squared distance from every surface voxel to the other surface, and the order
// statistics of those distances that numpy's percentile 95 interpolates between.  Integer work throughout: counts and histogram
// bins are integer atomic adds, the bounding boxes atomic min / max, the distance transform int32 minima -- nothing depends on the
// order in which workgroups run, so two runs give the same bits.
#include "n3d_common.h"

namespace n3d {

struct SegGeom {
  int64_t N;             // FX * FY * FZ
  int F[3], B[3], O[3];  // image, truth box, the box's corner in the image
  FastDiv fY, fZ;
};

// label -> bit r set when the label belongs to region r (0 WT, 1 TC, 2 ET)
__device__ __forceinline__ unsigned region_bits(unsigned l) {
  return (unsigned)(l != 0) | ((unsigned)(l == 1 || l == 4) << 1) | ((unsigned)(l == 4) << 2);
}
__device__ __forceinline__ unsigned pred_bits(const uint8_t* __restrict__ pred, const SegGeom& g, int x, int y, int z) {
  if ((unsigned)x >= (unsigned)g.F[0] || (unsigned)y >= (unsigned)g.F[1] || (unsigned)z >= (unsigned)g.F[2]) return 0;
  return region_bits(pred[((int64_t)x * g.F[1] + y) * g.F[2] + z]);
}
__device__ __forceinline__ unsigned truth_bits(const uint8_t* __restrict__ truth, const SegGeom& g, int x, int y, int z) {
  x -= g.O[0]; y -= g.O[1]; z -= g.O[2];
  if ((unsigned)x >= (unsigned)g.B[0] || (unsigned)y >= (unsigned)g.B[1] || (unsigned)z >= (unsigned)g.B[2]) return 0;
  return region_bits(truth[((int64_t)x * g.B[1] + y) * g.B[2] + z]);
}
// bits of the regions that hold all six neighbours (a neighbour outside the image or the box holds none)
template <typename F>
__device__ __forceinline__ unsigned neighbours_and(F&& at, int x, int y, int z) {
  return at(x - 1, y, z) & at(x + 1, y, z) & at(x, y - 1, z) & at(x, y + 1, z) & at(x, y, z - 1) & at(x, y, z + 1);
}

// Same-address atomics retire one at a time (tens of nanoseconds each), so the launches that end in atomics on a handful of
// addresses use FEW, LARGE workgroups: 1024 threads, at most a workgroup per CU, and several independent loads in flight per thread
// to make up for the shorter grid.
constexpr int SEG_THREADS = 1024, SEG_WAVES = SEG_THREADS / 64;
constexpr int REGION_UNROLL = 8, REGION_GRID = 256;

// grid (blocks): REGION_UNROLL voxels per thread and iteration, a grid stride apart.  The three regions of a side travel as three bits, so a voxel costs two
// label reads and, only where a label is set, six neighbour reads per side.  Per thread: 9 counters and 3 boxes; wave butterfly,
// LDS across the waves, then one atomic per workgroup and counter that is not zero / box that is not empty.
__global__ __launch_bounds__(SEG_THREADS) void seg_regions_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth, SegGeom g,
                                                          uint8_t* __restrict__ flags, unsigned long long* __restrict__ counts,
                                                          int* __restrict__ bbox) {
  unsigned cnt[9];
  int lo[9], hi[9];   // [region * 3 + axis]
#pragma unroll
  for (int k = 0; k < 9; ++k) { cnt[k] = 0; lo[k] = INT32_MAX; hi[k] = -1; }
  const int64_t stride = (int64_t)gridDim.x * SEG_THREADS;
  for (int64_t i0 = (int64_t)blockIdx.x * SEG_THREADS + threadIdx.x; i0 < g.N; i0 += REGION_UNROLL * stride) {
    // the labels of REGION_UNROLL voxels are requested together: one at a time a thread's walk is a chain of memory round trips
    int x[REGION_UNROLL], y[REGION_UNROLL], z[REGION_UNROLL];
    unsigned mp[REGION_UNROLL], mt[REGION_UNROLL];
#pragma unroll
    for (int u = 0; u < REGION_UNROLL; ++u) {
      const int64_t i = i0 + u * stride;
      mp[u] = mt[u] = 0;
      x[u] = y[u] = z[u] = 0;
      if (i < g.N) {
        uint32_t q, uz, ux, uy;
        g.fZ.divmod((uint32_t)i, q, uz);
        g.fY.divmod(q, ux, uy);
        x[u] = (int)ux; y[u] = (int)uy; z[u] = (int)uz;
        mp[u] = region_bits(pred[i]);
        mt[u] = truth_bits(truth, g, x[u], y[u], z[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < REGION_UNROLL; ++u) {
      const int64_t i = i0 + u * stride;
      if (i >= g.N) break;
      if (!(mp[u] | mt[u])) {   // background on both sides: nothing to count, no surface
        flags[i] = 0;
        continue;
      }
      unsigned sp = 0, st = 0;
      if (mp[u]) sp = mp[u] & ~neighbours_and([&](int a, int b, int c) { return pred_bits(pred, g, a, b, c); }, x[u], y[u], z[u]);
      if (mt[u]) st = mt[u] & ~neighbours_and([&](int a, int b, int c) { return truth_bits(truth, g, a, b, c); }, x[u], y[u], z[u]);
      flags[i] = (uint8_t)(sp | (st << 3));
      const unsigned tp = mp[u] & mt[u], fp = mp[u] & ~mt[u], fn = mt[u] & ~mp[u], su = sp | st;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        cnt[3 * r + 0] += (tp >> r) & 1;
        cnt[3 * r + 1] += (fp >> r) & 1;
        cnt[3 * r + 2] += (fn >> r) & 1;
        if ((su >> r) & 1) {
          lo[3 * r + 0] = min(lo[3 * r + 0], x[u]); hi[3 * r + 0] = max(hi[3 * r + 0], x[u]);
          lo[3 * r + 1] = min(lo[3 * r + 1], y[u]); hi[3 * r + 1] = max(hi[3 * r + 1], y[u]);
          lo[3 * r + 2] = min(lo[3 * r + 2], z[u]); hi[3 * r + 2] = max(hi[3 * r + 2], z[u]);
        }
      }
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      cnt[k] += __shfl_xor(cnt[k], d, 64);
      lo[k] = min(lo[k], __shfl_xor(lo[k], d, 64));
      hi[k] = max(hi[k], __shfl_xor(hi[k], d, 64));
    }
  }
  __shared__ unsigned s_cnt[SEG_WAVES][9];
  __shared__ int s_lo[SEG_WAVES][9], s_hi[SEG_WAVES][9];
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) { s_cnt[threadIdx.x >> 6][k] = cnt[k]; s_lo[threadIdx.x >> 6][k] = lo[k]; s_hi[threadIdx.x >> 6][k] = hi[k]; }
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    const int k = threadIdx.x;
    unsigned c = 0;
    int l = INT32_MAX, h = -1;
#pragma unroll
    for (int w = 0; w < SEG_WAVES; ++w) {
      c += s_cnt[w][k];
      l = min(l, s_lo[w][k]);
      h = max(h, s_hi[w][k]);
    }
    if (c) atomicAdd(counts + k, (unsigned long long)c);
    if (h >= 0) {
      const int r = k / 3, a = k - 3 * r;
      atomicMin(bbox + 6 * r + a, l);
      atomicMax(bbox + 6 * r + 3 + a, h);
    }
  }
}

// a job's box, clipped to the image (it is device data: nothing is addressed through it unclipped); false: empty
__device__ __forceinline__ bool seg_box(const int* __restrict__ bb, const int* F, int* lo, int* hi) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = max(bb[a], 0);
    hi[a] = min(bb[3 + a], F[a] - 1);
  }
  return lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2];
}

struct EdtGeom {
  int64_t N;
  int F[3];
  int nreg;
};

constexpr int EDT_GRID = 512;    // workgroups per job: they walk the tiles of the job's box, whose number only the device knows

// First pass, along z.  grid (<= EDT_GRID, 1, njobs), 1024 threads.  A tile is `zlines` (16, or 8 where FZ > 512) adjacent y lines
// of one x plane of job j's box; LDS holds f (0 on a source, INF elsewhere) of those lines over the box's z range, pitch L.  A wave
// takes a line; a lane computes the outputs i = lane, lane + 64, .. + 192 in one walk over j (every lane reads the same LDS word:
// a broadcast).  Dynamic LDS: zlines * FZ ints (<= 32 KB).
__global__ __launch_bounds__(SEG_THREADS) void seg_edt_z_kernel(const uint8_t* __restrict__ flags, EdtGeom g, int zlines,
                                                                const int* __restrict__ bbox, int32_t* __restrict__ dist) {
  extern __shared__ int lds[];
  const int job = blockIdx.y;
  int lo[3], hi[3];
  if (!seg_box(bbox + 6 * (job % g.nreg), g.F, lo, hi)) return;
  const int L = hi[2] - lo[2] + 1, ny = (hi[1] - lo[1]) / zlines + 1, ntiles = (hi[0] - lo[0] + 1) * ny;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int bx = tile / ny;
    const int x = lo[0] + bx, y0 = lo[1] + (tile - bx * ny) * zlines;
    const int nl = min(zlines, hi[1] - y0 + 1);
    const int64_t base = ((int64_t)x * g.F[1] + y0) * g.F[2] + lo[2];
    for (int l = wave; l < nl; l += SEG_WAVES)
      for (int j = lane; j < L; j += 64) lds[l * L + j] = ((flags[base + (int64_t)l * g.F[2] + j] >> job) & 1) ? 0 : N3D_SEG_INF;
    __syncthreads();
    int32_t* out = dist + (int64_t)job * g.N + base;
    for (int l = wave; l < nl; l += SEG_WAVES) {
      const int* row = lds + l * L;
      for (int i0 = lane; i0 < L; i0 += 256) {
        int m0 = INT32_MAX, m1 = INT32_MAX, m2 = INT32_MAX, m3 = INT32_MAX;
        for (int j = 0; j < L; ++j) {
          const int v = row[j], d = i0 - j;
          m0 = min(m0, v + d * d);
          m1 = min(m1, v + (d + 64) * (d + 64));
          m2 = min(m2, v + (d + 128) * (d + 128));
          m3 = min(m3, v + (d + 192) * (d + 192));
        }
        int32_t* o = out + (int64_t)l * g.F[2] + i0;
        o[0] = m0;
        if (i0 + 64 < L) o[64] = m1;
        if (i0 + 128 < L) o[128] = m2;
        if (i0 + 192 < L) o[192] = m3;
      }
    }
    __syncthreads();   // the tile's LDS is read to the end before the next tile's fill
  }
}

// Second and third pass, along `axis` (1: y, 0: x), in place.  grid (<= EDT_GRID, 1, njobs), 1024 threads.  A tile is T = 1 << tshift adjacent
// z columns of the lines at one position of the other axis, over the box's range along `axis`.  LDS holds it as
// [line position][z column], so the loads and stores run along z and a wave's LDS reads are consecutive words.  A thread computes
// four consecutive outputs of one column in one walk over the line: one LDS read per four min-steps.
// Values: f <= INF + 1023^2 going in; INF + 0 (j = i) comes out of a line without a source, so "no source" stays exactly INF.
// Dynamic LDS: T * F[axis] ints.
__global__ __launch_bounds__(SEG_THREADS) void seg_edt_line_kernel(EdtGeom g, int axis, int tshift, const int* __restrict__ bbox,
                                                           int32_t* __restrict__ dist) {
  extern __shared__ int lds[];
  const int job = blockIdx.y, other = 1 - axis, T = 1 << tshift;
  int lo[3], hi[3];
  if (!seg_box(bbox + 6 * (job % g.nreg), g.F, lo, hi)) return;
  const int L = hi[axis] - lo[axis] + 1, nzt = ((hi[2] - lo[2]) >> tshift) + 1, ntiles = (hi[other] - lo[other] + 1) * nzt;
  const int64_t sl = axis == 1 ? (int64_t)g.F[2] : (int64_t)g.F[1] * g.F[2];   // stride of the line
  const int64_t so = axis == 1 ? (int64_t)g.F[1] * g.F[2] : (int64_t)g.F[2];
  const int units = ((L + 3) >> 2) << tshift;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int bo = tile / nzt;
    const int o = lo[other] + bo, z0 = lo[2] + ((tile - bo * nzt) << tshift);
    const int nz = min(T, hi[2] - z0 + 1);
    int32_t* p = dist + (int64_t)job * g.N + (int64_t)o * so + (int64_t)lo[axis] * sl + z0;
    for (int e = threadIdx.x; e < (L << tshift); e += SEG_THREADS) {
      const int j = e >> tshift, t = e & (T - 1);
      lds[e] = t < nz ? p[(int64_t)j * sl + t] : N3D_SEG_INF;
    }
    __syncthreads();
    for (int u = threadIdx.x; u < units; u += SEG_THREADS) {
      const int t = u & (T - 1), i0 = (u >> tshift) << 2;
      int m0 = INT32_MAX, m1 = INT32_MAX, m2 = INT32_MAX, m3 = INT32_MAX;
      for (int j = 0; j < L; ++j) {
        const int v = lds[(j << tshift) + t], d = i0 - j;
        m0 = min(m0, v + d * d);
        m1 = min(m1, v + (d + 1) * (d + 1));
        m2 = min(m2, v + (d + 2) * (d + 2));
        m3 = min(m3, v + (d + 3) * (d + 3));
      }
      if (t < nz) {
        int32_t* q = p + (int64_t)i0 * sl + t;
        q[0] = m0;
        if (i0 + 1 < L) q[sl] = m1;
        if (i0 + 2 < L) q[2 * sl] = m2;
        if (i0 + 3 < L) q[3 * sl] = m3;
      }
    }
    __syncthreads();
  }
}

// The calling lanes each add 1 to h[d].  The lanes that share the first calling lane's bin go as ONE atomic of their number
// (a ballot and a compare: where prediction and truth agree that is every lane, bin 0); the others add for themselves.
__device__ __forceinline__ void hist_add(uint32_t* __restrict__ h, int d) {
  const int first = __builtin_amdgcn_readfirstlane(d);
  const unsigned long long same = __ballot(d == first);
  if (d == first) {
    if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(h + d, (uint32_t)__popcll(same));
  } else {
    atomicAdd(h + d, 1u);
  }
}

constexpr int SAMPLE_GRID = 128, SAMPLE_LDS_BINS = 2048;

// grid (<= SAMPLE_GRID), 1024 threads.  Every surface voxel lies in its region's box, so only the box around the three boxes is
// walked: a wave takes a z row of it, lanes along z.  A voxel without a surface bit costs its flag byte; a surface voxel requests
// its (up to six) distances together and then adds them.  Most distances of a subject fall into a few dozen small bins, and an
// atomic per distance on those few addresses would be the whole launch: bins below SAMPLE_LDS_BINS are counted in a histogram in
// LDS and flushed once per workgroup (nonzero bins only); larger bins, spread out and rare, go to memory directly.  A bin outside
// the histogram is not counted (INF: the other surface of the region is empty; n stays 0 and the host reports NaN).
__global__ __launch_bounds__(SEG_THREADS) void seg_sample_kernel(const uint8_t* __restrict__ flags, EdtGeom g, const int* __restrict__ bbox,
                                                                 const int32_t* __restrict__ dist, uint32_t* __restrict__ hist,
                                                                 int64_t hist_len) {
  __shared__ uint32_t lh[3 * SAMPLE_LDS_BINS];
  int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {-1, -1, -1};
  for (int r = 0; r < 3; ++r) {
    int l[3], h[3];
    if (!seg_box(bbox + 6 * r, g.F, l, h)) continue;
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], l[a]); hi[a] = max(hi[a], h[a]); }
  }
  if (hi[0] < 0) return;
  for (int b = threadIdx.x; b < 3 * SAMPLE_LDS_BINS; b += SEG_THREADS) lh[b] = 0;
  __syncthreads();
  const int ny = hi[1] - lo[1] + 1, nrows = (hi[0] - lo[0] + 1) * ny;
  const int lane = threadIdx.x & 63;
  for (int row = blockIdx.x * SEG_WAVES + (threadIdx.x >> 6); row < nrows; row += gridDim.x * SEG_WAVES) {
    const int bx = row / ny;
    const int64_t base = ((int64_t)(lo[0] + bx) * g.F[1] + lo[1] + (row - bx * ny)) * g.F[2];
    for (int z = lo[2] + lane; z <= hi[2]; z += 64) {
      const int64_t i = base + z;
      const unsigned f = flags[i];
      if (!f) continue;
      int d[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) d[q] = ((f >> q) & 1) ? dist[(int64_t)(q < 3 ? q + 3 : q - 3) * g.N + i] : -1;
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const int r = q < 3 ? q : q - 3;
        if ((unsigned)d[q] < (unsigned)SAMPLE_LDS_BINS) {
          if ((int64_t)d[q] < hist_len) hist_add(lh + r * SAMPLE_LDS_BINS, d[q]);
        } else if ((int64_t)(unsigned)d[q] < hist_len) {
          hist_add(hist + r * hist_len, d[q]);
        }
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 3 * SAMPLE_LDS_BINS; b += SEG_THREADS) {
    const uint32_t c = lh[b];
    const int r = b / SAMPLE_LDS_BINS, bin = b - r * SAMPLE_LDS_BINS;
    if (c) atomicAdd(hist + r * hist_len + bin, c);
  }
}

constexpr int ORDER_THREADS = 1024;

// grid (3): workgroup r scans hist[r][0 .. len), len = squared diagonal of bbox[r] + 1 (no distance of the region is larger).
// A thread sums its contiguous chunk and notes its last nonzero bin; a scan over the threads' sums gives every thread the ranks
// [mine, next) of its chunk; the threads whose ranks hold k / k + 1 walk their chunk again to the bin.  k = floor((n - 1) * 0.95) in fp64: one product,
// the one numpy's percentile forms.
__global__ __launch_bounds__(ORDER_THREADS) void seg_order_kernel(const uint32_t* __restrict__ hist, int64_t hist_len, long long* __restrict__ rec) {
  const int r = blockIdx.x;
  const int* bb = reinterpret_cast<const int*>(rec + N3D_SEG_REC_BBOX) + 6 * r;
  long long* out = rec + N3D_SEG_REC_ORDER + 4 * r;
  int64_t len = 0;
  if (bb[3] >= bb[0] && bb[4] >= bb[1] && bb[5] >= bb[2]) {
    const int64_t dx = (int64_t)bb[3] - bb[0], dy = (int64_t)bb[4] - bb[1], dz = (int64_t)bb[5] - bb[2];
    len = dx * dx + dy * dy + dz * dz + 1;
    if (len > hist_len) len = hist_len;
  }
  const uint32_t* h = hist + r * hist_len;
  const int64_t chunk = (len + ORDER_THREADS - 1) / ORDER_THREADS;
  int64_t c0 = (int64_t)threadIdx.x * chunk, c1 = c0 + chunk;
  if (c0 > len) c0 = len;
  if (c1 > len) c1 = len;
  unsigned long long s = 0;
  long long mx = -1;
  for (int64_t b = c0; b < c1; b += 8) {   // eight loads in flight: a chunk is a chain of memory round trips otherwise
    uint32_t c[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) c[u] = b + u < c1 ? h[b + u] : 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s += c[u];
      if (c[u]) mx = b + u;
    }
  }
  __shared__ unsigned long long scan[2][ORDER_THREADS];
  __shared__ long long smx[2][ORDER_THREADS];
  int p = 0;
  scan[0][threadIdx.x] = s;
  smx[0][threadIdx.x] = mx;
  __syncthreads();
  for (int d = 1; d < ORDER_THREADS; d <<= 1, p ^= 1) {   // inclusive scan of the sums, running maximum of the last nonzero bins
    unsigned long long v = scan[p][threadIdx.x];
    long long m = smx[p][threadIdx.x];
    if ((int)threadIdx.x >= d) {
      v += scan[p][threadIdx.x - d];
      m = max(m, smx[p][threadIdx.x - d]);
    }
    scan[p ^ 1][threadIdx.x] = v;
    smx[p ^ 1][threadIdx.x] = m;
    __syncthreads();
  }
  const unsigned long long n = scan[p][ORDER_THREADS - 1], next = scan[p][threadIdx.x], mine = next - s;
  if (n == 0) {
    if (threadIdx.x < 4) out[threadIdx.x] = 0;
    return;
  }
  const unsigned long long k = (unsigned long long)floor((double)(n - 1) * 0.95);
  const unsigned long long k1 = k + 1 < n ? k + 1 : n - 1;
  if (threadIdx.x == ORDER_THREADS - 1) {
    out[0] = (long long)n;
    out[3] = smx[p][ORDER_THREADS - 1];
  }
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const unsigned long long rank = w ? k1 : k;
    if (rank >= mine && rank < next) {
      unsigned long long cum = mine;
      for (int64_t b = c0; b < c1; ++b) {
        cum += h[b];
        if (cum > rank) {
          out[1 + w] = b;
          break;
        }
      }
    }
  }
}

}  // namespace n3d

using namespace n3d;

static int seg_full(const int32_t* full, const char* what, int64_t* N) {
  N3D_CHECK_ARG(full && full[0] > 0 && full[1] > 0 && full[2] > 0, "%s: bad image shape", what);
  *N = (int64_t)full[0] * full[1] * full[2];
  N3D_CHECK_ARG(*N < (1ll << 31), "%s: image (%d, %d, %d) = %lld voxels: the index arithmetic needs FX * FY * FZ < 2^31", what, full[0],
                full[1], full[2], (long long)*N);
  return N3D_OK;
}
static inline int64_t seg_hist_len(int FX, int FY, int FZ) {
  return (int64_t)(FX - 1) * (FX - 1) + (int64_t)(FY - 1) * (FY - 1) + (int64_t)(FZ - 1) * (FZ - 1) + 1;
}
static inline int64_t up256(int64_t b) { return (b + 255) & ~(int64_t)255; }
static inline unsigned seg_blocks(int64_t N) {
  const int64_t b = cdiv(N, SEG_THREADS * REGION_UNROLL);
  return (unsigned)(b < 1 ? 1 : (b > REGION_GRID ? REGION_GRID : b));
}

extern "C" size_t n3d_seg_workspace_bytes(int FX, int FY, int FZ, int64_t* offsets) {
  if (FX <= 0 || FY <= 0 || FZ <= 0 || (int64_t)FX * FY * FZ >= (1ll << 31)) return 0;
  const int64_t N = (int64_t)FX * FY * FZ, HL = seg_hist_len(FX, FY, FZ);
  const int64_t o_rec = 0, o_flags = up256(N3D_SEG_REC_WORDS * 8), o_dist = o_flags + up256(N), o_hist = o_dist + up256(6 * N * 4);
  if (offsets) {
    offsets[0] = o_rec; offsets[1] = o_flags; offsets[2] = o_dist; offsets[3] = o_hist; offsets[4] = HL;
  }
  return (size_t)(o_hist + up256(N3D_SEG_REGIONS * HL * 4));
}

extern "C" int n3d_seg_regions(const uint8_t* pred, const uint8_t* truth, const int32_t* full, const int32_t* box, const int32_t* origin,
                               uint8_t* flags, int64_t* rec, void* stream) {
  SegGeom g;
  if (int e = seg_full(full, "seg_regions", &g.N)) return e;
  N3D_CHECK_ARG(pred && truth && box && origin && flags && rec, "seg_regions: bad args");
  N3D_CHECK_ARG((reinterpret_cast<uintptr_t>(rec) & 7) == 0, "seg_regions: rec must be 8-byte aligned");
  for (int a = 0; a < 3; ++a) {
    N3D_CHECK_ARG(box[a] > 0 && origin[a] >= 0 && origin[a] + box[a] <= full[a],
                  "seg_regions: the truth box %d at %d on axis %d is not inside the image (%d)", box[a], origin[a], a, full[a]);
    g.F[a] = full[a]; g.B[a] = box[a]; g.O[a] = origin[a];
  }
  g.fY = FastDiv((uint32_t)full[1]);
  g.fZ = FastDiv((uint32_t)full[2]);
  N3D_LAUNCH(seg_regions_kernel, dim3(seg_blocks(g.N)), dim3(SEG_THREADS), 0, (hipStream_t)stream, pred, truth, g, flags,
             reinterpret_cast<unsigned long long*>(rec), reinterpret_cast<int*>(rec + N3D_SEG_REC_BBOX));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_seg_edt(const uint8_t* flags, int njobs, int nreg, const int32_t* full, const int32_t* bbox, int32_t* dist, void* stream) {
  EdtGeom g;
  if (int e = seg_full(full, "seg_edt", &g.N)) return e;
  N3D_CHECK_ARG(flags && bbox && dist && njobs >= 1 && njobs <= 6 && nreg >= 1 && nreg <= njobs, "seg_edt: bad args");
  N3D_CHECK_ARG(((reinterpret_cast<uintptr_t>(bbox) | reinterpret_cast<uintptr_t>(dist)) & 3) == 0, "seg_edt: bbox and dist must be 4-byte aligned");
  for (int a = 0; a < 3; ++a) {
    if (full[a] > N3D_SEG_MAX_AXIS)
      N3D_UNSUPPORTED("seg_edt: image (%d, %d, %d): axis %d is %d long, the distance transform takes lines up to %d (int32 squared distances, "
                      "one line in LDS)", full[0], full[1], full[2], a, full[a], N3D_SEG_MAX_AXIS);
    g.F[a] = full[a];
  }
  g.nreg = nreg;
  hipStream_t s = (hipStream_t)stream;
  // tiles of a box that is the whole image: an upper bound for the grid, the kernels walk what the device's box holds
  const int zlines = full[2] <= 512 ? 16 : 8;
  const int64_t zt = cdiv(full[1], zlines) * full[0];
  N3D_LAUNCH(seg_edt_z_kernel, dim3((unsigned)(zt < EDT_GRID ? zt : EDT_GRID), (unsigned)njobs), dim3(SEG_THREADS),
             (size_t)zlines * full[2] * sizeof(int), s, flags, g, zlines, bbox, dist);
  N3D_LAUNCH_CHECK();
  for (int axis = 1; axis >= 0; --axis) {
    const int tshift = full[axis] <= 256 ? 5 : 3;   // 32 columns of <= 256, or 8 of <= 1024: at most 32 KB of LDS
    const int64_t lt = cdiv(full[2], 1 << tshift) * full[1 - axis];
    N3D_LAUNCH(seg_edt_line_kernel, dim3((unsigned)(lt < EDT_GRID ? lt : EDT_GRID), (unsigned)njobs), dim3(SEG_THREADS),
               ((size_t)full[axis] << tshift) * sizeof(int), s, g, axis, tshift, bbox, dist);
    N3D_LAUNCH_CHECK();
  }
  return N3D_OK;
}

extern "C" int n3d_seg_sample(const uint8_t* flags, const int32_t* full, const int32_t* bbox, const int32_t* dist, uint32_t* hist,
                              int64_t hist_len, void* stream) {
  EdtGeom g;
  if (int e = seg_full(full, "seg_sample", &g.N)) return e;
  N3D_CHECK_ARG(flags && bbox && dist && hist && hist_len >= 1 && hist_len < (1ll << 31), "seg_sample: bad args");
  N3D_CHECK_ARG(((reinterpret_cast<uintptr_t>(bbox) | reinterpret_cast<uintptr_t>(dist) | reinterpret_cast<uintptr_t>(hist)) & 3) == 0,
                "seg_sample: bbox, dist and hist must be 4-byte aligned");
  for (int a = 0; a < 3; ++a) g.F[a] = full[a];
  g.nreg = N3D_SEG_REGIONS;
  const int64_t rows = cdiv((int64_t)full[0] * full[1], SEG_WAVES);
  N3D_LAUNCH(seg_sample_kernel, dim3((unsigned)(rows < SAMPLE_GRID ? rows : SAMPLE_GRID)), dim3(SEG_THREADS), 0, (hipStream_t)stream, flags, g, bbox,
             dist, hist, hist_len);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_seg_order(const uint32_t* hist, int64_t hist_len, int64_t* rec, void* stream) {
  N3D_CHECK_ARG(hist && rec && hist_len >= 1, "seg_order: bad args");
  N3D_CHECK_ARG((reinterpret_cast<uintptr_t>(hist) & 3) == 0 && (reinterpret_cast<uintptr_t>(rec) & 7) == 0,
                "seg_order: hist must be 4-byte and rec 8-byte aligned");
  N3D_LAUNCH(seg_order_kernel, dim3(N3D_SEG_REGIONS), dim3(ORDER_THREADS), 0, (hipStream_t)stream, hist, hist_len, reinterpret_cast<long long*>(rec));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}
