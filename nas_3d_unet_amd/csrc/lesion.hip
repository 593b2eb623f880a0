// Lesion-wise metrics (include/n3d.h, "Lesion-wise metrics"): the BraTS 2023 scoring of a predicted label volume, per region WT / TC /
// ET, without the volumes leaving the device.  The truth mask G is dilated (18-neighbourhood, `dilation` times); the 26-connected
// components of the dilated mask are the lesions, those of the prediction P its components (both by n3d_cc_label, on scratch of this
// workspace); a component matches every lesion whose dilated component it touches.  Per lesion come the voxel counts and the order
// statistics of the exact squared surface distances between the lesion and its matched components.
//
// Integer work and integer atomics (add / min / max / or) throughout, so the same inputs give the same bits.  Two places append to
// lists in an order that depends on scheduling -- the lesion roots and the surface voxels -- and neither order reaches the record:
// the roots are ranked by id before anything uses them, and of the surface lists only counts, minima and order statistics are kept.
// Termination: every loop is a grid-stride or tile loop bounded by a count clipped to its list's capacity, the bisection halves an
// integer interval, and no kernel waits on another workgroup.  Every index into a list is below the list's capacity: appends past
// it are dropped (the count alone goes on and becomes the overflow bit), readers clip the count.
#include "n3d_common.h"

namespace n3d {

constexpr int LW_THREADS = 256;
constexpr int LW_GRID = 1024;      // workgroups of the streaming launches and of the tile walk: they stride over what is left
constexpr int LW_CAP = N3D_LW_MAX_SURFACE, LW_LES = N3D_LW_MAX_LESIONS;
// the dilation's tile, the one of the component labelling: 8 x 8 x 32 voxels, z (contiguous) longest
constexpr int LW_TX = 8, LW_TY = 8, LW_TZ = 32;
constexpr int LW_DTILE = 256;      // entries of the other list per LDS tile of the distance launch
constexpr int LW_DGRID = 2048;     // workgroups per side of the distance launch
constexpr unsigned LW_NO_RANK = 0xFFFFFFFFu;

struct LwGeom {
  int N;                 // FX * FY * FZ < 2^31
  int F[3], B[3], O[3];  // image, truth box, the box's corner in the image
  int ntiles;
  FastDiv fY, fZ, tY, tZ;
};

// what the launches of a subject hand to each other besides the volumes
struct LwCtl {
  int tbbox[3][6];               // bounding box (lo, hi inclusive) of the truth's region mask; {INT32_MAX x 3, -1 x 3} when empty
  unsigned nroots[3], ng[3], np[3];   // appended lesion roots, truth-surface entries, prediction-surface entries (may pass the caps)
  int roots[3][LW_LES];
};

struct LwLists {
  uint32_t *gcoord, *grank, *pcoord, *prank;   // [LW_CAP] each: packed coordinate, lesion rank
  int32_t *gdist, *pdist;                      // [LW_CAP]: squared distance to the other side of the entry's lesion, INT32_MAX: none
};

__device__ __forceinline__ unsigned lw_region_bits(unsigned l) {
  return (unsigned)(l != 0) | ((unsigned)(l == 1 || l == 4) << 1) | ((unsigned)(l == 4) << 2);
}
__device__ __forceinline__ unsigned lw_pred_bits(const uint8_t* __restrict__ pred, const LwGeom& g, int x, int y, int z) {
  if ((unsigned)x >= (unsigned)g.F[0] || (unsigned)y >= (unsigned)g.F[1] || (unsigned)z >= (unsigned)g.F[2]) return 0;
  return lw_region_bits(pred[((int64_t)x * g.F[1] + y) * g.F[2] + z]);
}
__device__ __forceinline__ unsigned lw_truth_bits(const uint8_t* __restrict__ truth, const LwGeom& g, int x, int y, int z) {
  x -= g.O[0]; y -= g.O[1]; z -= g.O[2];
  if ((unsigned)x >= (unsigned)g.B[0] || (unsigned)y >= (unsigned)g.B[1] || (unsigned)z >= (unsigned)g.B[2]) return 0;
  return lw_region_bits(truth[((int64_t)x * g.B[1] + y) * g.B[2] + z]);
}
template <typename F>
__device__ __forceinline__ unsigned lw_neighbours_and(F&& at, int x, int y, int z) {
  return at(x - 1, y, z) & at(x + 1, y, z) & at(x, y - 1, z) & at(x, y + 1, z) & at(x, y, z - 1) & at(x, y, z + 1);
}
__device__ __forceinline__ void lw_decode(const LwGeom& g, int v, int& x, int& y, int& z) {
  uint32_t q, uz, ux, uy;
  g.fZ.divmod((uint32_t)v, q, uz);
  g.fY.divmod(q, ux, uy);
  x = (int)ux; y = (int)uy; z = (int)uz;
}
__device__ __forceinline__ uint32_t lw_pack(int x, int y, int z) { return ((uint32_t)x << 20) | ((uint32_t)y << 10) | (uint32_t)z; }
__device__ __forceinline__ int lw_d2(uint32_t a, uint32_t b) {
  const int dx = (int)(a >> 20) - (int)(b >> 20), dy = (int)((a >> 10) & 1023u) - (int)((b >> 10) & 1023u), dz = (int)(a & 1023u) - (int)(b & 1023u);
  return dx * dx + dy * dy + dz * dz;
}

// grid (1): clears the record and the control block of a subject
__global__ __launch_bounds__(LW_THREADS) void lw_init_kernel(long long* __restrict__ rec, LwCtl* __restrict__ ctl) {
  for (int i = threadIdx.x; i < N3D_LW_REC_WORDS; i += LW_THREADS) rec[i] = 0;
  if (threadIdx.x < 18) ctl->tbbox[threadIdx.x / 6][threadIdx.x % 6] = (threadIdx.x % 6) < 3 ? INT32_MAX : -1;
  if (threadIdx.x < 3) ctl->nroots[threadIdx.x] = ctl->ng[threadIdx.x] = ctl->np[threadIdx.x] = 0;
  for (int i = threadIdx.x; i < 3 * LW_LES; i += LW_THREADS) ctl->roots[i / LW_LES][i % LW_LES] = 0;
}

// grid (<= LW_GRID) over the voxels.  bits[v]: bits 0..2 the prediction's membership of WT / TC / ET, bits 3..5 the truth's (zero
// outside its box); surf[v]: the same six bits for "on the 6-neighbourhood surface"; the truth's bounding box per region.
__global__ __launch_bounds__(LW_THREADS) void lw_prep_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth, LwGeom g,
                                                             uint8_t* __restrict__ bits, uint8_t* __restrict__ surf, LwCtl* __restrict__ ctl) {
  __shared__ int s_lo[9], s_hi[9];
  if (threadIdx.x < 9) { s_lo[threadIdx.x] = INT32_MAX; s_hi[threadIdx.x] = -1; }
  __syncthreads();
  int lo[9], hi[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) { lo[k] = INT32_MAX; hi[k] = -1; }
  const int64_t stride = (int64_t)gridDim.x * LW_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * LW_THREADS + threadIdx.x; i < g.N; i += stride) {
    int x, y, z;
    lw_decode(g, (int)i, x, y, z);
    const unsigned mp = lw_region_bits(pred[i]), mt = lw_truth_bits(truth, g, x, y, z);
    bits[i] = (uint8_t)(mp | (mt << 3));
    unsigned sp = 0, st = 0;
    if (mp) sp = mp & ~lw_neighbours_and([&](int a, int b, int c) { return lw_pred_bits(pred, g, a, b, c); }, x, y, z);
    if (mt) st = mt & ~lw_neighbours_and([&](int a, int b, int c) { return lw_truth_bits(truth, g, a, b, c); }, x, y, z);
    surf[i] = (uint8_t)(sp | (st << 3));
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if ((mt >> r) & 1) {
        lo[3 * r + 0] = min(lo[3 * r + 0], x); hi[3 * r + 0] = max(hi[3 * r + 0], x);
        lo[3 * r + 1] = min(lo[3 * r + 1], y); hi[3 * r + 1] = max(hi[3 * r + 1], y);
        lo[3 * r + 2] = min(lo[3 * r + 2], z); hi[3 * r + 2] = max(hi[3 * r + 2], z);
      }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k)
    if (hi[k] >= 0) { atomicMin(s_lo + k, lo[k]); atomicMax(s_hi + k, hi[k]); }
  __syncthreads();
  if (threadIdx.x < 9 && s_hi[threadIdx.x] >= 0) {
    const int r = threadIdx.x / 3, a = threadIdx.x - 3 * r;
    atomicMin(&ctl->tbbox[r][a], s_lo[threadIdx.x]);
    atomicMax(&ctl->tbbox[r][3 + a], s_hi[threadIdx.x]);
  }
}

// grid (<= LW_GRID) over the voxels: the prediction's mask of region r as a byte volume (what n3d_cc_label takes) and the per-root
// sums of the region cleared
__global__ __launch_bounds__(LW_THREADS) void lw_select_kernel(const uint8_t* __restrict__ bits, int N, int r, uint8_t* __restrict__ pm,
                                                               int* __restrict__ psize, unsigned long long* __restrict__ pmatch) {
  const int64_t stride = (int64_t)gridDim.x * LW_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * LW_THREADS + threadIdx.x; i < N; i += stride) {
    pm[i] = (bits[i] >> r) & 1;
    psize[i] = 0;
    pmatch[i] = 0;
  }
}

// Dilation by generate_binary_structure(3, 2), D times, border value 0.  grid (<= LW_GRID), LW_THREADS threads; a workgroup walks
// the 8 x 8 x 32 tiles of the image.  A tile that does not meet the box `bbox` grown by D (bbox: DEVICE int32[6], lo and hi
// inclusive, of the mask's foreground; NULL: the image) is written as zeros.  Otherwise the tile with a halo of D goes to LDS, a byte
// per voxel (0 outside the image), and is dilated there D times between two buffers: after iteration t a cell is right if it lies t
// cells or more inside the LDS block, so the D-th iteration leaves the tile itself right.  A cell outside the image stays 0 in
// every iteration -- scipy's border_value=0 -- and a cell on the block's rim is not computed (nothing right depends on it).
// Foreground: (mask[v] & andmask) != 0.
template <int D>
__global__ __launch_bounds__(LW_THREADS) void lw_dilate_kernel(const uint8_t* __restrict__ mask, unsigned andmask, LwGeom g,
                                                               const int* __restrict__ bbox, uint8_t* __restrict__ out) {
  constexpr int LX = LW_TX + 2 * D, LY = LW_TY + 2 * D, LZ = LW_TZ + 2 * D, CELLS = LX * LY * LZ;
  __shared__ uint8_t buf[2][CELLS];
  int lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = bbox ? max(bbox[a] - D, 0) : 0;
    hi[a] = bbox ? min(bbox[3 + a] + D, g.F[a] - 1) : g.F[a] - 1;
  }
  const bool box = lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2];
  const int ty_ = threadIdx.x >> 5, tz_ = threadIdx.x & 31;   // the thread's (y, z) column of the tile
  for (int tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    uint32_t q, tz, tx, ty;
    g.tZ.divmod((uint32_t)tile, q, tz);
    g.tY.divmod(q, tx, ty);
    const int x0 = (int)tx * LW_TX, y0 = (int)ty * LW_TY, z0 = (int)tz * LW_TZ;
    const int oy = y0 + ty_, oz = z0 + tz_;
    const bool col = oy < g.F[1] && oz < g.F[2];
    const int nx = min(LW_TX, g.F[0] - x0);
    const int64_t obase = ((int64_t)x0 * g.F[1] + oy) * g.F[2] + oz, ostep = (int64_t)g.F[1] * g.F[2];
    const bool meets = box && x0 <= hi[0] && x0 + LW_TX - 1 >= lo[0] && y0 <= hi[1] && y0 + LW_TY - 1 >= lo[1] && z0 <= hi[2] &&
                       z0 + LW_TZ - 1 >= lo[2];
    bool any = false;
    if (meets) {
      for (int e = threadIdx.x; e < CELLS; e += LW_THREADS) {
        const int lz = e % LZ, t = e / LZ, ly = t % LY, lx = t / LY;
        const int x = x0 - D + lx, y = y0 - D + ly, z = z0 - D + lz;
        const bool in = (unsigned)x < (unsigned)g.F[0] && (unsigned)y < (unsigned)g.F[1] && (unsigned)z < (unsigned)g.F[2];
        const bool fg = in && (mask[((int64_t)x * g.F[1] + y) * g.F[2] + z] & andmask) != 0;
        buf[0][e] = fg;
        any |= fg;
      }
    }
    if (!__syncthreads_or(any)) {   // outside the grown box, or nothing to dilate in reach of the tile (`meets` is uniform)
      if (col)
        for (int lx = 0; lx < nx; ++lx) out[obase + lx * ostep] = 0;
      continue;
    }
#pragma unroll 1
    for (int it = 0; it < D; ++it) {
      const uint8_t* src = buf[it & 1];
      uint8_t* dst = buf[(it + 1) & 1];
      for (int e = threadIdx.x; e < CELLS; e += LW_THREADS) {
        const int lz = e % LZ, t = e / LZ, ly = t % LY, lx = t / LY;
        const int x = x0 - D + lx, y = y0 - D + ly, z = z0 - D + lz;
        const bool in = (unsigned)x < (unsigned)g.F[0] && (unsigned)y < (unsigned)g.F[1] && (unsigned)z < (unsigned)g.F[2];
        const bool rim = lx == 0 || lx == LX - 1 || ly == 0 || ly == LY - 1 || lz == 0 || lz == LZ - 1;
        unsigned v = 0;
        if (in && !rim) {
          constexpr int SX = LY * LZ, SY = LZ;
          const uint8_t* c = src + e;
          // the centre plane's 3 x 3 and the plus-shaped five of the planes before and behind: 19 cells, |dx| + |dy| + |dz| <= 2
          v = c[0] | c[-1] | c[1] | c[-SY] | c[SY] | c[-SY - 1] | c[-SY + 1] | c[SY - 1] | c[SY + 1];
          v |= c[-SX] | c[-SX - 1] | c[-SX + 1] | c[-SX - SY] | c[-SX + SY];
          v |= c[SX] | c[SX - 1] | c[SX + 1] | c[SX - SY] | c[SX + SY];
        }
        dst[e] = (uint8_t)v;
      }
      __syncthreads();
    }
    if (col) {
      const uint8_t* res = buf[D & 1];
      for (int lx = 0; lx < nx; ++lx) out[obase + lx * ostep] = res[((lx + D) * LY + ty_ + D) * LZ + tz_ + D];
    }
    __syncthreads();   // the result is read to the end before the next tile's fill
  }
}

// grid (<= LW_GRID) over the voxels: the roots of the dilated truth's components (comp[v] == v) append themselves; the order is the
// scheduler's and lw_rank_kernel removes it
__global__ __launch_bounds__(LW_THREADS) void lw_roots_kernel(const int* __restrict__ compg, int N, int r, LwCtl* __restrict__ ctl) {
  const int64_t stride = (int64_t)gridDim.x * LW_THREADS;
  for (int64_t v = (int64_t)blockIdx.x * LW_THREADS + threadIdx.x; v < N; v += stride) {
    if (compg[v] != (int)v) continue;
    const unsigned s = atomicAdd(&ctl->nroots[r], 1u);
    if (s < (unsigned)LW_LES) ctl->roots[r][s] = (int)v;
  }
}

// grid (1), LW_LES threads: a lesion's rank is the number of smaller ids; writes the ids into the record's rows in that order and
// rank_of[id] = rank (rank_of: the component labelling's parent array, free by now).  More roots than rows: the overflow bit.
__global__ __launch_bounds__(LW_LES) void lw_rank_kernel(const LwCtl* __restrict__ ctl, int r, int* __restrict__ rank_of, long long* __restrict__ rec) {
  long long* hdr = rec + (int64_t)r * N3D_LW_REGION_WORDS;
  const unsigned n = ctl->nroots[r];
  if (threadIdx.x == 0) hdr[N3D_LW_HDR_LESIONS] = (long long)n;
  if (n > (unsigned)LW_LES) {
    if (threadIdx.x == 0) hdr[N3D_LW_HDR_OVERFLOW] = N3D_LW_OVERFLOW_LESIONS;
    return;
  }
  if (threadIdx.x >= n) return;
  const int id = ctl->roots[r][threadIdx.x];
  int rank = 0;
  for (unsigned j = 0; j < n; ++j) rank += ctl->roots[r][j] < id;
  hdr[N3D_LW_HEADER_WORDS + rank * N3D_LW_ROW_WORDS + N3D_LW_ROW_ID] = id;
  rank_of[id] = rank;
}

// the calling lanes each add 1 to p[i]: the lanes that share the first calling lane's index go as one atomic of their number
__device__ __forceinline__ void lw_add_one(int* __restrict__ p, int i) {
  const int first = __builtin_amdgcn_readfirstlane(i);
  const unsigned long long same = __ballot(i == first);
  if (i == first) {
    if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(p + i, __popcll(same));
  } else {
    atomicAdd(p + i, 1);
  }
}

// grid (<= LW_GRID) over the voxels.  A prediction voxel adds 1 to its component's size and, inside a dilated lesion, sets the
// lesion's bit in its component's match mask (the word is read first: after the first few voxels of a pair no atomic is left); a
// truth voxel adds to its lesion's gt_voxels and, where the prediction is set too, tp -- counted in LDS, one atomic per workgroup
// and nonzero counter.
__global__ __launch_bounds__(LW_THREADS) void lw_match_kernel(const uint8_t* __restrict__ bits, const int* __restrict__ compp,
                                                              const int* __restrict__ compg, const int* __restrict__ rank_of, int N, int r,
                                                              int* __restrict__ psize, unsigned long long* __restrict__ pmatch,
                                                              long long* __restrict__ rec) {
  long long* hdr = rec + (int64_t)r * N3D_LW_REGION_WORDS;
  if (hdr[N3D_LW_HDR_OVERFLOW]) return;
  __shared__ unsigned s_gt[LW_LES], s_tp[LW_LES];
  if (threadIdx.x < LW_LES) s_gt[threadIdx.x] = s_tp[threadIdx.x] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * LW_THREADS;
  for (int64_t v = (int64_t)blockIdx.x * LW_THREADS + threadIdx.x; v < N; v += stride) {
    const int cp = compp[v], cg = compg[v];
    const unsigned b = bits[v];
    if (cp >= 0) lw_add_one(psize, cp);
    if (cg < 0) continue;
    const int l = rank_of[cg] & (LW_LES - 1);
    if (cp >= 0) {
      const unsigned long long bit = 1ull << l;
      if (!(__hip_atomic_load(pmatch + cp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(pmatch + cp, bit);
    }
    if ((b >> (3 + r)) & 1) {
      atomicAdd(s_gt + l, 1u);
      if ((b >> r) & 1) atomicAdd(s_tp + l, 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x < LW_LES) {
    unsigned long long* row = reinterpret_cast<unsigned long long*>(hdr + N3D_LW_HEADER_WORDS + threadIdx.x * N3D_LW_ROW_WORDS);
    if (s_gt[threadIdx.x]) atomicAdd(row + N3D_LW_ROW_GT, (unsigned long long)s_gt[threadIdx.x]);
    if (s_tp[threadIdx.x]) atomicAdd(row + N3D_LW_ROW_TP, (unsigned long long)s_tp[threadIdx.x]);
  }
}

// grid (<= LW_GRID) over the voxels, the roots of the prediction's components: a component without a matched lesion is a false
// positive, the others add their size and 1 to every lesion of their mask.  LDS sums, then one atomic per workgroup and nonzero sum.
__global__ __launch_bounds__(LW_THREADS) void lw_components_kernel(const int* __restrict__ compp, const int* __restrict__ psize,
                                                                   const unsigned long long* __restrict__ pmatch, int N, int r,
                                                                   long long* __restrict__ rec) {
  long long* hdr = rec + (int64_t)r * N3D_LW_REGION_WORDS;
  if (hdr[N3D_LW_HDR_OVERFLOW]) return;
  __shared__ unsigned long long s_pv[LW_LES], s_tot[3];
  __shared__ unsigned s_nm[LW_LES];
  if (threadIdx.x < LW_LES) { s_pv[threadIdx.x] = 0; s_nm[threadIdx.x] = 0; }
  if (threadIdx.x < 3) s_tot[threadIdx.x] = 0;
  __syncthreads();
  unsigned n = 0, nfp = 0;
  unsigned long long fpv = 0;
  const int64_t stride = (int64_t)gridDim.x * LW_THREADS;
  for (int64_t v = (int64_t)blockIdx.x * LW_THREADS + threadIdx.x; v < N; v += stride) {
    if (compp[v] != (int)v) continue;
    const unsigned long long s = (unsigned)psize[v];
    unsigned long long m = pmatch[v];
    n += 1;
    if (!m) { nfp += 1; fpv += s; }
    while (m) {   // <= 64 rounds: each clears a bit
      const int l = __ffsll((long long)m) - 1;
      m &= m - 1;
      atomicAdd(s_pv + l, s);
      atomicAdd(s_nm + l, 1u);
    }
  }
  if (n) atomicAdd(s_tot + 0, (unsigned long long)n);
  if (nfp) { atomicAdd(s_tot + 1, (unsigned long long)nfp); atomicAdd(s_tot + 2, fpv); }
  __syncthreads();
  unsigned long long* h = reinterpret_cast<unsigned long long*>(hdr);
  if (threadIdx.x < LW_LES) {
    unsigned long long* row = h + N3D_LW_HEADER_WORDS + threadIdx.x * N3D_LW_ROW_WORDS;
    if (s_nm[threadIdx.x]) {
      atomicAdd(row + N3D_LW_ROW_PRED, s_pv[threadIdx.x]);
      atomicAdd(row + N3D_LW_ROW_MATCHED, (unsigned long long)s_nm[threadIdx.x]);
    }
  }
  if (threadIdx.x < 3 && s_tot[threadIdx.x]) atomicAdd(h + N3D_LW_HDR_COMPONENTS + threadIdx.x, s_tot[threadIdx.x]);
}

// The lanes with `take` set append (coord, rank) to a list of LW_CAP entries, the entry's distance starting as "none": one atomic per
// wave for the slots, an entry past the capacity is dropped.  Called by whole waves.
__device__ __forceinline__ void lw_append(bool take, uint32_t coord, uint32_t rank, unsigned* __restrict__ count, uint32_t* __restrict__ lc,
                                          uint32_t* __restrict__ lr, int32_t* __restrict__ ld) {
  const unsigned long long m = __ballot(take);
  if (!m) return;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
  unsigned base = 0;
  if (lane == leader) base = atomicAdd(count, (unsigned)__popcll(m));
  base = __shfl(base, leader, 64);
  const unsigned slot = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
  if (take && slot < (unsigned)LW_CAP) {
    lc[slot] = coord;
    lr[slot] = rank;
    ld[slot] = INT32_MAX;
  }
}

// grid (<= LW_GRID) over the voxels, whole waves per iteration.  A truth-surface voxel of region r becomes an entry (coordinate, its
// lesion's rank); a prediction-surface voxel one entry per lesion of its component's mask (none: a false positive's surface takes
// part in no distance).
__global__ __launch_bounds__(LW_THREADS) void lw_compact_kernel(const uint8_t* __restrict__ surf, const int* __restrict__ compp,
                                                                const int* __restrict__ compg, const int* __restrict__ rank_of,
                                                                const unsigned long long* __restrict__ pmatch, LwGeom g, int r,
                                                                LwCtl* __restrict__ ctl, LwLists L, const long long* __restrict__ rec) {
  if (rec[(int64_t)r * N3D_LW_REGION_WORDS + N3D_LW_HDR_OVERFLOW]) return;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * LW_THREADS;
  for (int64_t base = (int64_t)blockIdx.x * LW_THREADS + (threadIdx.x & ~63); base < g.N; base += stride) {
    const int64_t v = base + lane;
    const unsigned s = v < g.N ? surf[v] : 0u;
    const bool isg = (s >> (3 + r)) & 1, isp = (s >> r) & 1;
    if (!__ballot(isg || isp)) continue;
    uint32_t coord = 0;
    if (isg || isp) {
      int x, y, z;
      lw_decode(g, (int)v, x, y, z);
      coord = lw_pack(x, y, z);
    }
    uint32_t gl = 0;
    if (isg) {
      const int cg = compg[v];
      gl = cg >= 0 ? (uint32_t)(rank_of[cg] & (LW_LES - 1)) : 0u;
    }
    lw_append(isg, coord, gl, &ctl->ng[r], L.gcoord, L.grank, L.gdist);
    unsigned long long m = 0;
    if (isp) {
      const int cp = compp[v];
      m = cp >= 0 ? pmatch[cp] : 0ull;
    }
    while (__ballot(m != 0)) {   // <= 64 rounds: each clears a bit of every lane that has one
      const bool has = m != 0;
      const uint32_t l = has ? (uint32_t)(__ffsll((long long)m) - 1) : 0u;
      m &= m - 1;
      lw_append(has, coord, l, &ctl->np[r], L.pcoord, L.prank, L.pdist);
    }
  }
}

// grid (LW_DGRID, 2), LW_THREADS threads.  Side 0: every truth entry's squared distance to the nearest prediction entry of the same
// lesion; side 1 the other way round.  Brute force.  A piece of work is a chunk of LW_THREADS entries of the side's own list (a
// thread keeps one) against a slice of the other list's tiles of LW_DTILE entries (tile t belongs to slice t % slices); the slices
// are as many as the grid has workgroups per chunk, so a short list still fills the chip.  A tile passes through LDS and every lane
// reads the same word (a broadcast); a piece ends in one atomicMin per entry onto the "none" the entry was appended with.  A list
// that passed its capacity: the overflow bits, and no distance.
__global__ __launch_bounds__(LW_THREADS) void lw_distance_kernel(const LwCtl* __restrict__ ctl, int r, LwLists L, long long* __restrict__ rec) {
  long long* hdr = rec + (int64_t)r * N3D_LW_REGION_WORDS;
  if (hdr[N3D_LW_HDR_OVERFLOW] & N3D_LW_OVERFLOW_LESIONS) return;
  const unsigned ng = ctl->ng[r], np = ctl->np[r];
  if (ng > (unsigned)LW_CAP || np > (unsigned)LW_CAP) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
      hdr[N3D_LW_HDR_OVERFLOW] = (ng > (unsigned)LW_CAP ? N3D_LW_OVERFLOW_TRUTH_SURFACE : 0) | (np > (unsigned)LW_CAP ? N3D_LW_OVERFLOW_PRED_SURFACE : 0);
    return;
  }
  const bool side = blockIdx.y != 0;
  const int na = (int)(side ? np : ng), nb = (int)(side ? ng : np);
  if (na == 0 || nb == 0) return;
  const uint32_t *ac = side ? L.pcoord : L.gcoord, *ar = side ? L.prank : L.grank;
  const uint32_t *bc = side ? L.gcoord : L.pcoord, *br = side ? L.grank : L.prank;
  int32_t* ad = side ? L.pdist : L.gdist;
  const int nchunks = (na + LW_THREADS - 1) / LW_THREADS, ntiles = (nb + LW_DTILE - 1) / LW_DTILE;   // both <= LW_CAP / 256 = 1024
  const int slices = min(max((int)gridDim.x / nchunks, 1), ntiles);
  __shared__ uint2 tile[LW_DTILE];
  for (int w = blockIdx.x; w < nchunks * slices; w += gridDim.x) {   // uniform in the workgroup
    const int slice = w / nchunks, i = (w - slice * nchunks) * LW_THREADS + threadIdx.x;
    const bool have = i < na;
    const uint32_t c = have ? ac[i] : 0u, l = have ? ar[i] : LW_NO_RANK;
    int best = INT32_MAX;
    for (int t = slice; t < ntiles; t += slices) {
      __syncthreads();   // the tile before is read to the end
      for (int q = threadIdx.x; q < LW_DTILE; q += LW_THREADS) {
        const int j = t * LW_DTILE + q;
        tile[q] = j < nb ? make_uint2(bc[j], br[j]) : make_uint2(0u, LW_NO_RANK - 1u);
      }
      __syncthreads();
      const int cnt = min(LW_DTILE, nb - t * LW_DTILE);
      for (int q = 0; q < cnt; ++q) {
        const uint2 e = tile[q];
        if (e.y == l) best = min(best, lw_d2(c, e.x));
      }
    }
    if (have && best != INT32_MAX) atomicMin(ad + i, best);
  }
}

// sum of a and minimum of b over the workgroup, in every thread; s: two words of LDS
__device__ __forceinline__ void lw_block_sum_min(unsigned& a, unsigned& b, unsigned* s) {
  __syncthreads();   // the words' last readers are done
  if (threadIdx.x == 0) { s[0] = 0; s[1] = 0xFFFFFFFFu; }
  __syncthreads();
  if (a) atomicAdd(s + 0, a);
  if (b != 0xFFFFFFFFu) atomicMin(s + 1, b);
  __syncthreads();
  a = s[0];
  b = s[1];
}

// grid (N3D_LW_MAX_LESIONS), LW_THREADS threads: workgroup l takes lesion l's distances -- the entries of both lists with rank l
// and a distance -- and writes n, D[k], D[min(k + 1, n - 1)] and max D, k = floor((n - 1) * 0.95) formed as one fp64 product.
// D[k] is the smallest t with |{d <= t}| >= k + 1, found by bisection on [0, max D]; D[k + 1] is t again when |{d <= t}| >= k + 2
// and the smallest distance above t otherwise.
__global__ __launch_bounds__(LW_THREADS) void lw_order_kernel(const LwCtl* __restrict__ ctl, int r, LwLists L, long long* __restrict__ rec) {
  long long* hdr = rec + (int64_t)r * N3D_LW_REGION_WORDS;
  const int l = blockIdx.x;
  if (hdr[N3D_LW_HDR_OVERFLOW] || (long long)l >= hdr[N3D_LW_HDR_LESIONS]) return;
  const int ng = (int)min(ctl->ng[r], (unsigned)LW_CAP), np = (int)min(ctl->np[r], (unsigned)LW_CAP);
  __shared__ unsigned s[2];
  // count of the lesion's distances <= t and the smallest one above t
  auto scan = [&](unsigned t, unsigned& cnt, unsigned& above) {
    cnt = 0;
    above = 0xFFFFFFFFu;
    for (int side = 0; side < 2; ++side) {
      const int n = side ? np : ng;
      const uint32_t* rk = side ? L.prank : L.grank;
      const int32_t* d = side ? L.pdist : L.gdist;
      for (int i = threadIdx.x; i < n; i += LW_THREADS) {
        if (rk[i] != (uint32_t)l) continue;
        const int v = d[i];
        if (v == INT32_MAX) continue;   // no entry of the lesion on the other side
        if ((unsigned)v <= t) cnt += 1;
        else above = min(above, (unsigned)v);
      }
    }
    lw_block_sum_min(cnt, above, s);
  };
  unsigned n, unused;
  scan(0x7FFFFFFFu, n, unused);
  if (n == 0) return;   // no matched component: no distance, the row's order statistics stay 0
  // the maximum: the complement trick keeps the helper to a sum and a minimum
  unsigned zero = 0, negmax = 0xFFFFFFFFu;
  for (int side = 0; side < 2; ++side) {
    const int m = side ? np : ng;
    const uint32_t* rk = side ? L.prank : L.grank;
    const int32_t* d = side ? L.pdist : L.gdist;
    for (int i = threadIdx.x; i < m; i += LW_THREADS)
      if (rk[i] == (uint32_t)l && d[i] != INT32_MAX) negmax = min(negmax, 0x7FFFFFFFu - (unsigned)d[i]);
  }
  lw_block_sum_min(zero, negmax, s);
  const unsigned dmax = 0x7FFFFFFFu - negmax;
  const unsigned k = (unsigned)floor((double)(n - 1) * 0.95), k1 = k + 1 < n ? k + 1 : n - 1;
  unsigned lo = 0, hi = dmax;
  while (lo < hi) {   // <= 31 rounds; lo and hi are the same in every thread
    const unsigned mid = lo + ((hi - lo) >> 1);
    unsigned cnt, above;
    scan(mid, cnt, above);
    if (cnt >= k + 1) hi = mid;
    else lo = mid + 1;
  }
  unsigned cnt, above;
  scan(lo, cnt, above);
  if (threadIdx.x == 0) {
    long long* row = hdr + N3D_LW_HEADER_WORDS + l * N3D_LW_ROW_WORDS;
    row[N3D_LW_ROW_N] = n;
    row[N3D_LW_ROW_DK] = lo;
    row[N3D_LW_ROW_DK1] = cnt >= k1 + 1 ? lo : above;
    row[N3D_LW_ROW_DMAX] = dmax;
  }
}

}  // namespace n3d

using namespace n3d;

static inline int64_t lw_up256(int64_t b) { return (b + 255) & ~(int64_t)255; }
static inline unsigned lw_blocks(int64_t n) {
  const int64_t b = cdiv(n, LW_THREADS);
  return (unsigned)(b < 1 ? 1 : (b > LW_GRID ? LW_GRID : b));
}

static int lw_geom(const int32_t* full, const char* what, LwGeom* g) {
  N3D_CHECK_ARG(full && full[0] > 0 && full[1] > 0 && full[2] > 0, "%s: bad image shape", what);
  const int64_t N = (int64_t)full[0] * full[1] * full[2];
  N3D_CHECK_ARG(N < (1ll << 31), "%s: image (%d, %d, %d) = %lld voxels: the index arithmetic needs FX * FY * FZ < 2^31", what, full[0],
                full[1], full[2], (long long)N);
  g->N = (int)N;
  for (int a = 0; a < 3; ++a) { g->F[a] = g->B[a] = full[a]; g->O[a] = 0; }
  const int64_t tx = cdiv(full[0], LW_TX), ty = cdiv(full[1], LW_TY), tz = cdiv(full[2], LW_TZ);
  g->ntiles = (int)(tx * ty * tz);
  g->fY = FastDiv((uint32_t)full[1]);
  g->fZ = FastDiv((uint32_t)full[2]);
  g->tY = FastDiv((uint32_t)ty);
  g->tZ = FastDiv((uint32_t)tz);
  return N3D_OK;
}

static int lw_dilate_launch(const uint8_t* mask, unsigned andmask, const LwGeom& g, const int* bbox, int iterations, uint8_t* out, hipStream_t s) {
  const dim3 grid((unsigned)(g.ntiles < LW_GRID ? g.ntiles : LW_GRID)), block(LW_THREADS);
  switch (iterations) {
    case 0: N3D_LAUNCH(lw_dilate_kernel<0>, grid, block, 0, s, mask, andmask, g, bbox, out); break;
    case 1: N3D_LAUNCH(lw_dilate_kernel<1>, grid, block, 0, s, mask, andmask, g, bbox, out); break;
    case 2: N3D_LAUNCH(lw_dilate_kernel<2>, grid, block, 0, s, mask, andmask, g, bbox, out); break;
    case 3: N3D_LAUNCH(lw_dilate_kernel<3>, grid, block, 0, s, mask, andmask, g, bbox, out); break;
    case 4: N3D_LAUNCH(lw_dilate_kernel<4>, grid, block, 0, s, mask, andmask, g, bbox, out); break;
    default: N3D_LAUNCH(lw_dilate_kernel<5>, grid, block, 0, s, mask, andmask, g, bbox, out);
  }
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" size_t n3d_lw_workspace_bytes(int FX, int FY, int FZ, int64_t* offsets) {
  if (FX <= 0 || FY <= 0 || FZ <= 0 || (int64_t)FX * FY * FZ >= (1ll << 31)) return 0;
  const int64_t N = (int64_t)FX * FY * FZ;
  int64_t o[N3D_LW_WS_PARTS + 1];
  const int64_t sizes[N3D_LW_WS_PARTS] = {N, N, N, N, 4 * N, 4 * N, 4 * N, 4 * N, 8 * N, 6 * 4 * (int64_t)LW_CAP, (int64_t)sizeof(LwCtl)};
  o[0] = 0;
  for (int k = 0; k < N3D_LW_WS_PARTS; ++k) o[k + 1] = o[k] + lw_up256(sizes[k]);
  if (offsets)
    for (int k = 0; k < N3D_LW_WS_PARTS; ++k) offsets[k] = o[k];
  return (size_t)o[N3D_LW_WS_PARTS];
}

extern "C" int n3d_lw_dilate(const uint8_t* mask, const int32_t* full, const int32_t* bbox, int iterations, uint8_t* out, void* stream) {
  LwGeom g;
  if (int e = lw_geom(full, "lw_dilate", &g)) return e;
  N3D_CHECK_ARG(mask && out && mask != out, "lw_dilate: bad args");
  N3D_CHECK_ARG(iterations >= 0 && iterations <= N3D_LW_MAX_DILATION, "lw_dilate: %d iterations: must lie in 0 .. %d (N3D_LW_MAX_DILATION)",
                iterations, N3D_LW_MAX_DILATION);
  N3D_CHECK_ARG((reinterpret_cast<uintptr_t>(bbox) & 3) == 0, "lw_dilate: bbox must be 4-byte aligned");
  return lw_dilate_launch(mask, 0xFFu, g, bbox, iterations, out, (hipStream_t)stream);
}

extern "C" int n3d_lw_phases(int first, int last, const uint8_t* pred, const uint8_t* truth, const int32_t* full, const int32_t* box,
                             const int32_t* origin, int dilation, void* workspace, int64_t* rec, void* stream) {
  LwGeom g;
  if (int e = lw_geom(full, "lw_score", &g)) return e;
  N3D_CHECK_ARG(pred && truth && box && origin && workspace && rec, "lw_score: bad args");
  N3D_CHECK_ARG(((reinterpret_cast<uintptr_t>(rec) | reinterpret_cast<uintptr_t>(workspace)) & 7) == 0,
                "lw_score: workspace and rec must be 8-byte aligned");
  N3D_CHECK_ARG(dilation >= 0 && dilation <= N3D_LW_MAX_DILATION, "lw_score: dilation %d: must lie in 0 .. %d (N3D_LW_MAX_DILATION)", dilation,
                N3D_LW_MAX_DILATION);
  N3D_CHECK_ARG(0 <= first && first <= last && last < N3D_LW_PHASES, "lw_score: phases %d .. %d: must lie in 0 .. %d", first, last, N3D_LW_PHASES - 1);
  for (int a = 0; a < 3; ++a) {
    N3D_CHECK_ARG(box[a] > 0 && origin[a] >= 0 && origin[a] + box[a] <= full[a],
                  "lw_score: the truth box %d at %d on axis %d is not inside the image (%d)", box[a], origin[a], a, full[a]);
    if (full[a] > N3D_LW_MAX_AXIS)
      N3D_UNSUPPORTED("lw_score: image (%d, %d, %d): axis %d is %d long, the packed surface coordinates take axes up to %d", full[0], full[1],
                      full[2], a, full[a], N3D_LW_MAX_AXIS);
    g.B[a] = box[a]; g.O[a] = origin[a];
  }
  int64_t off[N3D_LW_WS_PARTS];
  n3d_lw_workspace_bytes(full[0], full[1], full[2], off);
  char* ws = static_cast<char*>(workspace);
  uint8_t *bits = reinterpret_cast<uint8_t*>(ws + off[0]), *surf = reinterpret_cast<uint8_t*>(ws + off[1]), *gd = reinterpret_cast<uint8_t*>(ws + off[2]),
          *pm = reinterpret_cast<uint8_t*>(ws + off[3]);
  int32_t *parent = reinterpret_cast<int32_t*>(ws + off[4]), *compp = reinterpret_cast<int32_t*>(ws + off[5]),
          *compg = reinterpret_cast<int32_t*>(ws + off[6]), *psize = reinterpret_cast<int32_t*>(ws + off[7]);
  unsigned long long* pmatch = reinterpret_cast<unsigned long long*>(ws + off[8]);
  uint32_t* lists = reinterpret_cast<uint32_t*>(ws + off[9]);
  LwCtl* ctl = reinterpret_cast<LwCtl*>(ws + off[10]);
  LwLists L;
  L.gcoord = lists; L.grank = lists + LW_CAP; L.pcoord = lists + 2 * LW_CAP; L.prank = lists + 3 * LW_CAP;
  L.gdist = reinterpret_cast<int32_t*>(lists + 4 * LW_CAP); L.pdist = reinterpret_cast<int32_t*>(lists + 5 * LW_CAP);
  long long* rc = reinterpret_cast<long long*>(rec);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(lw_blocks(g.N)), block(LW_THREADS);
  for (int phase = first; phase <= last; ++phase) {
    if (phase == 0) {
      N3D_LAUNCH(lw_init_kernel, dim3(1), block, 0, s, rc, ctl);
    } else if (phase == 1) {
      N3D_LAUNCH(lw_prep_kernel, grid, block, 0, s, pred, truth, g, bits, surf, ctl);
    } else {
      const int r = (phase - 2) / N3D_LW_REGION_PHASES, step = (phase - 2) % N3D_LW_REGION_PHASES;
      switch (step) {
        case 0: N3D_LAUNCH(lw_select_kernel, grid, block, 0, s, bits, g.N, r, pm, psize, pmatch); break;
        case 1:
          if (int e = n3d_cc_label(pm, full, 26, parent, compp, stream)) return e;
          break;
        case 2:
          if (int e = lw_dilate_launch(bits, 8u << r, g, &ctl->tbbox[r][0], dilation, gd, s)) return e;
          break;
        case 3:
          if (int e = n3d_cc_label(gd, full, 26, parent, compg, stream)) return e;
          break;
        case 4: N3D_LAUNCH(lw_roots_kernel, grid, block, 0, s, compg, g.N, r, ctl); break;
        case 5: N3D_LAUNCH(lw_rank_kernel, dim3(1), dim3(LW_LES), 0, s, ctl, r, parent, rc); break;
        case 6: N3D_LAUNCH(lw_match_kernel, grid, block, 0, s, bits, compp, compg, parent, g.N, r, psize, pmatch, rc); break;
        case 7: N3D_LAUNCH(lw_components_kernel, grid, block, 0, s, compp, psize, pmatch, g.N, r, rc); break;
        case 8: N3D_LAUNCH(lw_compact_kernel, grid, block, 0, s, surf, compp, compg, parent, pmatch, g, r, ctl, L, rc); break;
        case 9: N3D_LAUNCH(lw_distance_kernel, dim3(LW_DGRID, 2), block, 0, s, ctl, r, L, rc); break;
        default: N3D_LAUNCH(lw_order_kernel, dim3(LW_LES), block, 0, s, ctl, r, L, rc);
      }
    }
    N3D_LAUNCH_CHECK();
  }
  return N3D_OK;
}

extern "C" int n3d_lw_score(const uint8_t* pred, const uint8_t* truth, const int32_t* full, const int32_t* box, const int32_t* origin,
                            int dilation, void* workspace, int64_t* rec, void* stream) {
  return n3d_lw_phases(0, N3D_LW_PHASES - 1, pred, truth, full, box, origin, dilation, workspace, rec, stream);
}
