// Label clean-up (include/n3d.h, "Label clean-up"): 3-D connected components of a label volume's foreground at connectivity 6 / 18 /
// 26 and the two BraTS clean-up rules on them, without the volume leaving the device.  A component's id is the smallest linear
// index (x * FY + y) * FZ + z of its voxels, so the result does not depend on the order in which anything runs.  Union-find on an
// int32 parent array; integer work and integer atomics (min / add / max) throughout: the same inputs give the same bits.
//
// Termination.  No kernel waits for another workgroup.  Every pointer walk follows parent[] to strictly smaller indices, and every
// round of a union strictly lowers the larger index of its pair, so both are bounded by the index they start from; the wave loop
// that aggregates the size counts retires at least one lane per round (<= 64); everything else is a grid-stride loop.
// Races.  While unions run (local and merge phase) parent[] is read with relaxed atomic loads and written with atomicMin only
// ("is foreground" is the sign of a word, which never changes: the merge phase tests it with plain loads).
// The union does not rely on those loads being fresh: every value ever stored in parent[v] is a voxel of v's component and <= v, so
// a walk from an older value still ends inside the component, and the atomicMin that follows returns the word's true content.
#include "n3d_common.h"

namespace n3d {

// The tile of the local phase: 8 x 8 x 32 voxels (z, the contiguous axis, longest).  Its labels take 8 KB of LDS and a workgroup
// has 256 threads, so LDS (160 KB per CU) and the wave slots both allow 8 workgroups per CU; 2048 voxels keep 56 % of a tile's
// voxels on its faces, and a 32-byte z run per row is the smallest piece a load still fetches whole.
constexpr int CC_TXS = 3, CC_TYS = 3, CC_TZS = 5;
constexpr int CC_TX = 1 << CC_TXS, CC_TY = 1 << CC_TYS, CC_TZ = 1 << CC_TZS, CC_TILE = CC_TX * CC_TY * CC_TZ;
constexpr int CC_THREADS = CC_TY * CC_TZ;   // a thread per (y, z) column of the tile, CC_TX voxels each
constexpr int CC_WAVES = CC_THREADS / 64;
constexpr int CC_LOCAL_GRID = 1024, CC_GRID = 1024;
constexpr int CC_UNROLL = 4;   // voxels per thread and iteration of the streaming launches: independent loads in flight

struct CcGeom {
  int N;          // FX * FY * FZ < 2^31
  int F[3];
  int ntiles;
  FastDiv fY, fZ, tY, tZ;   // image and tile-grid decoding
};

// The forward half of the 3 x 3 x 3 neighbourhood: offset k = 0 .. 12 is cell 14 + k of the cube in (dx, dy, dz) order, the cells
// behind the centre -- (dx, dy, dz) lexicographically positive.  Level ND keeps the offsets of Manhattan length <= ND: 3, 9 or 13
// of them, the forward halves of generate_binary_structure(3, ND).
__device__ __forceinline__ constexpr int cc_dx(int k) { return (14 + k) / 9 - 1; }
__device__ __forceinline__ constexpr int cc_dy(int k) { return ((14 + k) / 3) % 3 - 1; }
__device__ __forceinline__ constexpr int cc_dz(int k) { return (14 + k) % 3 - 1; }
__device__ __forceinline__ constexpr bool cc_in_level(int k, int nd) {
  return (cc_dx(k) != 0) + (cc_dy(k) != 0) + (cc_dz(k) != 0) <= nd;
}

template <bool LDS>
__device__ __forceinline__ int cc_ld(const int* p) {
  return LDS ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
             : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// a >= 0 a foreground voxel: follows parent[] while it leads to a smaller index (bounded by a)
template <bool LDS>
__device__ __forceinline__ int cc_find(const int* parent, int a) {
  for (;;) {
    const int q = cc_ld<LDS>(parent + a);
    if (q >= a || q < 0) return a;
    a = q;
  }
}
// Unites the components of the foreground voxels a and b.  Each round orders the pair as a > b and lowers parent[a] to b at most:
// `old == a`: a was a root and now hangs under b; `old == b`: the link was there; otherwise parent[a] = min(old, b) keeps a with
// one of the two and (old, b), both smaller than a, is what is left to unite.
template <bool LDS>
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
  a = cc_find<LDS>(parent, a);
  b = cc_find<LDS>(parent, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);
    if (old == a || old == b) break;
    a = old;
  }
}

// Local phase.  grid (<= CC_LOCAL_GRID), CC_THREADS threads; a workgroup walks tiles.  lab[] holds, per voxel of the tile, the
// local index of its parent (-1: background or outside the image); local indices order a tile's voxels as the image's linear
// indices do, so the local root is the tile component's smallest image index.  Writes parent[] for every voxel of the image
// (-1 on background) and clears the counters of the later phases.
template <int ND>
__global__ __launch_bounds__(CC_THREADS) void cc_local_kernel(const uint8_t* __restrict__ mask, CcGeom g, int* __restrict__ parent,
                                                              int* __restrict__ size, int* __restrict__ et, long long* __restrict__ rec) {
  __shared__ int lab[CC_TILE];
  if (rec && blockIdx.x == 0 && threadIdx.x < N3D_CC_REC_WORDS) rec[threadIdx.x] = 0;
  const int ly = threadIdx.x >> CC_TZS, lz = threadIdx.x & (CC_TZ - 1);
  for (int tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    uint32_t q, tz, tx, ty;
    g.tZ.divmod((uint32_t)tile, q, tz);
    g.tY.divmod(q, tx, ty);
    const int x0 = (int)tx << CC_TXS, y = ((int)ty << CC_TYS) + ly, z = ((int)tz << CC_TZS) + lz;
    const bool col = y < g.F[1] && z < g.F[2];
    const int nx = min(CC_TX, g.F[0] - x0);
    const int64_t gbase = ((int64_t)x0 * g.F[1] + y) * g.F[2] + z, gstep = (int64_t)g.F[1] * g.F[2];
    // A z row of the tile is half a wave: the ballot of the row gives every voxel the start of its run of foreground along z, and
    // the row starts as those runs -- the unions of offset (0, 0, 1) cost nothing.
    unsigned fgm = 0, prevm = 0;   // bit lx: the voxel is foreground / its z predecessor in the tile is
#pragma unroll
    for (int lx = 0; lx < CC_TX; ++lx) {
      const int i = lx * CC_THREADS + threadIdx.x;
      const bool fg = col && lx < nx && mask[gbase + lx * gstep];
      const uint32_t row = (uint32_t)(__ballot(fg) >> (threadIdx.x & 32));
      const uint32_t gaps = ~row & ((1u << lz) - 1u);
      lab[i] = fg ? i - lz + (gaps ? 32 - __clz(gaps) : 0) : -1;
      fgm |= (unsigned)fg << lx;
      prevm |= (lz > 0 ? (row >> (lz - 1)) & 1u : 0u) << lx;
    }
    if (!__syncthreads_or(fgm != 0)) {   // no foreground in the tile (most tiles of a subject)
      if (col)
        for (int lx = 0; lx < nx; ++lx) {
          const int64_t v = gbase + lx * gstep;
          parent[v] = -1;
          if (size) { size[v] = 0; et[v] = 0; }
        }
      __syncthreads();   // lab[] is rewritten by the next tile's fill
      continue;
    }
    // Offset k joins i and j.  When the z predecessors of both are foreground and in the tile they lie in the runs of i and j, and
    // the same offset joins them: the pair is left to the voxel before (by induction to the first pair of the two runs).
#pragma unroll
    for (int lx = 0; lx < CC_TX; ++lx) {
      const int i = lx * CC_THREADS + threadIdx.x;
      if (!((fgm >> lx) & 1)) continue;
      const bool prev = (prevm >> lx) & 1;
#pragma unroll
      for (int k = 1; k < 13; ++k) {
        if (!cc_in_level(k, ND)) continue;
        const int jx = lx + cc_dx(k), jy = ly + cc_dy(k), jz = lz + cc_dz(k);
        if (jx >= CC_TX || (unsigned)jy >= (unsigned)CC_TY || (unsigned)jz >= (unsigned)CC_TZ) continue;
        const int j = (jx * CC_TY + jy) * CC_TZ + jz;
        if (cc_ld<true>(lab + j) < 0) continue;
        if (prev && jz > 0 && cc_ld<true>(lab + j - 1) >= 0) continue;
        cc_union<true>(lab, i, j);
      }
    }
    __syncthreads();
    if (col) {
      for (int lx = 0; lx < nx; ++lx) {
        const int i = lx * CC_THREADS + threadIdx.x;
        int p = -1;
        if (lab[i] >= 0) {
          const int r = cc_find<true>(lab, i);
          const int rx = r >> (CC_TYS + CC_TZS), ry = (r >> CC_TZS) & (CC_TY - 1), rz = r & (CC_TZ - 1);
          p = (int)(gbase + (int64_t)rx * gstep + (int64_t)(ry - ly) * g.F[2] + (rz - lz));
        }
        const int64_t v = gbase + lx * gstep;
        parent[v] = p;
        if (size) { size[v] = 0; et[v] = 0; }
      }
    }
    __syncthreads();   // the tile's labels are read to the end before the next tile's fill
  }
}

// The local phase of the global-only variant (N3D_CC_GLOBAL_ONLY, kept for the comparison in profiles/postprocess_probe.log): every
// foreground voxel its own root, nothing united.
__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(const uint8_t* __restrict__ mask, int N, int* __restrict__ parent,
                                                             int* __restrict__ size, int* __restrict__ et, long long* __restrict__ rec) {
  if (rec && blockIdx.x == 0 && threadIdx.x < N3D_CC_REC_WORDS) rec[threadIdx.x] = 0;
  const int64_t stride = (int64_t)gridDim.x * CC_THREADS;
  for (int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; v < N; v += stride) {
    parent[v] = mask[v] ? (int)v : -1;
    if (size) { size[v] = 0; et[v] = 0; }
  }
}

// Merge phase.  grid (<= CC_GRID), grid stride over the voxels.  A foreground voxel on a face of its tile unites with its foreground
// forward neighbours in OTHER tiles (pairs inside a tile were united in LDS).  Neighbours by coordinate: the bounds are tested per axis.
// ALL (the global-only variant): every voxel, every forward neighbour.
template <int ND, bool ALL>
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(CcGeom g, int* parent) {
  const int64_t stride = (int64_t)gridDim.x * CC_THREADS;
  for (int64_t vv = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; vv < g.N; vv += stride) {
    const int v = (int)vv;
    // "is foreground" is the sign of the word, which never changes: plain loads, all of a voxel's requested before any union
    auto fg = [&](int i) { return parent[i] >= 0; };
    if (!fg(v)) continue;
    uint32_t q, uz, ux, uy;
    g.fZ.divmod((uint32_t)v, q, uz);
    g.fY.divmod(q, ux, uy);
    const int x = (int)ux, y = (int)uy, z = (int)uz;
    const int lx = x & (CC_TX - 1), ly = y & (CC_TY - 1), lz = z & (CC_TZ - 1);
    if (!ALL && lx != CC_TX - 1 && ly != 0 && ly != CC_TY - 1 && lz != 0 && lz != CC_TZ - 1) continue;
    // As in the local phase: a pair whose z predecessors are foreground in the same two tiles is left to that pair (the local phase
    // united each voxel with its predecessor); the global-only variant has no runs to lean on.
    const bool prev = !ALL && lz > 0 && fg(v - 1);
    unsigned need = 0;
#pragma unroll
    for (int k = 0; k < 13; ++k) {
      if (!cc_in_level(k, ND)) continue;
      const int nx = x + cc_dx(k), ny = y + cc_dy(k), nz = z + cc_dz(k);
      if (nx >= g.F[0] || (unsigned)ny >= (unsigned)g.F[1] || (unsigned)nz >= (unsigned)g.F[2]) continue;
      if (!ALL && (nx >> CC_TXS) == (x >> CC_TXS) && (ny >> CC_TYS) == (y >> CC_TYS) && (nz >> CC_TZS) == (z >> CC_TZS)) continue;
      const int n = v + (cc_dx(k) * g.F[1] + cc_dy(k)) * g.F[2] + cc_dz(k);
      if (!fg(n)) continue;
      if (prev && (nz & (CC_TZ - 1)) > 0 && fg(n - 1)) continue;
      need |= 1u << k;
    }
#pragma unroll
    for (int k = 0; k < 13; ++k) {
      if (!cc_in_level(k, ND)) continue;
      if ((need >> k) & 1) cc_union<false>(parent, v, v + (cc_dx(k) * g.F[1] + cc_dy(k)) * g.F[2] + cc_dz(k));
    }
  }
}

// Flatten phase.  grid (<= CC_GRID).  parent[] is only read here (every chain is strictly decreasing behind the launch boundary, so
// the walk ends on the component's smallest index) and comp[] only written.  COUNT: size[root] += 1 per voxel and et[root] += 1 per
// label-4 voxel, aggregated: per round the lanes that share the first open lane's root go as one count; a wave carries the count of
// its current root across its iterations and adds it when the root changes and at the end -- a component that fills the image
// costs one atomic per wave, not one per voxel.
template <bool COUNT>
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(const int* __restrict__ parent, const uint8_t* __restrict__ labels, int N,
                                                                int* __restrict__ comp, int* __restrict__ size, int* __restrict__ et) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * CC_THREADS;
  int carry_root = -1, carry_n = 0, carry_e = 0;
  auto flush = [&]() {
    if (carry_root >= 0 && lane == 0) {
      atomicAdd(size + carry_root, carry_n);
      if (carry_e) atomicAdd(et + carry_root, carry_e);
    }
  };
  // CC_UNROLL voxels per lane and iteration, a grid stride apart, their words requested together
  for (int64_t base = (int64_t)blockIdx.x * CC_THREADS + (threadIdx.x & ~63); base < N; base += CC_UNROLL * stride) {
    int root[CC_UNROLL];
    bool is4[CC_UNROLL];
#pragma unroll
    for (int u = 0; u < CC_UNROLL; ++u) {
      const int64_t v = base + u * stride + lane;
      root[u] = v < N ? parent[v] : -1;
    }
#pragma unroll
    for (int u = 0; u < CC_UNROLL; ++u) {
      const int64_t v = base + u * stride + lane;
      is4[u] = false;
      if (root[u] >= 0) {
        for (;;) {
          const int q = parent[root[u]];
          if (q >= root[u] || q < 0) break;
          root[u] = q;
        }
        if (COUNT) is4[u] = labels[v] == 4;
      }
      if (v < N) comp[v] = root[u];
    }
    if (COUNT) {
#pragma unroll
      for (int u = 0; u < CC_UNROLL; ++u) {
        unsigned long long todo = __ballot(root[u] >= 0);
        while (todo) {   // <= 64 rounds: each clears the leader's bit at least
          const int first = __shfl(root[u], __ffsll((long long)todo) - 1, 64);
          const unsigned long long same = __ballot(root[u] == first);
          const int n = __popcll(same), e = __popcll(__ballot(root[u] == first && is4[u]));
          todo &= ~same;
          if (first == carry_root) {
            carry_n += n;
            carry_e += e;
          } else {
            flush();
            carry_root = first; carry_n = n; carry_e = e;
          }
        }
      }
    }
  }
  if (COUNT) flush();
}

// sums of a, b, c and the maximum of m over the workgroup, valid in thread 0
__device__ __forceinline__ void cc_block_reduce(unsigned long long& a, unsigned long long& b, unsigned long long& c, unsigned long long& m) {
  __shared__ unsigned long long s[CC_WAVES][4];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    a += __shfl_xor(a, d, 64);
    b += __shfl_xor(b, d, 64);
    c += __shfl_xor(c, d, 64);
    const unsigned long long o = __shfl_xor(m, d, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    s[w][0] = a; s[w][1] = b; s[w][2] = c; s[w][3] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < CC_WAVES; ++w) {
      a += s[w][0]; b += s[w][1]; c += s[w][2];
      m = s[w][3] > m ? s[w][3] : m;
    }
  }
}

// Decide, first launch.  grid (<= CC_GRID) over the root voxels (comp[v] == v): the number of components, the voxels and
// label-4 voxels in them, and the largest size with the smallest id among equals: the maximum of (size << 32) | (0xFFFFFFFF - id).
__global__ __launch_bounds__(CC_THREADS) void cc_decide_max_kernel(const int* __restrict__ comp, const int* __restrict__ size,
                                                                   const int* __restrict__ et, int N, long long* __restrict__ rec) {
  unsigned long long n = 0, vox = 0, e = 0, best = 0;
  const int64_t stride = (int64_t)gridDim.x * CC_THREADS;
  for (int64_t v0 = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; v0 < N; v0 += CC_UNROLL * stride) {
    int c[CC_UNROLL];
#pragma unroll
    for (int u = 0; u < CC_UNROLL; ++u) c[u] = v0 + u * stride < N ? comp[v0 + u * stride] : -1;
#pragma unroll
    for (int u = 0; u < CC_UNROLL; ++u) {
      const int64_t v = v0 + u * stride;
      if (c[u] < 0 || c[u] != (int)v) continue;   // (-1: background or past the end)
      const unsigned long long s = (unsigned)size[v], pk = (s << 32) | (0xFFFFFFFFull - (unsigned)v);
      n += 1; vox += s; e += (unsigned)et[v];
      best = pk > best ? pk : best;
    }
  }
  cc_block_reduce(n, vox, e, best);
  if (threadIdx.x == 0 && n) {
    unsigned long long* r = reinterpret_cast<unsigned long long*>(rec);
    atomicAdd(r + N3D_CC_REC_COMPONENTS, n);
    atomicAdd(r + N3D_CC_REC_VOXELS_IN, vox);
    if (e) atomicAdd(r + N3D_CC_REC_ET_IN, e);
    atomicMax(r + N3D_CC_REC_PACKED, best);
  }
}

// Decide, second launch: the verdict per root -- kept iff size >= min_voxels and (not keep_largest or it is the largest) -- and what
// the kept components hold.
__global__ __launch_bounds__(CC_THREADS) void cc_decide_keep_kernel(const int* __restrict__ comp, const int* __restrict__ size,
                                                                    const int* __restrict__ et, int N, long long min_voxels, int keep_largest,
                                                                    uint8_t* __restrict__ verdict, long long* __restrict__ rec) {
  const unsigned long long packed = (unsigned long long)rec[N3D_CC_REC_PACKED];
  const int largest = (int)(0xFFFFFFFFu - (unsigned)(packed & 0xFFFFFFFFull));
  unsigned long long n = 0, vox = 0, e = 0, unused = 0;
  const int64_t stride = (int64_t)gridDim.x * CC_THREADS;
  for (int64_t v0 = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; v0 < N; v0 += CC_UNROLL * stride) {
    int c[CC_UNROLL];
#pragma unroll
    for (int u = 0; u < CC_UNROLL; ++u) c[u] = v0 + u * stride < N ? comp[v0 + u * stride] : -1;
#pragma unroll
    for (int u = 0; u < CC_UNROLL; ++u) {
      const int64_t v = v0 + u * stride;
      if (c[u] < 0 || c[u] != (int)v) continue;
      const int s = size[v];
      const bool keep = (long long)s >= min_voxels && (!keep_largest || (int)v == largest);
      verdict[v] = keep;
      if (keep) { n += 1; vox += (unsigned)s; e += (unsigned)et[v]; }
    }
  }
  cc_block_reduce(n, vox, e, unused);
  if (threadIdx.x == 0 && n) {
    unsigned long long* r = reinterpret_cast<unsigned long long*>(rec);
    atomicAdd(r + N3D_CC_REC_KEPT, n);
    atomicAdd(r + N3D_CC_REC_VOXELS_KEPT, vox);
    if (e) atomicAdd(r + N3D_CC_REC_ET_KEPT, e);
  }
}

// Apply.  grid (<= CC_GRID): out = the label where the voxel's component is kept, 0 elsewhere; label 4 becomes 1 when
// 0 < et_kept < et_min_voxels.  Thread 0 finishes the record (words no other thread of this launch reads).
__global__ __launch_bounds__(CC_THREADS) void cc_apply_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ comp,
                                                              const uint8_t* __restrict__ verdict, int N, long long et_min_voxels,
                                                              long long* __restrict__ rec, uint8_t* __restrict__ out) {
  const long long ek = rec[N3D_CC_REC_ET_KEPT];
  const bool relabel = ek > 0 && ek < et_min_voxels;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long packed = (unsigned long long)rec[N3D_CC_REC_PACKED];
    rec[N3D_CC_REC_LARGEST_SIZE] = (long long)(packed >> 32);
    rec[N3D_CC_REC_LARGEST_ID] = (long long)(int)(0xFFFFFFFFu - (unsigned)(packed & 0xFFFFFFFFull));   // -1 without a component
    rec[N3D_CC_REC_ET_RELABELLED] = relabel;
  }
  const int64_t stride = (int64_t)gridDim.x * CC_THREADS;
  for (int64_t v0 = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; v0 < N; v0 += CC_UNROLL * stride) {
    int c[CC_UNROLL];
#pragma unroll
    for (int u = 0; u < CC_UNROLL; ++u) c[u] = v0 + u * stride < N ? comp[v0 + u * stride] : -1;
#pragma unroll
    for (int u = 0; u < CC_UNROLL; ++u) {
      const int64_t v = v0 + u * stride;
      if (v >= N) break;
      uint8_t o = 0;
      if (c[u] >= 0 && verdict[c[u]]) {
        o = labels[v];
        if (relabel && o == 4) o = 1;
      }
      out[v] = o;
    }
  }
}

}  // namespace n3d

using namespace n3d;

static inline int64_t cc_up256(int64_t b) { return (b + 255) & ~(int64_t)255; }
static inline unsigned cc_blocks(int64_t n, int cap) {
  const int64_t b = cdiv(n, CC_THREADS);
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

static int cc_geom(const int32_t* full, int connectivity, const char* what, CcGeom* g, int* nd) {
  N3D_CHECK_ARG(full && full[0] > 0 && full[1] > 0 && full[2] > 0, "%s: bad image shape", what);
  const int64_t N = (int64_t)full[0] * full[1] * full[2];
  N3D_CHECK_ARG(N < (1ll << 31), "%s: image (%d, %d, %d) = %lld voxels: the int32 component ids need FX * FY * FZ < 2^31", what, full[0],
                full[1], full[2], (long long)N);
  N3D_CHECK_ARG(connectivity == 6 || connectivity == 18 || connectivity == 26, "%s: connectivity %d: must be 6, 18 or 26", what,
                connectivity);
  *nd = connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3);
  g->N = (int)N;
  for (int a = 0; a < 3; ++a) g->F[a] = full[a];
  const int64_t tx = cdiv(full[0], CC_TX), ty = cdiv(full[1], CC_TY), tz = cdiv(full[2], CC_TZ);
  g->ntiles = (int)(tx * ty * tz);   // <= N
  g->fY = FastDiv((uint32_t)full[1]);
  g->fZ = FastDiv((uint32_t)full[2]);
  g->tY = FastDiv((uint32_t)ty);
  g->tZ = FastDiv((uint32_t)tz);
  return N3D_OK;
}

struct CcBufs {
  const uint8_t* labels;
  int32_t *parent, *comp, *size, *et;   // size / et NULL (n3d_cc_label): no counting
  uint8_t* verdict;
  long long* rec;
  uint8_t* out;
  long long min_voxels, et_min_voxels;
  int keep_largest;
};

template <int ND>
static int cc_unite(int variant, int phase, const CcGeom& g, const CcBufs& b, hipStream_t s) {
  const dim3 lgrid((unsigned)(g.ntiles < CC_LOCAL_GRID ? g.ntiles : CC_LOCAL_GRID)), grid(cc_blocks(g.N, CC_GRID)), block(CC_THREADS);
  if (phase == 0) {
    if (variant == N3D_CC_TILED) N3D_LAUNCH(cc_local_kernel<ND>, lgrid, block, 0, s, b.labels, g, b.parent, b.size, b.et, b.rec);
    else N3D_LAUNCH(cc_init_kernel, grid, block, 0, s, b.labels, g.N, b.parent, b.size, b.et, b.rec);
  } else {
    if (variant == N3D_CC_TILED) N3D_LAUNCH((cc_merge_kernel<ND, false>), grid, block, 0, s, g, b.parent);
    else N3D_LAUNCH((cc_merge_kernel<ND, true>), grid, block, 0, s, g, b.parent);
  }
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

// the launches first .. last of the pipeline: 0 local, 1 merge, 2 flatten, 3 decide (maximum), 4 decide (verdicts), 5 apply
static int cc_run(int variant, int first, int last, const CcGeom& g, int nd, const CcBufs& b, hipStream_t s) {
  const dim3 dgrid(cc_blocks(g.N, CC_GRID)), grid(cc_blocks(g.N, CC_GRID)), block(CC_THREADS);
  for (int phase = first; phase <= last; ++phase) {
    switch (phase) {
      case 0:
      case 1:
        if (int e = nd == 1 ? cc_unite<1>(variant, phase, g, b, s) : (nd == 2 ? cc_unite<2>(variant, phase, g, b, s) : cc_unite<3>(variant, phase, g, b, s)))
          return e;
        break;
      case 2:
        if (b.size) N3D_LAUNCH(cc_flatten_kernel<true>, grid, block, 0, s, b.parent, b.labels, g.N, b.comp, b.size, b.et);
        else N3D_LAUNCH(cc_flatten_kernel<false>, grid, block, 0, s, b.parent, b.labels, g.N, b.comp, b.size, b.et);
        break;
      case 3:
        N3D_LAUNCH(cc_decide_max_kernel, dgrid, block, 0, s, b.comp, b.size, b.et, g.N, b.rec);
        break;
      case 4:
        N3D_LAUNCH(cc_decide_keep_kernel, dgrid, block, 0, s, b.comp, b.size, b.et, g.N, b.min_voxels, b.keep_largest, b.verdict, b.rec);
        break;
      default:
        N3D_LAUNCH(cc_apply_kernel, grid, block, 0, s, b.labels, b.comp, b.verdict, g.N, b.et_min_voxels, b.rec, b.out);
    }
    N3D_LAUNCH_CHECK();
  }
  return N3D_OK;
}

extern "C" size_t n3d_cc_workspace_bytes(int FX, int FY, int FZ, int64_t* offsets) {
  if (FX <= 0 || FY <= 0 || FZ <= 0 || (int64_t)FX * FY * FZ >= (1ll << 31)) return 0;
  const int64_t N = (int64_t)FX * FY * FZ;
  const int64_t o_parent = 0, o_comp = o_parent + cc_up256(4 * N), o_size = o_comp + cc_up256(4 * N), o_et = o_size + cc_up256(4 * N),
                o_verdict = o_et + cc_up256(4 * N), o_rec = o_verdict + cc_up256(N);
  if (offsets) {
    offsets[0] = o_parent; offsets[1] = o_comp; offsets[2] = o_size; offsets[3] = o_et; offsets[4] = o_verdict; offsets[5] = o_rec;
  }
  return (size_t)(o_rec + cc_up256(N3D_CC_REC_WORDS * 8));
}

extern "C" int n3d_cc_label(const uint8_t* mask, const int32_t* full, int connectivity, int32_t* parent, int32_t* comp, void* stream) {
  CcGeom g;
  int nd;
  if (int e = cc_geom(full, connectivity, "cc_label", &g, &nd)) return e;
  N3D_CHECK_ARG(mask && parent && comp && parent != comp, "cc_label: bad args");
  N3D_CHECK_ARG(((reinterpret_cast<uintptr_t>(parent) | reinterpret_cast<uintptr_t>(comp)) & 3) == 0, "cc_label: parent and comp must be 4-byte aligned");
  CcBufs b = {};
  b.labels = mask; b.parent = parent; b.comp = comp;
  return cc_run(N3D_CC_TILED, 0, 2, g, nd, b, (hipStream_t)stream);
}

extern "C" int n3d_cc_phases(int variant, int first, int last, const uint8_t* labels, const int32_t* full, int connectivity, int64_t min_voxels,
                             int keep_largest, int64_t et_min_voxels, void* workspace, uint8_t* out, void* stream) {
  CcGeom g;
  int nd;
  if (int e = cc_geom(full, connectivity, "cc_clean", &g, &nd)) return e;
  N3D_CHECK_ARG(labels && workspace && out && labels != out, "cc_clean: bad args");
  N3D_CHECK_ARG(variant == N3D_CC_TILED || variant == N3D_CC_GLOBAL_ONLY, "cc_clean: variant %d: must be N3D_CC_TILED or N3D_CC_GLOBAL_ONLY", variant);
  N3D_CHECK_ARG(0 <= first && first <= last && last < N3D_CC_PHASES, "cc_clean: phases %d .. %d: must lie in 0 .. %d", first, last, N3D_CC_PHASES - 1);
  N3D_CHECK_ARG(min_voxels >= 0 && et_min_voxels >= 0, "cc_clean: min_voxels %lld and et_min_voxels %lld must not be negative",
                (long long)min_voxels, (long long)et_min_voxels);
  N3D_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "cc_clean: the workspace must be 8-byte aligned");
  int64_t off[6];
  n3d_cc_workspace_bytes(full[0], full[1], full[2], off);
  char* ws = static_cast<char*>(workspace);
  CcBufs b;
  b.labels = labels;
  b.parent = reinterpret_cast<int32_t*>(ws + off[0]);
  b.comp = reinterpret_cast<int32_t*>(ws + off[1]);
  b.size = reinterpret_cast<int32_t*>(ws + off[2]);
  b.et = reinterpret_cast<int32_t*>(ws + off[3]);
  b.verdict = reinterpret_cast<uint8_t*>(ws + off[4]);
  b.rec = reinterpret_cast<long long*>(ws + off[5]);
  b.out = out;
  b.min_voxels = min_voxels; b.et_min_voxels = et_min_voxels; b.keep_largest = keep_largest != 0;
  return cc_run(variant, first, last, g, nd, b, (hipStream_t)stream);
}

extern "C" int n3d_cc_clean(const uint8_t* labels, const int32_t* full, int connectivity, int64_t min_voxels, int keep_largest,
                            int64_t et_min_voxels, void* workspace, uint8_t* out, void* stream) {
  return n3d_cc_phases(N3D_CC_TILED, 0, N3D_CC_PHASES - 1, labels, full, connectivity, min_voxels, keep_largest, et_min_voxels, workspace, out,
                       stream);
}
