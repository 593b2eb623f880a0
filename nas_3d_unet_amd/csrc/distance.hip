// Signed distance maps of a target batch (include/n3d.h, "Boundary loss"): for every one of the B * C binary maps of D0 x D1 x D2
// voxels, phi = the Euclidean distance to the nearest foreground voxel on the background and -(the distance to the nearest
// background voxel - 1) on the foreground -- what scipy.ndimage.distance_transform_edt gives Kervadec's one_hot2dist -- exact:
// squared distances are int32 minima of the separable transform, and each voxel takes one fp64 square root and one rounding to fp32.
// Integer minima throughout and one writer per word: two runs give the same bits.
//
// Three launches, every map of the batch in each:
//   z   a wave takes a line: the line's occupancy as 64-bit ballot words, and a lane finds the nearest set / clear bit on either
//       side of its voxel with clz / ffs -- no walk.  Writes BOTH fields, g_fg (squared distance to the line's nearest foreground
//       voxel) and g_bg, since the later passes minimise over voxels of either class.
//   y   in place on both fields: a thread takes one column of one field and forms the lower envelope of its parabolas, about 2 D1
//       steps whatever the map holds; lanes are consecutive z columns, so loads and stores run along z.
//   x   the same along x; a voxel needs only its own side's final value -- the foreground field on the background (a voxel is
//       background exactly where its foreground field is not 0) -- and phi is written from it.
// (A first form walked outwards from every voxel, bounded by the best so far: quick beside a boundary -- 43 us on empty maps, 55 us
// on 30 % speckle at 2 x 3 x 64^3 -- but a voxel far from any source walks all the way to it, and a step of that loop costs several
// times a step of a brute-force pass: 238 us on tumour-like maps, profiles/boundary_probe.log.)
#include "n3d_common.h"

namespace n3d {

constexpr int SDT_INF = 1 << 29;          // "no source": INF + 3 * 1023^2 stays below 2^31
constexpr int SDT_MAX_AXIS = 1024;        // N3D_SDT_MAX_AXIS
constexpr int SDT_THREADS = 256, SDT_WAVES = SDT_THREADS / 64;
constexpr int SDT_WORDS = SDT_MAX_AXIS / 64;

struct SdtGeom {
  int D[3];
  int C;          // maps per sample
  int64_t N;      // D0 * D1 * D2
};

// distance from bit `lane` of word k to the nearest set bit of the line's words at or below it (INF: none)
template <typename W>
__device__ __forceinline__ int sdt_nearest_down(W&& word, int k, int lane) {
  unsigned long long m = word(k) & (~0ull >> (63 - lane));
  if (m) return lane - (63 - __clzll((long long)m));
  for (int kk = k - 1; kk >= 0; --kk) {
    m = word(kk);
    if (m) return (k - kk) * 64 + lane - (63 - __clzll((long long)m));
  }
  return SDT_INF;
}
template <typename W>
__device__ __forceinline__ int sdt_nearest_up(W&& word, int k, int lane, int nw) {
  unsigned long long m = word(k) & (~0ull << lane);
  if (m) return (__ffsll((unsigned long long)m) - 1) - lane;
  for (int kk = k + 1; kk < nw; ++kk) {
    m = word(kk);
    if (m) return (kk - k) * 64 + (__ffsll((unsigned long long)m) - 1) - lane;
  }
  return SDT_INF;
}

// grid (<= lines / 4), 256 threads; wave w of workgroup g takes the lines 4 * (g + i * gridDim.x) + w.  field f of map m: ws + (2 m + f) * N
template <typename TT>
__global__ __launch_bounds__(SDT_THREADS) void sdt_z_kernel(const TT* __restrict__ t, int64_t tsb, int64_t tsc, int64_t tsv, SdtGeom g,
                                                            int64_t lines, int32_t* __restrict__ ws) {
  __shared__ unsigned long long msk[SDT_WAVES][SDT_WORDS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int L = g.D[2], nw = (L + 63) >> 6;
  const unsigned long long last = ~0ull >> (64 * nw - L);      // the valid bits of the last word
  const int64_t per_map = (int64_t)g.D[0] * g.D[1];
  for (int64_t l0 = (int64_t)blockIdx.x * SDT_WAVES; l0 < lines; l0 += (int64_t)gridDim.x * SDT_WAVES) {      // (uniform over the workgroup)
    const int64_t line = l0 + wave;
    const bool live = line < lines;
    const int64_t map = live ? line / per_map : 0, row = live ? line - map * per_map : 0;
    const int64_t b = map / g.C, c = map - b * g.C;
    const TT* src = t + b * tsb + c * tsc + row * L * tsv;
    for (int k = 0; k < nw; ++k) {
      const int z = k * 64 + lane;
      const bool f = live && z < L && src[(int64_t)z * tsv] != (TT)0;
      const unsigned long long w = __ballot(f);
      if (lane == 0) msk[wave][k] = w;
    }
    __syncthreads();
    if (live) {
      const unsigned long long* mw = msk[wave];
      auto fg = [&](int k) { return mw[k]; };
      auto bg = [&](int k) { return ~mw[k] & (k == nw - 1 ? last : ~0ull); };
      int32_t* o = ws + (2 * map) * g.N + row * L;
      for (int k = 0; k < nw; ++k) {
        const int z = k * 64 + lane;
        if (z >= L) break;
        const int df = min(sdt_nearest_down(fg, k, lane), sdt_nearest_up(fg, k, lane, nw));
        const int db = min(sdt_nearest_down(bg, k, lane), sdt_nearest_up(bg, k, lane, nw));
        o[z] = df >= SDT_INF ? SDT_INF : df * df;
        o[g.N + z] = db >= SDT_INF ? SDT_INF : db * db;
      }
    }
    __syncthreads();     // the words are read to the end before the next line's ballots
  }
}

// A line pass is the lower envelope of the parabolas w_j - 2 i j + i^2, w_j = f_j + j^2 (Felzenszwalb & Huttenlocher), in integers: a
// THREAD takes one column of one field.  Building: the sources j in rising order; the top parabola p of the stack, above o, is dropped
// when it is nowhere below both its neighbours, (w_p - w_o) (q - p) >= (w_q - w_p) (p - o) (the two intersections compared as
// fractions, in int64).  Filling: i rises, and the envelope's current parabola gives way to the next as soon as that one is not
// above it at i.  About 2 L steps per column whatever the map holds.
// A thread first brings its column into LDS, [line position][thread], SDT_LOAD requests in flight at a time (a wave's request is one
// run of consecutive words): taken from memory position by position as the build went, the column cost one memory round trip per
// eight positions with nothing to hide it behind (133 us at 2 x 3 x 64^3, 840 us at 128^3).  The w stack of a column OVERWRITES
// the column: entry n is written while position q >= n is being taken, after f[q] was read, and nothing reads f below q again.
// The j stack (uint16) sits beside it.
constexpr int SDT_LOAD = 32;      // values requested together
constexpr int SDT_STACK = 4096;   // line positions x z columns of a tile: 32 KB of columns / w stacks (two fields) and 16 KB of j stacks
constexpr int SDT_LINE_THREADS = 128;

// grid (tiles, maps), 2 T threads: thread (field, z column of the tile).  axis 1 (y): in place on both fields.  FINAL (axis 0, x):
// phi is written -- by the foreground field's thread on the background (where its result is not 0) and by the background field's
// thread on the foreground, so every voxel has one writer and takes its own side's value.  T = 1 << tshift <= 64, T * D[axis] <=
// SDT_STACK.  Dynamic LDS: 6 bytes per thread and line position.
template <bool FINAL>
__global__ __launch_bounds__(SDT_LINE_THREADS) void sdt_line_kernel(SdtGeom g, int tshift, int32_t* __restrict__ ws, float* __restrict__ phi,
                                                                    int64_t fsb, int64_t fsc, int64_t fsv) {
  extern __shared__ int sdt_lds[];
  constexpr int axis = FINAL ? 0 : 1;
  const int T = 1 << tshift, nt = 2 * T, L = g.D[axis];
  const int tid = threadIdx.x, field = tid >> tshift, tz = tid & (T - 1);
  const int nzt = ((g.D[2] - 1) >> tshift) + 1;
  const int map = blockIdx.y, tile = blockIdx.x;
  const int o = tile / nzt, z0 = (tile - o * nzt) << tshift;
  const bool live = z0 + tz < g.D[2];
  const int64_t sl = FINAL ? (int64_t)g.D[1] * g.D[2] : (int64_t)g.D[2];      // stride of the line
  const int64_t so = FINAL ? (int64_t)g.D[2] : (int64_t)g.D[1] * g.D[2];      // stride of the other axis
  const int64_t v0 = (int64_t)o * so + z0 + tz;                               // the column's first voxel
  int32_t* f = ws + (int64_t)(2 * map + field) * g.N + v0;                    // (addressed only where live)
  int32_t* wst = sdt_lds + tid;                                               // this thread's column, then its w stack: entry k at [k * nt]
  uint16_t* vst = reinterpret_cast<uint16_t*>(sdt_lds + L * nt) + tid;
  for (int j0 = 0; j0 < L; j0 += SDT_LOAD) {
    int fv[SDT_LOAD];
#pragma unroll
    for (int u = 0; u < SDT_LOAD; ++u) fv[u] = (live && j0 + u < L) ? f[(int64_t)(j0 + u) * sl] : SDT_INF;
#pragma unroll
    for (int u = 0; u < SDT_LOAD; ++u)
      if (j0 + u < L) wst[(j0 + u) * nt] = fv[u];
  }
  // (a thread reads back only what it stored itself: no barrier)
  if (!live) return;
  int n = 0, pv = 0, pw = 0, ov = 0, ow = 0;      // entries on the stack; its top and the entry below it
  for (int q = 0; q < L; ++q) {
    const int fq = wst[q * nt];
    if (fq >= SDT_INF) continue;
    const int wq = fq + q * q;
    while (n >= 2) {
      if ((long long)(pw - ow) * (q - pv) < (long long)(wq - pw) * (pv - ov)) break;
      --n; pv = ov; pw = ow;
      if (n >= 2) { ov = vst[(n - 2) * nt]; ow = wst[(n - 2) * nt]; }
    }
    vst[n * nt] = (uint16_t)q; wst[n * nt] = wq;      // n <= q: at most one entry per source, and f[q] has been read
    ov = pv; ow = pw; pv = q; pw = wq; ++n;
  }
  int k = 0, cv = 0, cw = SDT_INF, nv = 0, nw = 0;      // the envelope's current parabola and the next one
  if (n > 0) { cv = vst[0]; cw = wst[0]; }
  if (n > 1) { nv = vst[nt]; nw = wst[nt]; }
  const int b = map / g.C, c = map - b * g.C;
  float* out = FINAL ? phi + b * fsb + c * fsc : nullptr;
  for (int i = 0; i < L; ++i) {
    while (k + 1 < n && nw - 2 * i * nv <= cw - 2 * i * cv) {
      ++k; cv = nv; cw = nw;
      if (k + 1 < n) { nv = vst[(k + 1) * nt]; nw = wst[(k + 1) * nt]; }
    }
    const int d2 = n > 0 ? cw - 2 * i * cv + i * i : SDT_INF;      // f[cv] + (i - cv)^2
    if constexpr (!FINAL) {
      f[(int64_t)i * sl] = d2;
    } else if (d2 != 0) {         // a voxel of the other kind (0: the voxel is itself a source of this field): this field is its side
      float r = 0.f;              // no source of the wanted kind in the patch
      if (d2 < SDT_INF) {
        const double s = sqrt((double)d2);
        r = field ? (float)(-(s - 1.0)) : (float)s;
      }
      out[(v0 + (int64_t)i * sl) * fsv] = r;
    }
  }
}

static bool sdt_shape_ok(int B, int C, int D0, int D1, int D2) {
  return B > 0 && C > 0 && (int64_t)B * C <= 65535 && D0 >= 1 && D1 >= 1 && D2 >= 1 && D0 <= SDT_MAX_AXIS && D1 <= SDT_MAX_AXIS &&
         D2 <= SDT_MAX_AXIS;
}

// z columns per tile of a line pass along an axis of extent L: the largest power of two with T * L <= SDT_STACK, at most 64 (a
// workgroup of 128 threads holds both fields) and no more than D2 rounded up
static int sdt_tshift(int L, int D2) {
  int s = 6;
  while (s > 0 && (((int64_t)L << s) > SDT_STACK || (1 << (s - 1)) >= D2)) --s;
  return s;
}

}  // namespace n3d

using namespace n3d;

extern "C" {

size_t n3d_target_sdt_workspace_bytes(int B, int C, int D0, int D1, int D2) {
  if (!sdt_shape_ok(B, C, D0, D1, D2)) return 0;
  return (size_t)B * C * 2 * (size_t)D0 * D1 * D2 * sizeof(int32_t);
}

int n3d_target_sdt(const void* t, int t_dtype, int64_t tsb, int64_t tsc, int64_t tsv, int B, int C, int D0, int D1, int D2, float* phi,
                   int64_t fsb, int64_t fsc, int64_t fsv, void* ws, size_t ws_bytes, void* stream) {
  N3D_CHECK_ARG(t && phi, "target_sdt: bad args");
  N3D_CHECK_ARG(t_dtype == N3D_F32 || t_dtype == N3D_U8, "target_sdt: targets are N3D_F32 or N3D_U8 (t_dtype=%d)", t_dtype);
  if (!sdt_shape_ok(B, C, D0, D1, D2))
    N3D_UNSUPPORTED("target_sdt: B * C <= 65535 maps with extents 1..%d are built (B=%d C=%d D=%d,%d,%d)", SDT_MAX_AXIS, B, C, D0, D1, D2);
  const size_t need = n3d_target_sdt_workspace_bytes(B, C, D0, D1, D2);
  if (!ws || ws_bytes < need) { set_error("target_sdt: workspace too small (%zu < %zu)", ws_bytes, need); return N3D_ERR_WORKSPACE; }
  N3D_CHECK_ARG(reinterpret_cast<uintptr_t>(ws) % 4 == 0, "target_sdt: the workspace must be 4-byte aligned");
  SdtGeom g;
  g.D[0] = D0; g.D[1] = D1; g.D[2] = D2; g.C = C; g.N = (int64_t)D0 * D1 * D2;
  const int maps = B * C;
  hipStream_t s = (hipStream_t)stream;
  int32_t* w = (int32_t*)ws;
  const int64_t lines = (int64_t)maps * D0 * D1;
  const dim3 zgrid((unsigned)std::min<int64_t>(cdiv(lines, SDT_WAVES), 1 << 16)), blk(SDT_THREADS);
  if (t_dtype == N3D_U8) N3D_LAUNCH(sdt_z_kernel<uint8_t>, zgrid, blk, 0, s, (const uint8_t*)t, tsb, tsc, tsv, g, lines, w);
  else N3D_LAUNCH(sdt_z_kernel<float>, zgrid, blk, 0, s, (const float*)t, tsb, tsc, tsv, g, lines, w);
  const int ty = sdt_tshift(D1, D2), tx = sdt_tshift(D0, D2);
  const dim3 ygrid((unsigned)(D0 * (((D2 - 1) >> ty) + 1)), (unsigned)maps), xgrid((unsigned)(D1 * (((D2 - 1) >> tx) + 1)), (unsigned)maps);
  N3D_LAUNCH(sdt_line_kernel<false>, ygrid, dim3(2u << ty), (size_t)D1 * (2u << ty) * 6, s, g, ty, w, (float*)nullptr, (int64_t)0, (int64_t)0, (int64_t)0);
  N3D_LAUNCH(sdt_line_kernel<true>, xgrid, dim3(2u << tx), (size_t)D0 * (2u << tx) * 6, s, g, tx, w, phi, fsb, fsc, fsv);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

}  // extern "C"
