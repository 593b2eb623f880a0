// Order-3 (cubic B-spline) interpolation of the data in the patch gather: scipy.ndimage.map_coordinates(order=3, mode="constant")
// on the crop, behind n3d_patch_gather_spline (include/n3d.h states the rule operation by operation).  Unlike orders 0 and 1 the
// taps are not read from the volume: the crop is first turned into B-spline coefficients by a recursive filter along every axis, so
// a batch is five launches over a scratch of 12 bytes per voxel and channel:
//   spline_crop_kernel          the crop (zero padded, flipped) as fp32, channel-planar: what the mask reads and the filter starts from
//   spline_line_kernel x 3      the prefilter along axis 0, then 1, then 2 (fp64; the first pass reads the fp32 crop)
//   patch_gather_spline_kernel  coordinate, 12 weights, 64 fp64 taps per channel, the mask, the intensity map, the stores
// Every fp64 operation is rounded on its own: this file is compiled with -ffp-contract=off (Makefile).
#include "patch_gather.h"

#include <cfloat>

namespace n3d {

// ---- the crop -------------------------------------------------------------------------------------------------------------------
// raw[(b * Cv + c) * P^3 + q] = vol[c][corner + (aflip ? P-1-q : q)], 0.0f outside the volume.  One thread = one patch voxel q, all
// channels; stores are lane-consecutive per channel, loads too (reversed on a flipped last axis).  HBM-bound: 4 * Cv bytes each way.
__global__ __launch_bounds__(256) void spline_crop_kernel(const n3d_patch_volume* __restrict__ vols, int Cv, ElasticDescs descs, int P,
                                                          float* __restrict__ raw, FastDiv fP, FastDiv fPP) {
  const int b = blockIdx.y;
  const n3d_patch_wdesc& w = descs.d[b].w;
  const uint32_t P3 = (uint32_t)P * P * P;
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= P3) return;
  const n3d_patch_volume r = vols[w.g.vol];
  uint32_t q0, rem, q1, q2;
  fPP.divmod(q, q0, rem);
  fP.divmod(rem, q1, q2);
  const int idx[3] = {(int)q0, (int)q1, (int)q2};
  bool in = true;
  int s[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    s[a] = w.g.d.corner[a] + (w.aflip[a] ? P - 1 - idx[a] : idx[a]);
    in = in && s[a] >= 0 && s[a] < r.dims[a];
  }
  const int64_t XYZ = (int64_t)r.dims[0] * r.dims[1] * r.dims[2];
  const int64_t sv = in ? ((int64_t)s[0] * r.dims[1] + s[1]) * r.dims[2] + s[2] : 0;
  for (int c = 0; c < Cv; ++c) raw[((int64_t)b * Cv + c) * P3 + q] = in ? r.data[c * XYZ + sv] : 0.f;
}

// ---- the prefilter --------------------------------------------------------------------------------------------------------------
struct SplineConsts { double z, gain, zn, inv0, anti; };

// one line c(0) .. c(P-1), already multiplied by gain, in place: the mirror-boundary initial value, the causal pass, the
// anticausal initial value and pass (include/n3d.h, n3d_spline_prefilter).  A chain of about 3 P dependent fp64 operations.
template <typename Line>
__device__ __forceinline__ void spline_line(Line c, int P, const SplineConsts& k) {
  const double z = k.z, zn = k.zn;
  double c0 = c(0) + zn * c(P - 1);
  double zi = z;
  for (int i = 1; i <= P - 2; ++i) {
    c0 = c0 + zi * (c(i) + zn * c(P - 1 - i));
    zi = zi * z;
  }
  double prev = c0 * k.inv0;
  c(0) = prev;
  for (int i = 1; i <= P - 1; ++i) {
    prev = c(i) + z * prev;
    c(i) = prev;
  }
  // prev is c[P-1] of the causal pass, c(P - 2) the element before it
  prev = (z * c(P - 2) + prev) * k.anti;
  c(P - 1) = prev;
  for (int i = P - 2; i >= 0; --i) {
    prev = z * (prev - c(i));
    c(i) = prev;
  }
}

// where line m of n cubes starts, and the distance of its elements: lines along axis 0 are indexed by (cube, j1, j2), along axis 1 by
// (cube, j0, j2), along axis 2 by (cube, j0, j1) -- neighbouring m are neighbouring addresses on axes 0 and 1
__device__ __forceinline__ int64_t spline_line_base(int axis, int64_t m, int P, int64_t& stride) {
  const int64_t PP = (int64_t)P * P;
  const int64_t cube = m / PP, r = m - cube * PP;
  if (axis == 0) { stride = PP; return cube * PP * P + r; }
  if (axis == 1) { stride = P; return cube * PP * P + (r / P) * PP + r % P; }
  stride = 1;
  return m * P;
}

constexpr int kSplineLines = 32;        // lines per workgroup of the LDS plan
constexpr int kSplineLdsMaxP = 255;     // 32 lines * 255 doubles = 65 280 bytes of the 64 KiB a workgroup gets without an attribute

// The LDS plan (P <= 255): a workgroup of 64 threads takes 32 consecutive lines, loads them once (times gain) into LDS at a pitch of
// P | 1 doubles, lanes 0..31 run one line each there, and the workgroup stores them once.  The odd pitch makes the 32 lanes' ds_read_b64
// (and each 16 lanes' ds_write_b64) hit distinct banks.  On axes 0 and 1 consecutive lanes load consecutive lines at one position
// (coalesced 256-byte rows); on axis 2 the 32 lines are one contiguous run of 32 * P doubles, loaded in address order: that is the
// transpose.  Bound by the latency of the dependent chain: 8 bytes read and written per voxel, against ~3 P chained fp64 operations
// per line with half of each wave idle; 32 lines per workgroup keep more workgroups on the chip than 64 would (2 x 4 x 64^3 has
// 32 768 lines: 1024 workgroups over 256 CUs).
template <bool FIRST>
__global__ __launch_bounds__(64) void spline_line_kernel(const float* __restrict__ raw, double* __restrict__ coef, int64_t lines, int P, int axis,
                                                         SplineConsts k) {
  extern __shared__ double tile[];
  const int pitch = P | 1;
  const int64_t m0 = (int64_t)blockIdx.x * kSplineLines;
  const int here = (int)(lines - m0 < kSplineLines ? lines - m0 : kSplineLines);
  const int total = here * P;
  // element e of the tile <-> (line l, position i): address order on axis 2, line-fastest on axes 0 and 1
  for (int e = threadIdx.x; e < total; e += 64) {
    const int l = axis == 2 ? e / P : e % here, i = axis == 2 ? e % P : e / here;
    int64_t stride;
    const int64_t g = spline_line_base(axis, m0 + l, P, stride) + i * stride;
    const double x = FIRST ? (double)raw[g] : coef[g];
    tile[l * pitch + i] = x * k.gain;
  }
  __syncthreads();
  if ((int)threadIdx.x < here) {
    double* line = tile + threadIdx.x * pitch;
    spline_line([=](int i) -> double& { return line[i]; }, P, k);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < total; e += 64) {
    const int l = axis == 2 ? e / P : e % here, i = axis == 2 ? e % P : e / here;
    int64_t stride;
    coef[spline_line_base(axis, m0 + l, P, stride) + i * stride] = tile[l * pitch + i];
  }
}

// The plan for P >= 256, where 32 lines no longer fit 64 KiB of LDS: one thread per line, in place in memory.  Coalesced on axes 0
// and 1, strided over the lanes on axis 2 (each lane walks its own cache lines).  Patches of that size are not trained on; the plan
// exists so that the entry's P range is the gather's.
template <bool FIRST>
__global__ __launch_bounds__(64) void spline_line_direct_kernel(const float* __restrict__ raw, double* __restrict__ coef, int64_t lines, int P,
                                                                int axis, SplineConsts k) {
  const int64_t m = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (m >= lines) return;
  int64_t stride;
  const int64_t base = spline_line_base(axis, m, P, stride);
  for (int i = 0; i < P; ++i) {
    const int64_t g = base + i * stride;
    coef[g] = (FIRST ? (double)raw[g] : coef[g]) * k.gain;
  }
  double* line = coef + base;
  spline_line([=](int i) -> double& { return line[i * stride]; }, P, k);
}

// ---- the gather -----------------------------------------------------------------------------------------------------------------
// One thread = one output voxel, one patch per blockIdx.y (`elastic` uniform over the workgroup, as patch_gather_elastic_kernel).
// Per voxel: the coordinate, 12 weights and 12 mirrored tap indices, then per channel 64 eight-byte coefficient loads issued
// together (a voxel without a source reads the taps of coordinate 0 and drops the sum), one fp32 load of the crop for the mask and
// 64 multiply-adds in fp64.  Neighbouring voxels share most taps, so what reaches HBM is about the coefficient cube once (8 bytes per
// voxel and channel); the kernel waits for the latency of 64 L1 / L2 loads per channel and issues 3 * 64 fp64 operations per channel.
template <typename TT>
__global__ __launch_bounds__(256) void patch_gather_spline_kernel(const n3d_patch_volume* __restrict__ vols, int Cv, ElasticDescs descs, int P,
                                                                  int inclusive, const double* __restrict__ coef, const float* __restrict__ raw,
                                                                  float* __restrict__ x_out, int64_t xld, TT* __restrict__ t_out, FastDiv fP,
                                                                  FastDiv fPP) {
  __shared__ double lattice[3 * kElasticMaxG3];
  const int b = blockIdx.y;
  const n3d_patch_edesc& e = descs.d[b];
  const n3d_patch_wdesc& w = e.w;
  const uint32_t P3 = (uint32_t)P * P * P;
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  const bool elastic = e.elastic != 0;
  if (elastic) {
    elastic_lattice_fill(e, lattice);
    __syncthreads();      // every thread of the workgroup gets here: the ones past the patch's end leave only below
  }
  if (v >= P3) return;
  const n3d_patch_volume r = vols[w.g.vol];
  int j[3];
  patch_index(w.g.d, v, P, fP, fPP, j);
  double c[3];
  patch_warp_coordinate(w, j, c);
  if (elastic) elastic_displace(e, lattice, j, c);
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = ok && 0.0 <= c[a] && c[a] <= (double)(P - 1);
  // the nearest voxel: the labels' source in the volume, the mask's in the crop (which holds the flip already)
  bool in = ok;
  int64_t sv = 0;
  int near = 0;
  {
    int s[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int q = ok ? (int)floor(c[a] + 0.5) : 0;
      near = near * P + q;
      s[a] = w.g.d.corner[a] + (w.aflip[a] ? P - 1 - q : q);
      in = in && s[a] >= 0 && s[a] < r.dims[a];
    }
    if (in) sv = ((int64_t)s[0] * r.dims[1] + s[1]) * r.dims[2] + s[2];
  }
  // per axis the four weights and the four tap offsets f-1 .. f+2, mirrored into the crop; a voxel without a source takes f = 0, so
  // every address it forms is valid
  double u[3][4];
  int off[3][4];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double f = ok ? floor(c[a]) : 0.0;
    bspline_weights(ok ? c[a] - f : 0.0, u[a]);
    const int pitch = a == 0 ? P * P : (a == 1 ? P : 1);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      int q = (int)f - 1 + d;
      q = q < 0 ? -q : q;
      q = q > P - 1 ? 2 * (P - 1) - q : q;
      off[a][d] = q * pitch;
    }
  }
  const bool intensity = w.intensity != 0;
  const float* gain = w.gain;
  const float* bias = w.bias;
  patch_data_store(Cv, b, v, P3, x_out, xld, [=](int ch) {
    const int64_t plane = ((int64_t)b * Cv + ch) * P3;
    const double* __restrict__ src = coef + plane;
    double x[64];
#pragma unroll
    for (int t = 0; t < 64; ++t) x[t] = src[off[0][t >> 4] + off[1][(t >> 2) & 3] + off[2][t & 3]];
    const bool keep = ok && raw[plane + near] != 0.f;
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < 64; ++t) acc = acc + ((u[0][t >> 4] * u[1][(t >> 2) & 3]) * u[2][t & 3]) * x[t];
    float y = (float)acc;
    y = y == 0.f ? FLT_MIN : y;       // a kept voxel stays "brain" (x != 0) for every later stage
    y = keep ? y : 0.f;
    if (intensity && keep) {
      y = y * gain[ch & 3];
      y = y + bias[ch & 3];
    }
    return y;
  });
  if (t_out) patch_label_store<TT>(r.truth, in, sv, b, v, P3, inclusive, t_out);
}

static SplineConsts spline_consts(int P) {
  SplineConsts k;
  k.z = std::sqrt(3.0) - 2.0;
  k.gain = (1.0 - k.z) * (1.0 - 1.0 / k.z);
  k.zn = k.z;
  for (int i = 2; i <= P - 1; ++i) k.zn = k.zn * k.z;      // P - 1 factors
  k.inv0 = 1.0 / (1.0 - k.zn * k.zn);
  k.anti = k.z / (k.z * k.z - 1.0);
  return k;
}

// what both entry points require of (n, P) before any launch: P >= 4, P^3 < 2^31, n * P^3 < 2^40 and a grid that fits 31 bits
static int spline_extent_check(const char* fn, int64_t n, int P) {
  N3D_CHECK_ARG(P >= 4, "%s: order 3 needs cubes of at least 4 voxels an edge (got %d)", fn, P);
  N3D_CHECK_ARG((int64_t)P * P * P < (1ll << 31), "%s: P^3 must be below 2^31 (got P = %d)", fn, P);
  N3D_CHECK_ARG(n >= 1 && n <= (1ll << 40) / ((int64_t)P * P * P) && cdiv(n * P * P, kSplineLines) < (1ll << 31),
                "%s: %lld cubes of %d^3 are too many", fn, (long long)n, P);
  return N3D_OK;
}

// the three axis passes over n cubes: raw -> coef.  The caller ran spline_extent_check.
static int spline_prefilter_launch(const float* raw, int64_t n, int P, double* coef, hipStream_t stream) {
  const SplineConsts k = spline_consts(P);
  const int64_t lines = n * P * P;
  for (int axis = 0; axis < 3; ++axis) {
    if (P <= kSplineLdsMaxP) {
      const dim3 grid((unsigned)cdiv(lines, kSplineLines));
      const size_t lds = (size_t)kSplineLines * (P | 1) * sizeof(double);
      if (axis == 0)
        N3D_LAUNCH(spline_line_kernel<true>, grid, dim3(64), lds, stream, raw, coef, lines, P, axis, k);
      else
        N3D_LAUNCH(spline_line_kernel<false>, grid, dim3(64), lds, stream, raw, coef, lines, P, axis, k);
    } else {
      const dim3 grid((unsigned)cdiv(lines, 64));
      if (axis == 0)
        N3D_LAUNCH(spline_line_direct_kernel<true>, grid, dim3(64), 0, stream, raw, coef, lines, P, axis, k);
      else
        N3D_LAUNCH(spline_line_direct_kernel<false>, grid, dim3(64), 0, stream, raw, coef, lines, P, axis, k);
    }
    N3D_LAUNCH_CHECK();
  }
  return N3D_OK;
}

}  // namespace n3d

using namespace n3d;

extern "C" size_t n3d_patch_spline_scratch_bytes(int B, int Cv, int P) {
  if (B < 1 || Cv < 1 || P < 1) return 0;
  return (size_t)B * Cv * P * P * P * (sizeof(double) + sizeof(float));
}

extern "C" int n3d_spline_prefilter(const float* raw, int64_t n, int P, double* coef, void* stream) {
  N3D_CHECK_ARG(raw && coef, "spline_prefilter: bad args");
  if (int rc = spline_extent_check("spline_prefilter", n, P)) return rc;
  return spline_prefilter_launch(raw, n, P, coef, (hipStream_t)stream);
}

extern "C" int n3d_patch_gather_spline(const n3d_patch_volume* vols, int nvol, int Cv, const n3d_patch_edesc* descs, int B, int P, int flags,
                                       void* scratch, size_t scratch_bytes, float* x_out, int64_t xld, void* t_out, void* stream) {
  N3D_CHECK_ARG(vols && descs && x_out && nvol >= 1 && Cv >= 1 && P > 0 && B >= 1 && xld >= Cv, "patch_gather_spline: bad args");
  N3D_CHECK_ARG(B <= N3D_PATCH_ELASTIC_MAX_BATCH, "patch_gather_spline: at most N3D_PATCH_ELASTIC_MAX_BATCH = %d patches per call (got %d)",
                N3D_PATCH_ELASTIC_MAX_BATCH, B);
  if (int rc = spline_extent_check("patch_gather_spline", (int64_t)B * Cv, P)) return rc;
  static_assert(sizeof(ElasticDescs) + 96 <= 4096, "the descriptors travel by value in the kernel arguments (4 KB)");
  ElasticDescs ed;
  for (int i = 0; i < B; ++i) {
    ed.d[i] = descs[i];
    if (int rc = patch_wdesc_check("patch_gather_spline", descs[i].w, i, nvol, Cv, true)) return rc;
    if (int rc = patch_edesc_check("patch_gather_spline", descs[i], i)) return rc;
  }
  for (int i = B; i < N3D_PATCH_ELASTIC_MAX_BATCH; ++i) ed.d[i] = ed.d[0];
  N3D_CHECK_ARG((flags & ~(N3D_PATCH_INCLUSIVE | N3D_PATCH_T_U8)) == 0, "patch_gather_spline: unknown flag bits %d", flags);
  const size_t need = n3d_patch_spline_scratch_bytes(B, Cv, P);
  N3D_CHECK_ARG(scratch && scratch_bytes >= need, "patch_gather_spline: scratch of %zu bytes needed (n3d_patch_spline_scratch_bytes), got %zu%s",
                need, scratch_bytes, scratch ? "" : " (null)");
  N3D_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "patch_gather_spline: scratch must be 8-byte aligned");
  const uint32_t P3 = (uint32_t)P * P * P;
  const int64_t cubes = (int64_t)B * Cv;
  double* coef = (double*)scratch;                 // (B, Cv, P^3) fp64, then the crop (B, Cv, P^3) fp32
  float* raw = (float*)(coef + cubes * P3);
  const int inclusive = flags & N3D_PATCH_INCLUSIVE;
  const dim3 grid((unsigned)cdiv(P3, 256), B);
  const FastDiv fP((uint32_t)P), fPP((uint32_t)P * P);
  N3D_LAUNCH(spline_crop_kernel, grid, dim3(256), 0, (hipStream_t)stream, vols, Cv, ed, P, raw, fP, fPP);
  N3D_LAUNCH_CHECK();
  if (int rc = spline_prefilter_launch(raw, cubes, P, coef, (hipStream_t)stream)) return rc;
  if (flags & N3D_PATCH_T_U8)
    N3D_LAUNCH(patch_gather_spline_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, vols, Cv, ed, P, inclusive, coef, raw, x_out, xld,
               (uint8_t*)t_out, fP, fPP);
  else
    N3D_LAUNCH(patch_gather_spline_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, vols, Cv, ed, P, inclusive, coef, raw, x_out, xld,
               (float*)t_out, fP, fPP);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}
