// On-device data step: the per-batch work the reference's generator does on the host just before the
// hot path (train.py:117-119 receives its result): patch crop with zero padding (patches.py:99-115,152-169), one of
// the 48 cube isometries per patch (augment.py:73-131, the same key for data and truth) and the expansion of the
// BraTS label volume into three binary channels (generator.py:230-248).  ONE gather launch produces the NDHWC input
// batch and the target batch straight from the volume resident in HBM: integer index arithmetic, HBM-bound.
//
// patch_gather_aug_kernel adds the reference's other augmentation (augment.py:50-67: random axis flips and a random per-axis scale
// around the patch centre, resampled with nearest neighbour) to the same launch: an output voxel is still one source voxel or
// zero, so only the index changes -- per axis one fp64 add, multiply, add and floor (scipy's zoom-shift rule, include/n3d.h),
// each rounded on its own: this file is compiled with -ffp-contract=off (Makefile), its other kernels have no floating-point
// arithmetic to contract.  It stays HBM-bound: per output voxel 4 * Cv bytes stored (+ 3 or 12 of targets) and at most
// 4 * Cv + 1 loaded, against 3 fp64 adds + 3 multiplies + 3 floors -- 2 x 4 x 64^3 writes 14.7 MB (fp32 targets) and reads at most
// 8.9 MB, 3 us at 8 TB/s.  A scale > 1 (A < 1) repeats source voxels and reads fewer source bytes; a scale < 1 (A > 1) reads lines strided along z
// and leaves a border of zeros.
#include "patch_gather.h"

namespace n3d {

struct PatchDescs { n3d_patch_desc d[N3D_PATCH_MAX_BATCH]; };
struct GatherDescs { n3d_patch_gdesc d[N3D_PATCH_MAX_BATCH]; };

// the loads, the stores and the label expansion of output voxel v of patch b, given its source voxel s of the volume (ok = false:
// the patch voxel has no source -- resampled from outside the patch -- and reads as outside the volume does: zero, label 0)
template <typename TT>
__device__ __forceinline__ void patch_voxel_store(const float* __restrict__ vol, int Cv, const uint8_t* __restrict__ truth, int X, int Y, int Z,
                                                  const int (&s)[3], bool ok, int b, uint32_t v, int P, int inclusive,
                                                  float* __restrict__ x_out, int64_t xld, TT* __restrict__ t_out) {
  const uint32_t P3 = (uint32_t)P * P * P;
  const bool in = ok && s[0] >= 0 && s[0] < X && s[1] >= 0 && s[1] < Y && s[2] >= 0 && s[2] < Z;
  const int64_t sv = in ? ((int64_t)s[0] * Y + s[1]) * Z + s[2] : 0;
  const int64_t XYZ = (int64_t)X * Y * Z;
  patch_data_store(Cv, b, v, P3, x_out, xld, [=](int c) { return in ? vol[c * XYZ + sv] : 0.f; });
  if (t_out) patch_label_store<TT>(truth, in, sv, b, v, P3, inclusive, t_out);
}

// one output voxel (b, i0, i1, i2) of patch d drawn from the volume (vol, truth, X, Y, Z): the index mapping shared by
// patch_batch_kernel (one volume per launch) and patch_gather_kernel (a volume per patch).  v < P^3.
// TT: storage of the three target maps -- float, or uint8_t (N3D_PATCH_T_U8: the generator's booleans as bytes, what n3d_head_fwd /
// n3d_head_bwd read with t_dtype = N3D_U8)
template <typename TT>
__device__ __forceinline__ void patch_voxel(const float* __restrict__ vol, int Cv, const uint8_t* __restrict__ truth, int X, int Y, int Z,
                                            const n3d_patch_desc& d, int b, uint32_t v, int P, int inclusive, float* __restrict__ x_out,
                                            int64_t xld, TT* __restrict__ t_out, FastDiv fP, FastDiv fPP) {
  int s[3];
  patch_index(d, v, P, fP, fPP, s);
#pragma unroll
  for (int a = 0; a < 3; ++a) s[a] += d.corner[a];
  patch_voxel_store<TT>(vol, Cv, truth, X, Y, Z, s, true, b, v, P, inclusive, x_out, xld, t_out);
}

// one thread = one output voxel (b, i0, i1, i2); writes are lane-consecutive along i2 (x: Cv floats per voxel)
template <typename TT>
__global__ __launch_bounds__(256) void patch_batch_kernel(const float* __restrict__ vol, int Cv, const uint8_t* __restrict__ truth, int X, int Y, int Z,
                                                          PatchDescs descs, int P, int inclusive, float* __restrict__ x_out, int64_t xld,
                                                          TT* __restrict__ t_out, FastDiv fP, FastDiv fPP) {
  const int b = blockIdx.y;
  const n3d_patch_desc d = descs.d[b];
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= (uint32_t)P * P * P) return;
  patch_voxel<TT>(vol, Cv, truth, X, Y, Z, d, b, v, P, inclusive, x_out, xld, t_out, fP, fPP);
}

// the same voxels for a batch whose patches come from different volumes of one set (the reference's shuffled candidate list
// mixes volumes, generator.py:170-193): patch b reads the volume record vols[descs.d[b].vol] (the host checked the index)
template <typename TT>
__global__ __launch_bounds__(256) void patch_gather_kernel(const n3d_patch_volume* __restrict__ vols, int Cv, GatherDescs descs, int P, int inclusive,
                                                           float* __restrict__ x_out, int64_t xld, TT* __restrict__ t_out, FastDiv fP, FastDiv fPP) {
  const int b = blockIdx.y;
  const n3d_patch_gdesc g = descs.d[b];
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= (uint32_t)P * P * P) return;
  const n3d_patch_volume r = vols[g.vol];
  patch_voxel<TT>(r.data, Cv, r.truth, r.dims[0], r.dims[1], r.dims[2], g.d, b, v, P, inclusive, x_out, xld, t_out, fP, fPP);
}

// patch_gather_kernel with the scale / flip distortion between the isometry and the crop (include/n3d.h, n3d_patch_adesc): patch
// index j of the isometry -> c = (j + sh) * A, nearest voxel r = floor(c + 0.5) if 0 <= c <= P-1, else no source -> P-1-r on a
// flipped axis -> corner + r.  One thread = one output voxel, writes lane-consecutive along i2, as the kernels above.
struct AugDescs { n3d_patch_adesc d[N3D_PATCH_AUG_MAX_BATCH]; };

template <typename TT>
__global__ __launch_bounds__(256) void patch_gather_aug_kernel(const n3d_patch_volume* __restrict__ vols, int Cv, AugDescs descs, int P, int inclusive,
                                                               float* __restrict__ x_out, int64_t xld, TT* __restrict__ t_out, FastDiv fP,
                                                               FastDiv fPP) {
  const int b = blockIdx.y;
  const n3d_patch_adesc& ad = descs.d[b];
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= (uint32_t)P * P * P) return;
  const n3d_patch_volume r = vols[ad.g.vol];
  int s[3];
  patch_index(ad.g.d, v, P, fP, fPP, s);
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    int q = s[a];
    if (!ad.identity) {
      // scipy's zoom-shift coordinate: add, then multiply, each rounded to fp64; the bounds test is on the unrounded coordinate
      const double c = ((double)q + ad.sh[a]) * ad.A[a];
      const bool inside = 0.0 <= c && c <= (double)(P - 1);
      ok = ok && inside;
      q = inside ? (int)floor(c + 0.5) : 0;
    }
    s[a] = ad.g.d.corner[a] + (ad.aflip[a] ? P - 1 - q : q);
  }
  patch_voxel_store<TT>(r.data, Cv, r.truth, r.dims[0], r.dims[1], r.dims[2], s, ok, b, v, P, inclusive, x_out, xld, t_out);
}

// patch_gather_aug_kernel with a 3x4 resampling map, linear interpolation of the data and a per-channel intensity map (include/n3d.h,
// n3d_patch_wdesc, states the rule operation by operation).  The labels take the nearest voxel as above; the data takes it too (order
// 0) or the eight voxels around the coordinate (order 1), each tap flipped, offset by the corner and tested against the volume on its
// own.  mode, order and intensity are uniform over a workgroup (one patch per blockIdx.y).  Per output voxel at order 1: 8 * Cv loads
// against 4 * Cv bytes stored, but the two d_2 taps are adjacent in memory and neighbouring output voxels share six or more of their
// taps, so the source bytes that reach HBM stay those of the nearest gather; the taps are served by the L1 / L2 and what the kernel
// waits for is their latency: 2 x 4 x 64^3 rotated by 15 degrees takes 12.7 us at order 0 and 27.2 us at order 1, 27.6 us at order 1
// without a rotation (profiles/warp_probe.log; the plain gather: 11.4 us).
struct WarpDescs { n3d_patch_wdesc d[N3D_PATCH_WARP_MAX_BATCH]; };

// everything of the warp rule downstream of the coordinate c of output voxel v of patch b: bounds, nearest voxel, order 0 / 1, aflip,
// the crop's zero padding, the intensity map, the stores
template <typename TT>
__device__ __forceinline__ void patch_warp_resample(const n3d_patch_volume& r, const n3d_patch_wdesc& w, const double (&c)[3], int Cv, int b,
                                                    uint32_t v, int P, int inclusive, float* __restrict__ x_out, int64_t xld,
                                                    TT* __restrict__ t_out) {
  const uint32_t P3 = (uint32_t)P * P * P;
  const int X = r.dims[0], Y = r.dims[1], Z = r.dims[2];
  const int dims[3] = {X, Y, Z};
  const int64_t XYZ = (int64_t)X * Y * Z;
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = ok && 0.0 <= c[a] && c[a] <= (double)(P - 1);
  // the nearest voxel: the labels' source, and the data's at order 0
  bool in = ok;
  int64_t sv = 0;
  {
    int s[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int q = ok ? (int)floor(c[a] + 0.5) : 0;
      s[a] = w.g.d.corner[a] + (w.aflip[a] ? P - 1 - q : q);
      in = in && s[a] >= 0 && s[a] < dims[a];
    }
    if (in) sv = ((int64_t)s[0] * Y + s[1]) * Z + s[2];
  }
  const bool intensity = w.intensity != 0;
  const float* gain = w.gain;
  const float* bias = w.bias;
  // y != 0 is numpy's: -0.0 is zero and stays as it is (the lambdas capture by value: by reference the stores would be taken to alias)
  auto shade = [=](float y, int ch) {
    if (intensity && y != 0.f) {
      y = y * gain[ch & 3];
      y = y + bias[ch & 3];
    }
    return y;
  };
  if (w.order == 0) {
    patch_data_store(Cv, b, v, P3, x_out, xld, [=](int ch) { return shade(in ? r.data[ch * XYZ + sv] : 0.f, ch); });
  } else {
    // per axis the two tap indices (flipped, in the volume's frame), whether each is read, and its weight
    int64_t off[3][2];
    bool use[3][2];
    double u[3][2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double f = ok ? floor(c[a]) : 0.0;
      const double wa = ok ? c[a] - f : 0.0;
      u[a][0] = 1.0 - wa;
      u[a][1] = wa;
      const int64_t pitch = a == 0 ? (int64_t)Y * Z : (a == 1 ? (int64_t)Z : 1);
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const int q = (int)f + d;
        const int s = w.g.d.corner[a] + (w.aflip[a] ? P - 1 - q : q);
        use[a][d] = ok && q <= P - 1 && s >= 0 && s < dims[a];
        off[a][d] = use[a][d] ? s * pitch : 0;
      }
    }
    patch_data_store(Cv, b, v, P3, x_out, xld, [=](int ch) {
      const float* __restrict__ src = r.data + ch * XYZ;
      // the eight loads are issued together and unconditionally: a tap that is not used reads voxel 0 of the channel instead (its
      // offsets are 0) and is dropped by the select below.  One branch per tap would cost eight load round trips in a row.
      float x[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) x[t] = src[off[0][t >> 2] + off[1][(t >> 1) & 1] + off[2][t & 1]];
      double acc = 0.0;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int d0 = t >> 2, d1 = (t >> 1) & 1, d2 = t & 1;
        const double wt = (u[0][d0] * u[1][d1]) * u[2][d2];
        const double next = acc + wt * (double)x[t];
        acc = (use[0][d0] && use[1][d1] && use[2][d2]) ? next : acc;
      }
      return shade((float)acc, ch);
    });
  }
  if (t_out) patch_label_store<TT>(r.truth, in, sv, b, v, P3, inclusive, t_out);
}

template <typename TT>
__global__ __launch_bounds__(256) void patch_gather_warp_kernel(const n3d_patch_volume* __restrict__ vols, int Cv, WarpDescs descs, int P, int inclusive,
                                                                float* __restrict__ x_out, int64_t xld, TT* __restrict__ t_out, FastDiv fP,
                                                                FastDiv fPP) {
  const int b = blockIdx.y;
  const n3d_patch_wdesc& w = descs.d[b];
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= (uint32_t)P * P * P) return;
  const n3d_patch_volume r = vols[w.g.vol];
  int j[3];
  patch_index(w.g.d, v, P, fP, fPP, j);
  double c[3];
  patch_warp_coordinate(w, j, c);
  patch_warp_resample<TT>(r, w, c, Cv, b, v, P, inclusive, x_out, xld, t_out);
}

// patch_gather_warp_kernel with an elastic displacement added to the coordinate (include/n3d.h, n3d_patch_edesc, states the rule
// operation by operation): a cubic B-spline free-form deformation on a lattice of G = cells + 3 points per axis.  Each workgroup
// first writes its patch's 3 * G^3 control values into LDS -- at most 1331 Philox blocks per 256 threads, at most 31.9 KB of fp64;
// every workgroup of a patch regenerates the same lattice from the 8-byte key, nothing is read from memory -- and after a barrier
// every thread evaluates its voxel: 12 weights, then per component 64 LDS reads and 84 multiplies + 63 adds in the separable order.
// `elastic` is uniform over the workgroup (one patch per blockIdx.y): a patch without it skips the lattice and the barrier and is
// the warp kernel.  What a deformed voxel adds: 192 fp64 LDS reads (0.8 GB per 2 x 4 x 64^3 batch, some 10 us at the chip's LDS rate)
// and 441 fp64 operations (some 6 us).  2 x 4 x 64^3, both patches deformed: 27.2 us at cells 4 and order 0, 37.0 / 40.3 us at order 1
// and cells 4 / 8; with no patch deformed 13.4 us against the warp kernel's 11.5 (168 registers and the LDS leave fewer waves to
// hide the gather's loads): profiles/elastic_probe.log.  Not examined with counters.
// (ElasticDescs, the lattice and the displacement: patch_gather.h)
template <typename TT>
__global__ __launch_bounds__(256) void patch_gather_elastic_kernel(const n3d_patch_volume* __restrict__ vols, int Cv, ElasticDescs descs, int P,
                                                                   int inclusive, float* __restrict__ x_out, int64_t xld, TT* __restrict__ t_out,
                                                                   FastDiv fP, FastDiv fPP) {
  __shared__ double lattice[3 * kElasticMaxG3];
  const int b = blockIdx.y;
  const n3d_patch_edesc& e = descs.d[b];
  const n3d_patch_wdesc& w = e.w;
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  const bool elastic = e.elastic != 0;
  if (elastic) {
    elastic_lattice_fill(e, lattice);
    __syncthreads();      // every thread of the workgroup gets here: the ones past the patch's end leave only below
  }
  if (v >= (uint32_t)P * P * P) return;
  const n3d_patch_volume r = vols[w.g.vol];
  int j[3];
  patch_index(w.g.d, v, P, fP, fPP, j);
  double c[3];
  patch_warp_coordinate(w, j, c);
  if (elastic) elastic_displace(e, lattice, j, c);
  patch_warp_resample<TT>(r, w, c, Cv, b, v, P, inclusive, x_out, xld, t_out);
}

}  // namespace n3d

using namespace n3d;

extern "C" int n3d_patch_batch(const float* vol, int Cv, const uint8_t* truth, int X, int Y, int Z, const n3d_patch_desc* descs, int B, int P,
                               int flags, float* x_out, int64_t xld, void* t_out, void* stream) {
  N3D_CHECK_ARG(vol && descs && x_out && Cv >= 1 && X > 0 && Y > 0 && Z > 0 && P > 0 && B >= 1 && xld >= Cv, "patch_batch: bad args");
  N3D_CHECK_ARG(B <= N3D_PATCH_MAX_BATCH, "patch_batch: at most %d patches per call", N3D_PATCH_MAX_BATCH);
  N3D_CHECK_ARG(!t_out || truth, "patch_batch: targets requested without a truth volume");
  N3D_CHECK_ARG((int64_t)P * P * P < (1ll << 31) && (int64_t)X * Y * Z < (1ll << 40), "patch_batch: volume too large");
  PatchDescs pd;
  for (int i = 0; i < B; ++i) {
    pd.d[i] = descs[i];
    int seen = 0;
    for (int a = 0; a < 3; ++a) {
      N3D_CHECK_ARG(descs[i].perm[a] >= 0 && descs[i].perm[a] < 3, "patch_batch: perm entries must be 0..2");
      seen |= 1 << descs[i].perm[a];
    }
    N3D_CHECK_ARG(seen == 7, "patch_batch: perm must be a permutation of (0,1,2)");
  }
  for (int i = B; i < N3D_PATCH_MAX_BATCH; ++i) pd.d[i] = pd.d[0];
  const uint32_t P3 = (uint32_t)P * P * P;
  N3D_CHECK_ARG((flags & ~(N3D_PATCH_INCLUSIVE | N3D_PATCH_T_U8)) == 0, "patch_batch: unknown flag bits %d", flags);
  const int inclusive = flags & N3D_PATCH_INCLUSIVE;
  const dim3 grid((unsigned)cdiv(P3, 256), B);
  if (flags & N3D_PATCH_T_U8)
    N3D_LAUNCH(patch_batch_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, vol, Cv, truth, X, Y, Z, pd, P, inclusive, x_out, xld,
                       (uint8_t*)t_out, FastDiv((uint32_t)P), FastDiv((uint32_t)P * P));
  else
    N3D_LAUNCH(patch_batch_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, vol, Cv, truth, X, Y, Z, pd, P, inclusive, x_out, xld,
                       (float*)t_out, FastDiv((uint32_t)P), FastDiv((uint32_t)P * P));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_patch_gather(const n3d_patch_volume* vols, int nvol, int Cv, const n3d_patch_gdesc* descs, int B, int P, int flags,
                                float* x_out, int64_t xld, void* t_out, void* stream) {
  N3D_CHECK_ARG(vols && descs && x_out && nvol >= 1 && Cv >= 1 && P > 0 && B >= 1 && xld >= Cv, "patch_gather: bad args");
  N3D_CHECK_ARG(B <= N3D_PATCH_MAX_BATCH, "patch_gather: at most %d patches per call", N3D_PATCH_MAX_BATCH);
  N3D_CHECK_ARG((int64_t)P * P * P < (1ll << 31), "patch_gather: patch too large");
  GatherDescs gd;
  for (int i = 0; i < B; ++i) {
    gd.d[i] = descs[i];
    N3D_CHECK_ARG(descs[i].vol >= 0 && descs[i].vol < nvol, "patch_gather: descriptor %d names volume %d of a set of %d", i, descs[i].vol, nvol);
    int seen = 0;
    for (int a = 0; a < 3; ++a) {
      N3D_CHECK_ARG(descs[i].d.perm[a] >= 0 && descs[i].d.perm[a] < 3, "patch_gather: perm entries must be 0..2");
      seen |= 1 << descs[i].d.perm[a];
    }
    N3D_CHECK_ARG(seen == 7, "patch_gather: perm must be a permutation of (0,1,2)");
  }
  for (int i = B; i < N3D_PATCH_MAX_BATCH; ++i) gd.d[i] = gd.d[0];
  N3D_CHECK_ARG((flags & ~(N3D_PATCH_INCLUSIVE | N3D_PATCH_T_U8)) == 0, "patch_gather: unknown flag bits %d", flags);
  const uint32_t P3 = (uint32_t)P * P * P;
  const int inclusive = flags & N3D_PATCH_INCLUSIVE;
  const dim3 grid((unsigned)cdiv(P3, 256), B);
  if (flags & N3D_PATCH_T_U8)
    N3D_LAUNCH(patch_gather_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, vols, Cv, gd, P, inclusive, x_out, xld,
                       (uint8_t*)t_out, FastDiv((uint32_t)P), FastDiv((uint32_t)P * P));
  else
    N3D_LAUNCH(patch_gather_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, vols, Cv, gd, P, inclusive, x_out, xld,
                       (float*)t_out, FastDiv((uint32_t)P), FastDiv((uint32_t)P * P));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_patch_gather_aug(const n3d_patch_volume* vols, int nvol, int Cv, const n3d_patch_adesc* descs, int B, int P, int flags,
                                    float* x_out, int64_t xld, void* t_out, void* stream) {
  N3D_CHECK_ARG(vols && descs && x_out && nvol >= 1 && Cv >= 1 && P > 0 && B >= 1 && xld >= Cv, "patch_gather_aug: bad args");
  N3D_CHECK_ARG(B <= N3D_PATCH_AUG_MAX_BATCH, "patch_gather_aug: at most N3D_PATCH_AUG_MAX_BATCH = %d patches per call (got %d)",
                N3D_PATCH_AUG_MAX_BATCH, B);
  N3D_CHECK_ARG((int64_t)P * P * P < (1ll << 31), "patch_gather_aug: patch too large");
  static_assert(sizeof(AugDescs) + 64 <= 4096, "the descriptors travel by value in the kernel arguments (4 KB)");
  AugDescs ad;
  for (int i = 0; i < B; ++i) {
    const n3d_patch_adesc& d = descs[i];
    ad.d[i] = d;
    N3D_CHECK_ARG(d.g.vol >= 0 && d.g.vol < nvol, "patch_gather_aug: descriptor %d names volume %d of a set of %d", i, d.g.vol, nvol);
    int seen = 0;
    for (int a = 0; a < 3; ++a) {
      N3D_CHECK_ARG(d.g.d.perm[a] >= 0 && d.g.d.perm[a] < 3, "patch_gather_aug: perm entries must be 0..2");
      seen |= 1 << d.g.d.perm[a];
      N3D_CHECK_ARG(std::isfinite(d.A[a]) && d.A[a] != 0.0 && std::isfinite(d.sh[a]),
                    "patch_gather_aug: descriptor %d axis %d: A must be finite and nonzero and sh finite (got %g, %g)", i, a, d.A[a], d.sh[a]);
    }
    N3D_CHECK_ARG(seen == 7, "patch_gather_aug: perm must be a permutation of (0,1,2)");
  }
  for (int i = B; i < N3D_PATCH_AUG_MAX_BATCH; ++i) ad.d[i] = ad.d[0];
  N3D_CHECK_ARG((flags & ~(N3D_PATCH_INCLUSIVE | N3D_PATCH_T_U8)) == 0, "patch_gather_aug: unknown flag bits %d", flags);
  const uint32_t P3 = (uint32_t)P * P * P;
  const int inclusive = flags & N3D_PATCH_INCLUSIVE;
  const dim3 grid((unsigned)cdiv(P3, 256), B);
  if (flags & N3D_PATCH_T_U8)
    N3D_LAUNCH(patch_gather_aug_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, vols, Cv, ad, P, inclusive, x_out, xld,
                       (uint8_t*)t_out, FastDiv((uint32_t)P), FastDiv((uint32_t)P * P));
  else
    N3D_LAUNCH(patch_gather_aug_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, vols, Cv, ad, P, inclusive, x_out, xld,
                       (float*)t_out, FastDiv((uint32_t)P), FastDiv((uint32_t)P * P));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_patch_gather_warp(const n3d_patch_volume* vols, int nvol, int Cv, const n3d_patch_wdesc* descs, int B, int P, int flags,
                                     float* x_out, int64_t xld, void* t_out, void* stream) {
  N3D_CHECK_ARG(vols && descs && x_out && nvol >= 1 && Cv >= 1 && P > 0 && B >= 1 && xld >= Cv, "patch_gather_warp: bad args");
  N3D_CHECK_ARG(B <= N3D_PATCH_WARP_MAX_BATCH, "patch_gather_warp: at most N3D_PATCH_WARP_MAX_BATCH = %d patches per call (got %d)",
                N3D_PATCH_WARP_MAX_BATCH, B);
  N3D_CHECK_ARG((int64_t)P * P * P < (1ll << 31), "patch_gather_warp: patch too large");
  static_assert(sizeof(WarpDescs) + 64 <= 4096, "the descriptors travel by value in the kernel arguments (4 KB)");
  WarpDescs wd;
  for (int i = 0; i < B; ++i) {
    wd.d[i] = descs[i];
    if (int rc = patch_wdesc_check("patch_gather_warp", descs[i], i, nvol, Cv)) return rc;
  }
  for (int i = B; i < N3D_PATCH_WARP_MAX_BATCH; ++i) wd.d[i] = wd.d[0];
  N3D_CHECK_ARG((flags & ~(N3D_PATCH_INCLUSIVE | N3D_PATCH_T_U8)) == 0, "patch_gather_warp: unknown flag bits %d", flags);
  const uint32_t P3 = (uint32_t)P * P * P;
  const int inclusive = flags & N3D_PATCH_INCLUSIVE;
  const dim3 grid((unsigned)cdiv(P3, 256), B);
  if (flags & N3D_PATCH_T_U8)
    N3D_LAUNCH(patch_gather_warp_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, vols, Cv, wd, P, inclusive, x_out, xld,
                       (uint8_t*)t_out, FastDiv((uint32_t)P), FastDiv((uint32_t)P * P));
  else
    N3D_LAUNCH(patch_gather_warp_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, vols, Cv, wd, P, inclusive, x_out, xld,
                       (float*)t_out, FastDiv((uint32_t)P), FastDiv((uint32_t)P * P));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_patch_gather_elastic(const n3d_patch_volume* vols, int nvol, int Cv, const n3d_patch_edesc* descs, int B, int P, int flags,
                                        float* x_out, int64_t xld, void* t_out, void* stream) {
  N3D_CHECK_ARG(vols && descs && x_out && nvol >= 1 && Cv >= 1 && P > 0 && B >= 1 && xld >= Cv, "patch_gather_elastic: bad args");
  N3D_CHECK_ARG(B <= N3D_PATCH_ELASTIC_MAX_BATCH, "patch_gather_elastic: at most N3D_PATCH_ELASTIC_MAX_BATCH = %d patches per call (got %d)",
                N3D_PATCH_ELASTIC_MAX_BATCH, B);
  N3D_CHECK_ARG((int64_t)P * P * P < (1ll << 31), "patch_gather_elastic: patch too large");
  static_assert(sizeof(ElasticDescs) + 64 <= 4096, "the descriptors travel by value in the kernel arguments (4 KB)");
  static_assert(sizeof(n3d_patch_edesc) == 248, "n3d_patch_edesc: no hidden padding");
  ElasticDescs ed;
  for (int i = 0; i < B; ++i) {
    const n3d_patch_edesc& d = descs[i];
    ed.d[i] = d;
    if (int rc = patch_wdesc_check("patch_gather_elastic", d.w, i, nvol, Cv)) return rc;
    if (int rc = patch_edesc_check("patch_gather_elastic", d, i)) return rc;
  }
  for (int i = B; i < N3D_PATCH_ELASTIC_MAX_BATCH; ++i) ed.d[i] = ed.d[0];
  N3D_CHECK_ARG((flags & ~(N3D_PATCH_INCLUSIVE | N3D_PATCH_T_U8)) == 0, "patch_gather_elastic: unknown flag bits %d", flags);
  const uint32_t P3 = (uint32_t)P * P * P;
  const int inclusive = flags & N3D_PATCH_INCLUSIVE;
  const dim3 grid((unsigned)cdiv(P3, 256), B);
  if (flags & N3D_PATCH_T_U8)
    N3D_LAUNCH(patch_gather_elastic_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, vols, Cv, ed, P, inclusive, x_out, xld,
                       (uint8_t*)t_out, FastDiv((uint32_t)P), FastDiv((uint32_t)P * P));
  else
    N3D_LAUNCH(patch_gather_elastic_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, vols, Cv, ed, P, inclusive, x_out, xld,
                       (float*)t_out, FastDiv((uint32_t)P), FastDiv((uint32_t)P * P));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}
