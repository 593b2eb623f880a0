// What the patch gathers of data_step.hip and spline.hip share: the stores of an output voxel, the isometry's patch index, the warp
// rule's coordinate, the elastic displacement and the host checks of a descriptor (include/n3d.h states every rule operation by
// operation).  Both files are compiled with -ffp-contract=off (Makefile): every fp64 product and sum below is rounded on its own.
#pragma once
#include "n3d_common.h"

#include <cmath>

namespace n3d {

// the Cv data values of output voxel v of patch b, value(c) for channel c: one float4 for Cv == 4 on an aligned pitch
template <typename F>
__device__ __forceinline__ void patch_data_store(int Cv, int b, uint32_t v, uint32_t P3, float* __restrict__ x_out, int64_t xld, F value) {
  float* xo = x_out + ((int64_t)b * P3 + v) * xld;
  if (Cv == 4 && (xld & 3) == 0) {
    float4 q;
    q.x = value(0); q.y = value(1); q.z = value(2); q.w = value(3);
    *reinterpret_cast<float4*>(xo) = q;
  } else {
    for (int c = 0; c < Cv; ++c) xo[c] = value(c);
  }
}

// the three target maps of output voxel v of patch b from its label voxel sv (in = false: no source, label 0)
template <typename TT>
__device__ __forceinline__ void patch_label_store(const uint8_t* __restrict__ truth, bool in, int64_t sv, int b, uint32_t v, uint32_t P3,
                                                  int inclusive, TT* __restrict__ t_out) {
  // (a gathered patch whose volume has no truth reads as label 0 everywhere; n3d_patch_batch never gets here without truth)
  const int l = (in && truth) ? (int)truth[sv] : 0;
  // generator.py:241-243 -- the inclusive "whole tumour" channel is labels {1, 2}: np.logical_or's third argument
  // is its OUT array there, so label 4 does not enter (reproduced, not corrected)
  const TT c0 = inclusive ? (TT)(l == 1 || l == 4) : (TT)(l == 1);
  const TT c1 = inclusive ? (TT)(l == 1 || l == 2) : (TT)(l == 2);
  const TT c2 = (TT)(l == 4);
  TT* to = t_out + (int64_t)b * 3 * P3 + v;
  to[0] = c0; to[P3] = c1; to[2 * (int64_t)P3] = c2;
}

// patch index of output voxel v on source axis a under the isometry of d: j_a = i[perm[a]], or P-1-i[perm[a]] with flip[a]
__device__ __forceinline__ void patch_index(const n3d_patch_desc& d, uint32_t v, int P, FastDiv fP, FastDiv fPP, int (&j)[3]) {
  uint32_t i0, r, i1, i2;
  fPP.divmod(v, i0, r);
  fP.divmod(r, i1, i2);
  const int idx[3] = {(int)i0, (int)i1, (int)i2};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int t = d.perm[a] == 0 ? idx[0] : (d.perm[a] == 1 ? idx[1] : idx[2]);
    j[a] = d.flip[a] ? P - 1 - t : t;
  }
}

// the warp rule's coordinate of patch index j
__device__ __forceinline__ void patch_warp_coordinate(const n3d_patch_wdesc& w, const int (&j)[3], double (&c)[3]) {
  if (w.mode == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = ((double)j[a] + w.k[3 + a]) * w.k[a];
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double t = w.k[3 * a] * (double)j[0];
      t = t + w.k[3 * a + 1] * (double)j[1];
      t = t + w.k[3 * a + 2] * (double)j[2];
      c[a] = t + w.k[9 + a];
    }
  }
}

struct ElasticDescs { n3d_patch_edesc d[N3D_PATCH_ELASTIC_MAX_BATCH]; };
constexpr int kElasticMaxG = N3D_PATCH_ELASTIC_MAX_CELLS + 3;
constexpr int kElasticMaxG3 = kElasticMaxG * kElasticMaxG * kElasticMaxG;

// the four uniform cubic B-spline weights of f
__device__ __forceinline__ void bspline_weights(double f, double (&bw)[4]) {
  const double S = 1.0 / 6.0;
  const double g = 1.0 - f;
  bw[0] = ((g * g) * g) * S;
  bw[1] = ((((3.0 * f - 6.0) * f) * f) + 4.0) * S;
  bw[2] = ((((3.0 - 3.0 * f) * f + 3.0) * f) + 1.0) * S;
  bw[3] = ((f * f) * f) * S;
}

// the 3 * G^3 control values of e into `lattice` (LDS, 3 * kElasticMaxG3 doubles), by all 256 threads of the workgroup; the
// caller's barrier follows
__device__ __forceinline__ void elastic_lattice_fill(const n3d_patch_edesc& e, double* lattice) {
  const int G = e.cells + 3, G3 = G * G * G;               // the host checked 1 <= cells <= N3D_PATCH_ELASTIC_MAX_CELLS
  const int L = e.lock;
  for (int l = threadIdx.x; l < G3; l += 256) {
    const int l0 = l / (G * G), l1 = (l / G) % G, l2 = l % G;
    const bool locked = l0 < L || l0 >= G - L || l1 < L || l1 >= G - L || l2 < L || l2 >= G - L;
    uint32_t r[4];
    philox4x32_10((uint32_t)l, 1, 0, 0, e.key[0], e.key[1], r);
#pragma unroll
    for (int a = 0; a < 3; ++a) lattice[a * G3 + l] = locked ? 0.0 : 2.0 * ((double)r[a] * 0x1p-32) - 1.0;
  }
}

// c = c + delta at the patch index j, from the lattice elastic_lattice_fill wrote
__device__ __forceinline__ void elastic_displace(const n3d_patch_edesc& e, const double* lattice, const int (&j)[3], double (&c)[3]) {
  const int n = e.cells, G = n + 3, G3 = G * G * G;
  double bw[3][4];
  int cell[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double s = (double)j[a] * e.inv_h;
    cell[a] = (int)fmin(floor(s), (double)(n - 1));       // s >= 0 (inv_h >= 0 was checked): 0 <= cell <= n - 1, cell + 3 <= G - 1
    bspline_weights(s - (double)cell[a], bw[a]);
  }
  const int base = (cell[0] * G + cell[1]) * G + cell[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double* __restrict__ D = lattice + a * G3 + base;
    double U[4];
#pragma unroll
    for (int m0 = 0; m0 < 4; ++m0) {
      double T[4];
#pragma unroll
      for (int m1 = 0; m1 < 4; ++m1) {
        const double* d = D + (m0 * G + m1) * G;
        double t = bw[2][0] * d[0];
        t = t + bw[2][1] * d[1];
        t = t + bw[2][2] * d[2];
        T[m1] = t + bw[2][3] * d[3];
      }
      double u = bw[1][0] * T[0];
      u = u + bw[1][1] * T[1];
      u = u + bw[1][2] * T[2];
      U[m0] = u + bw[1][3] * T[3];
    }
    double acc = bw[0][0] * U[0];
    acc = acc + bw[0][1] * U[1];
    acc = acc + bw[0][2] * U[2];
    acc = acc + bw[0][3] * U[3];
    c[a] = c[a] + e.amp[a] * acc;
  }
}

// the checks of one n3d_patch_wdesc, for the entry point `fn`; spline: the entry takes order 3 only, else 0 / 1 only
static inline int patch_wdesc_check(const char* fn, const n3d_patch_wdesc& d, int i, int nvol, int Cv, bool spline = false) {
  N3D_CHECK_ARG(d.g.vol >= 0 && d.g.vol < nvol, "%s: descriptor %d names volume %d of a set of %d", fn, i, d.g.vol, nvol);
  int seen = 0;
  for (int a = 0; a < 3; ++a) {
    N3D_CHECK_ARG(d.g.d.perm[a] >= 0 && d.g.d.perm[a] < 3, "%s: perm entries must be 0..2", fn);
    seen |= 1 << d.g.d.perm[a];
  }
  N3D_CHECK_ARG(seen == 7, "%s: perm must be a permutation of (0,1,2)", fn);
  N3D_CHECK_ARG(d.mode == 0 || d.mode == 1, "%s: descriptor %d: mode must be 0 or 1 (got %d)", fn, i, d.mode);
  if (spline)
    N3D_CHECK_ARG(d.order == 3, "%s: descriptor %d: order must be 3 (got %d)", fn, i, d.order);
  else
    N3D_CHECK_ARG(d.order == 0 || d.order == 1, "%s: descriptor %d: order must be 0 or 1 (got %d)", fn, i, d.order);
  for (int n = 0; n < 12; ++n) N3D_CHECK_ARG(std::isfinite(d.k[n]), "%s: descriptor %d: coefficient %d must be finite (got %g)", fn, i, n, d.k[n]);
  for (int a = 0; a < 3 && d.mode == 0; ++a) N3D_CHECK_ARG(d.k[a] != 0.0, "%s: descriptor %d axis %d: A must be nonzero in mode 0", fn, i, a);
  for (int c = 0; c < 4; ++c)
    N3D_CHECK_ARG(std::isfinite(d.gain[c]) && std::isfinite(d.bias[c]), "%s: descriptor %d channel %d: gain and bias must be finite (got %g, %g)", fn,
                  i, c, d.gain[c], d.bias[c]);
  N3D_CHECK_ARG(!d.intensity || Cv <= 4, "%s: descriptor %d: the intensity map supports at most 4 channels (got %d)", fn, i, Cv);
  return N3D_OK;
}

// the lattice checks of one n3d_patch_edesc (its `w` is patch_wdesc_check's), for the entry point `fn`
static inline int patch_edesc_check(const char* fn, const n3d_patch_edesc& d, int i) {
  N3D_CHECK_ARG(d.cells >= 1 && d.cells <= N3D_PATCH_ELASTIC_MAX_CELLS, "%s: descriptor %d: cells must be 1..%d (got %d)", fn, i,
                N3D_PATCH_ELASTIC_MAX_CELLS, d.cells);
  N3D_CHECK_ARG(d.lock >= 0 && d.lock <= 3, "%s: descriptor %d: lock must be 0..3 (got %d)", fn, i, d.lock);
  N3D_CHECK_ARG(d.cells + 3 - 2 * d.lock >= 1, "%s: descriptor %d: lock %d leaves no free control point on a lattice of %d", fn, i, d.lock,
                d.cells + 3);
  for (int a = 0; a < 3; ++a)
    N3D_CHECK_ARG(std::isfinite(d.amp[a]) && d.amp[a] >= 0.0, "%s: descriptor %d axis %d: amp must be finite and >= 0 (got %g)", fn, i, a, d.amp[a]);
  N3D_CHECK_ARG(std::isfinite(d.inv_h) && d.inv_h >= 0.0, "%s: descriptor %d: inv_h must be finite and >= 0 (got %g)", fn, i, d.inv_h);
  return N3D_OK;
}

}  // namespace n3d
