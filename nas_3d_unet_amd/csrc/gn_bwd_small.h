// The GroupNorm-epilogue backward of the small levels, piece by piece: what gn_bwd_small2_kernel (elementwise.hip) and the data-gradient
// pair launch that rebuilds d(raw) in its prologue (conv_gemm16_gnpair_kernel, conv_mfma.hip) both call, so that the two produce the
// same bits -- the masked gradient of a channel quad, its wave-level class sums, the fp64 coefficient math of one (sample, channel)
// and the d(raw) of a quad.  Device code only; the argument record of a term is shared with the other epilogue kernels.
#pragma once
#include "n3d_common.h"

namespace n3d {

struct GnBwdTerm {
  const float* raw; int64_t rld; const float* a; const float* b; const double* sums; int rows; const float* gamma; const float* mean_rstd;
  const float* wptr; const double* sumraw; float* draw; int64_t drld; float* dgamma; float* dbeta; float* dalpha; float* dbias_conv; int relu;
  const float* cA; const float* cB; const float* cC;   // PRE variant: coefficients from n3d_gn_bwd_coeffs2
};

#ifdef __HIPCC__
// g = dout behind the term's ReLU mask and g * raw of one channel quad (ok: the quad exists -- idle lanes pad a sample to whole waves)
__device__ __forceinline__ void gn_small_masked(const float (&dd)[4], const float (&ra)[4], const float4 fa, const float4 fb, const bool ok,
                                                const float thr, float (&gmv)[4], float (&grv)[4]) {
  const float aa[4] = {fa.x, fa.y, fa.z, fa.w}, bb[4] = {fb.x, fb.y, fb.z, fb.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float z = fmaf(aa[j], ra[j], bb[j]);
    gmv[j] = (ok && z > thr) ? dd[j] : 0.f;
    grv[j] = gmv[j] * ra[j];
  }
}
// the wave's sums of S1 = sum g and S2 = sum g * raw per channel of the group, into one slot row [(S1 | S2) x 16 channels]: the four
// channels of the quad reduced together (wave_classsum4_f): row r of the wave ends up with channel {0,2,1,3}[r]
template <int CPB>
__device__ __forceinline__ void gn_small_wave_sums(const float (&gmv)[4], const float (&grv)[4], const int lane, float* __restrict__ row) {
  const float s1 = wave_classsum4_f<CPB>(gmv[0], gmv[1], gmv[2], gmv[3]), s2 = wave_classsum4_f<CPB>(grv[0], grv[1], grv[2], grv[3]);
  const int l16 = lane & 15, j = classsum4_sel(lane);
  if (l16 < CPB) { row[l16 * 4 + j] = s1; row[16 + l16 * 4 + j] = s2; }
}
// coefficients of d(raw) = A * g + B + C * raw of (sample gb, channel c of group g) and the sample's contributions to dgamma / dbeta /
// the conv-bias gradient, from the group's sums tot = [(S1 | S2) x 16 channels] (fp64)
struct GnSmallCoef { float A, B, C; double cdg, cdb, cdc; };
__device__ __forceinline__ GnSmallCoef gn_small_coeffs(const GnBwdTerm& tm, const double* __restrict__ tot, const int gb, const int g, const int c,
                                                       const int cg, const int C, const int G, const double count) {
  const double w = tm.wptr ? (double)*tm.wptr : 1.0;
  const double mn = tm.mean_rstd[(gb * G + g) * 2], rsd = tm.mean_rstd[(gb * G + g) * 2 + 1];
  double c1 = 0, c2 = 0;
  for (int cc = 0; cc < cg; ++cc) {
    const double gm = (double)tm.gamma[g * cg + cc];
    const double S1 = tot[cc], S2 = tot[16 + cc];
    c1 += gm * w * S1;
    c2 += gm * w * rsd * (S2 - mn * S1);
  }
  const double n = count * cg;
  c1 /= n; c2 /= n;
  const double gam = (double)tm.gamma[g * cg + c];
  const double S1 = tot[c], S2 = tot[16 + c];
  const double Av = rsd * gam * w, Bv = -rsd * c1 + rsd * rsd * c2 * mn, Cv = -rsd * rsd * c2;
  GnSmallCoef r;
  r.A = (float)Av; r.B = (float)Bv; r.C = (float)Cv;
  r.cdg = w * rsd * (S2 - mn * S1);
  r.cdb = w * S1;
  r.cdc = tm.dbias_conv ? Av * S1 + count * Bv + Cv * tm.sumraw[gb * C + g * cg + c] : 0.0;
  return r;
}
// d(raw) of one channel quad
__device__ __forceinline__ float4 gn_small_draw4(const float (&dd)[4], const float (&ra)[4], const float4 fa, const float4 fb, const float4 qA,
                                                 const float4 qB, const float4 qC, const float thr) {
  const float aa[4] = {fa.x, fa.y, fa.z, fa.w}, bb[4] = {fb.x, fb.y, fb.z, fb.w};
  const float A4[4] = {qA.x, qA.y, qA.z, qA.w}, B4[4] = {qB.x, qB.y, qB.z, qB.w}, C4[4] = {qC.x, qC.y, qC.z, qC.w};
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float z = fmaf(aa[j], ra[j], bb[j]);
    const float gm = z > thr ? dd[j] : 0.f;
    o[j] = fmaf(A4[j], gm, fmaf(C4[j], ra[j], B4[j]));
  }
  return make_float4(o[0], o[1], o[2], o[3]);
}
#endif

}  // namespace n3d
