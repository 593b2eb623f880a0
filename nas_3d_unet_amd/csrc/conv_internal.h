// What the conv files (conv_generic.hip, conv_mfma.hip, conv_bf16.hip) share on the host side: the operand records they hand to each
// other and the prototype of every function one of them calls in another.  Declarations only.
#pragma once
#include <atomic>
#include "n3d_common.h"

namespace n3d {

// One conv in gather form, as the entry points hand it to the kernel families.  data_grad is the gather direction: forward conv =
// false, transposed forward = true; data gradient of a conv = true, of a transposed conv = false.  relu_src / rld / out_gate are the
// data-gradient extras (ReLU mask source of the conv input and its pitch, per-(b,c) gate applied to the result).
struct ConvCall {
  const n3d_conv_geom* g; bool data_grad; const float* src; int64_t sld; const float* w; const float* bias; float* dst; int64_t dld; int flags;
  const float* in_gate; const float* relu_src; int64_t rld; const float* out_gate; double* stats; void* ws; size_t ws_bytes;
};

// one conv's backward operands (data + weight gradient) for the dual / quad launches; nch / ntl come back from mfma_bwd_dual_try
struct BwdOne {
  const n3d_conv_geom* g; bool transposed; const float* dy; int64_t dyld; const float* wp; float* dx; int64_t dxld; int flags_d;
  const float* relu_src; int64_t rld; const float* out_gate; const float* x; int64_t xld; int flags_w; const float* in_gate;
  float* partial; float* pbias; size_t avail; int nch, ntl;
};

// geometry and direction -> the gather map  src coordinate = (dst*sn + off + tap*dt) / den  with its source and destination extents
struct GatherGeom { int Ds, Hs, Ws, Cs, Dd, Hd, Wd, Cd, sn, off, dt, den; };
static inline GatherGeom gather_geom(const n3d_conv_geom* g, bool data_grad) {
  if (!data_grad) return GatherGeom{g->Di, g->Hi, g->Wi, g->Ci, g->Do, g->Ho, g->Wo, g->Co, g->stride, -g->pad, g->dil, 1};
  return GatherGeom{g->Do, g->Ho, g->Wo, g->Co, g->Di, g->Hi, g->Wi, g->Ci, 1, g->pad, -g->dil, g->stride};
}
// into the like-named members of a kernel argument struct (GatherArgs, MfArgs)
template <typename Args>
static inline void set_gather_geom(Args& a, const GatherGeom& m) {
  a.Ds = m.Ds; a.Hs = m.Hs; a.Ws = m.Ws; a.Cs = m.Cs; a.Dd = m.Dd; a.Hd = m.Hd; a.Wd = m.Wd; a.Cd = m.Cd;
  a.sn = m.sn; a.off = m.off; a.dt = m.dt; a.den = m.den;
}

// ---- conv_mfma.hip.  The *_try functions return 1 if they handled the call, 0 to fall through, < 0 on error
struct Wg16Args;
struct DualArgs;
extern std::atomic<int64_t> g_fold_launches[5];
int mfma_conv_try(const ConvCall& c, hipStream_t s);
int mfma_conv_stats_rows(const n3d_conv_geom* g, bool data_grad, int flags);
int mfma_pack_layout(const n3d_conv_geom* g, bool data_grad, int flags);  // 1 gemm16, 2 vox64, 3 vox_up, 0 none
void mfma_pack16(const float* w, float* wp, int Co, int Ci, int taps, int data_grad, hipStream_t s);
int mfma_conv_pair_try(const ConvCall& c0, const ConvCall& c1, hipStream_t s);
// the data-gradient pair of a node with its GroupNorm-epilogue backward rebuilt in the launch (c_i multiplies d(raw) of term t_i):
// 1 = taken (launched unless `launch` is false: the query and the entry point share the decision), 0 = declined, nothing touched
int mfma_gn_fold_pair(const float* dout, int64_t dld, const n3d_gn_bwd_term* t0, const n3d_gn_bwd_term* t1, int B, int64_t N, int C, int G,
                      const ConvCall& c0, const ConvCall& c1, hipStream_t s, bool launch);
int mfma_conv_multi_try(int n, const ConvCall* c, hipStream_t s);
int mfma_vox_multi_try(int n, const ConvCall* c, hipStream_t s);
int mfma_vox_multi_folds(int n, const ConvCall* c);      // 1 = mfma_vox_multi_try would launch (the same decision code)
int vox_wgrad_try(const n3d_conv_geom* g, const float* x, int64_t xld, const float* dy, int64_t dyld, int flags, const float* in_gate,
                  float* partial, size_t avail_floats, int* nchunks_out, hipStream_t s);
int vox_wgrad_s2_try(const n3d_conv_geom* g, const float* x, int64_t xld, const float* dy, int64_t dyld, int flags, const float* in_gate,
                     float* partial, size_t avail_floats, int* nchunks_out, hipStream_t s);
int wgrad_tile16_try(const n3d_conv_geom* g, const float* x, int64_t xld, const float* dy, int64_t dyld, int flags, const float* in_gate,
                     float* partial, size_t avail_floats, int* nchunks_out, float** pbias_out, hipStream_t s);
bool wgrad_tile16_plan(const n3d_conv_geom* g, int* chunks, int* tiles_per_wg, int* tw_out = nullptr);
int mfma_wgrad_try(const n3d_conv_geom* g, const float* x, int64_t xld, const float* dy, int64_t dyld, int flags, const float* in_gate,
                   float* partial, float* pbias, size_t avail_floats, int* nchunks_out, int* ntiles_out, hipStream_t s,
                   Wg16Args* prepared = nullptr);
// writes c->nch / c->ntl; with `prepared` it fills the launch arguments and the K split instead of launching (mfma_bwd_quad_try)
int mfma_bwd_dual_try(BwdOne* c, hipStream_t s, DualArgs* prepared = nullptr, int* ksplit_out = nullptr);
int mfma_bwd_quad_ok(const n3d_conv_geom* g0, bool t0, const n3d_conv_geom* g1, bool t1);
int mfma_bwd_quad_try(BwdOne* c0, BwdOne* c1, hipStream_t s);

// ---- conv_bf16.hip: the bf16-storage vox64 family (src / dst / relu_src of the record point at bf16 elements)
int vox16_layout(const n3d_conv_geom* g, bool data_grad, int flags);
int vox16_stats_rows(const n3d_conv_geom* g, bool data_grad, int flags);
int vox16_conv_try(const ConvCall& c, hipStream_t s);

}  // namespace n3d
