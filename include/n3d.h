/*
 * n3d.h -- C ABI of libn3d.so: gfx950 (MI355X) HIP kernels for the nas_3d_unet hot path.
 *
 * The reference (woodywff/nas_3d_unet) has NO native layer and NO FFI: its hot path is a
 * Python module API (prim_ops.py / cell.py) whose arithmetic is delegated to torch.nn.
 * Each entry point below therefore cites the reference *call site* whose torch op it replaces
 * (file:line relative to the reference root).  The Python host (nas_3d_unet_amd/) binds these
 * with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (n3d_last_error() has the text);
 *     nothing throws, allocates, or synchronises; all work is enqueued on `stream`
 *     (a hipStream_t passed as void*), so calls are HIP-graph capturable.
 *   - activations are fp32, NDHWC ("channels-last-3d"): element (b,d,h,w,c) of a tensor with
 *     voxel pitch `ld` (floats, ld >= C) lives at ((((b*D+d)*H+h)*W+w)*ld + c).  A pitch larger
 *     than C addresses a channel slice of a wider buffer (zero-copy concat, cell.py:82).
 *   - weights keep torch's native layouts: Conv3d (Cout, Cin/g, k,k,k), ConvTranspose3d
 *     (Cin, Cout/g, k,k,k), Linear (out, in), so reference state_dicts load unchanged.
 *   - per-(sample,channel) reductions are deterministic two-stage sums: a producer kernel writes
 *     one partial row of doubles per workgroup, `double[B][rows][C][nv]`, and a tiny coefficient
 *     kernel adds the rows in a fixed order.  `rows` comes from n3d_stats_rows() /
 *     n3d_conv_stats_rows() so the caller can size the buffer; no atomics, no zeroing.
 */
#ifndef N3D_H_
#define N3D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define N3D_OK 0
#define N3D_ERR_INVALID (-1)
#define N3D_ERR_UNSUPPORTED (-2)
#define N3D_ERR_HIP (-3)
#define N3D_ERR_WORKSPACE (-4)

/* flags */
#define N3D_RELU_IN 1     /* apply ReLU to the conv input on load ('act_weight_norm', cell.py:47-50) */
#define N3D_RELU 2        /* epilogue activation is ReLU (prim_ops.py:63,80) */
#define N3D_ACCUMULATE 4  /* destination += result instead of = result */
#define N3D_POOL_MAX 8    /* pooling type (prim_ops.py:160-163) */
#define N3D_NO_MFMA 16    /* force the generic VALU kernels (A/B testing) */
#define N3D_PREPACKED 32  /* `ws` already holds this conv's packed weights (written by n3d_pack_batch) */
/* storage types (bf16 configuration, BASELINE configs[4]): activation pointers are declared `float*` for the fp32 path; with one of
 * these flags the tensor holds bfloat16 elements instead (pitches then count bf16 elements, 4-channel groups must be 8-byte aligned)
 * and the kernel converts on load / store, computing in fp32.  Conv family: SRC = the first activation tensor of the call (x; dy of a
 * data gradient; x of a weight gradient), DST = the second (y; dx and relu_src of a data gradient; dy of a weight gradient).
 * Epilogue family (n3d_channel_stats / n3d_affine_act*): every activation tensor of one call shares ONE type, N3D_ACT_BF16 (or the
 * `dtype` field of the term structures).
 * READABLE SLACK: the 3x3x3 kernels of the bf16 path fill their LDS tiles 16 bytes per voxel (LDS-DMA), so a bf16 tensor with
 * 4 channels (an 8-byte voxel) is read up to 8 bytes past its last element.  Every bf16 activation tensor handed to the conv
 * family must therefore be followed by at least 16 readable bytes in the same allocation (their content is ignored); the
 * Python host allocates bf16 tensors with that slack and repacks foreign ones (kernels.as_view). */
#define N3D_SRC_BF16 64
#define N3D_DST_BF16 128
#define N3D_ACT_BF16 64
/* bf16 configuration, the C >= 16 levels (fp32 storage): the MFMA kernels of the conv family (forward, data and weight gradients with
 * channel counts that are multiples of 16) round BOTH operands of their matrix products to bfloat16 in registers and accumulate in
 * fp32 (v_mfma_f32_16x16x16_bf16 instead of four v_mfma_f32_16x16x4_f32).  Ignored by every other kernel.  Never set by the fp32
 * configuration, whose arithmetic is exact fp32. */
#define N3D_MM_BF16 256
/* Small pointwise convs (1x1x1, fp32, channel counts and pitches multiples of 4, 16-byte aligned rows, no node-planar operand:
 * forward at stride 1 or 2, data gradient at stride 1, data gradient at stride 2 without bias and statistics) that neither the MFMA
 * family nor the 1x1x1 streaming kernel takes run on an LDS-weight kernel (conv_point_kernel) that performs the generic gather
 * kernel's fp32 operations in its order: results and statistics rows are the same bit for bit.  This flag sends such a call down
 * the gather path it used to take (A/B timing, bit comparison), like N3D_NO_MFMA for the MFMA family. */
#define N3D_NO_POINTWISE 512

/* storage type of an activation tensor (entry points that take a dtype argument; all others are fp32) */
#define N3D_F32 0
#define N3D_BF16 1        /* bfloat16 storage, fp32 arithmetic: BASELINE configs[4] (4x128^3 patches, HBM-bound levels) */
#define N3D_U8 2          /* bytes holding exactly {0, 1}: the targets of n3d_head_fwd / n3d_head_bwd (n3d_head.t_dtype) and of n3d_patch_batch */

/* Geometry of a (possibly strided / dilated) 3-D convolution, torch Conv3d semantics:
 * o = floor((i + 2*pad - dil*(k-1) - 1)/stride) + 1.  "i side" is what the window slides over.
 * For a transposed convolution the i side is its OUTPUT and the o side its INPUT. */
#define N3D_MAX_GROUP_TERMS 8   /* terms / jobs per batched launch (the N-term entry points below) */
#define N3D_MAX_REDUCE_TERMS 16 /* n3d_affine_act_bwd_reduceN / n3d_node_bwd_coeffs: every term of a supernet node level in one launch */

typedef struct n3d_conv_geom {
  int32_t B;
  int32_t Di, Hi, Wi, Ci;
  int32_t Do, Ho, Wo, Co;
  int32_t k, stride, dil, pad;
  int32_t depthwise; /* 1: groups == Ci == Co (prim_ops.py:95-97,105-106) */
} n3d_conv_geom;

const char* n3d_last_error(void);
int n3d_version(void);
/* 1 if the library was built for gfx950 and a HIP device is usable, 0 otherwise */
int n3d_device_ok(void);

int n3d_zero(void* p, size_t bytes, void* stream);

/* ---- convolution family: nn.Conv3d / nn.ConvTranspose3d (prim_ops.py:95-110,140-147) -------------
 * workspace: packed weights; query with n3d_conv_workspace_bytes().
 * in_gate : optional (B, Ci_of_the_conv_input) per-sample channel scale applied on load: the SE
 *           gate x*y (prim_ops.py:152) or a Dropout3d mask (prim_ops.py:72-73).
 * stats   : optional double[B][rows][Cout][2] partial (sum, sum of squares) of the raw output incl.
 *           bias: GroupNorm statistics produced in the conv epilogue (prim_ops.py:58,77). */
size_t n3d_conv_workspace_bytes(const n3d_conv_geom* g);
/* rows per sample that n3d_conv_fwd (transposed=0) / n3d_convT_fwd (transposed=1) write into `stats` */
int n3d_conv_stats_rows(const n3d_conv_geom* g, int transposed, int flags);
/* rows per sample written by n3d_channel_stats / n3d_affine_act_bwd_reduce for N voxels, C channels */
int n3d_stats_rows(int64_t N, int C);

/* Batched weight packing: the conv kernels read weights from a kernel-friendly packed copy.  By default each
 * conv call packs into its workspace (one tiny extra launch); a trainer instead packs ALL weights of the net
 * with one launch per step (n3d_pack_batch) and passes N3D_PREPACKED + the packed slot as `ws`.
 * n3d_conv_pack_info: layout id / padded channel count / float count of the packed form that the kernel
 * selected for (geometry, forward or data-gradient) expects. */
typedef struct n3d_pack_job {
  const float* w; float* dst;   /* layout 4 (bf16-storage 3x3x3 kernels): dst holds bfloat16 elements */
  int32_t Co, Ci, taps, data_grad, layout, cdp;
} n3d_pack_job;
int n3d_conv_pack_info(const n3d_conv_geom* g, int data_grad, int flags, int32_t* layout, int32_t* cdp, int64_t* floats);
int n3d_pack_batch(const n3d_pack_job* jobs /* host array */, int njobs, void* stream);

/* Deferred weight-gradient reduction: n3d_conv(T)_bwd_weight leave their partial slabs in `ws` and describe the
 * remaining fixed-order reduction in *deferred; n3d_wgrad_finalize_batch then finishes many convs in one launch. */
typedef struct n3d_final_job {
  const float* partial; const float* pbias; float* dw; float* dbias;
  int32_t nchunks, ntiles, tci, tco, ci_t, co_t, Co, Ci, taps, pad_;
} n3d_final_job;
int n3d_wgrad_finalize_batch(const n3d_final_job* jobs /* host array */, int njobs, void* stream);
/* Both batch calls compact their job table into the kernel arguments (pointers as 3-bit segment + 29-bit float offset against
 * up to eight 2 GB address segments per launch); jobs whose addresses do not fit one table go to further launches.
 * n3d_selftest_job_tables: host-only check of that encoding on scattered fake addresses (no device needed);
 * returns the number of launches its 300 jobs take, < 0 on a mismatch. */
int n3d_selftest_job_tables(void);

/* ---- "weight_norm" 1x1x1 conv WITHOUT its raw output (round 4; stem0: ConvOps(in, 3 c, kernel_size=1, ops_order='weight_norm'),
 * nas.py:28 / searched.py:69, prim_ops.py:68-83).  With 4 (8) input channels, raw = W x + bias costs 4 (8) FMAs per channel to
 * recompute, while storing it and reading it back in the GroupNorm epilogue and in both passes of its backward -- and writing d(raw)
 * for the weight gradient -- moves the 12-channel tensor five more times (0.2 ms of a 4x128^3 step).  The op then runs as
 *   forward : n3d_conv_k1_norm_fwd(y = NULL, stats)   statistics of raw only, nothing stored
 *             n3d_gn_coeffs                           (a, b) per (sample, channel)
 *             n3d_conv_k1_norm_fwd(y, oscale = a, oshift = b)   y = a * (W x + bias) + b in one pass over x
 *   backward: n3d_conv_k1_norm_bwd_reduce             rows [B][n3d_conv_k1_norm_rows][Co][3] as n3d_affine_act_bwd_reduce writes them
 *             n3d_gn_bwd_coeffs                       (A, Bc, Cc), d gamma, d beta, d bias
 *             n3d_conv_k1_norm_bwd_apply_wgrad        d(raw) = A g + (Cc raw + Bc) in registers -> dW slabs (deferred as
 *                                                     n3d_conv_bwd_weight); d(raw) is never written, so the op has NO input gradient
 * (Ci, Co) in {(4,4), (4,8), (4,12), (8,4)}, stride 1, >= 32768 voxels per sample (n3d_conv_k1_norm_ok); x fp32 or bf16
 * (N3D_SRC_BF16), y / dout fp32 or bf16 (N3D_DST_BF16); flags & N3D_RELU: the op has a ReLU behind its norm.  w: the native
 * (Co, Ci) weight for the backward calls; ws of the forward call as n3d_conv_fwd (packed weights, N3D_PREPACKED honoured). */
int n3d_conv_k1_norm_ok(const n3d_conv_geom* g);
int n3d_conv_k1_norm_rows(const n3d_conv_geom* g);
int n3d_conv_k1_norm_fwd(const n3d_conv_geom* g, const float* x, int64_t xld, const float* w, const float* bias, float* y, int64_t yld,
                         int flags, const float* oscale, const float* oshift, double* stats, void* ws, size_t ws_bytes, void* stream);
int n3d_conv_k1_norm_bwd_reduce(const n3d_conv_geom* g, const void* x, int64_t xld, const float* w, const float* bias, const void* dout,
                                int64_t dld, const float* a, const float* b, int flags, double* sums, void* stream);
int n3d_conv_k1_norm_bwd_apply_wgrad(const n3d_conv_geom* g, const void* x, int64_t xld, const float* w, const float* bias,
                                     const void* dout, int64_t dld, const float* a, const float* b, const float* A, const float* Bc,
                                     const float* Cc, int flags, float* dw, void* ws, size_t ws_bytes, n3d_final_job* deferred,
                                     void* stream);


/* ---- node-planar tensors (round 5).  A cell's output is torch.cat of its node outputs (cell.py:82, searched.py:51); as channel slices of
 * one (B, n c) buffer every node epilogue writes 16 / 32 bytes on a 48 / 96-byte pitch (1.3-1.7x the algorithmic HBM traffic).  Where the
 * only reader of the concatenation is a 1x1x1 preprocess conv, the nodes stay n DENSE (B, c, D, H, W) NDHWC tensors in one allocation --
 * storage (n, B, D, H, W, c) -- and the conv entry points take the whole thing as ONE tensor whose PITCH IS SMALLER THAN ITS CHANNEL COUNT:
 * (pointer to node 0, ld = c) with C = n c channels means node k at pointer + k * B * voxels * c elements.  Accepted by
 *   n3d_conv_fwd        x     (xld < Ci)                      }  1x1x1, stride 1, no gates, >= 32768 voxels per sample, channels % 4 == 0,
 *   n3d_conv_bwd_data   dx and relu_src (dxld = rld < Ci)     }  <= 24 channels on the planar side, <= 12 per node for the data gradient (one
 *   n3d_conv_bwd_weight x     (xld < Ci)                      }  node per blockIdx.z); fp32 or bf16 storage -- N3D_ERR_UNSUPPORTED otherwise.
 * The fused head reads the same layout through n3d_head.node_c. */

/* y[o side] = conv(x[i side]) + bias */
int n3d_conv_fwd(const n3d_conv_geom* g, const float* x, int64_t xld, const float* w, const float* bias,
                 float* y, int64_t yld, int flags, const float* in_gate, double* stats,
                 void* ws, size_t ws_bytes, void* stream);
/* dx[i side] (+)= conv^T(dy[o side]); if relu_src != NULL (N3D_RELU_IN) dx is masked by relu_src > 0;
 * out_gate multiplies dx per (b, ci) */
int n3d_conv_bwd_data(const n3d_conv_geom* g, const float* dy, int64_t dyld, const float* w,
                      float* dx, int64_t dxld, int flags, const float* relu_src, int64_t rld,
                      const float* out_gate, void* ws, size_t ws_bytes, void* stream);
/* dw (native layout) = sum x * dy, dbias = sum dy (either may be NULL) */
int n3d_conv_bwd_weight(const n3d_conv_geom* g, const float* x, int64_t xld, const float* dy, int64_t dyld,
                        float* dw, float* dbias, int flags, const float* in_gate,
                        void* ws, size_t ws_bytes, n3d_final_job* deferred /* NULL: finish now */, void* stream);

/* Data gradient AND weight gradient of one convolution: exactly n3d_conv_bwd_data(...) followed by
 * n3d_conv_bwd_weight(...) (same arguments, same results), but issued as ONE launch when both halves are small
 * MFMA problems (channel counts multiples of 16 on the 2^3..8^3 levels), where each half alone leaves most of the
 * chip idle.  Replaces the autograd backward of nn.Conv3d (prim_ops.py:109-110) on those levels. */
int n3d_conv_bwd_both(const n3d_conv_geom* g, const float* x, int64_t xld, const float* dy, int64_t dyld, const float* w, float* dx,
                      int64_t dxld, int flags_data, const float* relu_src, int64_t rld, const float* out_gate, void* ws_data,
                      size_t ws_data_bytes, float* dw, float* dbias, int flags_weight, const float* in_gate, void* ws_weight,
                      size_t ws_weight_bytes, n3d_final_job* deferred, void* stream);

/* The same for nn.ConvTranspose3d (prim_ops.py:100-102): n3d_convT_bwd_data + n3d_convT_bwd_weight (weight gradient
 * only; the bias gradient of a transposed conv is a plain channel sum the hot path derives from the GroupNorm sums). */
int n3d_convT_bwd_both(const n3d_conv_geom* g, const float* x, int64_t xld, const float* dy, int64_t dyld, const float* w, float* dx,
                       int64_t dxld, int flags_data, void* ws_data, size_t ws_data_bytes, float* dw, int flags_weight, void* ws_weight,
                       size_t ws_weight_bytes, n3d_final_job* deferred, void* stream);

/* ---- two independent convolutions in one launch: the two ops of a searched-cell node (searched.py:45-50) or a cell's
 * two preprocess convs (cell.py:47-50).  Exactly the two single calls described by the structures (same arguments,
 * same results, same fallbacks); ONE launch when both are small MFMA problems of the same K-split plan (channel
 * counts multiples of 16 on the 2^3..16^3 levels), where each alone leaves most of the chip idle. */
typedef struct n3d_conv_fwd_call {     /* arguments of n3d_conv_fwd / n3d_convT_fwd */
  const n3d_conv_geom* g; int32_t transposed; int32_t flags;
  const float* x; int64_t xld; const float* w; const float* bias; float* y; int64_t yld;
  const float* in_gate; double* stats; void* ws; size_t ws_bytes;
} n3d_conv_fwd_call;
/* Two small pointwise convs (N3D_NO_POINTWISE above; plain convs, distinct outputs) that do not fold as an MFMA pair also share ONE
 * launch: the pointwise kernel takes two jobs.  With one such call of the two, that one runs on the pointwise kernel alone. */
int n3d_conv_fwd2(const n3d_conv_fwd_call* c0, const n3d_conv_fwd_call* c1, void* stream);
/* the same for up to four calls (`calls` = array): the plain-conv primitives of a supernet node (cell.py:76-81).  One launch when
 * all are small MFMA problems of one K-split plan, or all one-plane-tile 3x3x3 convs of one channel count in {4, 8} (stride 1 or 2,
 * distinct outputs); otherwise two at a time as n3d_conv_fwd2, a leftover alone.  Results and statistics rows are those of the
 * single calls bit for bit whatever the grouping.  Calls that are not N3D_PREPACKED should bring distinct workspaces: calls that share
 * one are never folded (a folded launch reads every call's packed weights at once) and run one after the other.
 * The one-plane-tile launch also takes the stride-2 transposed forms (n3d_convT_fwd of a stride-2 conv on an exactly doubled grid, the
 * data gradient of a stride-2 conv), and it is an entry-signal carrier ("Entry signals" below): a signal armed in front of a call whose
 * weights are N3D_PREPACKED rides in the folded launch; packing launches in front of it issue the signal stand-alone, as for a single conv. */
int n3d_conv_fwdN(const n3d_conv_fwd_call* calls, int n, void* stream);
/* 1 exactly when n3d_conv_fwd2(c0, c1, .) would be ONE launch of the one-plane-tile multi-conv kernel (the launch
 * n3d_conv_fold_counts counts in counts[0]), else 0.  Enqueues nothing and touches no memory: a pure function of the geometries, flags,
 * pointer alignment, destinations and workspaces of the two calls, decided by the code the launch path itself runs, so a scheduler can
 * choose between folding two convs and running one of them on another stream without launching anything. */
int n3d_conv_fwd2_folds(const n3d_conv_fwd_call* c0, const n3d_conv_fwd_call* c1);

/* The depthwise 3x3x3 convs of up to N3D_MAX_GROUP_TERMS primitives of a supernet node (one depthwise-separable primitive per
 * edge, cell.py:76-81) in ONE launch.  A job is one gather pass: data_grad = 0: dst[o side] = conv(src[i side]) + bias
 * (n3d_conv_fwd, or the data gradient of a transposed conv); data_grad = 1: dst[i side] (+)= conv^T(src[o side]) (n3d_conv_bwd_data,
 * or n3d_convT_fwd).  All jobs share batch, channel count and destination shape; destinations must not alias. */
typedef struct n3d_dw_job {
  const n3d_conv_geom* g; int32_t data_grad; int32_t flags /* N3D_ACCUMULATE */;
  const float* src; int64_t sld; const float* w; const float* bias; float* dst; int64_t dld;
} n3d_dw_job;
int n3d_dwconv_batch(const n3d_dw_job* jobs, int n, void* stream);

typedef struct n3d_conv_bwd_call {     /* arguments of n3d_conv_bwd_both / n3d_convT_bwd_both */
  const n3d_conv_geom* g; int32_t transposed; int32_t flags_data; int32_t flags_weight; int32_t pad_;
  const float* x; int64_t xld; const float* dy; int64_t dyld; const float* w; float* dx; int64_t dxld;
  const float* relu_src; int64_t rld; const float* out_gate; void* ws_data; size_t ws_data_bytes;
  float* dw; float* dbias; const float* in_gate; void* ws_weight; size_t ws_weight_bytes; n3d_final_job* deferred;
} n3d_conv_bwd_call;
/* the two data gradients must not alias (dx of c0 != dx of c1) for the one-launch form; aliasing falls back to two launches */
int n3d_conv_bwd_both2(const n3d_conv_bwd_call* c0, const n3d_conv_bwd_call* c1, void* stream);
/* Data gradients only of two convs (the architecture pass of the search step computes no weight gradients, search.py:223-231;
 * the reference runs loss.backward() through every conv's input there): fields x, dw, dbias, in_gate, ws_weight, deferred and
 * flags_weight of the calls are ignored.  One launch where both fit the small-tensor MFMA kernel and dx of c0 != dx of c1. */
int n3d_conv_bwd_data2(const n3d_conv_bwd_call* c0, const n3d_conv_bwd_call* c1, void* stream);
/* the same query as n3d_conv_fwd2_folds for n3d_conv_bwd_data2 (two data gradients into one buffer never fold) */
int n3d_conv_bwd_data2_folds(const n3d_conv_bwd_call* c0, const n3d_conv_bwd_call* c1);
/* (two small pointwise data gradients with dx of c0 != dx of c1 fold the same way as in n3d_conv_fwd2: one two-job launch)
 * n3d_conv_pointwise_counts: launches of the pointwise kernel / jobs they carried since the library was loaded (a two-job launch
 * counts 1 / 2): lets a test see which path a call took. */
int n3d_conv_pointwise_counts(int64_t* launches, int64_t* jobs);
/* n3d_conv_fold_counts: launches of the folded conv kernels since the library was loaded, counts[5] = one-wave-tile 3x3x3 convs in one
 * launch (n3d_conv_fwd2 / fwdN / bwd_data2), two K-split GEMM convs, three or four of them, data + weight gradient of one conv
 * (n3d_conv_bwd_both), of two (n3d_conv_bwd_both2): lets a test see that a call took the folded kernel and not single launches. */
int n3d_conv_fold_counts(int64_t* counts);
/* transposed convolution y[i side] = convT(x[o side]) + bias; same kernels with the roles swapped */
int n3d_convT_fwd(const n3d_conv_geom* g, const float* x, int64_t xld, const float* w, const float* bias,
                  float* y, int64_t yld, int flags, const float* in_gate, double* stats,
                  void* ws, size_t ws_bytes, void* stream);
int n3d_convT_bwd_data(const n3d_conv_geom* g, const float* dy, int64_t dyld, const float* w,
                       float* dx, int64_t dxld, int flags, void* ws, size_t ws_bytes, void* stream);
int n3d_convT_bwd_weight(const n3d_conv_geom* g, const float* x, int64_t xld, const float* dy, int64_t dyld,
                         float* dw, float* dbias, int flags, void* ws, size_t ws_bytes,
                         n3d_final_job* deferred /* NULL: finish now */, void* stream);

/* ---- per-(sample,channel) statistics and the normalise / activate / weighted-sum epilogue ----------
 * n3d_channel_stats: stats[b][row][c] = partial (sum x, sum x^2) over the N voxels (GroupNorm of a tensor
 *   that no conv of ours produced: IdentityOp prim_ops.py:170-174; SE mean prim_ops.py:149). */
int n3d_channel_stats(const float* x, int64_t ld, int B, int64_t N, int C, double* stats, void* stream);
/* the same with a storage type (N3D_F32 / N3D_BF16) */
int n3d_channel_stats_t(const void* x, int64_t ld, int dtype, int B, int64_t N, int C, double* stats, void* stream);
/* the same for up to N3D_MAX_GROUP_TERMS tensors of one (B, N, C) shape in one launch: xs / lds / stats are host arrays of n entries */
int n3d_channel_statsN(const float* const* xs, const int64_t* lds, double* const* stats, int n, int B, int64_t N, int C, void* stream);
/* ---- padded channels (round 5).  The reference takes feature maps of any channel count (nas.py:13-26, searched.py:55-66: init_n_kernels = 2,
 * 6, ...); the kernels move channels four at a time.  Such a net runs with every feature map zero-padded to a multiple of 4 (zero conv
 * weights / gamma / beta on the padded channels: they hold exactly 0 forward and receive exactly 0 backward).  Sums over a padded tensor
 * are the real tensor's sums, so one thing changes: the ELEMENT COUNT of a GroupNorm group.  Every entry point below that takes a group
 * count G accepts G < 0 = "ONE group whose real channel count is -G, stored in C >= -G channels": statistics are divided by N * (-G)
 * instead of N * C.  (A real count that needs padding is never a multiple of 16, i.e. always one group: prim_ops.py:57.)  Not taken with
 * G < 0: the one-launch small backward (n3d_bwd_small2_ok returns 0), n3d_node_fwd_coeffs / n3d_node_bwd_coeffs; conv-bias gradients out
 * of the GroupNorm sums (dbias_conv) need the true count and must not be requested. */
/* GroupNorm(G, C) statistics -> per-(b,c) affine y = a*x + b; mean_rstd[b][g] = (mean, rstd) (prim_ops.py:56-58) */
int n3d_gn_coeffs(const double* stats, int rows, const float* gamma, const float* beta, int B, int C, int G,
                  int64_t N, float eps, float* a, float* b, float* mean_rstd, double* sumraw /* [B][C] or NULL */,
                  void* stream);
/* out (+)= w * act(a[b,c]*raw + b[b,c]);  a,b NULL -> identity affine; wptr NULL -> 1.
 * This is GroupNorm-apply + ReLU (prim_ops.py:75-80) fused with the MixedOp weighting and the node
 * sum (cell.py:29-32,81; searched.py:50). */
int n3d_affine_act(const float* raw, int64_t rld, const float* a, const float* b, const float* wptr,
                   float* out, int64_t old_, int B, int64_t N, int C, int flags, void* stream);
/* Fused form for small tensors (rows <= n3d_fused_max_rows()): the GroupNorm coefficients are computed from the
 * statistics rows in every workgroup's prologue (no separate n3d_gn_coeffs launch); a / b / mean_rstd are also
 * stored for the backward pass. */
int n3d_fused_max_rows(void);
int n3d_affine_act_gn(const float* raw, int64_t rld, const double* stats, int rows, const float* gamma,
                      const float* beta, int G, float eps, const float* wptr, float* out, int64_t old_, int B,
                      int64_t N, int C, int flags, float* a_out, float* b_out, float* mean_rstd_out,
                      double* sumraw /* [B][C] per-channel sum of raw, or NULL */, void* stream);
/* backward, pass 1: sums[b][row][c] = partial (S1 = sum g, S2 = sum g*raw, Sz = sum dout*z),
 * g = dout * act'(a*raw+b), z = act(a*raw+b) */
int n3d_affine_act_bwd_reduce(const float* dout, int64_t dld, const float* raw, int64_t rld, const float* a,
                              const float* b, int B, int64_t N, int C, int flags, double* sums, void* stream);
/* GroupNorm backward coefficients: dgamma, dbeta (summed over b), dalpha = sum Sz (if not NULL),
 * and the per-(b,c) affine draw = A*g + Bc + Cc*raw.  wptr: the MixedOp weight (NULL -> 1).
 * If dbias_conv != NULL (needs sumraw[b][c] = sum_v raw, saved by the forward coefficient kernels) it also
 * writes the gradient of the bias of the conv that produced raw:  sum_v draw = A*S1 + N*Bc + Cc*sum(raw). */
int n3d_gn_bwd_coeffs(const double* sums, int rows, const float* gamma, const float* mean_rstd,
                      const float* wptr, int B, int C, int G, int64_t N, float* dgamma, float* dbeta,
                      float* dalpha, float* A, float* Bc, float* Cc, const double* sumraw,
                      float* dbias_conv, void* stream);
/* n3d_gn_bwd_coeffs + n3d_affine_act_bwd_apply in one launch for small tensors (rows <= n3d_fused_max_rows()) */
int n3d_affine_act_bwd_apply_gn(const float* dout, int64_t dld, const float* raw, int64_t rld, const float* a,
                                const float* b, const double* sums, int rows, const float* gamma,
                                const float* mean_rstd, const float* wptr, const double* sumraw,
                                float* draw, int64_t drld, int B, int64_t N, int C, int G, int flags, float* dgamma,
                                float* dbeta, float* dalpha, float* dbias_conv, void* stream);
/* ---- node-level pair epilogues: a searched-cell node is op_a(x_i) + op_b(x_j) (searched.py:45-50); both ops end in
 * GroupNorm -> [ReLU] -> weighted sum on tensors of one shape and share the node gradient in backward.  One launch
 * does the work of two n3d_affine_act_gn / n3d_affine_act_bwd_reduce / n3d_affine_act_bwd_apply_gn calls (same
 * results; the node buffer is written once, the node gradient read once).  Requirements: rows <= n3d_fused_max_rows(),
 * C a power of two <= 64, C / G <= 16, B <= 4 for the backward apply; otherwise N3D_ERR_UNSUPPORTED (call the single
 * forms). */
typedef struct n3d_gn_fwd_term {
  const float* raw; int64_t rld;          /* conv output (pitched NDHWC) */
  const double* stats; int32_t rows;      /* [B][rows][C][2] partial (sum, sum of squares) */
  int32_t relu;                           /* 1: ReLU after the norm */
  const float* gamma; const float* beta;  /* GroupNorm affine */
  const float* wptr;                      /* optional scalar weight (MixedOp alpha), NULL = 1 */
  float* a_out; float* b_out; float* mean_rstd_out; double* sumraw;  /* saved for backward, as n3d_affine_act_gn */
  int32_t dtype; int32_t pad_;            /* storage of raw (N3D_F32 / N3D_BF16); entry points with a `flags` argument use N3D_ACT_BF16 */
} n3d_gn_fwd_term;
int n3d_affine_act_gn2(const n3d_gn_fwd_term* t0, const n3d_gn_fwd_term* t1, int G, float eps, float* out, int64_t old_,
                       float* out1 /* NULL: out = term0 + term1 (a node); else two independent outputs (the two preprocess
                       ops of a cell, cell.py:47-50): term0 -> out, term1 -> out1.  With N3D_ACCUMULATE and out1 set, only
                       `out` is accumulated into; out1 is overwritten */, int64_t old1, int B, int64_t N, int C,
                       int flags /* N3D_ACCUMULATE */, void* stream);

typedef struct n3d_gn_bwd_term {
  const float* raw; int64_t rld; const float* a; const float* b;   /* forward operands / coefficients */
  double* sums; int32_t rows;             /* [B][rows][C][3]: written by n3d_affine_act_bwd_reduce2, read by ..._apply_gn2 */
  int32_t relu;
  const float* gamma; const float* mean_rstd; const float* wptr; const double* sumraw;
  float* draw; int64_t drld;              /* d(raw), output of the apply pass */
  float* dgamma; float* dbeta; float* dalpha; float* dbias_conv;   /* parameter gradients (dalpha / dbias_conv may be NULL) */
  float* cA; float* cB; float* cC;        /* [B][C] draw = cA*g + cB + cC*raw: written by n3d_gn_bwd_coeffs2, read by n3d_affine_act_bwd_apply2 */
  int32_t dtype; int32_t pad_;            /* storage of raw / draw and of the output gradient(s) of the call (N3D_F32 / N3D_BF16) */
} n3d_gn_bwd_term;
/* dout1: NULL = both terms share the output gradient dout (a node); else the gradient of term1's own output */
int n3d_affine_act_bwd_reduce2(const float* dout, int64_t dld, const float* dout1, int64_t dld1, const n3d_gn_bwd_term* t0,
                               const n3d_gn_bwd_term* t1, int B, int64_t N, int C, void* stream);
int n3d_affine_act_bwd_apply_gn2(const float* dout, int64_t dld, const float* dout1, int64_t dld1, const n3d_gn_bwd_term* t0,
                                 const n3d_gn_bwd_term* t1, int B, int64_t N, int C, int G, void* stream);
/* Small levels (n3d_bwd_small2_ok: B <= 4, B * roundup(N * (C/G)/4, 64) <= 2048 channel quads per group): the
 * whole epilogue backward of a node whose terms carry no MixedOp weight gradient -- reduction, coefficients, parameter
 * gradients and both d(raw) -- in ONE launch, one workgroup per GroupNorm group, elements held in registers between the passes.
 * Same outputs as n3d_affine_act_bwd_reduce2 + n3d_affine_act_bwd_apply_gn2 (sums / dalpha of the terms are not used). */
int n3d_bwd_small2_ok(int B, int64_t N, int C, int G);
int n3d_affine_act_bwd_small2(const float* dout, int64_t dld, const float* dout1 /* as in ..._reduce2 */, int64_t dld1, const n3d_gn_bwd_term* t0,
                              const n3d_gn_bwd_term* t1, int B, int64_t N, int C, int G, void* stream);
/* The general form (round 3).  n3d_bwd_small_mode: 0 = shape not taken, 1 = one workgroup per group as above, 2 = one workgroup per
 * (group, sample) for B = 2..4 samples of up to 2048 channel quads per group EACH (the 8^3 level at 16 channels per group): d(raw)
 * is per sample; each workgroup stores its parameter-gradient contribution to `scratch` (n3d_bwd_small_scratch_bytes) and the one
 * that draws the last of the group's tickets adds them in sample order.  `tickets`: G zero-initialised words that no other
 * launch in flight uses; they are zero again when the launch is over (atomicInc wrapping at B - 1), so a replayed graph needs
 * no reset.  scratch / tickets may be NULL for mode 1.  t1 == NULL: a single epilogue (dout1 must be NULL then). */
int n3d_bwd_small_mode(int B, int64_t N, int C, int G);
size_t n3d_bwd_small_scratch_bytes(int B, int G);
int n3d_affine_act_bwd_small(const float* dout, int64_t dld, const float* dout1, int64_t dld1, const n3d_gn_bwd_term* t0,
                             const n3d_gn_bwd_term* t1, int B, int64_t N, int C, int G, void* scratch, size_t scratch_bytes,
                             uint32_t* tickets, void* stream);
/* n3d_affine_act_bwd_small (mode 1, two terms, one output gradient) + n3d_conv_bwd_data2 of a searched-cell node in ONE launch: call c_i
 * is the data gradient of the conv that produced raw of term t_i (c_i->dy == t_i->draw, c_i->dyld == t_i->drld).  Every workgroup of the
 * K-split pair kernel rebuilds d(raw) of its own term for the one or two samples its rows draw from and multiplies it out of LDS; d(raw),
 * dgamma, dbeta, dbias_conv and both dx come out bit for bit as from the two calls (d(raw) is still written: weight gradients read it).
 * Taken for fp32 storage, n3d_bwd_small2_ok shapes with C / G == 16, G <= 4 and B * G * ceil(N / 16) <= 32, no dalpha, both convs dense
 * on the 16-way K-split plan with distinct dx, without N3D_MM_BF16 / N3D_NO_MFMA; relu_src, out_gate and N3D_ACCUMULATE of the calls
 * work as in n3d_conv_bwd_data2.  n3d_gn_bwd_conv_data2_ok answers 1 / 0 from the same decision code without launching; where it says 0
 * the entry point returns N3D_ERR_UNSUPPORTED and has touched nothing: keep the two calls. */
int n3d_gn_bwd_conv_data2_ok(const float* dout, int64_t dld, const n3d_gn_bwd_term* t0, const n3d_gn_bwd_term* t1, int B, int64_t N, int C,
                             int G, const n3d_conv_bwd_call* c0, const n3d_conv_bwd_call* c1);
int n3d_gn_bwd_conv_data2(const float* dout, int64_t dld, const n3d_gn_bwd_term* t0, const n3d_gn_bwd_term* t1, int B, int64_t N, int C, int G,
                          const n3d_conv_bwd_call* c0, const n3d_conv_bwd_call* c1, void* stream);
/* the same pairing for tensors with more partial rows than the fused prologues accept (the 32^3 / 64^3 levels):
 * n3d_gn_coeffs2 = two n3d_gn_coeffs in one launch (fills a_out, b_out, mean_rstd_out, sumraw of both terms);
 * n3d_affine_act2 = two n3d_affine_act into one output (reads a_out / b_out as the coefficients; stats unused);
 * n3d_gn_bwd_coeffs2 = two n3d_gn_bwd_coeffs (fills cA / cB / cC and the parameter gradients);
 * n3d_affine_act_bwd_apply2 = two n3d_affine_act_bwd_apply reading the node gradient once. */
int n3d_gn_coeffs2(const n3d_gn_fwd_term* t0, const n3d_gn_fwd_term* t1, int B, int C, int G, int64_t N, float eps, void* stream);
int n3d_affine_act2(const n3d_gn_fwd_term* t0, const n3d_gn_fwd_term* t1, float* out, int64_t old_, float* out1, int64_t old1, int B,
                    int64_t N, int C, int flags, void* stream);
int n3d_gn_bwd_coeffs2(const n3d_gn_bwd_term* t0, const n3d_gn_bwd_term* t1, int B, int C, int G, int64_t N, void* stream);
int n3d_affine_act_bwd_apply2(const float* dout, int64_t dld, const float* dout1, int64_t dld1, const n3d_gn_bwd_term* t0,
                              const n3d_gn_bwd_term* t1, int B, int64_t N, int C, void* stream);
/* N-term forms for a supernet node (cell.py:76-81: node = sum over its edges of sum_k alpha[e][k] * op_k(x_e); 8-16 of the
 * 10-22 terms end in a GroupNorm).  `terms`: array of n <= N3D_MAX_GROUP_TERMS descriptors, C a power of two in 4..64.
 * n3d_gn_coeffsN: n x n3d_gn_coeffs in one launch.  n3d_affine_actN: out (+)= sum_k w_k * act_k(a_k * raw_k + b_k) in term
 * order, one pass over the node buffer; a_k = a_out, b_k = b_out of the term, NULL meaning 1 / 0, so the node's other
 * primitives (SE gate: a = gate; pooling, identity-with-norm) ride in the same pass.  Backward: n3d_affine_act_bwd_reduceN (fills sums of every term; all terms read the
 * same node gradient; a / b NULL = 1 / 0 as in n3d_affine_act_bwd_reduce, so the other primitives' reductions ride along; this entry and n3d_affine_act_bwd_applyN take up to N3D_MAX_REDUCE_TERMS terms), n3d_gn_bwd_coeffsN (cA / cB / cC and the parameter gradients), n3d_affine_act_bwd_applyN (every draw). */
int n3d_gn_coeffsN(const n3d_gn_fwd_term* terms, int n, int B, int C, int G, int64_t N, float eps, void* stream);
int n3d_affine_actN(const n3d_gn_fwd_term* terms, int n, float* out, int64_t old_, int B, int64_t N, int C, int flags, void* stream);
int n3d_affine_act_bwd_reduceN(const float* dout, int64_t dld, const n3d_gn_bwd_term* terms, int n, int B, int64_t N, int C, void* stream);
int n3d_gn_bwd_coeffsN(const n3d_gn_bwd_term* terms, int n, int B, int C, int G, int64_t N, void* stream);
int n3d_affine_act_bwd_applyN(const float* dout, int64_t dld, const n3d_gn_bwd_term* terms, int n, int B, int64_t N, int C, void* stream);
/* The apply passes of a node level's single primitives (SE gates, identity-with-norm: cell.py:29-32) in ONE launch: every term is
 * draw' = cA * g + cB + cC * raw (g = dout behind the term's ReLU mask a * raw + b > 0 when relu and a are set; NULL a / b / cA / cB / cC
 * = 1 / 0 / 1 / 0 / 0); CONSECUTIVE terms with the same `draw` (at most 4) are summed into it in term order, on top of its previous
 * content if bit 0 of the first term's `pad_` is set -- what n3d_affine_act_bwd_apply launches in that order would leave there.
 * n <= N3D_MAX_REDUCE_TERMS terms, at most 8 distinct targets. */
int n3d_affine_act_bwd_apply_sum(const float* dout, int64_t dld, const n3d_gn_bwd_term* terms, int n, int B, int64_t N, int C, void* stream);
/* plain (no norm) epilogue backward coefficients: A = w, Bc = Cc = 0, dalpha = sum Sz */
int n3d_plain_bwd_coeffs(const double* sums, int rows, const float* wptr, int B, int C, float* dalpha,
                         float* A, void* stream);
/* the same for up to N3D_MAX_GROUP_TERMS primitives of a node in one launch (A or dalpha of a term may be NULL) */
typedef struct n3d_plain_coef_term { const double* sums; int32_t rows; int32_t pad_; const float* wptr; float* dalpha; float* A; } n3d_plain_coef_term;
int n3d_plain_bwd_coeffsN(const n3d_plain_coef_term* terms, int n, int B, int C, void* stream);
/* backward, pass 2: draw (+)= A[b,c]*g + Bc[b,c] + Cc[b,c]*raw   (Bc, Cc may be NULL) */
int n3d_affine_act_bwd_apply(const float* dout, int64_t dld, const float* raw, int64_t rld, const float* a,
                             const float* b, const float* A, const float* Bc, const float* Cc, float* draw,
                             int64_t drld, int B, int64_t N, int C, int flags, void* stream);

/* ---- squeeze-excitation gate (prim_ops.py:133-139,148-152) ----------------------------------------
 * fwd: mean = stats.sum/N; hidden = relu(w1.mean + b1); gate = sigmoid(w2*hidden + b2) */
int n3d_se_gate_fwd(const double* stats, int rows, int64_t N, const float* w1, const float* b1,
                    const float* w2, const float* b2, int B, int C, float* mean, float* hidden, float* gate,
                    void* stream);
/* bwd: dgate[b,c] = w * sums[b][c].S2; returns fc grads and the input-side affine
 * dx = A*g + Bc with A = w*gate, Bc = dmean/N; dalpha = sum Sz if not NULL */
int n3d_se_gate_bwd(const double* sums, int rows, const float* wptr, const float* mean, const float* hidden,
                    const float* gate, const float* w1, const float* w2, int B, int C, int64_t N,
                    float* dw1, float* db1, float* dw2, float* db2, float* dalpha, float* A, float* Bc,
                    void* stream);
/* the gates of up to N3D_MAX_GROUP_TERMS SE primitives of a supernet node (one per stride-1 edge, cell.py:76-81) in one launch.
 * `sums`: forward = the [B][rows][C][2] channel statistics of the gate input, backward = the [B][rows][C][3] reduction rows
 * of n3d_affine_act_bwd_reduce(N); other fields as the arguments of n3d_se_gate_fwd / n3d_se_gate_bwd. */
typedef struct n3d_se_term {
  const double* sums; int32_t rows; int32_t pad_;
  const float* w1; const float* b1; const float* w2; const float* b2;
  float* mean; float* hidden; float* gate;      /* forward outputs, backward inputs */
  const float* wptr; float* dw1; float* db1; float* dw2; float* db2; float* dalpha; float* A; float* Bc;   /* backward only */
} n3d_se_term;
int n3d_se_gate_fwdN(const n3d_se_term* terms, int n, int64_t N, int B, int C, void* stream);
int n3d_se_gate_bwdN(const n3d_se_term* terms, int n, int64_t N, int B, int C, void* stream);
/* All coefficient computations of one node level of the supernet backward (cell.py:76-81: a node's MixedOps all consume the node's
 * gradient) -- n3d_gn_bwd_coeffsN of up to N3D_MAX_REDUCE_TERMS GroupNorm-type terms and n3d_se_gate_bwdN of up to
 * N3D_MAX_GROUP_TERMS SE gates -- in ONE launch at B = 2 with both kinds present (the same per-term work, same results), else as
 * those launches. */
/* forward counterpart: n3d_gn_coeffsN of 1..8 GroupNorm-type terms and n3d_se_gate_fwdN of 1..8 SE gates of one group in one launch */
int n3d_node_fwd_coeffs(const n3d_gn_fwd_term* gn, int n_gn, const n3d_se_term* se, int n_se, int B, int C, int G, int64_t N, float eps, void* stream);
int n3d_node_bwd_coeffs(const n3d_gn_bwd_term* gn, int n_gn, const n3d_se_term* se, int n_se, int B, int C, int G, int64_t N, void* stream);


/* ---- 2x2x2 pooling, stride 2 (prim_ops.py:160-163) ------------------------------------------------
 * Every entry returns N3D_ERR_INVALID for an odd spatial dimension.  Max pooling is torch's bit for bit: the FIRST maximum of a
 * window in (d, h, w) order is the output (so -0.0 in front of +0.0 stays -0.0), it takes the whole gradient, and a NaN wins. */
int n3d_pool2_fwd(const float* x, int64_t xld, float* y, int64_t yld, int B, int Di, int Hi, int Wi, int C,
                  int flags, void* stream);
int n3d_pool2_bwd(const float* dy, int64_t dyld, const float* x, int64_t xld, float* dx, int64_t dxld, int B,
                  int Di, int Hi, int Wi, int C, int flags, void* stream);
/* dx (+)= w * pool^T(dy): the MixedOp weight of a pooling primitive (cell.py:29-32) folded into its backward (wptr NULL = 1) */
int n3d_pool2_bwd_scaled(const float* dy, int64_t dyld, const float* x, int64_t xld, float* dx, int64_t dxld, int B, int Di, int Hi,
                         int Wi, int C, int flags, const float* wptr, void* stream);
/* average AND max pooling of one tensor (both primitives sit on every stride-2 edge of a down cell, prim_ops.py:29-30; cell.py:16-22):
 * forward in one pass over x; backward dx (+)= w_avg * avgpool^T(dy) + w_max * maxpool^T(dy) in one pass over dx */
int n3d_pool2_fwd_both(const float* x, int64_t xld, float* y_avg, int64_t yald, float* y_max, int64_t ymld, int B, int Di, int Hi, int Wi,
                       int C, void* stream);
int n3d_pool2_bwd_both(const float* dy, int64_t dyld, const float* x, int64_t xld, float* dx, int64_t dxld, int B, int Di, int Hi, int Wi,
                       int C, int flags, const float* w_avg, const float* w_max, void* stream);

/* ---- sigmoid head + Dice loss (nas.py:52, searched.py:93, loss.py:12-14) --------------------------
 * element (b,c,v) of p / t / dp is at  ptr[b*sb + c*sc + v*sv]  (works for NCDHW and NDHWC).
 * partial: double[B][C][n3d_dice_rows(N)][3] scratch; sums: double[B][C][3] (sum p*t, sum p, sum t). */
int n3d_dice_rows(int64_t N);
int n3d_dice_fwd(const float* p, int64_t psb, int64_t psc, int64_t psv, const float* t, int64_t tsb, int64_t tsc,
                 int64_t tsv, int B, int C, int64_t N, float smooth, double* partial, double* sums,
                 float* loss, void* stream);
int n3d_dice_bwd(const float* p, int64_t psb, int64_t psc, int64_t psv, const float* t, int64_t tsb, int64_t tsc,
                 int64_t tsv, int B, int C, int64_t N, float smooth, const double* sums, const float* dloss,
                 float* dp, int64_t dsb, int64_t dsc, int64_t dsv, void* stream);

/* ---- fused head: Dropout3d -> Conv3d(k=1) -> Sigmoid (nas.py:50-52, searched.py:91-93) and, optionally in the same passes,
 * the Dice loss on its output (loss.py:12-14).  x: (B, Ci, N voxels) pitched NDHWC of dtype x_dtype; w: (Co, Ci) = the
 * Conv3d weight (Co, Ci, 1, 1, 1); gate: (B, Ci) Dropout3d gate (0 or 1/(1-p) per sample and channel; prim_ops.py:66,72-73)
 * or NULL.  Ci in {4, 8, 12, 16, 24, 32}, Co <= 4, otherwise N3D_ERR_UNSUPPORTED.  p / logits / t / dp are fp32 with element
 * (b, c, v) at ptr[b*sb + c*sc + v*sv] (NCDHW or NDHWC).
 * n3d_dropout3d_gate: draws the gate on the device: gate[i] = u(seed, counter, i) >= p ? 1/(1-p) : 0 with u =
 *   n3d_dropout3d_uniform (splitmix64, host-callable); state = device uint32[3] {seed_lo, seed_hi, counter}; the launch
 *   increments the counter, so a captured HIP graph draws a new mask on every replay.
 * n3d_head_fwd: p = sigmoid(conv(x * gate) + bias) (logits optionally stored too; p may be NULL when t is given: a training step
 *   needs the loss and the sums only, and the backward pass recomputes p); with t != NULL also
 *   sums[b][c] = (sum p*t, sum p, sum t) and *loss = 1 - mean_bc (2*sum pt + smooth) / (sum p + sum t + smooth);
 *   partial: double[B][Co][n3d_head_rows(N)][3] scratch.
 * n3d_head_bwd: one pass writes dx (+)= and the weight / bias gradient slabs.  Either dp (gradient w.r.t. p) is given, or
 *   (t, sums [, dloss]) and the Dice gradient is formed on the fly.  p is recomputed from x, nothing saved is read.
 *   ws: n3d_head_workspace_bytes(); deferred as in n3d_conv_bwd_weight. */
/* NODE-PLANAR input (round 4): the head's input is the concatenation of a cell's node outputs (cell.py:82, searched.py:51).
 * Written into one (B, Ci) buffer every node epilogue stores 16 bytes on a 48-byte voxel pitch (0.28 of the HBM roofline at
 * 128^3); with node_c > 0 the nodes stay DENSE tensors of their own -- channel c of voxel (b, v) is element
 * x[(c / node_c) * x_node_stride + (b * N + v) * xld + c % node_c], xld >= node_c -- and the head (its only consumer) gathers
 * the Ci / node_c pointers itself; dx of n3d_head_bwd is laid out the same way with dx_node_stride.  node_c == 0: the ordinary
 * pitched layout (the two strides are ignored). */
typedef struct n3d_head {
  const void* x; int64_t xld; int32_t x_dtype; int32_t B; int32_t Ci; int32_t Co; int64_t N;
  const float* w; const float* bias; const float* gate;
  int64_t x_node_stride; int64_t dx_node_stride; int32_t node_c;
  int32_t t_dtype;      /* storage of the targets t: N3D_F32, or N3D_U8 (Co = 3: generator.py:230-248 yields three boolean maps; the strides
                           count elements; same sums and gradients bit for bit, a quarter of the target bytes) */
} n3d_head;
float n3d_dropout3d_uniform(uint64_t seed, uint32_t counter, uint32_t index);
int n3d_dropout3d_gate(uint32_t* state, float p, int B, int C, float* gate, void* stream);
int n3d_head_rows(int64_t N);
size_t n3d_head_workspace_bytes(const n3d_head* h);
int n3d_head_fwd(const n3d_head* h, float* p, int64_t psb, int64_t psc, int64_t psv, float* logits, const void* t, int64_t tsb,
                 int64_t tsc, int64_t tsv, float smooth, double* partial, double* sums, float* loss, void* stream);
int n3d_head_bwd(const n3d_head* h, const float* dp, int64_t dsb, int64_t dsc, int64_t dsv, const void* t, int64_t tsb, int64_t tsc,
                 int64_t tsv, float smooth, const double* sums, const float* dloss, void* dx, int64_t dxld, int dx_dtype, int flags,
                 float* dw, float* dbias, void* ws, size_t ws_bytes, n3d_final_job* deferred, void* stream);
/* ---- evaluation head (train.py:138-157 validate(); prediction.py:150-170 thresholds at >= 0.5): the head of n3d_head_fwd in eval
 * mode -- no Dropout3d gate (h->gate must be NULL) -- with the Dice loss AND the region counts of the thresholded prediction in the
 * same pass over (x, t), then ONE finalize launch that forms the batch loss exactly as n3d_head_fwd does (bit for bit) and adds the
 * batch into a device accumulator.  Same input forms as n3d_head_fwd (pitched or node-planar x, fp32 / bf16, fp32 / byte t).
 *   p: probabilities written when not NULL (strides as n3d_head_fwd); the evaluation pass of the trainers passes NULL.
 *   thr: a voxel is predicted in class c when p >= thr.  B * Co <= 256.
 *   partial: double[B][Co][n3d_head_rows(N)][3], hpartial: double[B][Co][n3d_head_rows(N)][2] scratch; sums: double[B][Co][3] and
 *   *loss as n3d_head_fwd.
 *   acc: double[N3D_EVAL_ACC_LEN(Co)], zeroed by the caller at the start of an epoch; each call adds (fixed order, no atomics)
 *     acc[0] += loss, acc[1] += 1 (batches), acc[2] += B (samples), acc[3] unused;
 *     per class c at acc[4 + 4c]: += (sum_b I, sum_b P, sum_b T, sum_b Dice_b) with I = sum [p >= thr] * t, P = sum [p >= thr],
 *     T = sum t over the sample's voxels and Dice_b = 2 I / (P + T), = 1 when P + T == 0 (both regions empty).
 *   The counts are integers held in fp64 (exact in any order); the accumulator of several ranks is their SUM. */
#define N3D_EVAL_ACC_LEN(co) (4 + 4 * (co))
int n3d_head_eval(const n3d_head* h, float* p, int64_t psb, int64_t psc, int64_t psv, const void* t, int64_t tsb, int64_t tsc, int64_t tsv,
                  float smooth, float thr, double* partial, double* hpartial, double* sums, float* loss, double* acc, void* stream);

/* ---- Tversky / focal / cross-entropy loss in the head's passes and on probabilities.  For a (b, c) pair with A = sum p*t, P = sum p,
 * T = sum t over the sample's N voxels, logit z and p = sigmoid(z):
 *   TI = (A + smooth) / (A + alpha (P - A) + beta (T - A) + smooth),   u = max(1 - TI, 0),
 *   loss = mean_bc u^gamma + bce_weight * mean_bcv [max(z, 0) - z t + log1p(exp(-|z|))].
 * A pair with u == 0 contributes 0 and a zero gradient for every gamma.  alpha, beta >= 0, alpha + beta > 0, gamma > 0,
 * bce_weight >= 0, smooth > 0, otherwise N3D_ERR_INVALID.  alpha = beta = 0.5, gamma = 1, bce_weight = 0, smooth = s / 2 is the Dice
 * loss of n3d_head_fwd with smooth = s.
 * n3d_head_loss_fwd / _eval / _bwd: n3d_head_fwd / n3d_head_eval / n3d_head_bwd (same operands, layouts and scratch) with this loss.
 *   bce_weight == 0: every head shape of the Dice mode, records of S = 3 doubles.  bce_weight > 0: Co = 3 only (N3D_ERR_UNSUPPORTED
 *   otherwise), and the records hold S = 4 doubles, the fourth being the cross-entropy sum:
 *   partial: double[B][Co][n3d_head_rows(N)][S], sums: double[B][Co][S].
 *   coef: float[2 * B * Co + 1] written by n3d_head_loss_fwd and read by n3d_head_loss_bwd: per pair (k2, k0) with
 *   d loss / d p = k2 t + k0 for the Tversky term, then kb = bce_weight / (B Co N); d loss / d z = (k2 t + k0) p (1 - p) + kb (p - t).
 *   n3d_head_loss_eval adds the configured loss into acc[0]; the region counts are those of n3d_head_eval.
 * n3d_tversky_fwd / _bwd: the loss on probabilities (n3d_dice_fwd / n3d_dice_bwd operands; partial: double[B][C][n3d_dice_rows(N)][3],
 *   sums: double[B][C][3], coef: float[2 * B * C]).  The cross-entropy term is formed from logits and exists in the head only:
 *   bce_weight > 0 is N3D_ERR_UNSUPPORTED here. */
typedef struct n3d_loss { float alpha, beta, gamma, bce_weight, smooth; } n3d_loss;
int n3d_head_loss_fwd(const n3d_head* h, const n3d_loss* l, float* p, int64_t psb, int64_t psc, int64_t psv, float* logits, const void* t,
                      int64_t tsb, int64_t tsc, int64_t tsv, double* partial, double* sums, float* coef, float* loss, void* stream);
int n3d_head_loss_eval(const n3d_head* h, const n3d_loss* l, float* p, int64_t psb, int64_t psc, int64_t psv, const void* t, int64_t tsb,
                       int64_t tsc, int64_t tsv, float thr, double* partial, double* hpartial, double* sums, float* loss, double* acc,
                       void* stream);
int n3d_head_loss_bwd(const n3d_head* h, const void* t, int64_t tsb, int64_t tsc, int64_t tsv, const float* coef, const float* dloss, void* dx,
                      int64_t dxld, int dx_dtype, int flags, float* dw, float* dbias, void* ws, size_t ws_bytes, n3d_final_job* deferred,
                      void* stream);
int n3d_tversky_fwd(const float* p, int64_t psb, int64_t psc, int64_t psv, const float* t, int64_t tsb, int64_t tsc, int64_t tsv, int B, int C,
                    int64_t N, const n3d_loss* l, double* partial, double* sums, float* coef, float* loss, void* stream);
int n3d_tversky_bwd(const float* t, int64_t tsb, int64_t tsc, int64_t tsv, int B, int C, int64_t N, const float* coef, const float* dloss,
                    float* dp, int64_t dsb, int64_t dsc, int64_t dsv, void* stream);

/* ---- Boundary loss (Kervadec et al., MIDL 2019): loss = base + w * mean_bcv (p * phi), phi the signed distance map of the targets.
 * Its gradient with respect to p is phi itself: one more sum per row in the head's forward pass, one more term of d logit in its
 * backward pass.
 * n3d_target_sdt: phi of B x C binary maps of D0 x D1 x D2 voxels (each extent 1..N3D_SDT_MAX_AXIS, B * C <= 65535; otherwise
 *   N3D_ERR_UNSUPPORTED).  t: N3D_F32 or N3D_U8 holding {0, 1}, element (b, c, v) at t[b*tsb + c*tsc + v*tsv] with v the C-order
 *   voxel index (the head's target operand); phi: fp32 with strides of its own.  With d2_fg(v) / d2_bg(v) the smallest squared
 *   Euclidean index distance from v to a voxel of the same map with t = 1 / t = 0 (exact integers; only voxels of the patch count):
 *     t(v) = 0:  phi = (float) sqrt((double) d2_fg)
 *     t(v) = 1:  phi = (float) (-(sqrt((double) d2_bg) - 1.0))
 *   -- scipy.ndimage.distance_transform_edt under one_hot2dist, bit for bit -- and phi = 0.0f where the wanted distance has no source
 *   in the patch, so an empty map and a full map are all zero.
 *   ws: n3d_target_sdt_workspace_bytes(B, C, D0, D1, D2) bytes (two int32 fields per map; 0 on a bad shape), 4-byte aligned, nothing
 *   in it has to be cleared.  Three launches on the stream, integer minima, one writer per word: no host sync, same bits every run.
 * n3d_head_bnd_fwd: n3d_head_loss_fwd (same operands, layouts and base loss l) plus phi and the device scalar bnd_weight:
 *   *loss = base + w * mean_bcv (p * phi), w = *bnd_weight read by the finalize launch -- a schedule changes it between the replays
 *   of a captured graph.  Co = 3 only (N3D_ERR_UNSUPPORTED otherwise).  The records gain one double at their END, sum p * phi:
 *   partial: double[B][Co][n3d_head_rows(N)][S + 1], sums: double[B][Co][S + 1] with S of n3d_head_loss_fwd (3, or 4 with
 *   bce_weight > 0).  coef: float[2 * B * Co + 2]: n3d_head_loss_fwd's 2 * B * Co + 1, then k_phi = w / (B Co N).
 * n3d_head_bnd_bwd: n3d_head_loss_bwd plus phi: d loss / d z = (k2 t + k0 + k_phi phi) p (1 - p) + kb (p - t).
 * There is no evaluation form: an evaluation reports the base loss (n3d_head_loss_eval), whose definition does not move. */
#define N3D_SDT_MAX_AXIS 1024
size_t n3d_target_sdt_workspace_bytes(int B, int C, int D0, int D1, int D2);
int n3d_target_sdt(const void* t, int t_dtype, int64_t tsb, int64_t tsc, int64_t tsv, int B, int C, int D0, int D1, int D2, float* phi,
                   int64_t fsb, int64_t fsc, int64_t fsv, void* ws, size_t ws_bytes, void* stream);
int n3d_head_bnd_fwd(const n3d_head* h, const n3d_loss* l, float* p, int64_t psb, int64_t psc, int64_t psv, float* logits, const void* t,
                     int64_t tsb, int64_t tsc, int64_t tsv, const float* phi, int64_t fsb, int64_t fsc, int64_t fsv, const float* bnd_weight,
                     double* partial, double* sums, float* coef, float* loss, void* stream);
int n3d_head_bnd_bwd(const n3d_head* h, const void* t, int64_t tsb, int64_t tsc, int64_t tsv, const float* phi, int64_t fsb, int64_t fsc,
                     int64_t fsv, const float* coef, const float* dloss, void* dx, int64_t dxld, int dx_dtype, int flags, float* dw,
                     float* dbias, void* ws, size_t ws_bytes, n3d_final_job* deferred, void* stream);

/* ---- layout: NCDHW <-> NDHWC (caller tensors arrive NCDHW: train.py:118-119) ---------------------- */
int n3d_ncdhw_to_ndhwc(const float* src, float* dst, int64_t dld, int B, int C, int64_t N, void* stream);
int n3d_ndhwc_to_ncdhw(const float* src, int64_t sld, float* dst, int B, int C, int64_t N, void* stream);

/* ---- on-device data step (the work of the reference's generator just ahead of the hot path, train.py:117-119):
 * patch crop with zero padding (patches.py:99-115,152-169) + one cube isometry per patch (augment.py:73-131; the same
 * for data and truth) + label expansion to three binary channels (generator.py:230-248, including its quirk that the
 * inclusive "WT" channel is labels {1,2}).  out[b][i] = vol[corner + src(i)], src_a(i) = i[perm[a]] or P-1-i[perm[a]]
 * (flip[a]); zero outside the volume.  vol: (Cv, X, Y, Z) contiguous fp32; truth: (X, Y, Z) uint8 labels {0,1,2,4} or
 * NULL; x_out: pitched NDHWC (B, Cv, P, P, P); t_out: (B, 3, P, P, P) contiguous fp32 -- uint8 with N3D_PATCH_T_U8 -- or NULL.
 * flags: N3D_PATCH_INCLUSIVE (the reference's `inclusive_label`) | N3D_PATCH_T_U8.  descs: HOST array. */
#define N3D_PATCH_MAX_BATCH 64
#define N3D_PATCH_INCLUSIVE 1
#define N3D_PATCH_T_U8 2       /* the three boolean maps as bytes (generator.py:230-248 yields booleans; train.py:118 casts them) */
typedef struct n3d_patch_desc { int32_t corner[3]; int32_t perm[3]; int32_t flip[3]; } n3d_patch_desc;
int n3d_patch_batch(const float* vol, int Cv, const uint8_t* truth, int X, int Y, int Z, const n3d_patch_desc* descs, int B, int P,
                    int flags, float* x_out, int64_t xld, void* t_out, void* stream);

/* ---- the generator's epoch around that gather (generator.py:68-217): which candidate patches an epoch uses, and batches that
 * mix volumes.  A patch is "empty" when all of its modalities are zero and "healthy" when all of its labels are zero
 * (generator.py:202-207); "zero" is numpy's `== 0`: -0.0 is zero, NaN / inf / denormals are not ((bits & 0x7fffffff) != 0).
 *
 * Summed-area tables: sat is (X+1, Y+1, Z+1) int32 pairs, (mask 0, mask 1) interleaved, with a zero plane at the low end of every
 * axis: entry (i, j, k) counts the voxels x < i, y < j, z < k where some channel is nonzero (mask 0) / the label is nonzero
 * (mask 1; 0 throughout when truth is NULL).  Built once per volume; exact integers, equal to np.cumsum of the masks.
 * X * Y * Z < 2^31.  sat: 8 * (X+1) * (Y+1) * (Z+1) bytes of device memory. */
int n3d_volume_sat(const float* vol, int Cv, const uint8_t* truth, int X, int Y, int Z, int32_t* sat, void* stream);

/* A volume of a set (device-resident table of records: n3d_patch_qualify / n3d_patch_gather read it on the device).
 * data: (Cv, X, Y, Z) contiguous fp32 (Cv common to the set); truth: (X, Y, Z) uint8 labels or NULL; sat: its n3d_volume_sat table. */
typedef struct n3d_patch_volume {
  const float* data;
  const uint8_t* truth;
  const int32_t* sat;
  int32_t dims[3];
  int32_t pad_;
} n3d_patch_volume;

/* Qualification of N candidate patches of edge P: cand is a DEVICE int32 (N, 4) table of (volume index, corner x, y, z); each
 * patch [c, c + P) is clipped to its volume and answered from the tables by inclusion-exclusion (8 lookups per mask).
 * flags[i] (uint8, device): bit 0 = some modality is nonzero, bit 1 = some label is nonzero; 0 for a patch wholly outside its
 * volume and for a volume index outside [0, nvol). */
int n3d_patch_qualify(const n3d_patch_volume* vols, int nvol, const int32_t* cand, int64_t N, int P, uint8_t* flags, void* stream);

/* ---- random and foreground-centred crops, drawn on the device (none of it the reference's: nnU-Net's oversampled foreground,
 * MONAI's RandCropByPosNegLabel / RandCropByLabelClasses, TorchIO's LabelSampler).  Instead of the fixed candidate grid, an epoch's
 * candidate table is drawn: each sample is a uniformly random corner, or -- with probability fg_threshold / 2^32 -- the corner that
 * centres the patch on a uniformly random voxel of a mask.  The table has n3d_patch_qualify's format and goes through it unchanged.
 *
 * Masks (N3D_SAMPLE_MASKS of them; mask m is bit m of `masks`): 0 brain = some channel is nonzero ("nonzero" as above: -0.0 is
 * zero, NaN / inf / denormals are not), 1 tumour = label != 0, 2 = label 1, 3 = label 2, 4 = label 4.
 *
 * Line index of a volume: index is (N3D_SAMPLE_MASKS, X*Y + 1) int32.  A line is one (x, y), l = x*Y + y, its Z voxels in C order.
 * index[m][l] = the number of mask-m voxels in the lines before l; index[m][X*Y] = the mask's total: the exclusive prefix sum
 * np.concatenate(([0], np.cumsum(mask.reshape(X*Y, Z).sum(1)))).  With truth NULL rows 1 to 4 are zero.  X * Y * Z < 2^31.  Exact
 * integers (ballots and popcounts, an integer scan: no floating point, no atomics), so two runs give the same bits.  Two launches:
 * one wave per line, then one workgroup per mask.  index: 20 * (X*Y + 1) bytes of device memory. */
#define N3D_SAMPLE_MASKS 5
int n3d_volume_line_index(const float* vol, int Cv, const uint8_t* truth, int X, int Y, int Z, int32_t* index, void* stream);

/* N samples in ONE launch (one wave per sample; no sample waits for another).  vols: the DEVICE table of nvol records; index: a DEVICE
 * array of nvol pointers, entry v the line index of volume v (every volume named in ids must have one); ids: a DEVICE array of the
 * n_ids volume indices to draw from; cand: DEVICE (N, 4) int32, 16-byte aligned, rows (volume index, corner x, y, z); mode: DEVICE
 * uint8 (N).  P: the patch edge.  (key0, key1): the epoch's Philox key.  For sample n, 0 <= n < N <= N3D_SAMPLE_MAX = 2^24:
 *   draws:       w0..w3 = Philox4x32-10 (the constants and rounds of n3d_appear_desc's noise stage) of the counter (n, 2, 0, 0) and
 *                u0..u3 of the counter (n, 3, 0, 0), both under the key (key0, key1).  (Counter words 0 and 1 in the second place are
 *                the appearance noise's and the elastic lattice's.)
 *   reduction:   reduce(q, R) = (uint32_t)(((uint64_t)q * R) >> 32), in [0, R) for R >= 1; value i is taken by floor or ceil of
 *                2^32 / R words, so the bias of any value is below R / 2^32 relative.
 *   volume:      v = ids[reduce(u0, n_ids)], its dims D[3] = (X, Y, Z).
 *   foreground:  the sample is foreground-centred iff (uint64_t)u1 < fg_threshold; fg_threshold in [0, 2^32] (0: never; 2^32: always;
 *                the host passes round(p * 2^32)).
 *   mask:        of the masks whose bit is set in `masks`, those with index[m][X*Y] > 0 in volume v, in ascending m: k of them.
 *                k > 0: the mask is the reduce(u2, k)-th of them (from 0).  k == 0: the sample falls back to a uniform corner.
 *   voxel:       T = index[m][X*Y], r = reduce(w0, T); the line l is the largest with index[m][l] <= r (binary search:
 *                np.searchsorted(row, r, side="right") - 1); the voxel is the (r - index[m][l])-th mask voxel of line l (from 0) in
 *                ascending z.  That is voxel r of np.argwhere(mask): uniform over the mask's voxels.  (x, y) = (l / Y, l % Y).
 *   corner:      per axis a: D[a] >= P: lo = 0, hi = D[a] - P; else lo = hi = -((P - D[a]) / 2) (a box smaller than the patch is
 *                centred; the gather zero-pads it); integer division.  Foreground: c[a] = min(max(voxel[a] - P / 2, lo), hi) --
 *                unclamped, the voxel sits at patch index P / 2.  Uniform and fallback: c[a] = lo + reduce(w[1 + a], hi - lo + 1).
 *   outputs:     cand[n] = (v, c[0], c[1], c[2]);  mode[n] = the mask m for a foreground sample, N3D_SAMPLE_MODE_UNIFORM for a
 *                uniform one, N3D_SAMPLE_MODE_FALLBACK for the fallback.
 * An id outside [0, nvol) cannot be refused on the host (ids lives on the device): such a sample writes cand[n] = (id, 0, 0, 0) and
 * mode[n] = N3D_SAMPLE_MODE_BAD_ID and touches no volume; n3d_patch_qualify flags it 0.  A volume whose index pointer is NULL is
 * treated the same way.
 * The decision is per sample: there is no per-batch guarantee such as nnU-Net's "the last third of every batch is forced".
 * N3D_ERR_INVALID before any launch: masks == 0 with fg_threshold > 0, or bits beyond the five masks; fg_threshold > 2^32; n_ids,
 * P, nvol or Cv < 1; N < 0 or N > N3D_SAMPLE_MAX; a NULL table; cand not 16-byte aligned (vols, index: 8; ids: 4).  N == 0 (with
 * legal scalars) returns N3D_OK without a launch and reads no table. */
#define N3D_SAMPLE_MAX 16777216
#define N3D_SAMPLE_MODE_UNIFORM 255
#define N3D_SAMPLE_MODE_FALLBACK 254
#define N3D_SAMPLE_MODE_BAD_ID 253
int n3d_patch_sample(const n3d_patch_volume* vols, const int32_t* const* index, int nvol, int Cv, const int32_t* ids, int n_ids,
                     int64_t N, int P, uint32_t key0, uint32_t key1, uint64_t fg_threshold, int masks, int32_t* cand, uint8_t* mode,
                     void* stream);

/* n3d_patch_batch for a batch whose patches come from different volumes of a set: descriptor = n3d_patch_desc + volume index.
 * Output bit-identical to n3d_patch_batch on each patch's own volume.  vols: the DEVICE table of nvol records; descs: HOST array
 * of at most N3D_PATCH_MAX_BATCH (perm and volume index checked here).  With t_out, a record without truth gives label 0. */
typedef struct n3d_patch_gdesc { n3d_patch_desc d; int32_t vol; } n3d_patch_gdesc;
int n3d_patch_gather(const n3d_patch_volume* vols, int nvol, int Cv, const n3d_patch_gdesc* descs, int B, int P, int flags,
                     float* x_out, int64_t xld, void* t_out, void* stream);

/* n3d_patch_gather with the reference's scale / flip distortion (augment.py:50-67, generator.py:208-211) in the same launch.  The
 * reference crops the patch, flips it on the drawn axes, rescales it around its centre by resampling with nearest neighbour
 * (nilearn's resample_to_img -> scipy.ndimage.affine_transform with a diagonal matrix, order 0, mode "constant", cval 0), and only
 * then applies the isometry.  So for output voxel i, on each source axis a:
 *   j = the patch index the isometry of g.d gives (as n3d_patch_gather);
 *   unless `identity`:  c = ((double)j + sh[a]) * A[a]   -- scipy's zoom-shift coordinate: an fp64 add, then an fp64 multiply;
 *                       0 <= c && c <= P-1, tested on c itself, else the voxel is 0 (data and every target);
 *                       j = (int)floor(c + 0.5);
 *   with aflip[a]:      j = P-1-j;
 *   source voxel corner[a] + j, zero outside the volume (as n3d_patch_gather); the same voxel for data and labels.
 * A: the diagonal of the resampling matrix, finite and nonzero (negative allowed); sh = offset / A, finite; identity != 0: the
 * patch is not resampled (no scale drawn, or a scale so close to 1 that nilearn returns the image as it is) and A, sh are only
 * checked.  With identity set and aflip clear everywhere the output is bit-identical to n3d_patch_gather.  descs: HOST array of
 * at most N3D_PATCH_AUG_MAX_BATCH (the widened descriptors travel in the 4 KB of kernel arguments). */
#define N3D_PATCH_AUG_MAX_BATCH 32
typedef struct n3d_patch_adesc { n3d_patch_gdesc g; int32_t aflip[3]; int32_t identity; double A[3]; double sh[3]; } n3d_patch_adesc;
int n3d_patch_gather_aug(const n3d_patch_volume* vols, int nvol, int Cv, const n3d_patch_adesc* descs, int B, int P, int flags,
                         float* x_out, int64_t xld, void* t_out, void* stream);

/* n3d_patch_gather_aug with a full 3x4 resampling map (a small rotation composed with the scale), linear interpolation of the
 * DATA (the truth stays nearest neighbour) and a per-channel intensity scale and shift of the nonzero voxels, in the same single
 * launch.  For output voxel i of patch b, with j = the patch index the isometry of g.d gives (as n3d_patch_gather) and k[0..11]
 * the twelve fp64 coefficients:
 *   coordinate, mode 0:  c_a = ((double)j_a + sh[a]) * A[a],  A = k[0..2], sh = k[3..5]  -- n3d_patch_gather_aug's rule, bit for
 *                        bit (its `identity` is A = 1, sh = 0, which the formula reproduces exactly); k[6..11] are only checked;
 *   coordinate, mode 1:  c_a = ((m[a][0]*j_0 + m[a][1]*j_1) + m[a][2]*j_2) + off[a],  m = k[0..8] row-major, off = k[9..11]:
 *                        products in axis order, the offset last, every product and every sum rounded to fp64 on its own (what
 *                        scipy.ndimage.affine_transform does with a 2-D matrix);
 *   bounds:              the voxel has a source iff 0 <= c_a <= P-1 on all three axes, tested on c itself; otherwise the data and
 *                        every target are 0;
 *   labels:              always the one voxel r_a = (int)floor(c_a + 0.5);
 *   data, order 0:       the same voxel;
 *   data, order 1:       f_a = floor(c_a), w_a = c_a - f_a in fp64; the eight taps f + d, d in {0,1}^3, visited in lexicographic
 *                        order of (d_0, d_1, d_2); tap weight (u_0 * u_1) * u_2 with u_a = d_a ? w_a : 1.0 - w_a; acc = 0.0, then
 *                        acc = acc + weight * (double)x per tap (a separate multiply and add); a tap whose index exceeds P-1 (it
 *                        can only have w_a == 0) is skipped and never read, and so is a tap outside the volume (the crop's zero
 *                        padding) -- the kernel may load voxel 0 of the channel in such a tap's place and drop the value; the
 *                        result is (float)acc;
 *   flip:                on an axis with aflip[a] every tap index r becomes P-1-r before corner[a] is added (the flip acts on the
 *                        crop before it is resampled, as n3d_patch_gather_aug);
 *   intensity:           with `intensity` set and y the resampled value of channel c: if y != 0 (-0.0 is zero), y = y * gain[c]
 *                        rounded to fp32, then y = y + bias[c] rounded to fp32; a voxel that is 0 stays 0.  With `intensity` clear
 *                        the bits are left as they are and gain, bias are only checked.  `intensity` needs Cv <= 4.
 * mode and order are 0 or 1; all twelve coefficients, gain and bias are finite, and A is nonzero in mode 0.  With mode 0, order 0
 * and `intensity` clear the output is bit-identical to n3d_patch_gather_aug (to n3d_patch_gather with A = 1, sh = 0, no aflip).
 * descs: HOST array of at most N3D_PATCH_WARP_MAX_BATCH (the descriptors travel in the 4 KB of kernel arguments). */
#define N3D_PATCH_WARP_MAX_BATCH 16
typedef struct n3d_patch_wdesc {
  n3d_patch_gdesc g;
  int32_t aflip[3];
  int32_t mode;        /* 0: zoom-shift rule, 1: matrix rule */
  int32_t order;       /* 0: nearest, 1: linear -- the data only (3: cubic B-spline, taken by n3d_patch_gather_spline alone) */
  int32_t intensity;   /* != 0: gain and bias are applied to the nonzero voxels */
  double k[12];
  float gain[4];
  float bias[4];
} n3d_patch_wdesc;
int n3d_patch_gather_warp(const n3d_patch_volume* vols, int nvol, int Cv, const n3d_patch_wdesc* descs, int B, int P, int flags,
                          float* x_out, int64_t xld, void* t_out, void* stream);

/* n3d_patch_gather_warp with an elastic (non-rigid) displacement added to the coordinate, in the same single launch: a free-form
 * deformation on a coarse lattice of uniform cubic B-splines (batchgenerators' / TorchIO's / MONAI's elastic transform; none of it
 * the reference's) whose control values are generated on the device from an 8-byte key.  A descriptor is n3d_patch_wdesc `w` plus:
 *   lattice:     cells = n cells per axis, 1 <= n <= 8; G = n + 3 control points per axis, each holding a 3-vector; lattice point
 *                l = (l_0 * G + l_1) * G + l_2.
 *   values:      w0..w3 = Philox4x32-10 (the constants and rounds of n3d_appear_desc's noise stage) of the counter (l, 1, 0, 0)
 *                under the key (key[0], key[1]);  D[a][l] = 2.0 * ((double)w_a * 2^-32) - 1.0 for a = 0, 1, 2: in [-1, 1), exact.
 *   lock:        L, 0 <= L <= 3, G - 2 L >= 1:  D[a][l] = +0.0 where some lattice index l_i < L or l_i >= G - L.  L = 2 is TorchIO's
 *                locked_borders; L = 3 holds the patch's faces still (below).
 *   evaluation:  at the patch index j the isometry of w.g.d gives -- the j the warp rule starts from.  Per axis a:
 *                  s = (double)j_a * inv_h          inv_h = (double)n / (double)(P - 1), computed by the host and passed;
 *                  cell = (int)min(floor(s), (double)(n - 1));   f = s - (double)cell;   g = 1.0 - f;   with S = 1.0 / 6.0 (the fp64
 *                  constant 0.16666666666666666) the four weights of the axis are
 *                  b[0] = ((g * g) * g) * S
 *                  b[1] = ((((3.0 * f - 6.0) * f) * f) + 4.0) * S
 *                  b[2] = ((((3.0 - 3.0 * f) * f + 3.0) * f) + 1.0) * S
 *                  b[3] = ((f * f) * f) * S
 *                (b0, cell0), (b1, cell1), (b2, cell2) for the three axes.  For each component a the 64 control points cell + m,
 *                m in {0..3}^3, are summed separably, innermost along axis 2, every sum left to right starting from the m = 0 product:
 *                  T(m_0, m_1) = ((b2[0] * D(m_0, m_1, 0) + b2[1] * D(m_0, m_1, 1)) + b2[2] * D(m_0, m_1, 2)) + b2[3] * D(m_0, m_1, 3)
 *                  U(m_0)      = ((b1[0] * T(m_0, 0) + b1[1] * T(m_0, 1)) + b1[2] * T(m_0, 2)) + b1[3] * T(m_0, 3)
 *                  acc_a       = ((b0[0] * U(0) + b0[1] * U(1)) + b0[2] * U(2)) + b0[3] * U(3)
 *                with D(m) = D[a][((cell0 + m_0) * G + cell1 + m_1) * G + cell2 + m_2];  delta_a = amp[a] * acc_a.
 *   coordinate:  c'_a = c_a + delta_a, c the coordinate of n3d_patch_wdesc (mode 0 or 1, unchanged).  Everything downstream is the
 *                warp rule applied to c': the bounds test on c' itself, the nearest voxel of the labels, order 0 / 1 of the data,
 *                aflip, the crop's zero padding, the intensity map.
 * Every product, sum and difference is rounded to fp64 on its own (no contraction).  With `elastic` clear nothing above is
 * evaluated (cells, lock, amp and inv_h are still checked) and the output is bit-identical to n3d_patch_gather_warp; so it is
 * with `elastic` set and amp = 0.  The weights are non-negative on [0, 1] and sum to 1, so |delta_a| <= amp[a] (up to rounding),
 * and the field's slope is at most 2 amp / h, h = (P - 1) / n: for amp < h / 2 the map does not fold.  With L = 3 the field is
 * exactly 0 on the faces j_a = 0 (f = 0: b[3] = 0 and the three other points are locked); on the faces j_a = P - 1 it is exactly 0
 * when (double)(P - 1) * inv_h rounds to n (g = 0; it does for every n at P <= 25) and at most amp * 2^-149 in size otherwise (|g| <=
 * 2^-49), which is absorbed by every c of size 2^-96 or above.
 * cells and lock in range, amp finite and >= 0, inv_h finite and >= 0, and all n3d_patch_gather_warp checks, else
 * N3D_ERR_INVALID before any launch.  descs: HOST array of at most N3D_PATCH_ELASTIC_MAX_BATCH (the descriptors travel in the
 * 4 KB of kernel arguments: sixteen of them would leave under 100 bytes). */
#define N3D_PATCH_ELASTIC_MAX_BATCH 8
#define N3D_PATCH_ELASTIC_MAX_CELLS 8
typedef struct n3d_patch_edesc {
  n3d_patch_wdesc w;
  int32_t elastic;     /* != 0: the displacement is added */
  int32_t cells;       /* n */
  int32_t lock;        /* L */
  uint32_t key[2];     /* the Philox key of the control values */
  int32_t pad_;
  double amp[3];       /* largest displacement per axis, in voxels */
  double inv_h;        /* n / (P - 1) */
} n3d_patch_edesc;
int n3d_patch_gather_elastic(const n3d_patch_volume* vols, int nvol, int Cv, const n3d_patch_edesc* descs, int B, int P, int flags,
                             float* x_out, int64_t xld, void* t_out, void* stream);

/* n3d_patch_gather_elastic with the DATA interpolated by a cubic B-spline (order 3): what scipy.ndimage.map_coordinates(order=3,
 * mode="constant", cval=0) makes of the crop -- the default resampler of nnU-Net / batchgenerators / TorchIO; none of it the
 * reference's.  Every descriptor has w.order == 3; coordinate (mode 0 / 1, plus the displacement with `elastic`), bounds test, aflip,
 * labels (the nearest voxel) and the intensity map are n3d_patch_gather_elastic's.  Per patch b and channel c:
 *   crop:        raw[q] = volume voxel corner_a + (aflip[a] ? P-1-q_a : q_a), 0.0f outside the volume: fp32, P^3 per (b, c).
 *   prefilter:   coef = n3d_spline_prefilter(raw) (below): fp64, P^3 per (b, c).
 *   taps:        a voxel whose c_a lies outside [0, P-1] on some axis is 0 (the bounds test).  Otherwise per axis f = floor(c_a),
 *                t = c_a - f, the four weights b[0..3] of t as n3d_patch_edesc's evaluation forms them (g = 1.0 - t, ...), for the
 *                taps q = f-1, f, f+1, f+2, each mirrored into the crop: q < 0 -> -q, q > P-1 -> 2 (P-1) - q (hence P >= 4).
 *                acc = 0.0, then over the 64 taps in the order 16 i0 + 4 i1 + i2:  acc = acc + ((b0[i0] * b1[i1]) * b2[i2]) * coef[tap],
 *                every product and sum rounded to fp64 on its own;  y = (float)acc.
 *   mask:        the filter is recursive, so y is nonzero in the background too.  The voxel is stored as 0.0f when the NEAREST crop
 *                voxel raw[floor(c_a + 0.5)] of that channel is 0 (-0.0 is zero) -- the voxel order 0 reads; otherwise y is stored,
 *                and a y that rounded to +-0 is stored as FLT_MIN, so that x != 0 still says "brain".  No clamping: the spline
 *                overshoots at edges as scipy's does.
 *   intensity:   on the voxels the mask keeps, * gain[c] then + bias[c] in fp32, as n3d_patch_wdesc.
 * scratch: DEVICE, 8-byte aligned, n3d_patch_spline_scratch_bytes(B, Cv, P) = 12 bytes per voxel and channel (coef, then raw);
 * overwritten by every call, holds nothing between calls.  Five launches whatever the data (crop, three prefilter passes, gather),
 * no host synchronisation, no atomics: capturable.  B <= N3D_PATCH_ELASTIC_MAX_BATCH, P >= 4, P^3 < 2^31, order == 3 everywhere, a
 * scratch that is not null and large enough, and all n3d_patch_gather_elastic checks, else N3D_ERR_INVALID before any launch.
 *
 * n3d_spline_prefilter: scipy.ndimage.spline_filter(order=3, mode="mirror") of n contiguous P^3 fp32 cubes into n fp64 cubes (raw
 * and coef may not overlap), P >= 4: the lines along axis 0 are filtered first, then axis 1, then axis 2.  With z = sqrt(3.0) - 2.0
 * and, all computed on the host in fp64, gain = (1.0 - z) * (1.0 - 1.0 / z), zn = z * z * .. * z (P-1 factors, multiplied up one by
 * one), inv0 = 1.0 / (1.0 - zn * zn), anti = z / (z * z - 1.0), one line c[0..P-1] becomes, every operation rounded on its own:
 *   c[i] = c[i] * gain for every i  (the first pass converts the fp32 sample to fp64 first);
 *   s = c[0] + zn * c[P-1];  zi = z;  for i = 1 .. P-2:  s = s + zi * (c[i] + zn * c[P-1-i]),  zi = zi * z;   c[0] = s * inv0;
 *   for i = 1 .. P-1:  c[i] = c[i] + z * c[i-1];
 *   c[P-1] = (z * c[P-2] + c[P-1]) * anti;
 *   for i = P-2 .. 0:  c[i] = z * (c[i+1] - c[i]). */
size_t n3d_patch_spline_scratch_bytes(int B, int Cv, int P);
int n3d_spline_prefilter(const float* raw, int64_t n, int P, double* coef, void* stream);
int n3d_patch_gather_spline(const n3d_patch_volume* vols, int nvol, int Cv, const n3d_patch_edesc* descs, int B, int P, int flags,
                            void* scratch, size_t scratch_bytes, float* x_out, int64_t xld, void* t_out, void* stream);

/* ---- appearance augmentation of a gathered batch, in place (none of it the reference's: the four transforms of batchgenerators /
 * nnU-Net that the BraTS recipes train with).  x: DEVICE fp32 batch (B, Cv, P, P, P) in NDHWC storage with channel pitch ld >= Cv,
 * as n3d_patch_gather* write it; the lanes between Cv and ld are never touched.  descs: HOST array, one record per patch.
 *
 * The brain mask of a (patch, channel) is x != 0 on entry (-0.0 is zero, as in n3d_patch_gather_warp), taken ONCE before the first
 * stage.  Every stage writes only masked voxels and takes its statistics over them; the background stays exactly 0.0f; a (patch,
 * channel) without a masked voxel is left alone by contrast and gamma (n = 0: no division).  The stages run in the fixed order
 * noise, blur, contrast, gamma, each only on the patches whose flag is set, each on the values the earlier stages left.  All
 * arithmetic is fp64 on fp32 loads, every product, sum, quotient and library call rounded on its own in the association written;
 * "fp32(..)" is the one rounding to fp32 where a stage stores.  v = (i * P + j) * P + k is the voxel's index in its patch.
 *
 *   noise     w0..w3 = Philox4x32-10 (multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85, ten rounds) of the
 *             counter (v, 0, 0, 0) under the patch's key (key[0], key[1]);  u1 = ((double)w0 + 1) * 2^-32,  u2 = (double)w1 * 2^-32,
 *             rho = sqrt(-2 * log(u1)),  th = 6.283185307179586 * u2,  z0 = rho * cos(th),  z1 = rho * sin(th);  (w2, w3) give
 *             (z2, z3) the same way.  Channel c:  y = fp32(x + sigma * z_c).
 *   blur      y = fp32(G * x), G * x the separable Gaussian of the channel's whole P^3 patch (background zeros take part), what
 *             scipy.ndimage.gaussian_filter(x, sigma_c, mode="reflect", truncate=4.0) computes on fp64 input: three passes, axis 0,
 *             1, 2, each  out[i] = sum over k = -r .. +r IN THAT ORDER of weights[c][|k|] * in[refl(i + k)]  (the first product, then
 *             acc = acc + product), refl(i) = -i - 1 below 0 and 2 P - 1 - i from P on; the intermediates stay fp64 and the one
 *             rounding is at the end.  radius[c] = r = int(4 sigma_c + 0.5) and weights[c][0 .. r] = exp(-0.5 / sigma_c^2 * k^2) /
 *             (their sum over -r .. r) come from the host (numpy): the device evaluates no exp.  0 <= r <= N3D_APPEAR_MAX_RADIUS and
 *             r <= P (one reflection suffices), else N3D_ERR_INVALID.  The result does not depend on any read / write order: the
 *             launch writes to scratch and a second one lands the masked voxels in x.
 *   sums      "the sum" of the terms a[v] of a (patch, channel) below is this fixed order: terms of voxels outside the mask are
 *             +0.0; FOLD(a[0 .. 256 n)) = lane t adds a[t], a[t + 256], .. in that order onto 0.0, then the 256 lanes are folded
 *             in halves, lane[t] = lane[t] + lane[t + s] for s = 128, 64, .. 1; each chunk of 1024 consecutive voxels (the last
 *             padded with +0.0) gives FOLD(chunk); the sum is FOLD(the chunk results in chunk order, padded with +0.0 to a
 *             multiple of 256).  n counts the masked voxels; lo / hi are their minimum / maximum.
 *   contrast  n, lo, hi and m = S / n with S the sum of x;  y = fp32(min(max((x - m) * factor[c] + m, lo), hi))
 *             (batchgenerators' augment_contrast(preserve_range=True, per_channel=True)).
 *   gamma     n, lo, hi, m as above, sd = sqrt(sum((x - m) * (x - m)) / n);
 *             x' = fp32(pow((x - lo) / ((hi - lo) + 1e-7), gamma_c[c]) * (hi - lo) + lo);  then m' and sd' of x' the same way and
 *             y = fp32((x' - m') / (sd' + 1e-8) * sd + m)   (augment_gamma(retain_stats=True, per_channel=True)).
 *
 * How the parameters travel: each stage's share of the descriptors is repacked into that stage's own launch-argument block (the
 * blur's half kernels, 16 x 4 x 7 doubles, are 3.5 KB of the 4 KB a launch takes); nothing is copied to the device and nothing
 * synchronises.  A stage that no patch asks for launches nothing; with no flag set at all the call launches nothing and does not
 * look at the scratch.  Launches otherwise: the mask 1, noise 1, blur 2, contrast 2, gamma 4.  No floating-point atomics: two
 * runs on the same input give the same bits.  Bad arguments (B > N3D_APPEAR_MAX_BATCH, Cv > 4, a radius beyond the bounds, a
 * parameter that is not finite, sigma or gamma below 0, a scratch that is too small) return N3D_ERR_INVALID before any launch.
 * scratch: DEVICE, 8-byte aligned, n3d_patch_appearance_scratch(B, Cv, P) bytes (0 for arguments out of range): a mask byte per
 * voxel, the blur's fp32 output and the chunk partials. */
#define N3D_APPEAR_MAX_BATCH 16
#define N3D_APPEAR_MAX_RADIUS 6
#define N3D_APPEAR_MAX_PATCH 256
typedef struct n3d_appear_desc {
  int32_t noise, blur, contrast, gamma;            /* != 0: the stage acts on this patch */
  uint32_t key[2];                                 /* noise: the Philox key */
  double sigma;                                    /* noise */
  int32_t radius[4];                               /* blur, per channel */
  double weights[4][N3D_APPEAR_MAX_RADIUS + 1];    /* blur: weights[c][|k|] */
  double factor[4];                                /* contrast */
  double gamma_c[4];                               /* gamma */
} n3d_appear_desc;
int n3d_patch_appearance(void* x, int64_t ld, int B, int Cv, int P, const n3d_appear_desc* descs, void* scratch, size_t scratch_bytes,
                         void* stream);
size_t n3d_patch_appearance_scratch(int B, int Cv, int P);

/* ---- acquisition artefacts of a gathered batch, in place (none of it the reference's): simulated low resolution (nnU-Net v2's
 * SimulateLowResolutionTransform), a multiplicative bias field (TorchIO's RandomBiasField) and modality dropout (the BraTS
 * missing-modality recipes).  x, ld, B, Cv, P: as for n3d_patch_appearance -- DEVICE fp32 (B, Cv, P, P, P) in NDHWC storage with
 * channel pitch ld >= Cv, the lanes between Cv and ld never touched; B <= N3D_APPEAR_MAX_BATCH, Cv <= 4, 2 <= P <=
 * N3D_APPEAR_MAX_PATCH.  The descriptors are HOST arrays, one row per patch (plain arrays, not a record type: a caller fills only
 * the ones whose stage it uses; an array whose stage no patch asks for may be NULL):
 *   stages  int32 [B][3]   != 0: {low resolution, bias field, dropout} acts on this patch
 *   n       int32 [B][4]   low resolution: the extent the channel is sampled down to, 1 <= n[c] <= P; n[c] == P: untouched
 *   order   int32 [B][4]   bias field: the polynomial's order, 0 .. N3D_ARTEFACT_MAX_ORDER
 *   range   double [B][4]  bias field: the coefficients are uniform in [-range, range); finite, >= 0
 *   key     uint32 [B][2]  bias field: the patch's Philox key
 *   drop    int32 [B][4]   dropout: != 0: the channel is zeroed
 *
 * The brain mask of a (patch, channel) is x != 0 on entry (-0.0 is zero), taken ONCE before the first stage.  The stages run in the
 * fixed order low resolution, bias field, dropout, each only on the patches whose flag is set, each on the values the earlier
 * stages left.  Low resolution and the bias field write only masked voxels: the background stays exactly 0.0f.  All arithmetic is
 * fp64 on fp32 loads, every product, sum, quotient and library call rounded on its own in the association written; "fp32(..)" is
 * the one rounding to fp32 where a stage stores.  (i, j, k) is the voxel's index in its patch, k fastest.
 *
 *   low resolution  nearest-exact down-sampling of the channel's whole P^3 patch to n^3 followed by trilinear up-sampling back
 *             (align_corners = False), composed into eight taps of the patch itself.  Per axis, for the output index o:
 *               src = max(fma((double)n / (double)P, (double)o + 0.5, -0.5), 0.0);  i0 = min((int)src, n - 1);  i1 = i0 + (i0 < n - 1);
 *               l1 = src - (double)i0;  l0 = 1.0 - l1;  a0 = N(i0), a1 = N(i1) with the INTEGER N(i) = min(((2 i + 1) * P) / (2 n), P - 1)
 *             (N is what nearest-exact reads: floor((i + 0.5) * P / n), exactly.  The fma is the rule's ONE fused operation: the
 *             quotient is rounded, then quotient * (o + 0.5) - 0.5 is rounded once, which is how torch's fp64 interpolate
 *             evaluates its source coordinate.  Rounded in two steps the coordinate errs by up to an ulp of n, and the result
 *             drifts from torch's with the extent: 6.4e-15 at P = 21 and 2.6e-14 at P = 50 on values in +-3, against 4.4e-15 and
 *             1.8e-15 fused);
 *               y = fp32(sum over the taps (ti, tj, tk) = 000, 001, .. 111 (tk fastest), from +0.0, of
 *                        ((l_ti * l_tj) * l_tk) * x[a_ti, a_tj, a_tk])   (first the product, then acc = acc + product).
 *             Background zeros take part as taps.  The result does not depend on any read / write order: the launch writes to
 *             scratch and a second one lands the masked voxels in x.
 *   bias field  the terms t = 0, 1, .. are (pa, pb, pc) for pa in 0 .. order, pb in 0 .. order - pa, pc in 0 .. order - pa - pb, in
 *             that nesting (TorchIO's; 20 terms at order 3).  coef_t = (((double)w0 * 2^-32) * 2 - 1) * range[c], w0 the first word
 *             of Philox4x32-10 (the constants and rounds of n3d_appear_desc's noise stage) of the counter (t, 3, c, 0) under the
 *             patch's key.  (The second counter word keeps this stream apart from the appearance noise's 0, the elastic lattice's 1
 *             and the crop sampler's 2.)  X = (double)(2 i - P + 1) / (double)(P - 1), Y and Z the same of j and k (TorchIO's
 *             (arange(-P/2, P/2) + 0.5) / max); powers by repeated multiplication from 1.0: X^0 = 1, X^e = X^(e-1) * X;
 *               poly = sum in t order, from +0.0, of coef_t * ((X^pa * Y^pb) * Z^pc);   y = fp32(x * exp(poly)).
 *   dropout   drop[c] != 0: every voxel of the channel becomes 0.0f.
 *
 * How the parameters travel: repacked into the launch arguments of the stage's kernel; nothing is copied to the device and nothing
 * synchronises.  A stage with nothing to do launches nothing; with nothing to do at all (no flag set, or only n == P and drop == 0)
 * the call launches nothing and does not look at the scratch.  Launches otherwise: the mask 1, low resolution 2, bias field and
 * dropout together 1.  No atomics: two runs on the same input give the same bits.  Bad arguments (B, Cv or P out of range, n outside
 * 1 .. P, an order beyond N3D_ARTEFACT_MAX_ORDER, a range that is negative or not finite, a scratch that is too small) return
 * N3D_ERR_INVALID before any launch.  scratch: DEVICE, 16-byte aligned, n3d_patch_artefact_scratch(B, Cv, P) bytes (0 for
 * arguments out of range): a mask byte per voxel and the low-resolution stage's fp32 output, 16 bytes per voxel. */
#define N3D_ARTEFACT_MAX_ORDER 3
int n3d_patch_artefact(void* x, int64_t ld, int B, int Cv, int P, const int32_t* stages, const int32_t* n, const int32_t* order,
                       const double* range, const uint32_t* key, const int32_t* drop, void* scratch, size_t scratch_bytes, void* stream);
size_t n3d_patch_artefact_scratch(int B, int Cv, int P);

/* ---- the step before the data step (preprocess.py:77-144, create_h5:58-66): raw scanner counts to the statistics of the data
 * set and to each subject's normalised brain-wise box.  raw: DEVICE int16 (Cm, X, Y, Z) contiguous, 2-byte aligned (a modality's
 * base need not be 16-byte aligned: X * Y * Z may be odd); X * Y * Z < 2^31.  "Brain" = the voxels with raw != 0, per modality.
 * Nothing here synchronises.
 * n3d_brain_scan: ONE launch per subject.  totals: int64 [Cm][2] = {count, sum of values} of the brain voxels, ADDED to what is
 * there (zero it once, keep it across the subjects of a data set: exact integer totals).  rec: int32 [Cm][N3D_BRAIN_REC_WORDS] =
 * {min value, max value, min index x, y, z, max index x, y, z} over the brain voxels, combined with atomic min / max: the caller
 * fills it per subject with {INT32_MAX, INT32_MIN, INT32_MAX x 3, -1 x 3}, which is also what a modality without brain keeps. */
#define N3D_BRAIN_REC_WORDS 8
int n3d_brain_scan(const int16_t* raw, int Cm, int X, int Y, int Z, int64_t* totals, int32_t* rec, void* stream);
/* n3d_brain_sqdev: acc[c] += sum over modality c's brain voxels of (x - mean[c])^2 in fp64 (two roundings per term, no
 * contraction).  N = X * Y * Z.  mean, acc: DEVICE double [Cm]; ws: DEVICE double [Cm * n3d_brain_sqdev_rows(N)] partial rows,
 * reduced in a fixed order (no floating-point atomics): the same data at the same 16-byte phase gives the same bits, and
 * subjects enqueued on one stream accumulate in that order. */
int n3d_brain_sqdev_rows(int64_t N);
int n3d_brain_sqdev(const int16_t* raw, int Cm, int64_t N, const double* mean, double* ws, double* acc, void* stream);
/* n3d_brain_normalize: normalize (preprocess.py:87-93) fused with the crop to the box [lo, hi) (HOST int32[3] each, inside the
 * image): out is DEVICE fp32 (Cm, bx, by, bz), b = hi - lo.  A brain voxel becomes, each operation rounded once in fp64,
 *   z = (x - mean) / std;  q = (z - zmin) / (zmax - zmin);  v = (q + 0.1) * 100;  out = (float)(int16)v  (truncated toward zero:
 * the reference writes v back into its int16 array); other voxels 0.  mean_std: DEVICE double [Cm][2]; zmin / zmax are z of
 * rec's min / max value (rec as n3d_brain_scan left it for THIS subject, read on the device).  The caller rules out a modality
 * without brain or with min == max beforehand (the quotient is undefined there).  truth / truth_out: DEVICE uint8 (X, Y, Z) ->
 * (bx, by, bz) crop in the same launch, or both NULL. */
int n3d_brain_normalize(const int16_t* raw, int Cm, int X, int Y, int Z, const double* mean_std, const int32_t* rec, const int32_t* lo,
                        const int32_t* hi, float* out, const uint8_t* truth, uint8_t* truth_out, void* stream);
/* ---- a second normalisation, not the reference's: per subject and per modality, z-scoring over the brain voxels after clipping
 * the counts to two percentiles (lower < upper, in percent).  Needs no data-set statistics.  Four launches per subject:
 * n3d_brain_scan (above: the outline for the box, and rec's minimum), n3d_brain_hist, n3d_brain_robust, n3d_brain_zscore.
 * The rule.  Per modality, a[0..n-1] are its nonzero counts sorted ascending, n >= 2 (the caller refuses count < 2 and std == 0
 * from the record); every line is ONE correctly rounded fp64 operation (no contraction):
 *   1. for q in (lower, upper):  vi = (double)(n - 1) * (q / 100.0);  k = floor(vi);  t = vi - k;  A = a[k];
 *      B = a[min(k + 1, n - 1)];  d = B - A;  bound = A + d * t, or B - d * (1.0 - t) when t >= 0.5  (numpy's linear
 *      np.percentile in its own order of operations).  The two bounds are L and U.
 *   2. w(v) = min(max((double)v, L), U).  nL = voxels with v < L, nU = voxels with v > U, S_in = the exact integer sum of the
 *      others (|S_in| < 2^53: its conversion is exact).
 *   3. mean = ((nL * L + S_in) + nU * U) / n.
 *   4. sum of squared deviations, in this fixed order: the 65536 bins (bin b holds value v = b - 32768, h[b] voxels) are cut
 *      into 1024 runs of 64 consecutive bins; run i starts from 0.0 and adds h * ((v - mean) * (v - mean)) for its bins with
 *      L <= v <= U and h > 0 in ascending v; the 1024 run sums are then added in adjacent pairs, p[i] = p[2i] + p[2i + 1], ten
 *      rounds down to one value I;  sum = (nL * ((L - mean) * (L - mean)) + I) + nU * ((U - mean) * (U - mean));
 *      std = sqrt(sum / n).  No floating-point atomics: two runs give the same bits.
 *   5. a nonzero voxel stores r = (float)((w(v) - mean) / std), and FLT_MIN (0x00800000) where r == 0.0f; a zero voxel 0.0f:
 *      the output is nonzero exactly where raw is.
 * n3d_brain_hist: hist, DEVICE int32 [Cm][N3D_BRAIN_HIST_BINS], 16-byte aligned, is zeroed on the stream and then holds the exact
 * histogram of each modality's nonzero voxels, value v in bin v + 32768.  rec: as n3d_brain_scan left it for THIS subject (read
 * on the device): counts in [min, min + n3d_brain_hist_window()) are accumulated in LDS per workgroup, the others with global
 * integer atomics -- rec decides the speed, never the result.
 * n3d_brain_robust: one record per modality from hist, out: DEVICE [Cm][N3D_BRAIN_ROBUST_WORDS] 8-byte words:
 *   int64   0 count n;  1..4 a[kL], a[min(kL + 1, n - 1)], a[kU], a[min(kU + 1, n - 1)];  5 nL;  6 nU;  7 S_in
 *   double  8 L;  9 U;  10 mean;  11 std;  12 the sum of squared deviations
 *   13..15 reserved (zero).  count == 0 leaves every other word zero.
 * n3d_brain_zscore: n3d_brain_normalize's box, output and label crop, with rule 2 and 5 from the DEVICE record `robust`. */
#define N3D_BRAIN_HIST_BINS 65536
#define N3D_BRAIN_ROBUST_WORDS 16
int n3d_brain_hist_window(void);
int n3d_brain_hist(const int16_t* raw, int Cm, int X, int Y, int Z, const int32_t* rec, int32_t* hist, void* stream);
int n3d_brain_robust(const int32_t* hist, int Cm, double lower, double upper, int64_t* out, void* stream);
int n3d_brain_zscore(const int16_t* raw, int Cm, int X, int Y, int Z, const int64_t* robust, const int32_t* lo, const int32_t* hi,
                     float* out, const uint8_t* truth, uint8_t* truth_out, void* stream);

/* ---- step after the hot path (prediction.py:120-170): stitch the per-patch predictions into the brain-wide volume with
 * mean blending (patches.py:172-207) and fuse the three sigmoid channels into one label volume.
 * n3d_stitch: patches element (b, c, voxel v = (lx*P+ly)*P+lz) at patches[b*sb + c*sc + v*sv] (any of the layouts the
 * net produces); corners: DEVICE int32 [B][3] on the brain-wide grid (may be negative / hang over the border);
 * out: float64 (C, FX, FY, FZ) full image, the (X,Y,Z) brain-wide box is written at offset (ox,oy,oz); voxels of the box
 * no patch covers become 0.  Sums run in list order in fp64 like the reference's.  1 <= C <= 4.
 * n3d_tumor_labels: pred float64 (3, N) -> uint8 labels {0,1,2,4} (inclusive: TC/WT/ET channels; else NCR-NET/ED/ET). */
int n3d_stitch(const float* patches, int64_t sb, int64_t sc, int64_t sv, int C, int P, const int32_t* corners, int B, int X, int Y, int Z,
               double* out, int FX, int FY, int FZ, int ox, int oy, int oz, void* stream);
int n3d_tumor_labels(const double* pred, int64_t N, double threshold, int inclusive, uint8_t* out, void* stream);

/* ---- the same stitch for a whole subject, chunk by chunk (prediction.py:64-170): no patch prediction outlives its chunk.
 * Running buffers of the brain-wide box, zeroed by the caller per subject: sum float64 (C, X, Y, Z), cnt int32 (X, Y, Z).
 * n3d_stitch_add adds one chunk: patches as n3d_stitch (nslots patches; NULL with nslots == 0); entries: DEVICE table of n records
 * in list order.  A record is the descriptor its patch was GATHERED with (n3d_patch_desc: q[i] = x[s(i)]) and the patch's index in
 * the tensor: the prediction of q is brought back onto x's grid here (the kernel solves s(i) = l for i; the host does not
 * invert).  slot < 0 (or >= nslots): a patch the net never ran (all-zero input): it counts as covering and adds zeros, the reference's
 * rule (prediction.py:133-135).  lo / hi: HOST int32[3] each, the bounding box [lo, hi) of the chunk's patches on the brain-wide
 * grid (may hang over; clipped here): the launch covers that box only, so the cost follows the chunk; a record outside it is
 * not added.  Every voxel adds its covering records one by one in table order in fp64, no atomics: chunk after chunk this is bit
 * for bit the list-order sum of n3d_stitch.  1 <= C <= 4.
 * n3d_stitch_finish: ONE pass over the full image (FX, FY, FZ) with the box at (ox, oy, oz).  mean = sum / max(cnt, 1).  probs
 * (float64 (C, FX, FY, FZ)) and labels (uint8 (FX, FY, FZ); C == 3) may each be NULL (not both): probs takes the mean, labels
 * the fusion of n3d_tumor_labels on that mean; with mask_vol -- the subject's (Cv, X, Y, Z) fp32 box -- the label is 0 where
 * every channel is zero ("zero" as n3d_volume_sat: prediction.py:83-96, tumor_pred *= skull_mask).  Outside the box both are 0:
 * every voxel of an output is written exactly once, so the outputs need no clearing. */
typedef struct n3d_stitch_entry { n3d_patch_desc d; int32_t slot; } n3d_stitch_entry;
int n3d_stitch_add(const float* patches, int64_t sb, int64_t sc, int64_t sv, int C, int P, int nslots, const n3d_stitch_entry* entries, int n,
                   const int32_t* lo, const int32_t* hi, int X, int Y, int Z, double* sum, int32_t* cnt, void* stream);
int n3d_stitch_finish(const double* sum, const int32_t* cnt, int C, int X, int Y, int Z, double* probs, uint8_t* labels, double threshold,
                      int inclusive, const float* mask_vol, int Cv, int FX, int FY, int FZ, int ox, int oy, int oz, void* stream);

/* ---- the same subject-level stitch with an importance weight per covering patch (sliding-window inference with Gaussian
 * blending) and a running fp64 weight sum in place of the count: wsum float64 (X, Y, Z), zeroed by the caller with sum.
 * n3d_stitch_add_w: everything as n3d_stitch_add (records, the isometry solved in the kernel, the bounding-box launch, one thread
 * per voxel, no atomics, the records of the range in table order) but the weight.  profile: DEVICE double[P], P <= 1024 (staged in
 * LDS once per workgroup), positive and symmetric (profile[i] == profile[P-1-i]: the caller's to check).  For a covering record
 * with patch corner c at the voxel (x, y, z), l = (x, y, z) - c on the VOLUME's grid (not the net's own index: with a symmetric
 * profile the two differ in the order of the factors only, and the order is fixed here), operation by operation in fp64, each
 * `*` and `+` rounded once (no fused multiply-add):
 *   w = (profile[l0] * profile[l1]) * profile[l2];   sum[ch] = sum[ch] + w * (double)p[ch];   wsum = wsum + w
 * A dead record (slot < 0 or >= nslots) adds w to wsum only.  A voxel no record of the range covers is not stored to.  With a
 * profile of ones sum is bit for bit n3d_stitch_add's and wsum its count.
 * n3d_stitch_finish_w: n3d_stitch_finish with mean = wsum > 0 ? sum / wsum : 0 in place of sum / max(cnt, 1); box placement,
 * probs / labels, skull mask and "every output voxel written exactly once" as there. */
int n3d_stitch_add_w(const float* patches, int64_t sb, int64_t sc, int64_t sv, int C, int P, int nslots, const n3d_stitch_entry* entries, int n,
                     const double* profile, const int32_t* lo, const int32_t* hi, int X, int Y, int Z, double* sum, double* wsum, void* stream);
int n3d_stitch_finish_w(const double* sum, const double* wsum, int C, int X, int Y, int Z, double* probs, uint8_t* labels, double threshold,
                        int inclusive, const float* mask_vol, int Cv, int FX, int FY, int FZ, int ox, int oy, int oz, void* stream);

/* ---- whole-image prediction (prediction.py:102-119, `fs_pred`): one forward on the full image zero-padded at the high end; no
 * patches, no stitch.  full / padded / flip / origin: HOST int32[3] each.  The image (FX, FY, FZ) sits at the low corner of the
 * padded grid (PX, PY, PZ), P >= F per axis; FX * FY * FZ < 2^31 (and PX * PY * PZ < 2^31 for the embed).  flip[a] != 0 mirrors
 * the image within [0, F_a) -- the pad stays at the high end -- i.e. np.pad(permute_data(image, key)) for a flip-only key.
 * n3d_image_embed: box = the subject's (Cv, bx, by, bz) contiguous fp32 box at `origin` inside the image; x_out = the net's input,
 * pitched NDHWC (1, Cv, PX, PY, PZ), xld >= Cv.  Every voxel is written exactly once (the box, zeros around it and in the pad), so
 * the caller clears nothing; the pitch gap is not touched (as n3d_patch_batch).
 * n3d_image_add / n3d_image_finish: y = the net's fp32 prediction of the image embedded under `flip`, element (c, padded voxel v)
 * at y[c*sc + v*sv] (any layout the net produces, as n3d_stitch); it is un-flipped and cropped to the image here.  sum: the fp64
 * running sum (C, FX, FY, FZ) of an ensemble's earlier keys.  n3d_image_add (every key but the last): sum = y if `first`, else
 * sum + y -- the first key writes, so sum needs no clearing.  n3d_image_finish (the last key): ONE pass over the image,
 * mean = (sum + (double)y) / K in key order; sum NULL exactly when K == 1, and then mean is exactly (double)y.  probs (float64
 * (C, FX, FY, FZ)) and labels (uint8 (FX, FY, FZ); C == 3) may each be NULL (not both); labels = the fusion of n3d_tumor_labels on
 * the mean; with mask_box -- the subject's box again -- the label is 0 where every channel of the box is zero ("zero" as
 * n3d_volume_sat: prediction.py:83-96) and everywhere outside the box.  Every voxel of an output is written exactly once.  One
 * thread owns a voxel, fixed order, no atomics: the same inputs give the same bits.  1 <= C <= 4. */
int n3d_image_embed(const float* box, int Cv, int bx, int by, int bz, const int32_t* origin, const int32_t* full, const int32_t* padded,
                    const int32_t* flip, float* x_out, int64_t xld, void* stream);
int n3d_image_add(const float* y, int64_t sc, int64_t sv, int C, const int32_t* full, const int32_t* padded, const int32_t* flip, double* sum,
                  int first, void* stream);
int n3d_image_finish(const float* y, int64_t sc, int64_t sv, int C, const int32_t* full, const int32_t* padded, const int32_t* flip,
                     const double* sum, int K, double* probs, uint8_t* labels, double threshold, int inclusive, const float* mask_box, int Cv,
                     int bx, int by, int bz, const int32_t* origin, void* stream);

/* ---- Segmentation metrics: a predicted label volume scored against the truth per region -- the four columns plot.py:151-173
 * draws (Dice, Sensitivity, Specificity, Hausdorff95 of ET / WT / TC).  The reference has no code for them; the definitions are
 * the BraTS portal's and medpy.metric.binary.hd95's, at unit voxel spacing.
 *   labels: uint8 {0, 1, 2, 4}.  Regions, in tr.eval_result()'s order: 0 WT = label != 0, 1 TC = label in {1, 4}, 2 ET = label == 4.
 *   pred: DEVICE uint8 (FX, FY, FZ), the full image.  truth: DEVICE uint8 (BX, BY, BZ), the box at `origin` inside the image; the
 *     truth is zero outside its box.  full / box / origin: HOST int32[3] each.  FX * FY * FZ < 2^31.
 *   counts: TP, FP, FN per region over the full image (TN = FX * FY * FZ - TP - FP - FN is the host's).
 *   surface of a mask: a mask voxel with a 6-neighbour that is unset or outside the image
 *     (mask & ~binary_erosion(mask, generate_binary_structure(3, 1), border_value=0)).
 *   d2_B(v): squared Euclidean distance from voxel v to the nearest voxel of surface B: an integer.  Per region the multiset D =
 *     {d2_T(v): v on the prediction's surface} + {d2_P(v): v on the truth's surface}; HD95 is numpy's linear-interpolation
 *     percentile 95 of sqrt(D).  From the device come only n = |D|, the order statistics D[k] and D[min(k + 1, n - 1)] of the
 *     sorted D with k = floor((n - 1) * 0.95) (one fp64 product, as numpy forms it) and max D; the host interpolates.  D is
 *     empty (n = 0) when either mask of the region is.
 * Everything is integer work with integer atomics (add / min / max commute exactly): the same inputs give the same bits.
 *
 * rec: DEVICE int64[N3D_SEG_REC_WORDS], 8-byte aligned; the subject's one device -> host copy.  Words 0..8: counts[region][TP, FP,
 * FN]; 9..20: order[region][n, D[k], D[k + 1], max D]; 21..29 hold int32 bbox[region][lo x, y, z, hi x, y, z], the bounding box
 * (inclusive) of the union of both surfaces of the region.  Before n3d_seg_regions the caller fills counts and order with 0 and
 * every bbox with {INT32_MAX x 3, -1 x 3}, which is also what a region without surface keeps.
 * flags: DEVICE uint8 (FX, FY, FZ): bits 0..2 the prediction's surface of WT / TC / ET, bits 3..5 the truth's.
 * dist: DEVICE int32 [njobs][FX * FY * FZ]; hist: DEVICE uint32 [3][hist_len], zeroed by the caller per subject.
 * n3d_seg_workspace_bytes: bytes of one allocation holding rec, flags, dist (6 jobs) and hist for an image shape, 0 on a bad shape;
 * offsets (HOST int64[5], may be NULL) receives the byte offsets of rec, flags, dist, hist and hist_len itself. */
#define N3D_SEG_REGIONS 3
#define N3D_SEG_REC_WORDS 30
#define N3D_SEG_REC_ORDER 9      /* first word of order[][] */
#define N3D_SEG_REC_BBOX 21      /* first word of bbox[][] (int32 view: word * 2) */
#define N3D_SEG_INF (1 << 29)    /* "no source": INF + 1023^2 stays below 2^31 */
#define N3D_SEG_MAX_AXIS 1024
size_t n3d_seg_workspace_bytes(int FX, int FY, int FZ, int64_t* offsets);
/* ONE launch: every voxel's labels are read once (the six neighbours again, through the cache); writes flags, adds the counts
 * (per wave, then one atomic per workgroup and nonzero counter) and combines the bounding boxes (atomic min / max). */
int n3d_seg_regions(const uint8_t* pred, const uint8_t* truth, const int32_t* full, const int32_t* box, const int32_t* origin,
                    uint8_t* flags, int64_t* rec, void* stream);
/* Exact squared distance transform, separable: out[i] = min_j (f[j] + (i - j)^2) along z, then y, then x (three launches), brute
 * force over the line held in LDS.  Job j (0 <= j < njobs <= 6) takes bit j of flags as its sources (f = 0 there, N3D_SEG_INF
 * elsewhere) and writes dist[j]; it works inside bbox[j % nreg] only (bbox: DEVICE int32 [nreg][6] as in rec, read on the device
 * and clipped to the image; the workgroups walk the box's tiles; an empty box does nothing) -- voxels of dist[j] outside the box are left
 * untouched.  A box without a source voxel gives N3D_SEG_INF throughout.  Each pass after the first works in place (a workgroup
 * owns whole lines and holds them in LDS before it writes).  An axis longer than N3D_SEG_MAX_AXIS: N3D_ERR_UNSUPPORTED. */
int n3d_seg_edt(const uint8_t* flags, int njobs, int nreg, const int32_t* full, const int32_t* bbox, int32_t* dist, void* stream);
/* ONE launch: every prediction-surface voxel of region r adds 1 to hist[r][dist[3 + r][v]], every truth-surface voxel to
 * hist[r][dist[r][v]] (dist as n3d_seg_edt with njobs = 6, nreg = 3 wrote it from the same flags and bbox); only the box around
 * bbox's three boxes is walked (every surface voxel lies in it).  A distance >= hist_len (N3D_SEG_INF: the other surface is empty)
 * is not counted. */
int n3d_seg_sample(const uint8_t* flags, const int32_t* full, const int32_t* bbox, const int32_t* dist, uint32_t* hist, int64_t hist_len,
                   void* stream);
/* ONE launch of three workgroups: scans hist[r] up to the squared diagonal of bbox[r] and writes order[r] into rec. */
int n3d_seg_order(const uint32_t* hist, int64_t hist_len, int64_t* rec, void* stream);

/* ---- Label clean-up: the step between prediction and scoring -- connected components of a predicted label volume's foreground and
 * the two rules BraTS submissions apply to them.  The reference has no code for it; the definitions are scipy.ndimage.label's.
 *   labels / mask: DEVICE uint8 (FX, FY, FZ); any nonzero byte is foreground.  full: HOST int32[3].  FX * FY * FZ < 2^31.
 *   connectivity: 6, 18 or 26 -- scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3).  Neighbours are neighbours by coordinate:
 *     (x, y, FZ - 1) and (x, y + 1, 0) are not.
 *   id of a component: the smallest linear index (x * FY + y) * FZ + z of its voxels -- whatever order the work runs in; scipy's
 *     labels map onto it by "minimum linear index per label".  comp: DEVICE int32 (FX, FY, FZ), the id per voxel, -1 on background.
 *   Step A: a component is kept iff size >= min_voxels and (not keep_largest or it is the largest; equal sizes: the smallest id);
 *     voxels of the others become 0.  If the largest is smaller than min_voxels nothing is kept.
 *   Step B: e = label-4 voxels in kept components; if 0 < e < et_min_voxels they become 1 (e == et_min_voxels changes nothing).
 *   With every rule off (0, 0, 0) out equals labels and the record is still filled.
 * Union-find on the int32 parent array (parent[v] <= v, -1 on background): a workgroup labels an 8 x 8 x 32 tile in LDS, the
 * voxels on tile faces unite across tiles with atomicMin, a flatten pass writes comp from parent and counts the sizes.  Integer
 * atomics only (min, add, max): the same inputs give the same bits.  No kernel waits on another workgroup.
 *
 * rec: DEVICE int64[N3D_CC_REC_WORDS], 8-byte aligned, in the workspace at the offset the query reports; n3d_cc_clean clears and
 * fills it.  Words: 0 components, 1 components kept, 2 foreground voxels, 3 voxels kept, 4 size of the largest component, 5 its id
 * (-1 without a component), 6 label-4 voxels, 7 label-4 voxels in kept components, 8 whether step B relabelled them (0 / 1),
 * 9 scratch: max over components of (size << 32) | (0xFFFFFFFF - id).
 * n3d_cc_workspace_bytes: bytes of one allocation holding parent, comp, the per-root sizes and label-4 counts (int32 per voxel
 * each), the per-root verdicts (a byte per voxel) and rec -- 17 bytes per voxel; 0 on a bad shape.  offsets (HOST int64[6], may be
 * NULL) receives the byte offsets of those six, in that order. */
#define N3D_CC_REC_WORDS 10
#define N3D_CC_REC_COMPONENTS 0
#define N3D_CC_REC_KEPT 1
#define N3D_CC_REC_VOXELS_IN 2
#define N3D_CC_REC_VOXELS_KEPT 3
#define N3D_CC_REC_LARGEST_SIZE 4
#define N3D_CC_REC_LARGEST_ID 5
#define N3D_CC_REC_ET_IN 6
#define N3D_CC_REC_ET_KEPT 7
#define N3D_CC_REC_ET_RELABELLED 8
#define N3D_CC_REC_PACKED 9
size_t n3d_cc_workspace_bytes(int FX, int FY, int FZ, int64_t* offsets);
/* THREE launches (local, merge, flatten): comp = the component ids of mask; parent (DEVICE int32 (FX, FY, FZ), 4-byte aligned, not
 * comp) is scratch.  A connectivity other than 6 / 18 / 26, a NULL pointer or a bad shape: N3D_ERR_INVALID. */
int n3d_cc_label(const uint8_t* mask, const int32_t* full, int connectivity, int32_t* parent, int32_t* comp, void* stream);
/* SIX launches (local, merge, flatten with the size counts, two decide launches -- the verdicts need the maximum, the surviving
 * label-4 count needs the verdicts --, apply): out (DEVICE uint8 (FX, FY, FZ), not labels) = labels cleaned by steps A and B.
 * workspace: n3d_cc_workspace_bytes(FX, FY, FZ) bytes, 8-byte aligned; nothing in it has to be cleared.  Errors as n3d_cc_label;
 * negative thresholds: N3D_ERR_INVALID. */
int n3d_cc_clean(const uint8_t* labels, const int32_t* full, int connectivity, int64_t min_voxels, int keep_largest, int64_t et_min_voxels,
                 void* workspace, uint8_t* out, void* stream);
/* The launches first .. last (0 local, 1 merge, 2 flatten, 3 decide: maximum, 4 decide: verdicts, 5 apply) of n3d_cc_clean, for
 * measuring them one by one: a launch expects the workspace as the launches before it leave it, and 0 .. k repeats (launch 0
 * clears what the later ones add to).  n3d_cc_clean is variant N3D_CC_TILED, launches 0 .. 5.  N3D_CC_GLOBAL_ONLY is the design
 * without the LDS tile phase -- launch 0 only makes every foreground voxel its own root, launch 1 unites every voxel with all its
 * forward neighbours in memory -- kept so that the two can be timed against each other; same results. */
#define N3D_CC_PHASES 6
#define N3D_CC_TILED 0
#define N3D_CC_GLOBAL_ONLY 1
int n3d_cc_phases(int variant, int first, int last, const uint8_t* labels, const int32_t* full, int connectivity, int64_t min_voxels,
                  int keep_largest, int64_t et_min_voxels, void* workspace, uint8_t* out, void* stream);

/* ---- Lesion-wise metrics: the BraTS 2023 scoring -- lesion-wise Dice and Hausdorff95 per region -- of a predicted label volume.
 * The reference has no code for it; the definitions are pinned to scipy.ndimage (tests/golden/make_golden_lesion.py).
 *   pred / truth / full / box / origin, labels and regions (0 WT, 1 TC, 2 ET): as in "Segmentation metrics".  Axes up to
 *     N3D_LW_MAX_AXIS (surface coordinates are packed 10 bits per axis), FX * FY * FZ < 2^31.
 * Per region, operation by operation:
 *   Masks.  G: the truth's region mask in full-image coordinates, zero outside the box; P: the prediction's.
 *   Dilation.  Gd = scipy.ndimage.binary_dilation(G, generate_binary_structure(3, 2), iterations=dilation), border value 0:
 *     `dilation` times "a voxel of the image is set when it or one of its 18 neighbours (|dx| + |dy| + |dz| <= 2, no corner) was";
 *     nothing outside the image is ever set.  0 <= dilation <= N3D_LW_MAX_DILATION; 0: Gd = G.
 *   Lesions.  The 26-connected components of Gd.  Lesion l owns the G voxels in its component; its id is the component's id as
 *     n3d_cc_label defines it, the smallest linear index of the DILATED component.  Lesions are listed by ascending id; a lesion's
 *     position in that list is its rank.
 *   Predicted components.  The 26-connected components of P.
 *   Matching.  Component c matches lesion l iff some voxel has P-component c and Gd-component l; a component may match several
 *     lesions and counts for each, and may match through the dilation rim alone.
 *   Per lesion l.  gt_voxels = |G_l|; tp = |P & G_l|; pred_voxels = the summed sizes of the matched components; n_matched = their
 *     number.  Distances: the surface (6-neighbourhood, as in "Segmentation metrics") of P restricted to the matched components
 *     against the surface of G restricted to the lesion: D = {d2 from every voxel of one to the nearest voxel of the other}, both
 *     directions concatenated, exact integers; n = |D|, D[k], D[min(k + 1, n - 1)] of the sorted D with k = floor((n - 1) * 0.95)
 *     (one fp64 product) and max D.  n_matched == 0: n = 0 and the three distances 0.
 *   False positives.  n_fp = the predicted components that match no lesion, fp_voxels = their voxels.
 * The host folds these into the two numbers (nas_3d_unet_amd.metrics.finish_lesions).
 *
 * rec: DEVICE int64[N3D_LW_REC_WORDS], 8-byte aligned; the subject's one device -> host copy; n3d_lw_score clears and fills it.
 * Per region N3D_LW_REGION_WORDS words: a header of N3D_LW_HEADER_WORDS (n_lesions, n_pred_components, n_fp, fp_voxels, overflow
 * bits, 0, 0, 0), then N3D_LW_MAX_LESIONS rows of N3D_LW_ROW_WORDS (id, gt_voxels, tp, pred_voxels, n_matched, n, D[k], D[k + 1],
 * max D), rows past n_lesions zero.
 * Caps.  N3D_LW_MAX_LESIONS lesions per region; N3D_LW_MAX_SURFACE entries per region and side of the surface lists (a truth
 * surface voxel is one entry; a prediction surface voxel is one entry per lesion its component matches, none for a false positive).
 * Exceeding a cap sets its overflow bit and the call returns normally: N3D_LW_OVERFLOW_LESIONS leaves n_lesions (the true number)
 * and no other word of the region; a surface bit leaves the counts and no distance (n = 0 in every row).
 * Integer atomics only (add / min / max / or): the same inputs give the same bits.  The launch count is fixed (47) whatever the
 * data; no kernel waits on another workgroup.
 *
 * n3d_lw_workspace_bytes: bytes of one allocation (28 per voxel + 6 MiB of lists) for an image shape, 0 on a bad shape; offsets
 * (HOST int64[N3D_LW_WS_PARTS], may be NULL) receives the byte offsets of: region bits, surface bits, the dilated mask, the
 * prediction's region mask (a byte per voxel each), parent, the prediction's component ids, the dilated truth's component ids,
 * component sizes (int32 per voxel each), component match masks (uint64 per voxel), the surface lists, the control block.
 * Nothing in the workspace has to be cleared. */
#define N3D_LW_MAX_DILATION 5
#define N3D_LW_MAX_LESIONS 64
#define N3D_LW_MAX_SURFACE (1 << 18)
#define N3D_LW_MAX_AXIS 1024
#define N3D_LW_HEADER_WORDS 8
#define N3D_LW_ROW_WORDS 9
#define N3D_LW_REGION_WORDS (N3D_LW_HEADER_WORDS + N3D_LW_MAX_LESIONS * N3D_LW_ROW_WORDS)   /* 584 */
#define N3D_LW_REC_WORDS (3 * N3D_LW_REGION_WORDS)                                          /* 1752 */
#define N3D_LW_HDR_LESIONS 0
#define N3D_LW_HDR_COMPONENTS 1
#define N3D_LW_HDR_FP 2
#define N3D_LW_HDR_FP_VOXELS 3
#define N3D_LW_HDR_OVERFLOW 4
#define N3D_LW_ROW_ID 0
#define N3D_LW_ROW_GT 1
#define N3D_LW_ROW_TP 2
#define N3D_LW_ROW_PRED 3
#define N3D_LW_ROW_MATCHED 4
#define N3D_LW_ROW_N 5
#define N3D_LW_ROW_DK 6
#define N3D_LW_ROW_DK1 7
#define N3D_LW_ROW_DMAX 8
#define N3D_LW_OVERFLOW_LESIONS 1
#define N3D_LW_OVERFLOW_TRUTH_SURFACE 2
#define N3D_LW_OVERFLOW_PRED_SURFACE 4
#define N3D_LW_WS_PARTS 11
size_t n3d_lw_workspace_bytes(int FX, int FY, int FZ, int64_t* offsets);
/* ONE launch: out (DEVICE uint8 (FX, FY, FZ), not mask) = 1 where the dilation of `mask != 0` (any nonzero byte) is set, 0
 * elsewhere.  bbox: DEVICE int32[6] (lo x, y, z, hi x, y, z inclusive) holding every nonzero voxel of mask, or NULL: only the
 * 8 x 8 x 32 tiles that meet the box grown by `iterations` are dilated (in LDS, with a halo of `iterations`), the others are
 * written as zeros; a mask voxel outside bbox is ignored there.  iterations outside 0 .. N3D_LW_MAX_DILATION: N3D_ERR_INVALID. */
int n3d_lw_dilate(const uint8_t* mask, const int32_t* full, const int32_t* bbox, int iterations, uint8_t* out, void* stream);
/* 47 launches: init, the region and surface bits with the truth's boxes, then per region: the prediction's mask, its components
 * (n3d_cc_label), the dilation, its components (n3d_cc_label), roots, ranks, matching and per-lesion counts, component sums,
 * surface lists, distances (brute force over the lists in LDS tiles, filtered by lesion), order statistics (bisection on the
 * value).  workspace: n3d_lw_workspace_bytes(FX, FY, FZ) bytes, 8-byte aligned. */
int n3d_lw_score(const uint8_t* pred, const uint8_t* truth, const int32_t* full, const int32_t* box, const int32_t* origin, int dilation,
                 void* workspace, int64_t* rec, void* stream);
/* The phases first .. last of n3d_lw_score, for measuring them one by one: 0 init, 1 region bits, then per region r the
 * N3D_LW_REGION_PHASES phases 2 + 11 r + (0 select, 1 label P, 2 dilate, 3 label Gd, 4 roots, 5 ranks, 6 match, 7 components,
 * 8 surface lists, 9 distances, 10 order statistics).  A phase expects the workspace as the phases before it leave it; 0 .. k
 * repeats. */
#define N3D_LW_REGION_PHASES 11
#define N3D_LW_PHASES (2 + 3 * N3D_LW_REGION_PHASES)
int n3d_lw_phases(int first, int last, const uint8_t* pred, const uint8_t* truth, const int32_t* full, const int32_t* box,
                  const int32_t* origin, int dilation, void* workspace, int64_t* rec, void* stream);

/* ---- RCCL exchange step of data-parallel training (no reference counterpart: config.yml:54 `multi_gpus` is never read;
 * SURVEY 8(e)).  One process per GPU; the hot path's only exchange is a SUM all-reduce of the flat fp32 gradient buffer, in
 * place, stream-ordered on `stream` (a side HIP stream lets it run under the backward kernels of the next bucket).
 * RCCL is bound with dlopen at first use (the copy already in the process -- torch's -- wins).
 * n3d_comm_unique_id: rank 0 fills 128 bytes (ncclUniqueId) that the host distributes out of band;
 * n3d_comm_init: ncclCommInitRank on the CURRENT HIP device (collective: every rank calls it). */
#define N3D_COMM_ID_BYTES 128
int n3d_comm_available(void);
int n3d_comm_unique_id(void* id_out /* N3D_COMM_ID_BYTES */);
int n3d_comm_init(const void* id, int world, int rank, void** comm_out);
int n3d_comm_allreduce_sum(void* comm, float* buf, int64_t n, void* stream);
int n3d_comm_allreduce_sum_f64(void* comm, double* buf, int64_t n, void* stream);   /* the same in fp64 (the evaluation accumulator) */
/* in-place broadcast of n floats from rank `root` (the one-off weight broadcast when a trainer is built), stream-ordered */
int n3d_comm_broadcast(void* comm, float* buf, int64_t n, int root, void* stream);
int n3d_comm_destroy(void* comm);

/* ---- flat Adam (train.py:49,128; search.py:103-104,228,238): torch.optim.Adam defaults ------------
 * step_ptr: device int32 holding the number of steps already taken; inc_step == 1: a second tiny launch
 * increments it after the update (graph-replay safe); inc_step == 2: step_ptr points to int32[2] =
 * {steps, ticket counter (zero between launches)} and the last workgroup of the update launch itself counts
 * the step (no second launch).  grad_scale multiplies g (DP mean). */
int n3d_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                  const float* lr_ptr /* if not NULL the learning rate is read from this device float instead of
                  `lr`: a captured graph then follows the ReduceLROnPlateau schedule (train.py:50,77) */,
                  float beta1, float beta2, float eps, float weight_decay, float grad_scale, int32_t* step_ptr,
                  int inc_step, void* stream);

/* Guarded update (round 4): the stream hand-offs below are BOUNDED waits -- one that gives up lets its stream go on with operands
 * that are not there yet.  Such a step must never reach the weights (train.py:121-128: a step is forward, backward, update --
 * there is no "update from garbage" in the reference).  n3d_adam_step_guarded is n3d_adam_step with a test in front, uniform
 * over the grid: if *timeouts != *acked (uint32: time-outs counted by n3d_sync_wait vs. time-outs the host has acknowledged;
 * both NULL = no test) or *peer_flag != 0 (data parallel: the flags of all ranks, SUM-all-reduced together with the
 * gradients; NULL = no test) the launch updates NOTHING -- parameters, moments and the step counter stay as they are -- writes
 * NaN to *loss (if not NULL) and 1 to *host_word (if not NULL; a word from n3d_host_word_alloc, which the host polls without a
 * HIP call).  inc_step must be 0 or 2 when a test is requested.  n3d_guard_flag writes the local test (1.0 / 0.0) to *flag for
 * the all-reduce. */
int n3d_adam_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                          const float* lr_ptr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                          int32_t* step_ptr, int inc_step, const void* timeouts, const void* acked, const float* peer_flag,
                          float* loss, void* host_word, void* stream);
int n3d_guard_flag(const void* timeouts, const void* acked, float* flag, void* stream);
/* n3d_adam_step_guarded with a clip coefficient: *coef (a device float, e.g. out + 1 of n3d_grad_clip_coef; NULL = 1) multiplies
 * grad_scale, read once per launch.  With coef == NULL this IS n3d_adam_step_guarded (the two entry points above pass NULL). */
int n3d_adam_step_coef(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, const float* lr_ptr,
                       float beta1, float beta2, float eps, float weight_decay, float grad_scale, const float* coef, int32_t* step_ptr,
                       int inc_step, const void* timeouts, const void* acked, const float* peer_flag, float* loss, void* host_word,
                       void* stream);

/* ---- flat AdaBound / AdaBoundW (adabound.py:50-118 / 164-234; imported by train.py:10, search.py:14) ----------------
 * The same flat buffers, step counter (inc_step 0 / 1 / 2), device learning rate, guard and clip coefficient as the Adam entry
 * points; max_exp_avg_sq is the AMSBound buffer (NULL = amsbound off).  Per element, in fp32 and in the reference's order:
 *   g' = coef * grad_scale * g;  coupled (decoupled == 0) and weight_decay != 0: g' += wd * p
 *   m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  vh = amsbound ? (vmax = max(vmax, v)) : v
 *   r = clamp(step_size / (sqrt(vh) + eps), lo, hi);  p -= r m;  decoupled and weight_decay != 0: p -= wd * p_old (NOT times lr)
 * Once per launch, in double from the device step t and the device rate lr, each rounded to fp32 once:
 *   step_size = lr sqrt(1 - b2^t) / (1 - b1^t);  final = final_lr * lr / base_lr
 *   lo = final (1 - 1 / (gamma t + 1));  hi = final (1 + 1 / (gamma t))
 * base_lr: the fp32 rate the trainer started with (adabound.py:43), so lr / base_lr is exact while a plateau schedule halves it.
 * Unlike Adam's there is no 1/sqrt(1 - b2^t) on sqrt(v).  betas, eps, weight_decay, final_lr and gamma are doubles -- the
 * reference's Python floats -- and 1 - beta is taken in double before the one rounding, as torch does for an fp32 tensor.
 * Traffic per element: 16 B in + 12 B out (20 + 16 with amsbound). */
int n3d_adabound_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, int64_t n, float lr,
                      const float* lr_ptr, float base_lr, double beta1, double beta2, double eps, double weight_decay,
                      double final_lr, double gamma, int decoupled, float grad_scale, const float* coef, int32_t* step_ptr,
                      int inc_step, void* stream);
int n3d_adabound_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, int64_t n,
                              float lr, const float* lr_ptr, float base_lr, double beta1, double beta2, double eps,
                              double weight_decay, double final_lr, double gamma, int decoupled, float grad_scale,
                              const float* coef, int32_t* step_ptr, int inc_step, const void* timeouts, const void* acked,
                              const float* peer_flag, float* loss, void* host_word, void* stream);

/* ---- flat SGD (torch.optim.SGD, maximize=False) and AdamW (torch.optim.AdamW, amsgrad=False) -------------------------
 * The same flat buffers, step counter (inc_step 0 / 1 / 2), device learning rate, guard and clip coefficient as the Adam entry
 * points.  momentum, dampening, weight_decay, betas and eps are doubles -- torch's Python floats --, each rounded to fp32 once;
 * 1 - dampening and 1 - beta are taken in double before that rounding.  No floating-point atomics.
 * n3d_sgd_step, per element in fp32, with t = *step_ptr + 1 and lr the device rate:
 *   1. g' = coef * grad_scale * g          (coef, when given, is folded into grad_scale once per launch)
 *   2. weight_decay != 0:  g' = g' + wd * p
 *   3. momentum != 0:  buf = g' when t == 1 (torch clones the first gradient, whatever the dampening),
 *                      otherwise buf = momentum * buf + (1 - dampening) * g'
 *   4. nesterov: g' = g' + momentum * buf;  otherwise (momentum != 0) g' = buf
 *   5. p = p - lr * g'
 * buf is the momentum buffer (NULL allowed when momentum == 0; then nothing but p is written).  nesterov needs momentum > 0 and
 * dampening == 0, momentum and weight_decay must not be negative (N3D_ERR_INVALID).  Traffic per element: 12 B in + 8 B out.
 * n3d_adamw_step, per element in fp32:
 *   1. p = p * (1 - lr * wd)               (the factor is formed in fp64 once per launch and rounded to fp32 once)
 *   2. g' = coef * grad_scale * g;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2
 *   3. p = p - (lr / (1 - b1^t)) * (m / (sqrt(v) / sqrt(1 - b2^t) + eps))       (n3d_adam_step's order; no coupled decay term)
 * Traffic per element: 16 B in + 12 B out. */
int n3d_sgd_step(float* param, const float* grad, float* buf, int64_t n, float lr, const float* lr_ptr, double momentum,
                 double dampening, double weight_decay, int nesterov, float grad_scale, const float* coef, int32_t* step_ptr,
                 int inc_step, void* stream);
int n3d_sgd_step_guarded(float* param, const float* grad, float* buf, int64_t n, float lr, const float* lr_ptr, double momentum,
                         double dampening, double weight_decay, int nesterov, float grad_scale, const float* coef,
                         int32_t* step_ptr, int inc_step, const void* timeouts, const void* acked, const float* peer_flag,
                         float* loss, void* host_word, void* stream);
int n3d_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, const float* lr_ptr,
                   double beta1, double beta2, double eps, double weight_decay, float grad_scale, const float* coef,
                   int32_t* step_ptr, int inc_step, void* stream);
int n3d_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                           const float* lr_ptr, double beta1, double beta2, double eps, double weight_decay, float grad_scale,
                           const float* coef, int32_t* step_ptr, int inc_step, const void* timeouts, const void* acked,
                           const float* peer_flag, float* loss, void* host_word, void* stream);

/* ---- learning-rate schedule on the device: linear warm-up, then polynomial or cosine decay -------------------------
 * One lane, fp64, issued on the step's stream anywhere in front of the optimiser launch that reads *lr_out as its lr_ptr: a
 * captured step follows a per-step schedule with no host call.  s = *step_ptr is the number of updates applied so far (a
 * withheld update does not advance it).  rec: N3D_LR_REC_LEN device doubles, 8-byte aligned,
 *   rec[0] kind (N3D_LR_POLY / N3D_LR_COSINE), rec[1] base_lr, rec[2] min_lr, rec[3] warmup_steps W, rec[4] warmup_start a,
 *   rec[5] total_steps T (> W), rec[6] power (poly only)
 *   s < W:      lr = base * (a + (1 - a) * s / W)
 *   otherwise:  u = min(s - W, T - W), n = T - W
 *     poly:     lr = max(min_lr, base * (1 - u / n)^power)
 *     cosine:   lr = min_lr + (base - min_lr) * (1 + cos(pi * u / n)) / 2        (u == n: the cosine is taken as -1)
 *   *lr_out = (float)lr
 * The closed forms of torch's SequentialLR([LinearLR(start_factor=a, total_iters=W), PolynomialLR | CosineAnnealingLR]) up to
 * s = T; past T the rate stays at its end value.  A new base rate is one 8-byte write to rec[1] between launches. */
#define N3D_LR_REC_LEN 7
#define N3D_LR_POLY 0
#define N3D_LR_COSINE 1
int n3d_lr_schedule(const int32_t* step_ptr, const double* rec, float* lr_out, void* stream);

/* ---- exponential moving average of the weights, and the exchange of two flat buffers ----------------------------------
 * n3d_ema_step is torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)).update_parameters over one flat
 * buffer, issued behind an optimiser launch.  state: N3D_EMA_STATE_WORDS device int32 {n_averaged, last_step, ticket}, the ticket
 * zero between launches, last_step the value *step_ptr had when the average last moved (at the start: when it was set up).
 *   *step_ptr == last_step: the optimiser launch in front was withheld -> nothing is touched
 *   n_averaged == 0:        ema = p
 *   otherwise:              ema = ema + w * (p - ema),  w = (float)(1.0 - decay)       (lerp's weight < 0.5 branch: 0.5 < decay < 1)
 *   then n_averaged += 1, last_step = *step_ptr   (every workgroup reads state before it draws its ticket; the last ticket writes)
 * n3d_swap_f32 exchanges the contents of two flat buffers that do not overlap.  Both use the float4 layout of the update kernels,
 * with an element-wise tail and an element-wise path for buffers off a 16-byte boundary. */
#define N3D_EMA_STATE_WORDS 3
int n3d_ema_step(float* ema, const float* param, int64_t n, double decay, const int32_t* step_ptr, int32_t* state, void* stream);
int n3d_swap_f32(float* a, float* b, int64_t n, void* stream);

/* ---- global gradient norm and clip coefficient (config.yml:49 grad_clip; train.py:126-127, search.py:236-237) --------
 * torch.nn.utils.clip_grad_norm_(params, max_norm) with norm_type 2 and error_if_nonfinite=False over ONE flat buffer, in one
 * launch and without a host sync:  out[0] = || grad_scale * grad ||_2 (fp64 sums, rounded to fp32 once),
 * out[1] = min(1, max_norm / (out[0] + 1e-6)) (quotient in fp64, rounded once).  A NaN norm gives a NaN coefficient.  The
 * optimiser entry points read out + 1 as `coef`.  The grid depends on n alone, every workgroup adds its elements in a fixed
 * order and the workgroup that draws the last ticket adds the partial sums in index order: the same input gives the same bits
 * on every launch and every graph replay.  scratch: n3d_grad_clip_scratch_bytes() bytes, 8-byte aligned, zeroed once (word 0
 * is the ticket, cleared again by the launch). */
size_t n3d_grad_clip_scratch_bytes(void);
int n3d_grad_clip_coef(const float* grad, int64_t n, float grad_scale, double max_norm, void* scratch, float* out, void* stream);
/* 64 bytes of pinned, device-mapped, coherent host memory (zeroed); the pointer is valid on the host and in kernels */
int n3d_host_word_alloc(void** host_ptr);
int n3d_host_word_free(void* host_ptr);

/* ---- stream hand-off (no reference counterpart: the reference runs one CUDA stream, train.py:117-128) ----------------
 * Device-side ordering between two HIP streams whose work was launched as SEPARATE graphs: the weight-gradient kernels of
 * a train step run on a side stream next to the backward chain (train.Trainer).  On this stack an event between two graph
 * launches costs ~190 us per hand-off and an intra-graph fork ~19 us per edge without overlap; a flag in device memory costs
 * a ~2 us kernel on each side (tools/handoff_cost.cpp).
 * Protocol: each stream owns a device uint32 STEP counter (starts at 1, bumped once per step by that stream's last sync
 * call, bump != 0).  n3d_sync_signal stores *step to *flag (release, agent scope) behind everything enqueued so far on
 * `stream`; n3d_sync_wait holds `stream` until *flag >= *step (its own stream's counter; wrap-safe compare), polling with
 * one lane.  The poll is bounded: after max_polls tries (~0.3 us each) the wait gives up, adds 1 to *timeouts and lets the
 * stream continue -- results are then wrong, the GPU is never hung; callers read *timeouts (train.Trainer.check_sync).
 * The two streams must map to different hardware queues (a wait at the head of the queue that also carries the signal
 * would time out); train.Trainer probes this once. */
int n3d_sync_signal(void* flag, void* step, int bump, void* stream);
/* diagnostic: stores the 100 MHz wall clock (s_memrealtime) to *out (device uint64) when the stream gets there -- rocprofv3's
 * kernel trace serialises the two streams, so the timeline of the side-stream schedule is taken with these (tools/side_timeline.py) */
int n3d_stamp(void* out, void* stream);
int n3d_sync_wait(const void* flag, void* step, void* timeouts, int bump, int64_t max_polls, void* stream);
/* the same for TWO flags in one launch (both must have reached *step; one time-out is counted if either has not) */
int n3d_sync_wait2(const void* flag0, const void* flag1, void* step, void* timeouts, int bump, int64_t max_polls, void* stream);
/* Entry signals: a signal carried by the NEXT kernel of its stream instead of a launch of its own.  n3d_entry_signal_arm attaches
 * (flag, step, bump) -- the arguments of n3d_sync_signal -- to the next n3d_* launch the calling thread issues; it may be called
 * twice (two signals, executed in arming order).  If that launch is on `stream` and its kernel is a carrier, one lane of the
 * kernel's first workgroup does what the signal kernel does before anything else of the kernel runs: the store is ordered behind
 * everything enqueued on `stream` so far, exactly like n3d_sync_signal, and one dependent kernel boundary goes.  In every other
 * case (a kernel that carries nothing, a launch on another stream, and the calls that enqueue stream work without a kernel of the
 * library: n3d_zero, the n3d_comm_* collectives, n3d_stream_capture_end, n3d_graph_launch) the library issues the stand-alone
 * signal kernel on `stream` IN FRONT OF that work: an armed signal is never lost and never later than "in front of the next
 * launch".  Calls that enqueue nothing (queries, n3d_host_word_*, n3d_stream_capture_begin, ...) leave it armed.  n3d_entry_signal_flush issues what is armed for `stream` at once (for places with no next launch).
 * The state is per host thread.  n3d_entry_signal_pending: signals armed and not yet issued (0, 1 or 2);
 * n3d_entry_signal_counts: signals carried by a kernel / issued stand-alone by the library since the library was loaded. */
int n3d_entry_signal_arm(void* flag, void* step, int bump, void* stream);
int n3d_entry_signal_flush(void* stream);
int n3d_entry_signal_pending(void);
int n3d_entry_signal_counts(int64_t* carried, int64_t* standalone);
/* The side streams and their graphs, made through the HIP runtime libn3d is linked against (the one that launches the kernels):
 * a non-blocking stream of the lowest priority the device offers; thread-local capture of a stream into an instantiated
 * executable graph (the side streams are captured NEXT TO torch's capture of the main stream); launch / destroy. */
int n3d_stream_create_low_priority(void** stream_out);
int n3d_stream_capture_begin(void* stream);
int n3d_stream_capture_end(void* stream, void** graph_exec_out);
int n3d_graph_launch(void* graph_exec, void* stream);
int n3d_graph_destroy(void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* N3D_H_ */
