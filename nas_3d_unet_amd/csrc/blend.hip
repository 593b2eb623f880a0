// Importance-weighted stitching (predict.SubjectPredictor(blend=...), predict.EnsemblePredictor): n3d_stitch_add / n3d_stitch_finish
// of post_step.hip with a weight per covering patch -- the separable profile at the voxel's position inside the patch -- and a
// running fp64 weight sum in place of the int32 covering count.  Same shape: one thread per voxel of the chunk's bounding box, no
// atomics, the entries of the range in table order.  Every fp64 product and sum below is one separately rounded operation in the
// association written (include/n3d.h states them): this file is compiled with contraction off (Makefile), which would otherwise
// fuse w * p + sum.
#include "n3d_common.h"

namespace n3d {

constexpr int BLEND_MAX_P = 1024;      // the profile is staged in LDS: 8 KB

// The profile goes to LDS once per workgroup: three dependent global loads per hit would sit on the entry loop's chain.  Inside
// a wave l[0] and l[1] are all but uniform (broadcast reads) and l[2] runs with the lane: no bank conflict to pad for.
__global__ __launch_bounds__(256) void stitch_add_w_kernel(const float* __restrict__ patches, int64_t sb, int64_t sc, int64_t sv, int C, int P,
                                                           int nslots, const n3d_stitch_entry* __restrict__ entries, int n,
                                                           const double* __restrict__ profile, int X, int Y, int Z, int b0x, int b0y, int b0z,
                                                           uint32_t nvox, FastDiv fbz, FastDiv fbyz, double* __restrict__ sum,
                                                           double* __restrict__ wsum) {
  __shared__ double prof[BLEND_MAX_P];
  for (int i = threadIdx.x; i < P; i += 256) prof[i] = profile[i];
  __syncthreads();
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nvox) return;
  uint32_t ux, r, uy, uz;
  fbyz.divmod(v, ux, r);
  fbz.divmod(r, uy, uz);
  const int x = (int)ux + b0x, y = (int)uy + b0y, z = (int)uz + b0z;
  const int64_t N = (int64_t)X * Y * Z;
  const int64_t o = ((int64_t)x * Y + y) * Z + z;
  double acc[4] = {0, 0, 0, 0};
  N3D_EACH_CHANNEL(c, C) acc[c] = sum[c * N + o];
  double wacc = wsum[o];
  bool hit = false;
  for (int e = 0; e < n; ++e) {
    const n3d_stitch_entry t = entries[e];      // uniform load
    const int l[3] = {x - t.d.corner[0], y - t.d.corner[1], z - t.d.corner[2]};
    if ((unsigned)l[0] < (unsigned)P && (unsigned)l[1] < (unsigned)P && (unsigned)l[2] < (unsigned)P) {
      hit = true;
      const double w = (prof[l[0]] * prof[l[1]]) * prof[l[2]];      // at l on the volume's grid, not at the net's own index
      wacc = wacc + w;
      if ((unsigned)t.slot < (unsigned)nslots) {                    // a dead entry covers and adds zeros: its weight only
        const float* p = patches + t.slot * sb + stitch_entry_voxel(t.d, l, P) * sv;
        N3D_EACH_CHANNEL(c, C) acc[c] = acc[c] + w * (double)p[c * sc];
      }
    }
  }
  if (hit) {
    N3D_EACH_CHANNEL(c, C) sum[c * N + o] = acc[c];
    wsum[o] = wacc;
  }
}

// stitch_finish_kernel (post_step.hip) with mean = wsum > 0 ? sum / wsum : 0 in place of sum / max(cnt, 1): one pass over the FULL
// image, every voxel of either output written exactly once.
__global__ __launch_bounds__(256) void stitch_finish_w_kernel(const double* __restrict__ sum, const double* __restrict__ wsum, int C, int X, int Y,
                                                              int Z, double* __restrict__ probs, uint8_t* __restrict__ labels, double thr,
                                                              int inclusive, const float* __restrict__ mask_vol, int Cv, int FY, int FZ,
                                                              int ox, int oy, int oz, uint32_t FN, FastDiv fZ, FastDiv fYZ) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= FN) return;
  uint32_t fx, r, fy, fz;
  fYZ.divmod(v, fx, r);
  fZ.divmod(r, fy, fz);
  const int x = (int)fx - ox, y = (int)fy - oy, z = (int)fz - oz;
  double m[4] = {0, 0, 0, 0};
  bool keep = false;
  if ((unsigned)x < (unsigned)X && (unsigned)y < (unsigned)Y && (unsigned)z < (unsigned)Z) {
    const int64_t N = (int64_t)X * Y * Z;
    const int64_t o = ((int64_t)x * Y + y) * Z + z;
    const double ws = wsum[o];
    if (ws > 0) {
      N3D_EACH_CHANNEL(c, C) m[c] = sum[c * N + o] / ws;
    }
    keep = true;
    if (labels && mask_vol) {
      int any = 0;
      for (int c = 0; c < Cv; ++c) any |= nonzero_f32(mask_vol[c * N + o]);
      keep = any != 0;
    }
  }
  if (probs) {
    N3D_EACH_CHANNEL(c, C) probs[(int64_t)c * FN + v] = m[c];
  }
  if (labels) labels[v] = (uint8_t)(keep ? fuse_labels(m[0], m[1], m[2], thr, inclusive) : 0);
}

}  // namespace n3d

using namespace n3d;

extern "C" int n3d_stitch_add_w(const float* patches, int64_t sb, int64_t sc, int64_t sv, int C, int P, int nslots,
                                const n3d_stitch_entry* entries, int n, const double* profile, const int32_t* lo, const int32_t* hi, int X,
                                int Y, int Z, double* sum, double* wsum, void* stream) {
  N3D_CHECK_ARG(entries && lo && hi && sum && wsum && C >= 1 && C <= 4 && P > 0 && n >= 1 && nslots >= 0 && X > 0 && Y > 0 && Z > 0,
                "stitch_add_w: bad args (1 <= C <= 4)");
  N3D_CHECK_ARG(profile, "stitch_add_w: no profile");
  N3D_CHECK_ARG(P <= BLEND_MAX_P, "stitch_add_w: the profile of a patch of %d does not fit the kernel's table (P <= %d)", P, BLEND_MAX_P);
  N3D_CHECK_ARG(patches || nslots == 0, "stitch_add_w: %d slots but no patch tensor", nslots);
  N3D_CHECK_ARG((int64_t)X * Y * Z < (1ll << 31), "stitch_add_w: volume too large");
  const int dims[3] = {X, Y, Z};
  int b0[3], bs[3];
  if (!stitch_clip_box(lo, hi, dims, b0, bs)) return N3D_OK;     // wholly outside the box: nothing to add
  const uint32_t nvox = (uint32_t)((int64_t)bs[0] * bs[1] * bs[2]);
  N3D_LAUNCH(stitch_add_w_kernel, dim3((unsigned)cdiv(nvox, 256)), dim3(256), 0, (hipStream_t)stream, patches, sb, sc, sv, C, P, nslots, entries,
             n, profile, X, Y, Z, b0[0], b0[1], b0[2], nvox, FastDiv((uint32_t)bs[2]), FastDiv((uint32_t)bs[1] * bs[2]), sum, wsum);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_stitch_finish_w(const double* sum, const double* wsum, int C, int X, int Y, int Z, double* probs, uint8_t* labels,
                                   double threshold, int inclusive, const float* mask_vol, int Cv, int FX, int FY, int FZ, int ox, int oy,
                                   int oz, void* stream) {
  N3D_CHECK_ARG(sum && wsum && C >= 1 && C <= 4 && X > 0 && Y > 0 && Z > 0, "stitch_finish_w: bad args (1 <= C <= 4)");
  N3D_CHECK_ARG(probs || labels, "stitch_finish_w: neither probabilities nor labels asked for");
  N3D_CHECK_ARG(!labels || C == 3, "stitch_finish_w: labels fuse 3 channels (got %d)", C);
  N3D_CHECK_ARG(!mask_vol || Cv >= 1, "stitch_finish_w: the skull mask needs the subject's channel count");
  N3D_CHECK_ARG(ox >= 0 && oy >= 0 && oz >= 0 && ox + X <= FX && oy + Y <= FY && oz + Z <= FZ,
                "stitch_finish_w: brain-wide box outside the full image");
  N3D_CHECK_ARG((int64_t)FX * FY * FZ < (1ll << 31), "stitch_finish_w: image too large");
  const uint32_t FN = (uint32_t)((int64_t)FX * FY * FZ);
  N3D_LAUNCH(stitch_finish_w_kernel, dim3((unsigned)cdiv(FN, 256)), dim3(256), 0, (hipStream_t)stream, sum, wsum, C, X, Y, Z, probs, labels,
             threshold, inclusive, mask_vol, Cv, FY, FZ, ox, oy, oz, FN, FastDiv((uint32_t)FZ), FastDiv((uint32_t)FY * FZ));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}
