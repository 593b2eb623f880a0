// Step after the hot path: stitching of the per-patch predictions into the brain-wide volume with
// mean blending (patches.py:172-207, used by prediction.py:132-148) and threshold + label fusion (prediction.py:150-170).
// Both are HBM-bound gathers with integer index work: one thread per output voxel, no atomics -- every voxel visits
// the covering patches in list order and sums in fp64, which reproduces the reference's patch-by-patch float64
// accumulation bit for bit.
#include "n3d_common.h"

namespace n3d {

__global__ __launch_bounds__(256) void stitch_kernel(const float* __restrict__ patches, int64_t sb, int64_t sc, int64_t sv, int C, int P,
                                                     const int32_t* __restrict__ corners, int B, int X, int Y, int Z, double* __restrict__ out,
                                                     int FX, int FY, int FZ, int ox, int oy, int oz, FastDiv fZ, FastDiv fYZ) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  const uint32_t N = (uint32_t)X * Y * Z;
  if (v >= N) return;
  uint32_t x, r, y, z;
  fYZ.divmod(v, x, r);
  fZ.divmod(r, y, z);
  double acc[4] = {0, 0, 0, 0};
  int cnt = 0;
  for (int b = 0; b < B; ++b) {
    const int lx = (int)x - corners[b * 3], ly = (int)y - corners[b * 3 + 1], lz = (int)z - corners[b * 3 + 2];  // uniform loads
    if ((unsigned)lx < (unsigned)P && (unsigned)ly < (unsigned)P && (unsigned)lz < (unsigned)P) {
      const float* p = patches + b * sb + (((int64_t)lx * P + ly) * P + lz) * sv;
      for (int c = 0; c < C; ++c) acc[c] += (double)p[c * sc];
      ++cnt;
    }
  }
  const double inv = 1.0 / (double)(cnt > 0 ? cnt : 1);  // uncovered voxels stay 0 (patches.py:203-205)
  const int64_t FN = (int64_t)FX * FY * FZ;
  const int64_t o = ((int64_t)(x + ox) * FY + (y + oy)) * FZ + (z + oz);
  for (int c = 0; c < C; ++c) out[c * FN + o] = acc[c] / (double)(cnt > 0 ? cnt : 1);
  (void)inv;
}

// threshold + label fusion of the three sigmoid channels (prediction.py:150-170)
__device__ __forceinline__ int fuse_labels(double p0, double p1, double p2, double thr, int inclusive) {
  const bool a = p0 >= thr, b = p1 >= thr, c = p2 >= thr;
  if (inclusive) return c ? 4 : (a ? 1 : (b ? 2 : 0));          // later assignments win: WT(2), then TC(1), then ET(4)
  // channels vote; two votes are settled by the larger probability, the earlier channel on equality (np.argmax)
  int t = (a && b) ? (p0 >= p1 ? 1 : 2) : (a ? 1 : 0) + (b ? 2 : 0);
  if (c) t = t == 1 ? (p0 >= p2 ? 1 : 4) : (t == 2 ? (p1 >= p2 ? 2 : 4) : t + 4);
  return t;
}

__global__ __launch_bounds__(256) void tumor_labels_kernel(const double* __restrict__ pred, int64_t N, double thr, int inclusive,
                                                           uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  out[i] = (uint8_t)fuse_labels(pred[i], pred[N + i], pred[2 * N + i], thr, inclusive);
}

// (registers, not a runtime-indexed array: 1 <= C <= 4)
#define N3D_EACH_CHANNEL(c, C) _Pragma("unroll") for (int c = 0; c < 4; ++c) if (c < (C))

// Subject-level stitching, chunk by chunk (predict.SubjectPredictor): the running fp64 sums and covering counts of the brain-wide
// box live in HBM between the chunks of a subject, so no patch prediction outlives its chunk.  One thread per voxel of the
// chunk's bounding box (bx, by, bz at b0 inside the box), no atomics: the voxel loads its running sum, visits the chunk's table
// entries in order (uniform loads) and stores -- chunk after chunk that is the list-order fp64 sum of stitch_kernel.  An entry
// carries the descriptor its patch was gathered with (q[i] = x[s(i)], s_a = i[perm[a]] or P-1-i[perm[a]]); the prediction of q
// comes back at the voxel's local coordinates l = s by solving for i here.  slot < 0: a patch the net never saw (all of its
// modalities zero): it covers and adds zeros (prediction.py:133-135).
__global__ __launch_bounds__(256) void stitch_add_kernel(const float* __restrict__ patches, int64_t sb, int64_t sc, int64_t sv, int C, int P,
                                                         int nslots, const n3d_stitch_entry* __restrict__ entries, int n, int X, int Y, int Z,
                                                         int b0x, int b0y, int b0z, uint32_t nvox, FastDiv fbz, FastDiv fbyz,
                                                         double* __restrict__ sum, int32_t* __restrict__ cnt) {
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
  int hits = 0;
  for (int e = 0; e < n; ++e) {
    const n3d_stitch_entry t = entries[e];      // uniform load
    const int l[3] = {x - t.d.corner[0], y - t.d.corner[1], z - t.d.corner[2]};
    if ((unsigned)l[0] < (unsigned)P && (unsigned)l[1] < (unsigned)P && (unsigned)l[2] < (unsigned)P) {
      ++hits;
      if ((unsigned)t.slot < (unsigned)nslots) {
        int i0 = 0, i1 = 0, i2 = 0;             // i[perm[a]] = l[a] or P-1-l[a]; a perm that is none leaves an index at 0, never outside
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const int s = t.d.flip[a] ? P - 1 - l[a] : l[a];
          const int pa = t.d.perm[a];
          i0 = pa == 0 ? s : i0;
          i1 = pa == 1 ? s : i1;
          i2 = pa == 2 ? s : i2;
        }
        const float* p = patches + t.slot * sb + (((int64_t)i0 * P + i1) * P + i2) * sv;
        N3D_EACH_CHANNEL(c, C) acc[c] += (double)p[c * sc];
      }
    }
  }
  if (hits) {
    N3D_EACH_CHANNEL(c, C) sum[c * N + o] = acc[c];
    cnt[o] += hits;
  }
}

// One pass over the FULL image: inside the box the mean sum / max(cnt, 1) (uncovered voxels stay 0, patches.py:203-205), written as
// fp64 probabilities (probs != NULL) and / or fused into the label byte (labels != NULL; with mask_vol the label is 0 where every
// channel of the subject's box is zero -- prediction.py:83-96); outside the box zeros.  Every voxel of either output is written
// exactly once, so the caller's buffers need no clearing.
__global__ __launch_bounds__(256) void stitch_finish_kernel(const double* __restrict__ sum, const int32_t* __restrict__ cnt, int C, int X, int Y,
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
    const int k = cnt[o];
    const double div = (double)(k > 0 ? k : 1);
    N3D_EACH_CHANNEL(c, C) m[c] = sum[c * N + o] / div;
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

extern "C" int n3d_stitch_add(const float* patches, int64_t sb, int64_t sc, int64_t sv, int C, int P, int nslots,
                              const n3d_stitch_entry* entries, int n, const int32_t* lo, const int32_t* hi, int X, int Y, int Z, double* sum,
                              int32_t* cnt, void* stream) {
  N3D_CHECK_ARG(entries && lo && hi && sum && cnt && C >= 1 && C <= 4 && P > 0 && n >= 1 && nslots >= 0 && X > 0 && Y > 0 && Z > 0,
                "stitch_add: bad args (1 <= C <= 4)");
  N3D_CHECK_ARG(patches || nslots == 0, "stitch_add: %d slots but no patch tensor", nslots);
  N3D_CHECK_ARG((int64_t)X * Y * Z < (1ll << 31), "stitch_add: volume too large");
  // the chunk's bounding box [lo, hi) on the brain-wide grid, clipped to the box here: the launch covers it and nothing else
  const int dims[3] = {X, Y, Z};
  int b0[3], bs[3];
  for (int a = 0; a < 3; ++a) {
    const int l = lo[a] < 0 ? 0 : lo[a], h = hi[a] > dims[a] ? dims[a] : hi[a];
    if (h <= l) return N3D_OK;     // wholly outside the box: nothing to add
    b0[a] = l;
    bs[a] = h - l;
  }
  const uint32_t nvox = (uint32_t)((int64_t)bs[0] * bs[1] * bs[2]);
  N3D_LAUNCH(stitch_add_kernel, dim3((unsigned)cdiv(nvox, 256)), dim3(256), 0, (hipStream_t)stream, patches, sb, sc, sv, C, P, nslots, entries, n,
             X, Y, Z, b0[0], b0[1], b0[2], nvox, FastDiv((uint32_t)bs[2]), FastDiv((uint32_t)bs[1] * bs[2]), sum, cnt);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_stitch_finish(const double* sum, const int32_t* cnt, int C, int X, int Y, int Z, double* probs, uint8_t* labels,
                                 double threshold, int inclusive, const float* mask_vol, int Cv, int FX, int FY, int FZ, int ox, int oy, int oz,
                                 void* stream) {
  N3D_CHECK_ARG(sum && cnt && C >= 1 && C <= 4 && X > 0 && Y > 0 && Z > 0, "stitch_finish: bad args (1 <= C <= 4)");
  N3D_CHECK_ARG(probs || labels, "stitch_finish: neither probabilities nor labels asked for");
  N3D_CHECK_ARG(!labels || C == 3, "stitch_finish: labels fuse 3 channels (got %d)", C);
  N3D_CHECK_ARG(!mask_vol || Cv >= 1, "stitch_finish: the skull mask needs the subject's channel count");
  N3D_CHECK_ARG(ox >= 0 && oy >= 0 && oz >= 0 && ox + X <= FX && oy + Y <= FY && oz + Z <= FZ,
                "stitch_finish: brain-wide box outside the full image");
  N3D_CHECK_ARG((int64_t)FX * FY * FZ < (1ll << 31), "stitch_finish: image too large");
  const uint32_t FN = (uint32_t)((int64_t)FX * FY * FZ);
  N3D_LAUNCH(stitch_finish_kernel, dim3((unsigned)cdiv(FN, 256)), dim3(256), 0, (hipStream_t)stream, sum, cnt, C, X, Y, Z, probs, labels,
             threshold, inclusive, mask_vol, Cv, FY, FZ, ox, oy, oz, FN, FastDiv((uint32_t)FZ), FastDiv((uint32_t)FY * FZ));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_stitch(const float* patches, int64_t sb, int64_t sc, int64_t sv, int C, int P, const int32_t* corners, int B, int X, int Y, int Z,
                          double* out, int FX, int FY, int FZ, int ox, int oy, int oz, void* stream) {
  N3D_CHECK_ARG(patches && corners && out && C >= 1 && C <= 4 && P > 0 && B >= 1 && X > 0 && Y > 0 && Z > 0, "stitch: bad args (1 <= C <= 4)");
  N3D_CHECK_ARG(ox >= 0 && oy >= 0 && oz >= 0 && ox + X <= FX && oy + Y <= FY && oz + Z <= FZ, "stitch: brain-wide box outside the full image");
  N3D_CHECK_ARG((int64_t)X * Y * Z < (1ll << 31), "stitch: volume too large");
  const uint32_t N = (uint32_t)X * Y * Z;
  N3D_LAUNCH(stitch_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, patches, sb, sc, sv, C, P, corners, B, X, Y, Z, out,
                     FX, FY, FZ, ox, oy, oz, FastDiv((uint32_t)Z), FastDiv((uint32_t)Y * Z));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_tumor_labels(const double* pred, int64_t N, double threshold, int inclusive, uint8_t* out, void* stream) {
  N3D_CHECK_ARG(pred && out && N > 0, "tumor_labels: bad args");
  N3D_LAUNCH(tumor_labels_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, pred, N, threshold, inclusive, out);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}
