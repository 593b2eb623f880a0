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

// threshold + label fusion of the three sigmoid channels (prediction.py:150-170): fuse_labels, n3d_common.h
__global__ __launch_bounds__(256) void tumor_labels_kernel(const double* __restrict__ pred, int64_t N, double thr, int inclusive,
                                                           uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  out[i] = (uint8_t)fuse_labels(pred[i], pred[N + i], pred[2 * N + i], thr, inclusive);
}

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
        const float* p = patches + t.slot * sb + stitch_entry_voxel(t.d, l, P) * sv;
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

// Whole-image prediction (predict.ImagePredictor; prediction.py:102-119, `fs_pred`): the net runs ONCE on the full image zero-padded
// at the high end, so there is no patch list and no stitch.  Two bandwidth passes stand around that forward, one thread per voxel,
// integer index work only.  A flip f[a] mirrors the image inside [0, F_a) -- the pad stays at the high end -- which is
// np.pad(permute_data(image, key)) for a flip-only key; the same map brings a prediction back (a mirror is its own inverse).
struct Int3 { int v[3]; };

// image_embed: one thread per voxel of the PADDED grid writes the net's input (pitched NDHWC, Cv floats; the pitch gap is left
// alone, as patch_batch_kernel leaves it): the subject's box (Cv, bx, by, bz) where the mirrored voxel falls inside it, zeros in
// the rest of the image and in the pad.  Every voxel is written exactly once: the caller clears nothing.
__global__ __launch_bounds__(256) void image_embed_kernel(const float* __restrict__ box, int Cv, Int3 b, Int3 o, Int3 F, Int3 f,
                                                          float* __restrict__ x_out, int64_t xld, uint32_t PN, FastDiv fPZ, FastDiv fPYZ) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= PN) return;
  uint32_t px, r, py, pz;
  fPYZ.divmod(v, px, r);
  fPZ.divmod(r, py, pz);
  const int p[3] = {(int)px, (int)py, (int)pz};
  bool in = true;
  int l[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int s = f.v[a] ? F.v[a] - 1 - p[a] : p[a];      // negative in the pad of a mirrored axis: outside the box either way
    l[a] = s - o.v[a];
    in = in && p[a] < F.v[a] && (unsigned)l[a] < (unsigned)b.v[a];
  }
  const int64_t BN = (int64_t)b.v[0] * b.v[1] * b.v[2];
  const int64_t sv = in ? ((int64_t)l[0] * b.v[1] + l[1]) * b.v[2] + l[2] : 0;
  float* xo = x_out + (int64_t)v * xld;
  if (Cv == 4 && (xld & 3) == 0) {
    float4 q;
    q.x = in ? box[sv] : 0.f; q.y = in ? box[BN + sv] : 0.f; q.z = in ? box[2 * BN + sv] : 0.f; q.w = in ? box[3 * BN + sv] : 0.f;
    *reinterpret_cast<float4*>(xo) = q;
  } else {
    for (int c = 0; c < Cv; ++c) xo[c] = in ? box[c * BN + sv] : 0.f;
  }
}

// the padded-grid voxel that holds the prediction of full-image voxel (x, y, z) under flip f
__device__ __forceinline__ int64_t image_src_voxel(int x, int y, int z, const Int3& F, const Int3& P, const Int3& f) {
  const int px = f.v[0] ? F.v[0] - 1 - x : x, py = f.v[1] ? F.v[1] - 1 - y : y, pz = f.v[2] ? F.v[2] - 1 - z : z;
  return ((int64_t)px * P.v[1] + py) * P.v[2] + pz;
}

// image_add (every key of an ensemble but the last): sum = (first ? 0 : sum) + (double)y brought back and cropped to the image.
// The first key writes, so the running sum needs no clearing; one thread owns a voxel: the key-order fp64 sum, no atomics.
__global__ __launch_bounds__(256) void image_add_kernel(const float* __restrict__ y, int64_t sc, int64_t sv, int C, Int3 F, Int3 P, Int3 f,
                                                        double* __restrict__ sum, int first, uint32_t FN, FastDiv fZ, FastDiv fYZ) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= FN) return;
  uint32_t x, r, yy, z;
  fYZ.divmod(v, x, r);
  fZ.divmod(r, yy, z);
  const float* p = y + image_src_voxel((int)x, (int)yy, (int)z, F, P, f) * sv;
  N3D_EACH_CHANNEL(c, C) {
    const double t = (double)p[c * sc];
    sum[(int64_t)c * FN + v] = first ? t : sum[(int64_t)c * FN + v] + t;
  }
}

// image_finish (the last key, or the only one): ONE pass over the full image.  mean = (sum + (double)y) / K in key order -- without a
// running sum exactly (double)y -- written as fp64 probabilities (probs != NULL) and / or fused into the label byte (labels != NULL;
// with the mask box the label is 0 where every channel of the subject's box is zero and everywhere outside the box:
// prediction.py:83-96).  Every voxel of either output is written exactly once.
__global__ __launch_bounds__(256) void image_finish_kernel(const float* __restrict__ y, int64_t sc, int64_t sv, int C, Int3 F, Int3 P, Int3 f,
                                                           const double* __restrict__ sum, double K, double* __restrict__ probs,
                                                           uint8_t* __restrict__ labels, double thr, int inclusive,
                                                           const float* __restrict__ mask_box, int Cv, Int3 b, Int3 o, uint32_t FN,
                                                           FastDiv fZ, FastDiv fYZ) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= FN) return;
  uint32_t x, r, yy, z;
  fYZ.divmod(v, x, r);
  fZ.divmod(r, yy, z);
  const float* p = y + image_src_voxel((int)x, (int)yy, (int)z, F, P, f) * sv;
  double m[4] = {0, 0, 0, 0};
  N3D_EACH_CHANNEL(c, C) {
    const double t = (double)p[c * sc];
    m[c] = sum ? (sum[(int64_t)c * FN + v] + t) / K : t;
  }
  if (probs) {
    N3D_EACH_CHANNEL(c, C) probs[(int64_t)c * FN + v] = m[c];
  }
  if (labels) {
    bool keep = true;
    if (mask_box) {
      const int lx = (int)x - o.v[0], ly = (int)yy - o.v[1], lz = (int)z - o.v[2];
      int any = 0;
      if ((unsigned)lx < (unsigned)b.v[0] && (unsigned)ly < (unsigned)b.v[1] && (unsigned)lz < (unsigned)b.v[2]) {
        const int64_t BN = (int64_t)b.v[0] * b.v[1] * b.v[2];
        const int64_t q = ((int64_t)lx * b.v[1] + ly) * b.v[2] + lz;
        for (int c = 0; c < Cv; ++c) any |= nonzero_f32(mask_box[c * BN + q]);
      }
      keep = any != 0;
    }
    labels[v] = (uint8_t)(keep ? fuse_labels(m[0], m[1], m[2], thr, inclusive) : 0);
  }
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
  if (!stitch_clip_box(lo, hi, dims, b0, bs)) return N3D_OK;     // wholly outside the box: nothing to add
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

// the geometry shared by the three whole-image entry points: full image inside the padded grid, FX * FY * FZ < 2^31
static int image_geometry(const char* what, const int32_t* full, const int32_t* padded, const int32_t* flip, Int3* F, Int3* P, Int3* f) {
  N3D_CHECK_ARG(full && padded && flip, "%s: full / padded / flip are int32[3] host arrays", what);
  for (int a = 0; a < 3; ++a) {
    N3D_CHECK_ARG(full[a] > 0 && padded[a] >= full[a], "%s: axis %d: the padded grid (%d) must hold the image (%d)", what, a, padded[a], full[a]);
    F->v[a] = full[a]; P->v[a] = padded[a]; f->v[a] = flip[a] ? 1 : 0;
  }
  N3D_CHECK_ARG((int64_t)full[0] * full[1] * full[2] < (1ll << 31), "%s: image too large", what);
  return N3D_OK;
}

static int image_box(const char* what, int bx, int by, int bz, const int32_t* origin, const Int3& F, Int3* b, Int3* o) {
  N3D_CHECK_ARG(origin && bx > 0 && by > 0 && bz > 0, "%s: bad box", what);
  const int bs[3] = {bx, by, bz};
  for (int a = 0; a < 3; ++a) {
    N3D_CHECK_ARG(origin[a] >= 0 && origin[a] + bs[a] <= F.v[a], "%s: axis %d: box [%d, %d) outside the image (%d)", what, a, origin[a],
                  origin[a] + bs[a], F.v[a]);
    b->v[a] = bs[a]; o->v[a] = origin[a];
  }
  return N3D_OK;
}

extern "C" int n3d_image_embed(const float* box, int Cv, int bx, int by, int bz, const int32_t* origin, const int32_t* full,
                               const int32_t* padded, const int32_t* flip, float* x_out, int64_t xld, void* stream) {
  N3D_CHECK_ARG(box && x_out && Cv >= 1 && xld >= Cv, "image_embed: bad args");
  Int3 F, P, f, b, o;
  if (int e = image_geometry("image_embed", full, padded, flip, &F, &P, &f)) return e;
  if (int e = image_box("image_embed", bx, by, bz, origin, F, &b, &o)) return e;
  const int64_t PN = (int64_t)P.v[0] * P.v[1] * P.v[2];
  N3D_CHECK_ARG(PN < (1ll << 31), "image_embed: padded grid too large");
  N3D_CHECK_ARG(!(Cv == 4 && (xld & 3) == 0) || aligned16(x_out), "image_embed: a 4-channel output with a pitch of whole quads must be 16-byte aligned");
  N3D_LAUNCH(image_embed_kernel, dim3((unsigned)cdiv(PN, 256)), dim3(256), 0, (hipStream_t)stream, box, Cv, b, o, F, f, x_out, xld, (uint32_t)PN,
             FastDiv((uint32_t)P.v[2]), FastDiv((uint32_t)P.v[1] * P.v[2]));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_image_add(const float* y, int64_t sc, int64_t sv, int C, const int32_t* full, const int32_t* padded, const int32_t* flip,
                             double* sum, int first, void* stream) {
  N3D_CHECK_ARG(y && sum && C >= 1 && C <= 4, "image_add: bad args (1 <= C <= 4)");
  Int3 F, P, f;
  if (int e = image_geometry("image_add", full, padded, flip, &F, &P, &f)) return e;
  const uint32_t FN = (uint32_t)((int64_t)F.v[0] * F.v[1] * F.v[2]);
  N3D_LAUNCH(image_add_kernel, dim3((unsigned)cdiv(FN, 256)), dim3(256), 0, (hipStream_t)stream, y, sc, sv, C, F, P, f, sum, first ? 1 : 0, FN,
             FastDiv((uint32_t)F.v[2]), FastDiv((uint32_t)F.v[1] * F.v[2]));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_image_finish(const float* y, int64_t sc, int64_t sv, int C, const int32_t* full, const int32_t* padded, const int32_t* flip,
                                const double* sum, int K, double* probs, uint8_t* labels, double threshold, int inclusive,
                                const float* mask_box, int Cv, int bx, int by, int bz, const int32_t* origin, void* stream) {
  N3D_CHECK_ARG(y && C >= 1 && C <= 4 && K >= 1, "image_finish: bad args (1 <= C <= 4, K >= 1)");
  N3D_CHECK_ARG(probs || labels, "image_finish: neither probabilities nor labels asked for");
  N3D_CHECK_ARG(!labels || C == 3, "image_finish: labels fuse 3 channels (got %d)", C);
  N3D_CHECK_ARG((sum != nullptr) == (K > 1), "image_finish: a running sum goes with K > 1 and only with it (K = %d)", K);
  Int3 F, P, f, b = {{1, 1, 1}}, o = {{0, 0, 0}};
  if (int e = image_geometry("image_finish", full, padded, flip, &F, &P, &f)) return e;
  if (mask_box) {
    N3D_CHECK_ARG(Cv >= 1, "image_finish: the skull mask needs the subject's channel count");
    if (int e = image_box("image_finish", bx, by, bz, origin, F, &b, &o)) return e;
  }
  const uint32_t FN = (uint32_t)((int64_t)F.v[0] * F.v[1] * F.v[2]);
  N3D_LAUNCH(image_finish_kernel, dim3((unsigned)cdiv(FN, 256)), dim3(256), 0, (hipStream_t)stream, y, sc, sv, C, F, P, f, sum, (double)K, probs,
             labels, threshold, inclusive, mask_box, Cv, b, o, FN, FastDiv((uint32_t)F.v[2]), FastDiv((uint32_t)F.v[1] * F.v[2]));
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}
