// Crops drawn on the device (include/n3d.h, "random and foreground-centred crops"): a per-volume line index -- for each of five masks
// the number of mask voxels in the z lines before each (x, y) -- and a sampler that turns Philox words into N patch corners in one
// launch: a uniform corner, or the corner that centres the patch on the r-th voxel of a mask, r uniform.  Integer work throughout:
// exact counts, no floating point, no atomics; two runs give the same bits.
#include "n3d_common.h"

namespace n3d {

constexpr int kMasks = N3D_SAMPLE_MASKS;
constexpr int kScanBlock = 1024;

// the five mask bits of one voxel (bit m = mask m): some channel nonzero; label != 0; label 1; label 2; label 4
__device__ __forceinline__ uint32_t sample_mask_bits(const float* __restrict__ vol, int Cv, int64_t XYZ, const uint8_t* __restrict__ truth,
                                                     int64_t at) {
  int any = 0;
  for (int c = 0; c < Cv; ++c) any |= nonzero_f32(vol[c * XYZ + at]);
  uint32_t b = (uint32_t)any;
  if (truth) {
    const uint32_t t = truth[at];
    b |= (t != 0 ? 2u : 0u) | (t == 1 ? 4u : 0u) | (t == 2 ? 8u : 0u) | (t == 4 ? 16u : 0u);
  }
  return b;
}

// counts: one wave per line l = x * Y + y, lanes along z (coalesced loads of the planar volume, as sat_z_kernel); per 64-voxel chunk
// one ballot and one popcount per mask.  The count of line l goes to index[m][l + 1]: the scan below then leaves, in place, the
// number of mask voxels in the lines before l + 1.
__global__ __launch_bounds__(256) void line_count_kernel(const float* __restrict__ vol, int Cv, const uint8_t* __restrict__ truth, int L, int Z,
                                                         int64_t XYZ, int32_t* __restrict__ index) {
  const int lane = threadIdx.x & 63;
  const int64_t line = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (line >= L) return;
  const int64_t row = line * Z;
  int cnt[kMasks] = {0, 0, 0, 0, 0};
  for (int base = 0; base < Z; base += 64) {
    const int z = base + lane;
    const uint32_t b = z < Z ? sample_mask_bits(vol, Cv, XYZ, truth, row + z) : 0u;
#pragma unroll
    for (int m = 0; m < kMasks; ++m) cnt[m] += __popcll(__ballot((b >> m) & 1u));
  }
  if (lane < kMasks) {
    int c = cnt[0];
#pragma unroll
    for (int m = 1; m < kMasks; ++m) c = lane == m ? cnt[m] : c;
    index[(int64_t)lane * (L + 1) + line + 1] = c;
  }
}

// scan: one workgroup per mask walks its row in tiles of 1024 lines, carrying the running total: an inclusive scan of the counts in
// index[m][1 .. L], and index[m][0] = 0.  Wave scans by shuffles, the 16 wave totals through LDS.
__global__ __launch_bounds__(kScanBlock) void line_scan_kernel(int32_t* __restrict__ index, int L) {
  __shared__ int32_t wave_tot[kScanBlock / 64];
  int32_t* row = index + (int64_t)blockIdx.x * (L + 1);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) row[0] = 0;
  int32_t carry = 0;
  for (int base = 0; base < L; base += kScanBlock) {
    const int l = base + tid;
    int32_t s = l < L ? row[l + 1] : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t u = __shfl_up(s, d, 64);
      if (lane >= d) s += u;
    }
    if (lane == 63) wave_tot[wave] = s;
    __syncthreads();
    int32_t before = carry, all = carry;
#pragma unroll
    for (int w = 0; w < kScanBlock / 64; ++w) {
      const int32_t t = wave_tot[w];
      before += w < wave ? t : 0;
      all += t;
    }
    if (l < L) row[l + 1] = before + s;
    carry = all;
    __syncthreads();
  }
}

__device__ __forceinline__ uint32_t sample_reduce(uint32_t q, uint32_t R) { return (uint32_t)(((uint64_t)q * R) >> 32); }

// one wave per sample; every lane carries the sample's scalars (the draws, the volume, the mask, the line), the lanes differ only
// where the chosen line is read: 64 voxels per step, one ballot, and the rank of each set bit below its lane picks the voxel.
__global__ __launch_bounds__(256) void patch_sample_kernel(const n3d_patch_volume* __restrict__ vols, const int32_t* const* __restrict__ index,
                                                           int nvol, int Cv, const int32_t* __restrict__ ids, int n_ids, int64_t N, int P,
                                                           uint32_t key0, uint32_t key1, uint64_t fg_threshold, int masks,
                                                           int4* __restrict__ cand, uint8_t* __restrict__ mode) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  uint32_t w[4], u[4];
  philox4x32_10((uint32_t)n, 2u, 0u, 0u, key0, key1, w);
  philox4x32_10((uint32_t)n, 3u, 0u, 0u, key0, key1, u);
  const int v = ids[sample_reduce(u[0], (uint32_t)n_ids)];
  const int32_t* idx = (v >= 0 && v < nvol) ? index[v] : nullptr;
  if (!idx) {      // an id outside the set (or a volume without an index): no volume is touched
    if (lane == 0) {
      cand[n] = make_int4(v, 0, 0, 0);
      mode[n] = N3D_SAMPLE_MODE_BAD_ID;
    }
    return;
  }
  const n3d_patch_volume r = vols[v];
  const int D[3] = {r.dims[0], r.dims[1], r.dims[2]};
  const int L = D[0] * D[1], Z = D[2];
  int md = N3D_SAMPLE_MODE_UNIFORM, m = -1;
  if ((uint64_t)u[1] < fg_threshold) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < kMasks; ++i) k += ((masks >> i) & 1) && idx[(int64_t)i * (L + 1) + L] > 0;
    md = N3D_SAMPLE_MODE_FALLBACK;
    if (k > 0) {
      int j = (int)sample_reduce(u[2], (uint32_t)k);
#pragma unroll
      for (int i = 0; i < kMasks; ++i)
        if (((masks >> i) & 1) && idx[(int64_t)i * (L + 1) + L] > 0 && m < 0 && j-- == 0) m = i;
      md = m;
    }
  }
  int vox[3] = {0, 0, 0};
  if (m >= 0) {
    const int32_t* row = idx + (int64_t)m * (L + 1);
    const int32_t rr = (int32_t)sample_reduce(w[0], (uint32_t)row[L]);
    int lo = 0, hi = L;      // row[lo] <= rr < row[hi]
    while (hi - lo > 1) {
      const int mid = (int)(((int64_t)lo + hi) >> 1);
      if (row[mid] <= rr) lo = mid; else hi = mid;
    }
    int kk = rr - row[lo];
    const int64_t XYZ = (int64_t)L * Z, at = (int64_t)lo * Z;
    int zsel = 0;
    for (int base = 0; base < Z; base += 64) {
      const int z = base + lane;
      const uint32_t bit = z < Z ? (sample_mask_bits(r.data, Cv, XYZ, r.truth, at + z) >> m) & 1u : 0u;
      const uint64_t b = __ballot(bit);
      const int c = __popcll(b);
      if (kk < c) {
        const int rank = __popcll(b & ((1ull << lane) - 1ull));
        const uint64_t sel = __ballot(bit && rank == kk);
        zsel = base + __ffsll((unsigned long long)sel) - 1;
        break;
      }
      kk -= c;
    }
    vox[0] = lo / D[1];
    vox[1] = lo - vox[0] * D[1];
    vox[2] = zsel;
  }
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int lo = D[a] >= P ? 0 : -((P - D[a]) / 2), hi = D[a] >= P ? D[a] - P : lo;
    if (m >= 0) {
      const int t = vox[a] - P / 2;
      c[a] = t < lo ? lo : (t > hi ? hi : t);
    } else {
      c[a] = lo + (int)sample_reduce(w[1 + a], (uint32_t)(hi - lo + 1));
    }
  }
  if (lane == 0) {
    cand[n] = make_int4(v, c[0], c[1], c[2]);
    mode[n] = (uint8_t)md;
  }
}

}  // namespace n3d

using namespace n3d;

extern "C" int n3d_volume_line_index(const float* vol, int Cv, const uint8_t* truth, int X, int Y, int Z, int32_t* index, void* stream) {
  N3D_CHECK_ARG(vol && index && Cv >= 1 && X > 0 && Y > 0 && Z > 0, "volume_line_index: bad args");
  N3D_CHECK_ARG((int64_t)X * Y * Z < (1ll << 31), "volume_line_index: X * Y * Z = %lld voxels: the counts need X * Y * Z < 2^31",
                (long long)X * Y * Z);
  hipStream_t s = (hipStream_t)stream;
  const int L = X * Y;
  N3D_LAUNCH(line_count_kernel, dim3((unsigned)cdiv(L, 4)), dim3(256), 0, s, vol, Cv, truth, L, Z, (int64_t)L * Z, index);
  N3D_LAUNCH_CHECK();
  N3D_LAUNCH(line_scan_kernel, dim3(kMasks), dim3(kScanBlock), 0, s, index, L);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_patch_sample(const n3d_patch_volume* vols, const int32_t* const* index, int nvol, int Cv, const int32_t* ids, int n_ids,
                                int64_t N, int P, uint32_t key0, uint32_t key1, uint64_t fg_threshold, int masks, int32_t* cand,
                                uint8_t* mode, void* stream) {
  N3D_CHECK_ARG(N >= 0 && N <= N3D_SAMPLE_MAX, "patch_sample: N = %lld is outside 0 .. 2^24", (long long)N);
  N3D_CHECK_ARG(n_ids >= 1 && P >= 1 && nvol >= 1 && Cv >= 1, "patch_sample: bad args (n_ids, P, nvol and Cv are at least 1)");
  N3D_CHECK_ARG(fg_threshold <= (1ull << 32), "patch_sample: fg_threshold is a probability scaled by 2^32: at most 2^32");
  N3D_CHECK_ARG((masks & ~((1 << kMasks) - 1)) == 0, "patch_sample: masks has bits beyond the %d masks", kMasks);
  N3D_CHECK_ARG(masks != 0 || fg_threshold == 0, "patch_sample: foreground samples need at least one mask");
  if (N == 0) return N3D_OK;
  N3D_CHECK_ARG(vols && index && ids && cand && mode, "patch_sample: a table is NULL");
  N3D_CHECK_ARG(aligned16(cand), "patch_sample: the candidate table must be 16-byte aligned");
  N3D_CHECK_ARG((reinterpret_cast<uintptr_t>(vols) & 7) == 0 && (reinterpret_cast<uintptr_t>(index) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(ids) & 3) == 0,
                "patch_sample: the record and pointer tables must be 8-byte aligned, ids 4-byte aligned");
  N3D_LAUNCH(patch_sample_kernel, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, vols, index, nvol, Cv, ids, n_ids, N, P, key0,
             key1, fg_threshold, masks, reinterpret_cast<int4*>(cand), mode);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}
