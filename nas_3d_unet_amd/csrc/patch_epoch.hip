// The generator's epoch on the device (generator.py:68-217): which of an epoch's candidate patches pass add_data's two filters --
// not all four modalities zero, and (skip_health) not all labels zero (generator.py:202-207).  Instead of reading every candidate
// (the reference crops each one on the host, twice per epoch), each volume gets two summed-area tables once, when it is loaded:
// inclusive 3-D prefix counts of "some channel is nonzero" and "the label is nonzero".  Any box of any size is then answered by
// 8 lookups per table.  Integer index work throughout: exact, order-independent counts, no atomics.
#include "n3d_common.h"

namespace n3d {

// z pass, fused with the indicator test: one wave per (x', y') line of the padded table (X+1, Y+1, Z+1); the plane x' = 0 and
// the row y' = 0 are zeros, entry z' = 0 of every line too.  Lanes along z (coalesced loads of the planar volume); a 64-voxel
// chunk is scanned in the wave with both counts packed in one word (a chunk adds at most 64 per count), then carried on.
__global__ __launch_bounds__(256) void sat_z_kernel(const float* __restrict__ vol, int Cv, const uint8_t* __restrict__ truth, int X, int Y,
                                                    int Z, int2* __restrict__ sat) {
  const int lane = threadIdx.x & 63;
  const int64_t line = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (line >= (int64_t)(X + 1) * (Y + 1)) return;
  const int xp = (int)(line / (Y + 1)), yp = (int)(line % (Y + 1));
  int2* out = sat + line * (Z + 1);
  if (xp == 0 || yp == 0) {
    for (int z = lane; z <= Z; z += 64) out[z] = make_int2(0, 0);
    return;
  }
  if (lane == 0) out[0] = make_int2(0, 0);
  const int64_t XYZ = (int64_t)X * Y * Z;
  const int64_t row = ((int64_t)(xp - 1) * Y + (yp - 1)) * Z;
  int c0 = 0, c1 = 0;   // counts carried in from the chunks before
  for (int base = 0; base < Z; base += 64) {
    const int z = base + lane;
    uint32_t s = 0;
    if (z < Z) {
      int any = 0;
      for (int c = 0; c < Cv; ++c) any |= nonzero_f32(vol[c * XYZ + row + z]);
      s = (uint32_t)any | (truth && truth[row + z] != 0 ? 0x10000u : 0u);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t u = __shfl_up(s, d, 64);
      if (lane >= d) s += u;
    }
    if (z < Z) out[z + 1] = make_int2(c0 + (int)(s & 0xffffu), c1 + (int)(s >> 16));
    const uint32_t tot = __shfl(s, 63, 64);
    c0 += (int)(tot & 0xffffu);
    c1 += (int)(tot >> 16);
  }
}

// running sum along one axis of the padded table: thread = one line, lanes along z' (coalesced); `n` lines of `len` entries at
// `lstride` apart, line (o, z') starting at o * ostride + z'.  Loads go out 8 at a time ahead of the dependent adds.
__global__ __launch_bounds__(256) void sat_scan_kernel(int2* __restrict__ sat, int64_t nlines, int Zp, int64_t ostride, int64_t lstride, int len,
                                                       int first) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nlines) return;
  const int64_t o = t / Zp, zp = t % Zp;
  int2* p = sat + (o + first) * ostride + zp;
  int2 acc = p[0];
  for (int i = 1; i < len; i += 8) {
    int2 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (i + k < len) v[k] = p[(int64_t)(i + k) * lstride];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (i + k < len) {
        acc.x += v[k].x;
        acc.y += v[k].y;
        p[(int64_t)(i + k) * lstride] = acc;
      }
  }
}

// one thread per candidate (grid-stride): clip [c, c + P) to the volume, then inclusion-exclusion on the 8 corners of the box
// in the padded table (entry i counts the voxels < i, so the box [lo, hi) is T[hi] - T[lo] over every axis).  Sums in uint32:
// the true counts are < 2^31, so the wrap-around terms cancel exactly.
__global__ __launch_bounds__(256) void patch_qualify_kernel(const n3d_patch_volume* __restrict__ vols, int nvol, const int4* __restrict__ cand,
                                                            int64_t N, int P, uint8_t* __restrict__ flags) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const int4 c = cand[i];
    uint8_t f = 0;
    if (c.x >= 0 && c.x < nvol) {
      const n3d_patch_volume r = vols[c.x];
      const int cc[3] = {c.y, c.z, c.w};
      int64_t lo[3], hi[3];
      bool empty = false;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = cc[a] < 0 ? 0 : (int64_t)cc[a];
        hi[a] = (int64_t)cc[a] + P;
        if (hi[a] > r.dims[a]) hi[a] = r.dims[a];
        empty |= hi[a] <= lo[a];
      }
      if (!empty) {
        const int64_t sy = (int64_t)r.dims[2] + 1, sx = ((int64_t)r.dims[1] + 1) * sy;
        const int2* T = reinterpret_cast<const int2*>(r.sat);
        uint32_t s0 = 0, s1 = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int64_t ix = (k & 4) ? hi[0] : lo[0], iy = (k & 2) ? hi[1] : lo[1], iz = (k & 1) ? hi[2] : lo[2];
          const int2 e = T[ix * sx + iy * sy + iz];
          // + for an even number of `lo` coordinates, i.e. (3 axes) an odd number of `hi` bits in k
          if (__builtin_popcount(k) & 1) { s0 += (uint32_t)e.x; s1 += (uint32_t)e.y; }
          else { s0 -= (uint32_t)e.x; s1 -= (uint32_t)e.y; }
        }
        f = (uint8_t)((s0 != 0) | ((s1 != 0) << 1));
      }
    }
    flags[i] = f;
  }
}

}  // namespace n3d

using namespace n3d;

extern "C" int n3d_volume_sat(const float* vol, int Cv, const uint8_t* truth, int X, int Y, int Z, int32_t* sat, void* stream) {
  N3D_CHECK_ARG(vol && sat && Cv >= 1 && X > 0 && Y > 0 && Z > 0, "volume_sat: bad args");
  N3D_CHECK_ARG((int64_t)X * Y * Z < (1ll << 31), "volume_sat: X * Y * Z = %lld voxels: the counts need X * Y * Z < 2^31",
                (long long)X * Y * Z);
  hipStream_t s = (hipStream_t)stream;
  int2* T = reinterpret_cast<int2*>(sat);
  const int64_t lines = (int64_t)(X + 1) * (Y + 1);
  N3D_LAUNCH(sat_z_kernel, dim3((unsigned)cdiv(lines, 4)), dim3(256), 0, s, vol, Cv, truth, X, Y, Z, T);
  N3D_LAUNCH_CHECK();
  const int64_t Zp = Z + 1, Yp = Y + 1;
  // y pass: lines (x' >= 1, z'), running along y' (stride Z+1); x pass: lines (y', z'), running along x' (stride (Y+1)(Z+1))
  const int64_t ny = (int64_t)X * Zp;
  N3D_LAUNCH(sat_scan_kernel, dim3((unsigned)cdiv(ny, 256)), dim3(256), 0, s, T, ny, (int)Zp, Yp * Zp, Zp, Y + 1, 1);
  N3D_LAUNCH_CHECK();
  const int64_t nx = Yp * Zp;
  N3D_LAUNCH(sat_scan_kernel, dim3((unsigned)cdiv(nx, 256)), dim3(256), 0, s, T, nx, (int)Zp, Zp, Yp * Zp, X + 1, 0);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}

extern "C" int n3d_patch_qualify(const n3d_patch_volume* vols, int nvol, const int32_t* cand, int64_t N, int P, uint8_t* flags, void* stream) {
  N3D_CHECK_ARG(N >= 0 && nvol >= 0 && P > 0, "patch_qualify: bad args");
  if (N == 0) return N3D_OK;
  N3D_CHECK_ARG(cand && flags && (vols || nvol == 0), "patch_qualify: bad args");
  N3D_CHECK_ARG((reinterpret_cast<uintptr_t>(cand) & 15) == 0, "patch_qualify: the candidate table must be 16-byte aligned");
  const int64_t blocks = cdiv(N, 256) < 8192 ? cdiv(N, 256) : 8192;
  N3D_LAUNCH(patch_qualify_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, vols, nvol,
                     reinterpret_cast<const int4*>(cand), N, P, flags);
  N3D_LAUNCH_CHECK();
  return N3D_OK;
}
