// Shared by the kernels that tile the half-resolution grid 8 x 16 per 256-thread workgroup: the fused front and back kernels
// (fused.hip), the expanding blocks (dec_block.hip) and the backward of the last block (train_back.hip, geometry only: it walks
// its tiles persistently).  Also the fixed-order reduction over workgroup rows that both fused backward files end with
// (train_back.hip, train_fused.hip).
#pragma once
#include "nlt_common.h"

namespace {

constexpr int TH = 8, TW = 16;             // input-resolution tile owned by one workgroup
constexpr int HH = TH + 1, HW = TW + 1;    // with the 1-texel halo the stride-1 conv needs
constexpr int HT = HH * HW;                // 153 haloed texels
constexpr int NT = (HT + 15) / 16;         // 10 MFMA column tiles
constexpr int FH = 2 * TH + 1, FW = 2 * TW + 1;   // the tile at twice the resolution incl. its 1-texel halo: 17 x 33

__device__ __forceinline__ f32x4 lrelu4(f32x4 v, float alpha) {
  return (f32x4){v[0] > 0.f ? v[0] : alpha * v[0], v[1] > 0.f ? v[1] : alpha * v[1],
                 v[2] > 0.f ? v[2] : alpha * v[2], v[3] > 0.f ? v[3] : alpha * v[3]};
}

// XCD-aware tile order: the dispatcher places workgroup b on XCD b % 8; give each XCD a contiguous run
// of tiles so that neighbouring tiles (which share halo lines) meet in the same L2.
__device__ __forceinline__ int xcd_tile(int b, int nblocks) {
  return (nblocks & 7) ? b : (b & 7) * (nblocks >> 3) + (b >> 3);
}

// this workgroup's tile: first texel (ty0, tx0) of frame f
struct TileAt {
  int tx0, ty0, f;
  __device__ __forceinline__ TileAt(int tiles_y, int tiles_x) {
    int t = xcd_tile(blockIdx.x, gridDim.x);
    tx0 = (t % tiles_x) * TW; t /= tiles_x;
    ty0 = (t % tiles_y) * TH;
    f = t / tiles_y;
  }
};

// Texel t = 16 mt + j of the haloed tile, flattened into MFMA column tiles.  HALO = -1: the halo is above / left (the
// transposed stride-1 conv reads (y - a, x - b)); 0: below / right.  Not live: padding of the last column tile; not inside:
// beyond the image (the stride-1 conv's zero padding).
template <int HALO>
struct HaloTexel {
  int t, hy, hx, gy, gx;
  bool live, inside;
  __device__ __forceinline__ HaloTexel(int mt, int j, int ty0, int tx0, int h, int w) {
    t = mt * 16 + j;
    live = t < HT;
    hy = live ? t / HW : 0; hx = live ? t % HW : 0;
    gy = ty0 + HALO + hy; gx = tx0 + HALO + hx;
    inside = live && (HALO == 0 || (gy >= 0 && gx >= 0)) && gy < h && gx < w;
  }
  // whether the k2s2 transposed conv's output sub-texel ab = (a, b) of this texel lands in the FH x FW tile, and in which slot
  __device__ __forceinline__ bool scatter(int ab, int& slot) const {
    static_assert(HALO == -1, "the doubled tile has its halo above / left");
    const int ly = 2 * hy + (ab >> 1) - 1, lx = 2 * hx + (ab & 1) - 1;
    slot = ly * FW + lx;
    return live && ly >= 0 && lx >= 0;
  }
};

// Entry idx summed over the nrows rows (len floats each) of a workspace of per-workgroup partial sums, in a fixed order: 256
// threads = 16 entries (threadIdx.x & 15) x 16 row groups x 4 running sums (a serial walk over ~1000 rows is pure load latency),
// then (s0 + s1) + (s2 + s3), then the 16 groups in order.  The total is returned to row group 0; the others get 0.
__device__ __forceinline__ float ordered_row_sum(const float* __restrict__ ws, int nrows, int len, int idx, float (&part)[16][17]) {
  const int e = threadIdx.x & 15, g = threadIdx.x >> 4;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int bl = g;
  for (; bl + 48 < nrows; bl += 64) {
    s0 += ws[(long)bl * len + idx];
    s1 += ws[(long)(bl + 16) * len + idx];
    s2 += ws[(long)(bl + 32) * len + idx];
    s3 += ws[(long)(bl + 48) * len + idx];
  }
  for (; bl < nrows; bl += 16) s0 += ws[(long)bl * len + idx];
  part[g][e] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (g) return 0.f;
  float t = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) t += part[q][e];
  return t;
}

}  // namespace
