// Deterministic mode (`deterministic = true`): atomic-free forms of the train step's scatter adjoints and of the two reductions
// of the layer-by-layer plan's ends.  Every sum here runs in an order fixed by shapes and launch geometry alone; the only
// atomics are INTEGER ones (counters / cursors), whose result does not depend on arrival order.
//   nlt_warp_backward_det              resampler adjoint: count -> scan -> fill -> ordered reduce (a CSR of contributions per texel)
//   nlt_resize_bilinear_backward_gather  bilinear-resize adjoint, one thread per input element walking its outputs in ascending order
//   nlt_stem_backward_det / nlt_head_backward_det   per-thread partials -> LDS rows -> workgroup rows in a workspace -> ordered sum
// Built with -ffp-contract=off (csrc/Makefile): a term such as wt * g is rounded before it is added, as the float atomics of
// csrc/train_ops.hip add it.
#include "nlt_common.h"

namespace {

inline unsigned blocks_for(long total) { return (unsigned)((total + 255) / 256); }

// ---------------------------------------------------------------------------------------------------- resampler adjoint
// One contribution = (camera pixel p, corner) with corner = 2 * row + right: 0 (fx,fy), 1 (cx,fy), 2 (fx,cy), 3 (cx,cy).
// Texel and weight are formed exactly as warp_bwd_kernel (csrc/train_ops.hip) forms them; false = that kernel skips it.
__device__ __forceinline__ bool warp_corner(const float* __restrict__ warp, long p, int corner, int uvh, int uvw, int hcwc,
                                            long* tex, float* wt) {
  const int f = (int)(p / hcwc);
  const float x = warp[p * 2 + 0] * (float)uvw;
  const float y = warp[p * 2 + 1] * (float)uvh;
  if (!(x > -1.f && y > -1.f && x < (float)uvw && y < (float)uvh)) return false;
  const int fx = (int)floorf(x), fy = (int)floorf(y);
  const int cx = fx + 1, cy = fy + 1;
  const float dx = (float)cx - x, dy = (float)cy - y;
  const int right = corner & 1, r = corner >> 1;
  const float wx = right ? 1.f - dx : dx;
  const int xi = fx + right;
  if (xi < 0 || xi > uvw - 1) return false;
  const int yi = r ? cy : fy;
  const float w = wx * (r ? 1.f - dy : dy);
  if (yi < 0 || yi > uvh - 1 || (xi == 0 && yi == 0) || w == 0.f) return false;
  *tex = ((long)f * uvh + yi) * uvw + xi;
  *wt = w;
  return true;
}

// (a) count: cnt[texel] += 1 per contribution
__global__ __launch_bounds__(256) void warp_det_count_kernel(const float* __restrict__ warp, int uvh, int uvw, int hcwc, long total4,
                                                             int* cnt) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  long tex; float wt;
  if (warp_corner(warp, i >> 2, (int)(i & 3), uvh, uvw, hcwc, &tex, &wt)) atomicAdd(cnt + tex, 1);
}

// (b) exclusive scan of the counters in three plain launches: per-chunk sums, one workgroup over the chunk sums, per-chunk rescan
constexpr int SCAN_PER_THREAD = 8;
constexpr int SCAN_CHUNK = 256 * SCAN_PER_THREAD;

// inclusive scan of one value per thread over the workgroup (Hillis-Steele in LDS); returns the inclusive prefix
__device__ __forceinline__ int block_scan_inclusive(int v, int* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int add = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
    __syncthreads();
    sh[threadIdx.x] += add;
    __syncthreads();
  }
  const int r = sh[threadIdx.x];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void scan_chunk_sums_kernel(const int* __restrict__ cnt, long count, int* chunk_sum) {
  __shared__ int sh[256];
  const long base = (long)blockIdx.x * SCAN_CHUNK + (long)threadIdx.x * SCAN_PER_THREAD;
  int s = 0;
#pragma unroll
  for (int j = 0; j < SCAN_PER_THREAD; ++j) s += base + j < count ? cnt[base + j] : 0;
  const int incl = block_scan_inclusive(s, sh);
  if (threadIdx.x == 255) chunk_sum[blockIdx.x] = incl;
}

// chunk_sum[i] <- exclusive prefix; chunk_sum[chunks] <- total.  One workgroup, 256 chunk sums per step with a carry.
__global__ __launch_bounds__(256) void scan_chunk_offsets_kernel(int* chunk_sum, int chunks) {
  __shared__ int sh[256];
  __shared__ int carry_sh;
  if (threadIdx.x == 0) carry_sh = 0;
  __syncthreads();
  for (int base = 0; base < chunks; base += 256) {
    const int i = base + (int)threadIdx.x;
    const int v = i < chunks ? chunk_sum[i] : 0;
    const int incl = block_scan_inclusive(v, sh);
    const int carry = carry_sh;
    if (i < chunks) chunk_sum[i] = carry + incl - v;
    __syncthreads();
    if (threadIdx.x == 255) carry_sh = carry + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) chunk_sum[chunks] = carry_sh;
}

__global__ __launch_bounds__(256) void scan_downsweep_kernel(const int* __restrict__ cnt, long count, const int* __restrict__ chunk_sum,
                                                             int chunks, int* off) {
  __shared__ int sh[256];
  const long base = (long)blockIdx.x * SCAN_CHUNK + (long)threadIdx.x * SCAN_PER_THREAD;
  int v[SCAN_PER_THREAD];
  int s = 0;
#pragma unroll
  for (int j = 0; j < SCAN_PER_THREAD; ++j) { v[j] = base + j < count ? cnt[base + j] : 0; s += v[j]; }
  const int incl = block_scan_inclusive(s, sh);
  int run = chunk_sum[blockIdx.x] + incl - s;
#pragma unroll
  for (int j = 0; j < SCAN_PER_THREAD; ++j) {
    if (base + j < count) off[base + j] = run;
    run += v[j];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) off[count] = chunk_sum[chunks];
}

// (c) fill: the contribution takes a slot of its texel's segment through the (now falling) counter; the slot order is arbitrary
__global__ __launch_bounds__(256) void warp_det_fill_kernel(const float* __restrict__ warp, int uvh, int uvw, int hcwc, long total4,
                                                            int* cnt, const int* __restrict__ off, int* keys) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  long tex; float wt;
  if (!warp_corner(warp, i >> 2, (int)(i & 3), uvh, uvw, hcwc, &tex, &wt)) return;
  const int slot = off[tex] + atomicSub(cnt + tex, 1) - 1;
  keys[slot] = (int)i;                                  // key = pixel * 4 + corner
}

constexpr int WARP_DET_SHORT = 32;

// (d) reduce: one lane per texel.  Keys ascending = camera pixels in raster order, corners 0..3 inside a pixel.  A short segment
// is walked by repeated selection of the next larger key (segments are ~1 long on chart maps); a long one goes on a list.
__global__ __launch_bounds__(256) void warp_det_reduce_kernel(const float* __restrict__ dcam, const float* __restrict__ warp,
                                                              int uvh, int uvw, int hcwc, long texels,
                                                              const int* __restrict__ off, const int* __restrict__ keys,
                                                              int* long_count, int* long_list, int long_cap, float* dpred) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= texels) return;
  const int b = off[t], L = off[t + 1] - b;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  if (L > WARP_DET_SHORT) {
    const int slot = atomicAdd(long_count, 1);
    if (slot < long_cap) long_list[slot] = (int)t;      // (long_cap bounds every possible count: see the workspace layout)
    return;                                             // the second launch writes this texel
  }
  int last = -1;
  for (int i = 0; i < L; ++i) {
    int best = 0x7fffffff;
    for (int j = 0; j < L; ++j) {
      const int k = keys[b + j];
      if (k > last && k < best) best = k;
    }
    last = best;
    long tex; float wt;
    const long p = best >> 2;
    warp_corner(warp, p, best & 3, uvh, uvw, hcwc, &tex, &wt);
    s0 += wt * dcam[p * 3 + 0];
    s1 += wt * dcam[p * 3 + 1];
    s2 += wt * dcam[p * 3 + 2];
  }
  dpred[t * 3 + 0] = s0; dpred[t * 3 + 1] = s1; dpred[t * 3 + 2] = s2;
}

// long segments: workgroups stride over the list; each sorts its segment by rank (keys are distinct: rank = number of smaller
// keys, L^2 / 256 comparisons per thread) into `sorted`, then one thread per channel adds in that order
__global__ __launch_bounds__(256) void warp_det_long_kernel(const float* __restrict__ dcam, const float* __restrict__ warp,
                                                            int uvh, int uvw, int hcwc, const int* __restrict__ off,
                                                            const int* __restrict__ keys, int* sorted,
                                                            const int* __restrict__ long_count, const int* __restrict__ long_list,
                                                            int long_cap, float* dpred) {
  int n_long = *long_count;
  if (n_long > long_cap) n_long = long_cap;
  for (int seg = blockIdx.x; seg < n_long; seg += gridDim.x) {
    const long t = long_list[seg];
    const int b = off[t], L = off[t + 1] - b;
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
      const int k = keys[b + i];
      int rank = 0;
      for (int j = 0; j < L; ++j) rank += keys[b + j] < k ? 1 : 0;
      sorted[b + rank] = k;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      const int ch = threadIdx.x;
      float s = 0.f;
      for (int i = 0; i < L; ++i) {
        const int k = sorted[b + i];
        long tex; float wt;
        const long p = k >> 2;
        warp_corner(warp, p, k & 3, uvh, uvw, hcwc, &tex, &wt);
        s += wt * dcam[p * 3 + ch];
      }
      dpred[t * 3 + ch] = s;
    }
    __syncthreads();
  }
}

// workspace layout in ints: cnt[T] long_count[1] | off[T + 1] | chunk_sum[chunks + 1] | keys[4P] | sorted[4P] | long_list[cap]
struct WarpDetLayout { long T, P4, chunks, cap, cnt, off, chunk_sum, keys, sorted, long_list, total; };

bool warp_det_layout(int n, int uvh, int uvw, int hc, int wc, WarpDetLayout* L) {
  if (n <= 0 || uvh <= 0 || uvw <= 0 || hc <= 0 || wc <= 0) return false;
  const long T = (long)n * uvh * uvw, P = (long)n * hc * wc;
  if (P >= (1l << 29) || T >= (1l << 30)) return false;          // keys (pixel * 4 + corner) and offsets are int32
  L->T = T; L->P4 = 4 * P;
  L->chunks = (T + SCAN_CHUNK - 1) / SCAN_CHUNK;
  const long by_len = 4 * P / (WARP_DET_SHORT + 1) + 1;           // a long segment holds > WARP_DET_SHORT of the 4P contributions
  L->cap = by_len < T ? by_len : T;
  long o = 0;
  L->cnt = o; o += T + 1;
  L->off = o; o += T + 1;
  L->chunk_sum = o; o += L->chunks + 1;
  L->keys = o; o += 4 * P;
  L->sorted = o; o += 4 * P;
  L->long_list = o; o += L->cap;
  L->total = o;
  return true;
}

// ------------------------------------------------------------------------------------------------------ resize adjoint
// dx[f,y,x,ch] = sum over the outputs (oy, ox), ascending, whose footprint {ylo,yhi} x {xlo,xhi} holds (y, x), of the taps of
// resize_bwd_kernel (csrc/train_ops.hip) that address it, in that kernel's statement order.  The candidate range per axis is a
// generous estimate; membership is decided by the adjoint's own expressions.
__device__ __forceinline__ void resize_axis(int o, float scale, int size, int* lo, int* hi, float* l) {
  const float src = ((float)o + 0.5f) * scale - 0.5f;
  const float fl = floorf(src);
  *lo = max((int)fl, 0);
  *hi = min((int)ceilf(src), size - 1);
  *l = src - fl;
}

__device__ __forceinline__ void resize_candidates(int i, float scale, int osize, int* a, int* b) {
  const float lo = ((float)i - 0.5f) / scale - 0.5f, hi = ((float)i + 1.5f) / scale - 0.5f;
  int ia = (int)floorf(lo) - 1, ib = (int)ceilf(hi) + 1;
  *a = ia < 0 ? 0 : ia;
  *b = ib > osize - 1 ? osize - 1 : ib;
}

__global__ __launch_bounds__(256) void resize_bwd_gather_kernel(const float* __restrict__ dout, int h, int w, int c, int oh, int ow,
                                                                long total, float* __restrict__ dx) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int ch = idx % c;
  const int x = (idx / c) % w;
  const int y = (idx / ((long)c * w)) % h;
  const long f = idx / ((long)c * w * h);
  const float sy = (float)h / (float)oh, sx = (float)w / (float)ow;
  int oy0, oy1, ox0, ox1;
  resize_candidates(y, sy, oh, &oy0, &oy1);
  resize_candidates(x, sx, ow, &ox0, &ox1);
  float s = 0.f;
  for (int oy = oy0; oy <= oy1; ++oy) {
    int ylo, yhi; float ly;
    resize_axis(oy, sy, h, &ylo, &yhi, &ly);
    if (ylo != y && yhi != y) continue;
    for (int ox = ox0; ox <= ox1; ++ox) {
      int xlo, xhi; float lx;
      resize_axis(ox, sx, w, &xlo, &xhi, &lx);
      if (xlo != x && xhi != x) continue;
      const float g = dout[((f * oh + oy) * ow + ox) * c + ch];
      if (ylo == y && xlo == x) s += (1.f - ly) * (1.f - lx) * g;
      if (ylo == y && xhi == x) s += (1.f - ly) * lx * g;
      if (yhi == y && xlo == x) s += ly * (1.f - lx) * g;
      if (yhi == y && xhi == x) s += ly * lx * g;
    }
  }
  dx[idx] = s;
}

// -------------------------------------------------------------------------------------------- stem / head weight gradients
// Same per-term arithmetic as stem_bwd_kernel / head_bwd_kernel (csrc/train_ops.hip).  Each thread's register partials go to
// its own LDS row; the rows are added in texel-lane order into one row per workgroup in the workspace; a second launch adds the
// workgroup rows in workgroup order into the gradient.
__global__ __launch_bounds__(256) void stem_bwd_det_kernel(
    const float* __restrict__ base, const float* __restrict__ cvis, const float* __restrict__ lvis,
    const float* __restrict__ nn_rgb, const float* __restrict__ nn_base, const float* __restrict__ obs_w,
    int k, int hw, int c, long texels, const float* __restrict__ dfm0, const float* __restrict__ dobs0, float* ws) {
  extern __shared__ __attribute__((aligned(16))) float part[];   // [tpb][10 rows][c]: wq 5, bq 1, wo 3, bo 1
  const int quads = c >> 2;
  const int tpb = blockDim.x / quads;
  const int tl = threadIdx.x / quads, q = threadIdx.x % quads;
  const int row = 10 * c;
  if (tl < tpb) {
    const int co = 4 * q;
    f32x4 aq[6], ao[4];
#pragma unroll
    for (int j = 0; j < 6; ++j) aq[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) ao[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (long tex = (long)blockIdx.x * tpb + tl; tex < texels; tex += (long)gridDim.x * tpb) {
      const int f = tex / hw;
      const long pix = tex - (long)f * hw;
      const f32x4 gq = *reinterpret_cast<const f32x4*>(dfm0 + tex * 2 * c + co);
      const f32x4 gm = *reinterpret_cast<const f32x4*>(dfm0 + tex * 2 * c + c + co) * (1.f / (float)k);
      aq[0] += base[tex * 3 + 0] * gq; aq[1] += base[tex * 3 + 1] * gq; aq[2] += base[tex * 3 + 2] * gq;
      aq[3] += cvis[tex] * gq; aq[4] += lvis[tex] * gq; aq[5] += gq;
      for (int i = 0; i < k; ++i) {
        const long ot = ((long)f * k + i) * hw + pix;
        f32x4 g = obs_w ? obs_w[f * k + i] * gm : gm;
        if (dobs0) g += *reinterpret_cast<const f32x4*>(dobs0 + ot * c + co);
        ao[0] += (nn_rgb[ot * 3 + 0] - nn_base[ot * 3 + 0]) * g;
        ao[1] += (nn_rgb[ot * 3 + 1] - nn_base[ot * 3 + 1]) * g;
        ao[2] += (nn_rgb[ot * 3 + 2] - nn_base[ot * 3 + 2]) * g;
        ao[3] += g;
      }
    }
    float* mine = part + (long)tl * row;
#pragma unroll
    for (int j = 0; j < 6; ++j) *reinterpret_cast<f32x4*>(mine + j * c + co) = aq[j];
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(mine + (6 + j) * c + co) = ao[j];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < row; i += blockDim.x) {
    float s = 0.f;
    for (int t = 0; t < tpb; ++t) s += part[(long)t * row + i];
    ws[(long)blockIdx.x * row + i] = s;
  }
}

__global__ __launch_bounds__(256) void stem_bwd_det_finish_kernel(const float* __restrict__ ws, int blocks, int c, float* dwq,
                                                                  float* dbq, float* dwo, float* dbo) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 10 * c) return;
  float s = 0.f;
  for (int b = 0; b < blocks; ++b) s += ws[(long)b * 10 * c + i];
  const int row = i / c, col = i - row * c;
  float* dst = row < 5 ? dwq + row * c + col : row == 5 ? dbq + col : row < 9 ? dwo + (row - 6) * c + col : dbo + col;
  *dst += s;
}

__global__ __launch_bounds__(256) void head_bwd_det_kernel(const float* __restrict__ dec, int ldd, int cd,
                                                           const float* __restrict__ skip, int lds, int cs,
                                                           const float* __restrict__ wk, const float* __restrict__ dpred,
                                                           int hw, long texels, float* __restrict__ d_dec, int ldgd,
                                                           float* __restrict__ d_skip, int ldgs, float* ws) {
  extern __shared__ __attribute__((aligned(16))) float part[];   // [tpb][cin*3 + 3]
  const int cin = cd + cs;
  const int quads = cin >> 2;
  const int tpb = blockDim.x / quads;
  const int tl = threadIdx.x / quads, q = threadIdx.x % quads;
  const int row = cin * 3 + 3;
  if (tl < tpb) {
    const int c0 = 4 * q;
    const bool from_dec = c0 < cd;
    float wr[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int o = 0; o < 3; ++o) wr[j][o] = wk[(c0 + j) * 3 + o];
    float aw[4][3] = {{0.f}};
    float ab[3] = {0.f, 0.f, 0.f};
    for (long tex = (long)blockIdx.x * tpb + tl; tex < texels; tex += (long)gridDim.x * tpb) {
      float g[3] = {dpred[tex * 3 + 0], dpred[tex * 3 + 1], dpred[tex * 3 + 2]};
      if (tex % hw == 0) { g[0] = 0.f; g[1] = 0.f; g[2] = 0.f; }       // d(set_left_top_corner)
      const float* xp = from_dec ? dec + tex * ldd + c0 : skip + tex * lds + (c0 - cd);
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xp);
      f32x4 dx;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dx[j] = g[0] * wr[j][0] + g[1] * wr[j][1] + g[2] * wr[j][2];
#pragma unroll
        for (int o = 0; o < 3; ++o) aw[j][o] += xv[j] * g[o];
      }
      float* dp = from_dec ? d_dec + tex * ldgd + c0 : d_skip + tex * ldgs + (c0 - cd);
      *reinterpret_cast<f32x4*>(dp) = dx;
      if (q == 0) { ab[0] += g[0]; ab[1] += g[1]; ab[2] += g[2]; }
    }
    float* mine = part + (long)tl * row;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int o = 0; o < 3; ++o) mine[(c0 + j) * 3 + o] = aw[j][o];
    if (q == 0)
#pragma unroll
      for (int o = 0; o < 3; ++o) mine[cin * 3 + o] = ab[o];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < row; i += blockDim.x) {
    float s = 0.f;
    for (int t = 0; t < tpb; ++t) s += part[(long)t * row + i];
    ws[(long)blockIdx.x * row + i] = s;
  }
}

__global__ __launch_bounds__(256) void head_bwd_det_finish_kernel(const float* __restrict__ ws, int blocks, int cin, float* dw,
                                                                  float* db) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int row = cin * 3 + 3;
  if (i >= row) return;
  float s = 0.f;
  for (int b = 0; b < blocks; ++b) s += ws[(long)b * row + i];
  if (i < cin * 3) dw[i] += s; else db[i - cin * 3] += s;
}

constexpr int STEM_DET_BLOCKS = 1024, HEAD_DET_BLOCKS = 1024;

long stem_det_blocks(long texels, int c) {
  const int tpb = 256 / (c >> 2);
  long blocks = (texels + tpb - 1) / tpb;
  return blocks > STEM_DET_BLOCKS ? STEM_DET_BLOCKS : blocks;
}

long head_det_blocks(long texels, int cin) {
  const int tpb = 256 / (cin >> 2);
  long blocks = (texels + tpb - 1) / tpb;
  return blocks > HEAD_DET_BLOCKS ? HEAD_DET_BLOCKS : blocks;
}

}  // namespace

extern "C" long nlt_warp_backward_det_workspace_bytes(int n, int uvh, int uvw, int hc, int wc) {
  WarpDetLayout L;
  if (!warp_det_layout(n, uvh, uvw, hc, wc, &L)) return -1;
  return L.total * (long)sizeof(int);
}

extern "C" int nlt_warp_backward_det(const float* dpred_cam, const float* warp, int n, int uvh, int uvw, int hc, int wc,
                                     float* dpred, void* workspace, long workspace_bytes, void* stream) {
  if (!dpred_cam || !warp || !dpred || !workspace || n <= 0 || uvh <= 0 || uvw <= 0 || hc <= 0 || wc <= 0) return NLT_ERR_BAD_ARG;
  WarpDetLayout L;
  if (!warp_det_layout(n, uvh, uvw, hc, wc, &L)) return NLT_ERR_UNSUPPORTED;
  if (workspace_bytes < L.total * (long)sizeof(int) || (reinterpret_cast<uintptr_t>(workspace) & 3u)) return NLT_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int* ws = static_cast<int*>(workspace);
  int *cnt = ws + L.cnt, *off = ws + L.off, *chunk_sum = ws + L.chunk_sum, *keys = ws + L.keys, *sorted = ws + L.sorted;
  int *long_list = ws + L.long_list, *long_count = cnt + L.T;
  if (hipMemsetAsync(cnt, 0, (size_t)(L.T + 1) * sizeof(int), s) != hipSuccess) return NLT_ERR_LAUNCH;
  const int hcwc = hc * wc;
  hipLaunchKernelGGL(warp_det_count_kernel, dim3(blocks_for(L.P4)), dim3(256), 0, s, warp, uvh, uvw, hcwc, L.P4, cnt);
  hipLaunchKernelGGL(scan_chunk_sums_kernel, dim3((unsigned)L.chunks), dim3(256), 0, s, cnt, L.T, chunk_sum);
  hipLaunchKernelGGL(scan_chunk_offsets_kernel, dim3(1), dim3(256), 0, s, chunk_sum, (int)L.chunks);
  hipLaunchKernelGGL(scan_downsweep_kernel, dim3((unsigned)L.chunks), dim3(256), 0, s, cnt, L.T, chunk_sum, (int)L.chunks, off);
  hipLaunchKernelGGL(warp_det_fill_kernel, dim3(blocks_for(L.P4)), dim3(256), 0, s, warp, uvh, uvw, hcwc, L.P4, cnt, off, keys);
  hipLaunchKernelGGL(warp_det_reduce_kernel, dim3(blocks_for(L.T)), dim3(256), 0, s, dpred_cam, warp, uvh, uvw, hcwc, L.T, off,
                     keys, long_count, long_list, (int)L.cap, dpred);
  const unsigned long_blocks = (unsigned)(L.cap < 1024 ? L.cap : 1024);
  hipLaunchKernelGGL(warp_det_long_kernel, dim3(long_blocks), dim3(256), 0, s, dpred_cam, warp, uvh, uvw, hcwc, off, keys, sorted,
                     long_count, long_list, (int)L.cap, dpred);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_resize_bilinear_backward_gather(const float* dout, int n, int h, int w, int c, int oh, int ow, float* dx,
                                                   void* stream) {
  if (!dout || !dx || n <= 0 || h <= 0 || w <= 0 || c <= 0 || oh <= 0 || ow <= 0) return NLT_ERR_BAD_ARG;
  const long total = (long)n * h * w * c;
  if ((total + 255) / 256 >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(resize_bwd_gather_kernel, dim3(blocks_for(total)), dim3(256), 0, static_cast<hipStream_t>(stream), dout, h, w,
                     c, oh, ow, total, dx);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" long nlt_stem_backward_det_workspace_floats(int n, int h, int w, int c) {
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || (c & 3) || c > 64) return -1;
  return stem_det_blocks((long)n * h * w, c) * 10 * c;
}

extern "C" int nlt_stem_backward_det(const float* base, const float* cvis, const float* lvis, const float* nn_rgb,
                                     const float* nn_base, const float* obs_weights, int n, int k, int h, int w, int c,
                                     const float* dfm0, const float* dobs0_partial,
                                     float* dwq, float* dbq, float* dwo, float* dbo, float* workspace, long workspace_floats,
                                     void* stream) {
  if (!base || !cvis || !lvis || !nn_rgb || !nn_base || !dfm0 || !dwq || !dbq || !dwo || !dbo || !workspace) return NLT_ERR_BAD_ARG;
  if (n <= 0 || k <= 0 || h <= 0 || w <= 0 || c <= 0) return NLT_ERR_BAD_ARG;
  if ((c & 3) || c > 64) return NLT_ERR_UNSUPPORTED;
  if (!nlt_aligned16(dfm0) || (dobs0_partial && !nlt_aligned16(dobs0_partial))) return NLT_ERR_BAD_ARG;
  const long texels = (long)n * h * w;
  const long blocks = stem_det_blocks(texels, c);
  if (workspace_floats < blocks * 10 * c) return NLT_ERR_BAD_ARG;
  const int tpb = 256 / (c >> 2);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(stem_bwd_det_kernel, dim3((unsigned)blocks), dim3(256), (size_t)tpb * 10 * c * sizeof(float), s,
                     base, cvis, lvis, nn_rgb, nn_base, obs_weights, k, h * w, c, texels, dfm0, dobs0_partial, workspace);
  hipLaunchKernelGGL(stem_bwd_det_finish_kernel, dim3(blocks_for(10 * c)), dim3(256), 0, s, workspace, (int)blocks, c, dwq, dbq,
                     dwo, dbo);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" long nlt_head_backward_det_workspace_floats(int n, int h, int w, int cd, int cs) {
  if (n <= 0 || h <= 0 || w <= 0 || cd <= 0 || cs < 0 || (cd & 3) || (cs & 3) || cd + cs > 256) return -1;
  return head_det_blocks((long)n * h * w, cd + cs) * ((cd + cs) * 3 + 3);
}

extern "C" int nlt_head_backward_det(const float* dec, int ldd, int cd, const float* skip, int lds, int cs,
                                     const float* w_keras, const float* dpred, int n, int h, int w,
                                     float* d_dec, int ldgd, float* d_skip, int ldgs, float* dw, float* db,
                                     float* workspace, long workspace_floats, void* stream) {
  if (!dec || !w_keras || !dpred || !d_dec || !dw || !db || !workspace || n <= 0 || h <= 0 || w <= 0 || cd <= 0 || cs < 0)
    return NLT_ERR_BAD_ARG;
  if (cs > 0 && (!skip || !d_skip)) return NLT_ERR_BAD_ARG;
  if ((cd & 3) || (cs & 3) || (ldd & 3) || (ldgd & 3) || (cs > 0 && ((lds & 3) || (ldgs & 3)))) return NLT_ERR_UNSUPPORTED;
  if (cd + cs > 256) return NLT_ERR_UNSUPPORTED;
  const long texels = (long)n * h * w;
  const int cin = cd + cs;
  const long blocks = head_det_blocks(texels, cin);
  const int row = cin * 3 + 3;
  if (workspace_floats < blocks * row) return NLT_ERR_BAD_ARG;
  const int tpb = 256 / (cin >> 2);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(head_bwd_det_kernel, dim3((unsigned)blocks), dim3(256), (size_t)tpb * row * sizeof(float), s, dec, ldd, cd,
                     skip, lds, cs, w_keras, dpred, h * w, texels, d_dec, ldgd, d_skip, ldgs, workspace);
  hipLaunchKernelGGL(head_bwd_det_finish_kernel, dim3(blocks_for(row)), dim3(256), 0, s, workspace, (int)blocks, cin, dw, db);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}
