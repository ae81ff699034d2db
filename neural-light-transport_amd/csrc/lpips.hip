// LPIPS v0.1 "alex / lin" (Zhang et al. 2018): the per-image perceptual distance and its gradient w.r.t. the prediction.
//   replaces: nlt/losses.py:121-169 (losses.LPIPS running third_party/lpips/net-lin_alex_v0.1.pb) and
//             third_party/xiuminglib/xiuminglib/metric.py:187-258 (xm.metric.LPIPS)
// Exact fp32 throughout, NHWC, Keras weight arrays (kh,kw,Cin,Cout).  The chain (nlt_lpips_loss) runs pred and gt as one batch of
// 2n frames through conv1 .. conv5 (conv3-5 on csrc/conv_k3.hip), takes the head per level, and for the gradient walks back over
// the first n frames only: head adjoint (+ what came down from above, times the ReLU mask) -> backward-data -> pool gather.
//   conv1   11x11 s4 p2, 3 -> 64: implicit GEMM on v_mfma_f32_16x16x4_f32.  A workgroup owns kC1Tile x kC1Tile output texels; the
//           39 x 39 x 3 input patch goes to LDS with the affine ((2x - 1) - shift) / scale applied (zero outside the image: the
//           padding is in scaled space), K = 363 padded to 384 and walked in chunks of 64 rows of the weight array.
//   conv1^T gather: pixel (y, x) reads the taps a = (y + 2) mod 4 (+ 4, + 8), at most 3 x 3 taps x 64 channels; a workgroup holds
//           pixels of one phase (y mod 4, x mod 4), so its weight reads are uniform.  Ends in the 2 / scale chain factor.
//   conv2   5x5 s1 p2, 64 -> 192, and its backward-data (mirrored taps, channel axes swapped): conv_k3.hip's tile + halo implicit
//           GEMM with the weights staged one tap row at a time.
//   pool    3x3 s2, floor; backward is a gather over the <= 2 x 2 windows covering a texel, first maximum in window order.
//   head    one wave per texel: channel norms of both maps, lin-weighted squared difference; float64 per-workgroup partials in
//           the workspace, added in index order.  The adjoint goes through the normalisation and folds the ReLU mask.
// No float atomics anywhere and no host synchronisation: one form, which is also the deterministic one.
#include "nlt_common.h"

namespace {

constexpr int kC1Tile = 8;                                  // conv1: output texels per tile edge
constexpr int kC1K = 11, kC1S = 4, kC1P = 2, kC1Cout = 64;
constexpr int kC1In = (kC1Tile - 1) * kC1S + kC1K;          // 39
constexpr int kC1Row = kC1In * 3;                           // floats per patch row
constexpr int kC1Kdim = kC1K * kC1K * 3;                    // 363
constexpr int kC1Kpad = 384, kC1Chunk = 64;
constexpr int kC1BwdThreads = 256;                          // conv1 backward-data: pixels of one phase per workgroup

constexpr int kC2Tile = 8;                                  // conv2: texels per tile edge
constexpr int kC2K = 5, kC2P = 2, kC2Cin = 64, kC2Cout = 192;
constexpr int kC2In = kC2Tile + kC2K - 1;                   // 12
constexpr int kC2KC = 16, kC2XS = kC2KC + 4, kC2TN = 64;

constexpr int kPoolThreads = 256;                           // pool pair: elements per workgroup
constexpr int kHeadTexels = 64, kHeadThreads = 256;         // head: texels per workgroup (16 per wave)
constexpr int kHeadMaxC = 512;
constexpr float kEps = 1e-10f;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

inline int tiles_of(int extent, int tile) { return (extent + tile - 1) / tile; }

// ---------------------------------------------------------------------------------------------------------------- conv1
// grid (tiles_y * tiles_x, n).  y[f, oy, ox, o] = relu(bias[o] + sum_{a,b,c} t[4 oy + a - 2, 4 ox + b - 2, c] W[a,b,c,o])
__global__ __launch_bounds__(256) void conv1_fwd_kernel(const float* __restrict__ x, int h, int w, const float* __restrict__ affine,
                                                        const float* __restrict__ wgt, const float* __restrict__ bias,
                                                        float* __restrict__ y, int oh, int ow, int tiles_x) {
  __shared__ float xs[kC1In * kC1Row];
  __shared__ __attribute__((aligned(16))) float ws[kC1Chunk * kC1Cout];
  __shared__ int koff[kC1Kpad];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kg = lane >> 4;
  const int f = blockIdx.y;
  const int oy0 = (blockIdx.x / tiles_x) * kC1Tile, ox0 = (blockIdx.x % tiles_x) * kC1Tile;
  const int iy0 = oy0 * kC1S - kC1P, ix0 = ox0 * kC1S - kC1P;
  const float* xf = x + (long)f * h * w * 3;

  for (int i = tid; i < kC1Kpad; i += 256) koff[i] = i < kC1Kdim ? (i / (kC1K * 3)) * kC1Row + i % (kC1K * 3) : 0;
  for (int i = tid; i < kC1In * kC1Row; i += 256) {
    const int r = i / kC1Row, rem = i - r * kC1Row, cc = rem / 3, ch = rem - cc * 3;
    const int iy = iy0 + r, ix = ix0 + cc;
    float v = 0.f;
    if (iy >= 0 && iy < h && ix >= 0 && ix < w) v = (fmaf(2.f, xf[((long)iy * w + ix) * 3 + ch], -1.f) - affine[ch]) / affine[3 + ch];
    xs[i] = v;
  }

  f32x4 acc[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int lr = 2 * wave + (li >> 3), lc = li & 7;               // this lane's A row: a texel of the tile
  const float* xa = xs + lr * kC1S * kC1Row + lc * kC1S * 3;

  for (int k0 = 0; k0 < kC1Kpad; k0 += kC1Chunk) {
    __syncthreads();                                              // (first pass: xs / koff are complete; later: ws was read)
    for (int i = tid; i < kC1Chunk * kC1Cout / 4; i += 256) {
      const int k = k0 + i / (kC1Cout / 4);
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (k < kC1Kdim) v = *reinterpret_cast<const f32x4*>(wgt + (long)k * kC1Cout + 4 * (i % (kC1Cout / 4)));
      *reinterpret_cast<f32x4*>(ws + 4 * i) = v;
    }
    __syncthreads();
    for (int kk = 0; kk < kC1Chunk; kk += 16) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kl = kk + 4 * kg + r;
        const float a = xa[koff[k0 + kl]];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ws[kl * kC1Cout + nb * 16 + li], acc[nb], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    const int o = nb * 16 + li;
    const float bv = bias[o];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * kg + r;                                 // D: row = 4 (lane >> 4) + r, column = lane & 15
      const int oy = oy0 + 2 * wave + (row >> 3), ox = ox0 + (row & 7);
      if (oy >= oh || ox >= ow) continue;
      const float v = acc[nb][r] + bv;
      y[(((long)f * oh + oy) * ow + ox) * kC1Cout + o] = v > 0.f ? v : 0.f;
    }
  }
}

// grid (blocks over the (h/4) x (w/4) pixels of a phase, 16 phases, n).
// dx[f, y, x, c] = 2 / scale[c] * sum over taps a = y + 2 - 4 oy, b = x + 2 - 4 ox (0 <= a, b <= 10) and o of dpre[f, oy, ox, o] W[a,b,c,o]
__global__ __launch_bounds__(kC1BwdThreads) void conv1_bwd_kernel(const float* __restrict__ dpre, int h, int w, int oh, int ow,
                                                                  const float* __restrict__ affine, const float* __restrict__ wgt,
                                                                  float* __restrict__ dx) {
  const int qw = (w + 3) >> 2, qh = (h + 3) >> 2;
  const int q = blockIdx.x * kC1BwdThreads + threadIdx.x;
  const int py = blockIdx.y >> 2, px = blockIdx.y & 3, f = blockIdx.z;
  if (q >= qh * qw) return;
  const int y = 4 * (q / qw) + py, x = 4 * (q % qw) + px;
  if (y >= h || x >= w) return;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int a = (py + kC1P) & 3; a < kC1K; a += 4) {
    const int ny = y + kC1P - a;                                  // 4 oy
    if (ny < 0 || ny >= 4 * oh) continue;
    for (int b = (px + kC1P) & 3; b < kC1K; b += 4) {
      const int nx = x + kC1P - b;
      if (nx < 0 || nx >= 4 * ow) continue;
      const float* g = dpre + (((long)f * oh + (ny >> 2)) * ow + (nx >> 2)) * kC1Cout;
      const float* wt = wgt + (long)(a * kC1K + b) * 3 * kC1Cout;
      for (int o = 0; o < kC1Cout; o += 4) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a0 = fmaf(gv[j], wt[o + j], a0);
          a1 = fmaf(gv[j], wt[kC1Cout + o + j], a1);
          a2 = fmaf(gv[j], wt[2 * kC1Cout + o + j], a2);
        }
      }
    }
  }
  float* d = dx + (((long)f * h + y) * w + x) * 3;
  d[0] = a0 * (2.f / affine[3]);
  d[1] = a1 * (2.f / affine[4]);
  d[2] = a2 * (2.f / affine[5]);
}

// ---------------------------------------------------------------------------------------------------------------- conv2
// 5x5 stride 1 pad 2 on [n,h,w,cin] -> [n,h,w,cout], cin % 16 == 0, cout % 64 == 0.  grid (n * tiles_y * tiles_x, cout / 64).
// flip = 0: y = relu(bias + sum x[g + a - 2] W[a,b,c,o]), array (5,5,cin,cout).
// flip = 1: backward-data, y = sum x[g + 2 - a] W[a,b,o,c], array (5,5,cout,cin): no bias, no activation.
__global__ __launch_bounds__(256) void conv2_kernel(const float* __restrict__ x, int h, int w, int cin, const float* __restrict__ wgt,
                                                    const float* __restrict__ bias, int cout, float* __restrict__ y, int flip,
                                                    int tiles_y, int tiles_x) {
  __shared__ __attribute__((aligned(16))) float xs[kC2In * kC2In * kC2XS];
  __shared__ __attribute__((aligned(16))) float ws[kC2K * 4 * kC2TN * 4];             // [tap of the row][4 k groups][TN][4]
  constexpr int TN = kC2TN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kg = lane >> 4;
  int t = blockIdx.x;
  const int tx = t % tiles_x; t /= tiles_x;
  const int ty = t % tiles_y;
  const int f = t / tiles_y;
  const int gy0 = ty * kC2Tile, gx0 = tx * kC2Tile;
  const int o0 = blockIdx.y * TN;
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) acc[nb] = zero4;
  const int lr = 2 * wave + (li >> 3), lc = li & 7;

  for (int c0 = 0; c0 < cin; c0 += kC2KC) {
    __syncthreads();
    for (int idx = tid; idx < kC2In * kC2In * 4; idx += 256) {                         // input tile + halo, one channel quad per thread
      const int tex = idx >> 2, q = idx & 3;
      const int iy = gy0 - kC2P + tex / kC2In, ix = gx0 - kC2P + tex % kC2In;
      f32x4 v = zero4;
      if (iy >= 0 && iy < h && ix >= 0 && ix < w)
        v = *reinterpret_cast<const f32x4*>(x + (((long)f * h + iy) * w + ix) * cin + c0 + 4 * q);
      *reinterpret_cast<f32x4*>(xs + tex * kC2XS + 4 * q) = v;
    }
    for (int a = 0; a < kC2K; ++a) {
      if (a) __syncthreads();                                                          // the previous row's weights were read
      for (int idx = tid; idx < kC2K * 4 * TN; idx += 256) {                           // float4s of tap row a's weight slice
        if (flip) {                                                                    // (5,5,Cout,Cin): the vector runs along Cin
          const int c4 = idx & 3, ol = (idx >> 2) % TN, b = idx / (4 * TN);
          const f32x4 v = *reinterpret_cast<const f32x4*>(wgt + ((long)(a * kC2K + b) * cout + o0 + ol) * cin + c0 + 4 * c4);
          *reinterpret_cast<f32x4*>(ws + ((b * 4 + c4) * TN + ol) * 4) = v;
        } else {                                                                       // (5,5,Cin,Cout): the vector runs along Cout
          const int o4 = idx % (TN / 4), cl = (idx / (TN / 4)) & 15, b = idx / (4 * TN);
          const f32x4 v = *reinterpret_cast<const f32x4*>(wgt + ((long)(a * kC2K + b) * cin + c0 + cl) * cout + o0 + 4 * o4);
          float* d = ws + ((b * 4 + (cl >> 2)) * TN + 4 * o4) * 4 + (cl & 3);
          d[0] = v[0]; d[4] = v[1]; d[8] = v[2]; d[12] = v[3];
        }
      }
      __syncthreads();
      const int dy = flip ? kC2K - 1 - a : a;
      for (int b = 0; b < kC2K; ++b) {
        const int dx = flip ? kC2K - 1 - b : b;
        const f32x4 av = *reinterpret_cast<const f32x4*>(xs + ((lr + dy) * kC2In + lc + dx) * kC2XS + 4 * kg);
        const float* wt = ws + ((b * 4 + kg) * TN + li) * 4;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(wt + nb * 64);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], bv[r], acc[nb], 0, 0, 0);
        }
      }
    }
  }

#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    const int o = o0 + nb * 16 + li;
    const float bv = bias ? bias[o] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * kg + r;
      const int gy = gy0 + 2 * wave + (row >> 3), gx = gx0 + (row & 7);
      if (gy >= h || gx >= w) continue;
      float v = acc[nb][r] + bv;
      if (!flip) v = v > 0.f ? v : 0.f;
      y[(((long)f * h + gy) * w + gx) * cout + o] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- pool
__global__ __launch_bounds__(kPoolThreads) void pool_fwd_kernel(const float* __restrict__ x, int h, int w, int c, int oh, int ow,
                                                                long total, float* __restrict__ y) {
  const long idx = (long)blockIdx.x * kPoolThreads + threadIdx.x;
  if (idx >= total) return;
  const int ch = (int)(idx % c);
  long t = idx / c;
  const int ox = (int)(t % ow); t /= ow;
  const int oy = (int)(t % oh);
  const long f = t / oh;
  const float* p = x + ((f * h + 2 * oy) * w + 2 * ox) * c + ch;
  float m = p[0];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const float v = p[((long)a * w + b) * c];
      m = v > m ? v : m;
    }
  y[idx] = m;
}

__global__ __launch_bounds__(kPoolThreads) void pool_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, int h, int w,
                                                                int c, int oh, int ow, long total, float* __restrict__ dx) {
  const long idx = (long)blockIdx.x * kPoolThreads + threadIdx.x;
  if (idx >= total) return;
  const int ch = (int)(idx % c);
  long t = idx / c;
  const int j = (int)(t % w); t /= w;
  const int i = (int)(t % h);
  const long f = t / h;
  float acc = 0.f;
  const int oy_hi = min(oh - 1, i >> 1), ox_hi = min(ow - 1, j >> 1);
  for (int oy = max(0, (i - 1) / 2); oy <= oy_hi; ++oy)
    for (int ox = max(0, (j - 1) / 2); ox <= ox_hi; ++ox) {
      const float* p = x + ((f * h + 2 * oy) * w + 2 * ox) * c + ch;
      float m = p[0];
      int at = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const float v = p[((long)a * w + b) * c];
          if (v > m) { m = v; at = a * 3 + b; }                   // strict: the first maximum in window order keeps it
        }
      if (at == (i - 2 * oy) * 3 + (j - 2 * ox)) acc += dy[((f * oh + oy) * ow + ox) * c + ch];
    }
  dx[idx] = acc;
}

// ---------------------------------------------------------------------------------------------------------------- head
// grid (workgroups over texels, n).  partial[f][wg] = sum over the workgroup's texels of sum_c lin[c] (fp / Dp - fg / Dg)^2
__global__ __launch_bounds__(kHeadThreads) void head_fwd_kernel(const float* __restrict__ fp, const float* __restrict__ fg, long texels,
                                                                int c, const float* __restrict__ lin, double* __restrict__ partial) {
  __shared__ double red[kHeadThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = blockIdx.y;
  constexpr int per_wave = kHeadTexels / (kHeadThreads / 64);
  double local = 0.0;
  for (int k = 0; k < per_wave; ++k) {
    const long t = (long)blockIdx.x * kHeadTexels + wave * per_wave + k;
    if (t >= texels) break;
    const float* p = fp + ((long)f * texels + t) * c;
    const float* g = fg + ((long)f * texels + t) * c;
    float sp = 0.f, sg = 0.f;
    for (int ch = lane; ch < c; ch += 64) { sp = fmaf(p[ch], p[ch], sp); sg = fmaf(g[ch], g[ch], sg); }
    const float dp = sqrtf(wave_sum(sp)) + kEps, dg = sqrtf(wave_sum(sg)) + kEps;
    float s = 0.f;
    for (int ch = lane; ch < c; ch += 64) {
      const float d = p[ch] / dp - g[ch] / dg;
      s = fmaf(lin[ch], d * d, s);
    }
    local += (double)wave_sum(s);
  }
  if (lane == 0) red[wave] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = red[0];
    for (int i = 1; i < kHeadThreads / 64; ++i) s += red[i];
    partial[(long)f * gridDim.x + blockIdx.x] = s;
  }
}

// acc[f] = (first ? 0 : acc[f]) + (sum of the example's partials, in workgroup order) / texels; out[f] = float(acc[f]) when asked
__global__ __launch_bounds__(64) void head_final_kernel(const double* __restrict__ partial, int wgs, double texels, int first,
                                                        double* __restrict__ acc, float* __restrict__ out) {
  const int f = blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < wgs; i += 64) s += partial[(long)f * wgs + i];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    const double v = (first ? 0.0 : acc[f]) + s / texels;
    acc[f] = v;
    if (out) out[f] = (float)v;
  }
}

// One wave per texel.  With D = sqrt(sum fp^2) + eps, n = fp / D and q_c = 2 lin_c (n_c - m_c) / texels:
// d d / d fp_k = q_k / D - fp_k (sum_c q_c fp_c) / (D^2 (D - eps)); an all-zero texel gets 0.  dpre = (dup + that) * (fp > 0).
__global__ __launch_bounds__(kHeadThreads) void head_bwd_kernel(const float* __restrict__ fp, const float* __restrict__ fg, long texels,
                                                                int c, const float* __restrict__ lin, float inv_texels,
                                                                const float* __restrict__ dup, float* __restrict__ dpre) {
  constexpr int kPer = kHeadMaxC / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = blockIdx.y;
  constexpr int per_wave = kHeadTexels / (kHeadThreads / 64);
  for (int k = 0; k < per_wave; ++k) {
    const long t = (long)blockIdx.x * kHeadTexels + wave * per_wave + k;
    if (t >= texels) break;
    const long base = ((long)f * texels + t) * c;
    float pv[kPer], qv[kPer];
    float sp = 0.f, sg = 0.f;
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      const int ch = lane + 64 * m;
      pv[m] = ch < c ? fp[base + ch] : 0.f;
      qv[m] = ch < c ? fg[base + ch] : 0.f;
      sp = fmaf(pv[m], pv[m], sp);
      sg = fmaf(qv[m], qv[m], sg);
    }
    const float s = sqrtf(wave_sum(sp));
    const float dp = s + kEps, dg = sqrtf(wave_sum(sg)) + kEps;
    float dot = 0.f;
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      const int ch = lane + 64 * m;
      const float l = ch < c ? lin[ch] : 0.f;
      qv[m] = 2.f * l * (pv[m] / dp - qv[m] / dg) * inv_texels;
      dot = fmaf(qv[m], pv[m], dot);
    }
    dot = wave_sum(dot);
    const float back = s > 0.f ? dot / (dp * dp * s) : 0.f;
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      const int ch = lane + 64 * m;
      if (ch < c) {
        const float v = qv[m] / dp - pv[m] * back + (dup ? dup[base + ch] : 0.f);
        dpre[base + ch] = pv[m] > 0.f ? v : 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side
constexpr long long kLim = 1ll << 31;

inline int pool_out(int v) { return (v - 3) / 2 + 1; }

int conv1_check(int n, int h, int w, int* oh, int* ow) {
  if (n <= 0 || h <= 0 || w <= 0) return NLT_ERR_BAD_ARG;
  if (h < kC1K || w < kC1K || n > 65535) return NLT_ERR_UNSUPPORTED;
  *oh = (h + 2 * kC1P - kC1K) / kC1S + 1; *ow = (w + 2 * kC1P - kC1K) / kC1S + 1;
  if ((long long)n * h * w * 3 >= kLim || (long long)n * *oh * *ow * kC1Cout >= kLim) return NLT_ERR_UNSUPPORTED;
  return NLT_OK;
}

int conv1_forward(const float* x, int n, int h, int w, const float* affine, const float* wgt, const float* bias, float* y, hipStream_t s) {
  int oh, ow;
  const int st = conv1_check(n, h, w, &oh, &ow);
  if (st != NLT_OK) return st;
  if (!nlt_aligned16(wgt)) return NLT_ERR_BAD_ARG;
  const int ty = tiles_of(oh, kC1Tile), tx = tiles_of(ow, kC1Tile);
  hipLaunchKernelGGL(conv1_fwd_kernel, dim3((unsigned)(ty * tx), (unsigned)n), dim3(256), 0, s, x, h, w, affine, wgt, bias, y, oh, ow, tx);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

int conv1_backward(const float* dpre, int n, int h, int w, const float* affine, const float* wgt, float* dx, hipStream_t s) {
  int oh, ow;
  const int st = conv1_check(n, h, w, &oh, &ow);
  if (st != NLT_OK) return st;
  if (!nlt_aligned16(dpre)) return NLT_ERR_BAD_ARG;
  const int q = ((h + 3) / 4) * ((w + 3) / 4);
  hipLaunchKernelGGL(conv1_bwd_kernel, dim3((unsigned)tiles_of(q, kC1BwdThreads), 16u, (unsigned)n), dim3(kC1BwdThreads), 0, s,
                     dpre, h, w, oh, ow, affine, wgt, dx);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

int conv2_launch(const float* x, int n, int h, int w, int cin, const float* wgt, const float* bias, int cout, float* y, int flip,
                 hipStream_t s) {
  if (n <= 0 || h <= 0 || w <= 0) return NLT_ERR_BAD_ARG;
  if (!nlt_aligned16(x) || !nlt_aligned16(wgt)) return NLT_ERR_BAD_ARG;
  const long long tiles = (long long)n * tiles_of(h, kC2Tile) * tiles_of(w, kC2Tile);
  if (tiles >= kLim || (long long)n * h * w * kC2Cout >= kLim) return NLT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(conv2_kernel, dim3((unsigned)tiles, (unsigned)(cout / kC2TN)), dim3(256), 0, s, x, h, w, cin, wgt, bias, cout, y,
                     flip, tiles_of(h, kC2Tile), tiles_of(w, kC2Tile));
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

int pool_check(int n, int h, int w, int c, int* oh, int* ow) {
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return NLT_ERR_BAD_ARG;
  if (h < 3 || w < 3) return NLT_ERR_UNSUPPORTED;
  *oh = pool_out(h); *ow = pool_out(w);
  if ((long long)n * h * w * c >= kLim) return NLT_ERR_UNSUPPORTED;
  return NLT_OK;
}

int pool_forward(const float* x, int n, int h, int w, int c, float* y, hipStream_t s) {
  int oh, ow;
  const int st = pool_check(n, h, w, c, &oh, &ow);
  if (st != NLT_OK) return st;
  const long total = (long)n * oh * ow * c;
  hipLaunchKernelGGL(pool_fwd_kernel, dim3((unsigned)((total + kPoolThreads - 1) / kPoolThreads)), dim3(kPoolThreads), 0, s, x, h, w, c,
                     oh, ow, total, y);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

int pool_backward(const float* dy, const float* x, int n, int h, int w, int c, float* dx, hipStream_t s) {
  int oh, ow;
  const int st = pool_check(n, h, w, c, &oh, &ow);
  if (st != NLT_OK) return st;
  const long total = (long)n * h * w * c;
  hipLaunchKernelGGL(pool_bwd_kernel, dim3((unsigned)((total + kPoolThreads - 1) / kPoolThreads)), dim3(kPoolThreads), 0, s, dy, x, h, w,
                     c, oh, ow, total, dx);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

// 0: not a shape the head launches
long head_wgs(int n, long texels) {
  if (n <= 0 || n > 65535 || texels <= 0) return 0;
  const long wgs = (texels + kHeadTexels - 1) / kHeadTexels;
  return wgs < kLim ? wgs : 0;
}

long head_floats(int n, long texels) {
  const long wgs = head_wgs(n, texels);
  return wgs ? 2 * ((long)n * wgs + n) : -1;                      // float64: the partials, then one accumulator per example
}

bool head_shape_ok(int n, long texels, int c) { return c <= kHeadMaxC && (long long)n * texels * c < kLim; }

// partials at `ws`, accumulators right behind them
int head_forward(const float* fp, const float* fg, int n, long texels, int c, const float* lin, double* ws, int first, double* acc,
                 float* out, hipStream_t s) {
  const long wgs = head_wgs(n, texels);
  hipLaunchKernelGGL(head_fwd_kernel, dim3((unsigned)wgs, (unsigned)n), dim3(kHeadThreads), 0, s, fp, fg, texels, c, lin, ws);
  hipLaunchKernelGGL(head_final_kernel, dim3((unsigned)n), dim3(64), 0, s, ws, (int)wgs, (double)texels, first, acc, out);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

int head_backward(const float* fp, const float* fg, int n, long texels, int c, const float* lin, const float* dup, float* dpre,
                  hipStream_t s) {
  const long wgs = head_wgs(n, texels);
  hipLaunchKernelGGL(head_bwd_kernel, dim3((unsigned)wgs, (unsigned)n), dim3(kHeadThreads), 0, s, fp, fg, texels, c, lin,
                     (float)(1.0 / (double)texels), dup, dpre);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

// the weights blob: offsets in floats, all multiples of 4
constexpr int kCh[6] = {3, 64, 192, 384, 256, 256};
constexpr int kKs[5] = {11, 5, 3, 3, 3};
struct Blob { long w[5], b[5], lin[5], total; };
Blob blob() {
  Blob o;
  long at = 8;
  for (int l = 0; l < 5; ++l) {
    o.w[l] = at; at += (long)kKs[l] * kKs[l] * kCh[l] * kCh[l + 1];
    o.b[l] = at; at += kCh[l + 1];
  }
  for (int l = 0; l < 5; ++l) { o.lin[l] = at; at += kCh[l + 1]; }
  o.total = at;
  return o;
}

// geometry and workspace layout of the chain; offsets in floats, every one a multiple of 4
struct Chain {
  int hh[5], ww[5];             // feature maps of the five levels
  int hp1, wp1;                 // pool1's output is conv2's map: hh[1], ww[1]; pool2's is hh[2], ww[2]
  long head, f[5], p[2], ga, gb, total;
};

bool chain_of(int n, int h, int w, int want_grad, Chain* c) {
  if (n <= 0 || n > 32767 || h < 31 || w < 31) return false;
  if ((long long)n * h * w * 3 >= kLim) return false;
  c->hh[0] = (h + 2 * kC1P - kC1K) / kC1S + 1; c->ww[0] = (w + 2 * kC1P - kC1K) / kC1S + 1;
  c->hh[1] = pool_out(c->hh[0]); c->ww[1] = pool_out(c->ww[0]);
  c->hh[2] = pool_out(c->hh[1]); c->ww[2] = pool_out(c->ww[1]);
  for (int l = 3; l < 5; ++l) { c->hh[l] = c->hh[2]; c->ww[l] = c->ww[2]; }
  const long long n2 = 2ll * n;
  if (n2 * c->hh[0] * c->ww[0] * 64 >= kLim || n2 * c->hh[1] * c->ww[1] * 192 >= kLim) return false;
  long at = (head_floats(n, (long)c->hh[0] * c->ww[0]) + 3) / 4 * 4;      // level 1 has the most texels
  c->head = 0;
  long gmax = 0;
  for (int l = 0; l < 5; ++l) {
    const long fl = (long)c->hh[l] * c->ww[l] * kCh[l + 1];
    c->f[l] = at; at += n2 * fl;
    if (l < 2) { c->p[l] = at; at += n2 * c->hh[l + 1] * c->ww[l + 1] * kCh[l + 1]; }
    if (n * fl > gmax) gmax = n * fl;
  }
  c->ga = c->gb = -1;
  if (want_grad) { c->ga = at; at += gmax; c->gb = at; at += gmax; }
  c->total = at;
  return true;
}

}  // namespace

extern "C" int nlt_lpips_conv1_forward(const float* x, int n, int h, int w, const float* affine, const float* w_keras, const float* bias,
                                       float* y, void* stream) {
  if (!x || !affine || !w_keras || !bias || !y) return NLT_ERR_BAD_ARG;
  return conv1_forward(x, n, h, w, affine, w_keras, bias, y, static_cast<hipStream_t>(stream));
}

extern "C" int nlt_lpips_conv1_backward_data(const float* dpre, int n, int h, int w, const float* affine, const float* w_keras, float* dx,
                                             void* stream) {
  if (!dpre || !affine || !w_keras || !dx) return NLT_ERR_BAD_ARG;
  return conv1_backward(dpre, n, h, w, affine, w_keras, dx, static_cast<hipStream_t>(stream));
}

extern "C" int nlt_lpips_conv2_forward(const float* x, int n, int h, int w, const float* w_keras, const float* bias, float* y, void* stream) {
  if (!x || !w_keras || !bias || !y) return NLT_ERR_BAD_ARG;
  return conv2_launch(x, n, h, w, kC2Cin, w_keras, bias, kC2Cout, y, 0, static_cast<hipStream_t>(stream));
}

extern "C" int nlt_lpips_conv2_backward_data(const float* dpre, int n, int h, int w, const float* w_keras, float* dx, void* stream) {
  if (!dpre || !w_keras || !dx) return NLT_ERR_BAD_ARG;
  return conv2_launch(dpre, n, h, w, kC2Cout, w_keras, nullptr, kC2Cin, dx, 1, static_cast<hipStream_t>(stream));
}

extern "C" int nlt_lpips_pool_forward(const float* x, int n, int h, int w, int c, float* y, void* stream) {
  if (!x || !y) return NLT_ERR_BAD_ARG;
  return pool_forward(x, n, h, w, c, y, static_cast<hipStream_t>(stream));
}

extern "C" int nlt_lpips_pool_backward(const float* dy, const float* x, int n, int h, int w, int c, float* dx, void* stream) {
  if (!dy || !x || !dx) return NLT_ERR_BAD_ARG;
  return pool_backward(dy, x, n, h, w, c, dx, static_cast<hipStream_t>(stream));
}

extern "C" long nlt_lpips_head_workspace_floats(int n, long texels) { return head_floats(n, texels); }

extern "C" int nlt_lpips_head_forward(const float* fp, const float* fg, int n, long texels, int c, const float* lin, float* workspace,
                                      long workspace_floats, float* d, void* stream) {
  if (!fp || !fg || !lin || !workspace || !d || n <= 0 || texels <= 0 || c <= 0) return NLT_ERR_BAD_ARG;
  const long need = head_floats(n, texels);
  if (need < 0 || !head_shape_ok(n, texels, c)) return NLT_ERR_UNSUPPORTED;
  if (workspace_floats < need || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return NLT_ERR_BAD_ARG;
  double* ws = reinterpret_cast<double*>(workspace);
  return head_forward(fp, fg, n, texels, c, lin, ws, 1, ws + need / 2 - n, d, static_cast<hipStream_t>(stream));
}

extern "C" int nlt_lpips_head_backward(const float* fp, const float* fg, int n, long texels, int c, const float* lin, const float* dup,
                                       float* dpre, void* stream) {
  if (!fp || !fg || !lin || !dpre || n <= 0 || texels <= 0 || c <= 0) return NLT_ERR_BAD_ARG;
  if (!head_wgs(n, texels) || !head_shape_ok(n, texels, c)) return NLT_ERR_UNSUPPORTED;
  return head_backward(fp, fg, n, texels, c, lin, dup, dpre, static_cast<hipStream_t>(stream));
}

extern "C" long nlt_lpips_weights_floats(void) { return blob().total; }

extern "C" long nlt_lpips_workspace_floats(int n, int h, int w, int want_grad) {
  Chain c;
  return chain_of(n, h, w, want_grad, &c) ? c.total : -1;
}

extern "C" int nlt_lpips_loss(const float* pred, const float* gt, int n, int h, int w, const float* weights, float* workspace,
                              long workspace_floats, float* loss, float* dunit, void* stream) {
  if (!pred || !gt || !weights || !workspace || !loss || n <= 0 || h <= 0 || w <= 0) return NLT_ERR_BAD_ARG;
  Chain c;
  if (!chain_of(n, h, w, dunit != nullptr, &c)) return NLT_ERR_UNSUPPORTED;
  if (workspace_floats < c.total || !nlt_aligned16(workspace) || !nlt_aligned16(weights)) return NLT_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Blob bl = blob();
  const float* W[5]; const float* B[5]; const float* L[5]; float* F[5];
  for (int l = 0; l < 5; ++l) { W[l] = weights + bl.w[l]; B[l] = weights + bl.b[l]; L[l] = weights + bl.lin[l]; F[l] = workspace + c.f[l]; }
  float* P1 = workspace + c.p[0];
  float* P2 = workspace + c.p[1];
  const int n2 = 2 * n;
  long tex[5], per[5];                                            // texels and floats of one frame's map
  for (int l = 0; l < 5; ++l) { tex[l] = (long)c.hh[l] * c.ww[l]; per[l] = tex[l] * kCh[l + 1]; }
  int st;
#define NLT_TRY(call) do { st = (call); if (st != NLT_OK) return st; } while (0)
  // features of pred (frames 0 .. n-1) and gt (frames n .. 2n-1)
  NLT_TRY(conv1_forward(pred, n, h, w, weights, W[0], B[0], F[0], s));
  NLT_TRY(conv1_forward(gt, n, h, w, weights, W[0], B[0], F[0] + n * per[0], s));
  NLT_TRY(pool_forward(F[0], n2, c.hh[0], c.ww[0], 64, P1, s));
  NLT_TRY(conv2_launch(P1, n2, c.hh[1], c.ww[1], kC2Cin, W[1], B[1], kC2Cout, F[1], 0, s));
  NLT_TRY(pool_forward(F[1], n2, c.hh[1], c.ww[1], 192, P2, s));
  NLT_TRY(nlt_conv_k3_forward(NLT_CONV_K3S1, NLT_ALGO_AUTO, P2, n2, c.hh[2], c.ww[2], 192, W[2], B[2], 384, F[2], 1, 0.f, stream));
  NLT_TRY(nlt_conv_k3_forward(NLT_CONV_K3S1, NLT_ALGO_AUTO, F[2], n2, c.hh[2], c.ww[2], 384, W[3], B[3], 256, F[3], 1, 0.f, stream));
  NLT_TRY(nlt_conv_k3_forward(NLT_CONV_K3S1, NLT_ALGO_AUTO, F[3], n2, c.hh[2], c.ww[2], 256, W[4], B[4], 256, F[4], 1, 0.f, stream));
  // the five levels, added in level order
  double* hws = reinterpret_cast<double*>(workspace + c.head);
  double* acc = hws + head_floats(n, tex[0]) / 2 - n;
  for (int l = 0; l < 5; ++l)
    NLT_TRY(head_forward(F[l], F[l] + n * per[l], n, tex[l], kCh[l + 1], L[l], hws, l == 0, acc, l == 4 ? loss : nullptr, s));
  if (dunit) {
    float* A = workspace + c.ga;
    float* G = workspace + c.gb;
    NLT_TRY(head_backward(F[4], F[4] + n * per[4], n, tex[4], 256, L[4], nullptr, A, s));
    NLT_TRY(nlt_conv_k3_backward_data(NLT_CONV_K3S1, NLT_ALGO_AUTO, A, n, c.hh[2], c.ww[2], 256, W[4], 256, G, stream));
    NLT_TRY(head_backward(F[3], F[3] + n * per[3], n, tex[3], 256, L[3], G, A, s));
    NLT_TRY(nlt_conv_k3_backward_data(NLT_CONV_K3S1, NLT_ALGO_AUTO, A, n, c.hh[2], c.ww[2], 384, W[3], 256, G, stream));
    NLT_TRY(head_backward(F[2], F[2] + n * per[2], n, tex[2], 384, L[2], G, A, s));
    NLT_TRY(nlt_conv_k3_backward_data(NLT_CONV_K3S1, NLT_ALGO_AUTO, A, n, c.hh[2], c.ww[2], 192, W[2], 384, G, stream));
    NLT_TRY(pool_backward(G, F[1], n, c.hh[1], c.ww[1], 192, A, s));
    NLT_TRY(head_backward(F[1], F[1] + n * per[1], n, tex[1], 192, L[1], A, G, s));
    NLT_TRY(conv2_launch(G, n, c.hh[1], c.ww[1], kC2Cout, W[1], nullptr, kC2Cin, A, 1, s));
    NLT_TRY(pool_backward(A, F[0], n, c.hh[0], c.ww[0], 64, G, s));
    NLT_TRY(head_backward(F[0], F[0] + n * per[0], n, tex[0], 64, L[0], G, A, s));
    NLT_TRY(conv1_backward(A, n, h, w, weights, W[0], dunit, s));
  }
#undef NLT_TRY
  return NLT_OK;
}
