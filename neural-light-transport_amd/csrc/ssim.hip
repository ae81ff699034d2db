// SSIM as tf.image.ssim(img1, img2, max_val) of TF 2.2 fixes it (11x11 Gaussian window, sigma 1.5, k1 0.01, k2 0.03, 'VALID'):
// the per-image value, the loss (1 - ssim) / 2 and d(loss)/d(pred).
//   replaces: nlt/losses.py:75-87 (losses.SSIM) and third_party/xiuminglib/xiuminglib/metric.py:154-184 (xm.metric.SSIM)
// A workgroup owns a kTileW x kTileH tile.  Forward: the haloed tile of both images (every channel, NHWC) goes to LDS, then per
// channel a horizontal pass over the four filtered quantities F(x), F(y), F(xy), F(x^2 + y^2) and a vertical pass that ends in
// lum * cs.  When a gradient is wanted the forward also writes three coefficient maps per channel and the adjoint kernel runs
// the same separable window over them (F^T is a gather over each pixel's footprint: no scatter, no atomics).
// Sums: one partial per workgroup in the workspace, added in workgroup order by ssim_final_kernel -- the only form there is, so
// it is also the deterministic one.  Filter sums and the per-position quotient run in float64 (the variance terms cancel on
// flat images; float32 there is TF's own error, which the tolerance rule of tests/test_gpu_ssim.py does not grant twice).
#include "nlt_common.h"

namespace {

constexpr int kWin = 11;                        // filter_size
constexpr int kHalo = kWin - 1;
constexpr int kTileW = 32, kTileH = 16;         // tile per workgroup: output positions (forward), image pixels (adjoint)
constexpr int kInW = kTileW + kHalo, kInH = kTileH + kHalo;
constexpr int kThreads = 256;
constexpr double kK1 = 0.01, kK2 = 0.03;

// g[i] = softmax_i(-(i - 5)^2 * 0.5 / 1.5^2) in float64
__constant__ double kG[kWin] = {1.02838008447911008e-03, 7.59875813523918503e-03, 3.60007721284308288e-02,
                                1.09360689509700015e-01, 2.13005537711253690e-01, 2.66011724861794363e-01,
                                2.13005537711253690e-01, 1.09360689509700015e-01, 3.60007721284308288e-02,
                                7.59875813523918503e-03, 1.02838008447911008e-03};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// 0.2126 r + 0.7152 g + 0.0722 b in float64, left to right with every operation rounded (NumPy's), then float32 (img.py:600-611)
__device__ __forceinline__ float luma_f32(const float* p) {
  const double l = __dadd_rn(__dadd_rn(__dmul_rn(0.2126, (double)p[0]), __dmul_rn(0.7152, (double)p[1])),
                             __dmul_rn(0.0722, (double)p[2]));
  return (float)l;
}

// lum * cs at one position from the four filtered quantities; with GRAD the partials of it with respect to F(y), F(xy) and
// F(x^2 + y^2) (the last one times the 2 of d(y^2)/dy).  No contraction: identical images then give exactly 1.
template <bool GRAD>
__device__ __forceinline__ double ssim_point(double m0, double m1, double sxy, double sqq, double c1, double c2,
                                             double* A, double* B, double* C) {
#pragma clang fp contract(off)
  const double num0 = 2.0 * m0 * m1, den0 = m0 * m0 + m1 * m1;
  const double ld = den0 + c1;
  const double lum = (num0 + c1) / ld;
  const double csd = sqq - den0 + c2;
  const double cs = (2.0 * sxy - num0 + c2) / csd;
  if (GRAD) {
    const double icsd = 1.0 / csd;
    *A = cs * (2.0 * m0 - 2.0 * m1 * lum) / ld + lum * (2.0 * m1 * cs - 2.0 * m0) * icsd;
    *B = 2.0 * lum * icsd;
    *C = -2.0 * lum * cs * icsd;
  }
  return lum * cs;
}

// img1 = x, img2 = y: [n,h,w,CIN] float32.  LUMA (CIN = 3): SSIM of the luma channel.  Grid (tiles x, tiles y, n).
// partial [n][tiles] float64: the workgroup's sum of lum * cs over its positions and channels.
// GRAD: maps [n][C][3][ho][wo] = gscale * (A + s (B + C), B, C) with s = x[f,0,0,ch] -- the adjoint multiplies B and C by
// (x(q) - s) and (y(q) - s), so on a nearly flat image the three stored terms do not cancel against each other in float32.
template <int CIN, bool LUMA, bool GRAD>
__global__ __launch_bounds__(kThreads) void ssim_fwd_kernel(const float* __restrict__ img1, const float* __restrict__ img2,
                                                            int h, int w, double c1, double c2, double gscale,
                                                            double* __restrict__ partial, float* __restrict__ maps) {
  constexpr int C = LUMA ? 1 : CIN;
  constexpr int kPlane = kInH * kInW;
  __shared__ float sx[C * kPlane], sy[C * kPlane];
  __shared__ double hb[4][kInH][kTileW];
  __shared__ double red[kThreads / 64];
  const int tid = threadIdx.x, f = blockIdx.z;
  const int ox0 = blockIdx.x * kTileW, oy0 = blockIdx.y * kTileH;
  const int ho = h - kHalo, wo = w - kHalo;
  const float* xf = img1 + (long)f * h * w * CIN;
  const float* yf = img2 + (long)f * h * w * CIN;

  for (int i = tid; i < kPlane; i += kThreads) {
    const int r = i / kInW, cc = i - r * kInW;
    const int iy = oy0 + r, ix = ox0 + cc;
    const bool in = iy < h && ix < w;
    const long p = ((long)iy * w + ix) * CIN;
    if (LUMA) {
      sx[i] = in ? luma_f32(xf + p) : 0.f;
      sy[i] = in ? luma_f32(yf + p) : 0.f;
    } else {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        sx[ch * kPlane + i] = in ? xf[p + ch] : 0.f;
        sy[ch * kPlane + i] = in ? yf[p + ch] : 0.f;
      }
    }
  }
  __syncthreads();

  double local = 0.0;
  for (int ch = 0; ch < C; ++ch) {
    // rows: the window along x for every row of the haloed tile
    for (int i = tid; i < kInH * kTileW; i += kThreads) {
      const int r = i / kTileW, cc = i % kTileW;
      const float* px = sx + ch * kPlane + r * kInW + cc;
      const float* py = sy + ch * kPlane + r * kInW + cc;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
      for (int k = 0; k < kWin; ++k) {
        const double xv = px[k], yv = py[k], g = kG[k];
        a0 += g * xv;
        a1 += g * yv;
        a2 += g * (xv * yv);                          // exact: two float32 factors
        a3 += g * (xv * xv + yv * yv);
      }
      hb[0][r][cc] = a0; hb[1][r][cc] = a1; hb[2][r][cc] = a2; hb[3][r][cc] = a3;
    }
    __syncthreads();
    // columns, then the quotient
    for (int i = tid; i < kTileH * kTileW; i += kThreads) {
      const int r = i / kTileW, cc = i % kTileW;
      const int oy = oy0 + r, ox = ox0 + cc;
      if (oy < ho && ox < wo) {
        double m0 = 0.0, m1 = 0.0, sxy = 0.0, sqq = 0.0;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
          const double g = kG[k];
          m0 += g * hb[0][r + k][cc];
          m1 += g * hb[1][r + k][cc];
          sxy += g * hb[2][r + k][cc];
          sqq += g * hb[3][r + k][cc];
        }
        double A, B, Cc;
        local += ssim_point<GRAD>(m0, m1, sxy, sqq, c1, c2, &A, &B, &Cc);
        if (GRAD) {
          const double s = (double)xf[ch];
          float* m = maps + (((long)f * C + ch) * 3) * ((long)ho * wo) + (long)oy * wo + ox;
          m[0] = (float)(gscale * (A + s * (B + Cc)));
          m[(long)ho * wo] = (float)(gscale * B);
          m[2l * ho * wo] = (float)(gscale * Cc);
        }
      }
    }
    __syncthreads();                                  // hb is rewritten by the next channel
  }
  local = wave_sum(local);
  if ((tid & 63) == 0) red[tid >> 6] = local;
  __syncthreads();
  if (tid == 0) {
    double s = red[0];
    for (int i = 1; i < kThreads / 64; ++i) s += red[i];
    partial[((long)f * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
  }
}

// value = (sum of the example's partials, in workgroup order) / count; loss[f] = (1 - value) / 2 (float32) or values[f] = value
__global__ __launch_bounds__(64) void ssim_final_kernel(const double* __restrict__ partial, int tiles, double count,
                                                        float* __restrict__ loss, double* __restrict__ values) {
  const int f = blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < tiles; i += 64) s += partial[(long)f * tiles + i];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    const double v = s / count;
    if (loss) loss[f] = (float)((1.0 - v) * 0.5); else values[f] = v;
  }
}

// dunit[f,q,ch] = F^T(A_s)(q) + (x(q) - s) F^T(B)(q) + (y(q) - s) F^T(C)(q), maps as ssim_fwd_kernel<GRAD> wrote them.  F^T(M)(q)
// = sum_{i,j} g[i] g[j] M(q - (i,j)) over the valid positions: the window is symmetric, so on the tile of maps that starts kHalo
// before the pixel tile (zero outside the valid grid) it is the forward's separable pass again.  Grid (tiles x, tiles y, n)
// over IMAGE pixels.
template <int C>
__global__ __launch_bounds__(kThreads) void ssim_adj_kernel(const float* __restrict__ img1, const float* __restrict__ img2,
                                                            int h, int w, const float* __restrict__ maps,
                                                            float* __restrict__ dunit) {
  __shared__ float sm[3][kInH][kInW];
  __shared__ double hb[3][kInH][kTileW];
  const int tid = threadIdx.x, f = blockIdx.z;
  const int qx0 = blockIdx.x * kTileW, qy0 = blockIdx.y * kTileH;
  const int ho = h - kHalo, wo = w - kHalo;
  const long plane = (long)ho * wo;
  const float* xf = img1 + (long)f * h * w * C;
  const float* yf = img2 + (long)f * h * w * C;
  float* df = dunit + (long)f * h * w * C;

  for (int ch = 0; ch < C; ++ch) {
    const float* mf = maps + (((long)f * C + ch) * 3) * plane;
    for (int i = tid; i < kInH * kInW; i += kThreads) {
      const int r = i / kInW, cc = i - r * kInW;
      const int py = qy0 - kHalo + r, px = qx0 - kHalo + cc;
      const bool in = py >= 0 && py < ho && px >= 0 && px < wo;
      const long p = (long)py * wo + px;
#pragma unroll
      for (int m = 0; m < 3; ++m) sm[m][r][cc] = in ? mf[m * plane + p] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < kInH * kTileW; i += kThreads) {
      const int r = i / kTileW, cc = i % kTileW;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
      for (int k = 0; k < kWin; ++k) {
        const double g = kG[k];
        a0 += g * (double)sm[0][r][cc + k];
        a1 += g * (double)sm[1][r][cc + k];
        a2 += g * (double)sm[2][r][cc + k];
      }
      hb[0][r][cc] = a0; hb[1][r][cc] = a1; hb[2][r][cc] = a2;
    }
    __syncthreads();
    const double s = (double)xf[ch];
    for (int i = tid; i < kTileH * kTileW; i += kThreads) {
      const int r = i / kTileW, cc = i % kTileW;
      const int qy = qy0 + r, qx = qx0 + cc;
      if (qy < h && qx < w) {
        double vA = 0.0, vB = 0.0, vC = 0.0;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
          const double g = kG[k];
          vA += g * hb[0][r + k][cc];
          vB += g * hb[1][r + k][cc];
          vC += g * hb[2][r + k][cc];
        }
        const long p = ((long)qy * w + qx) * C + ch;
        df[p] = (float)(vA + ((double)xf[p] - s) * vB + ((double)yf[p] - s) * vC);
      }
    }
    __syncthreads();                                  // sm / hb are rewritten by the next channel
  }
}

inline int tiles_of(int extent, int tile) { return (extent + tile - 1) / tile; }

struct Shape { int ho, wo, tx, ty; long tiles, partial_floats, map_floats; };

// false: not a shape SSIM is defined for / this file launches
bool shape_of(int n, int h, int w, int c, Shape* s) {
  if (n <= 0 || n > 65535 || h < kWin || w < kWin || (c != 1 && c != 3)) return false;
  s->ho = h - kHalo; s->wo = w - kHalo;
  s->tx = tiles_of(s->wo, kTileW); s->ty = tiles_of(s->ho, kTileH);
  if (tiles_of(h, kTileH) > 65535) return false;
  s->tiles = (long)s->tx * s->ty;
  s->partial_floats = 2 * (long)n * s->tiles;           // float64 partials
  s->map_floats = 3l * n * c * s->ho * s->wo;
  return true;
}

// x = img1, y = img2; the gradient (dunit != NULL) is with respect to img2
int ssim_impl(const float* img1, const float* img2, int n, int h, int w, int c, bool luma, float max_val, float* workspace,
              long workspace_floats, float* loss, float* dunit, double* values, void* stream) {
  if (!img1 || !img2 || !workspace || (!loss && !values) || n <= 0 || !(max_val > 0.f)) return NLT_ERR_BAD_ARG;
  Shape sh;
  if (!shape_of(n, h, w, c, &sh)) return NLT_ERR_UNSUPPORTED;
  const bool grad = dunit != nullptr;
  if (workspace_floats < sh.partial_floats + (grad ? sh.map_floats : 0)) return NLT_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 7u) return NLT_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* partial = reinterpret_cast<double*>(workspace);
  float* maps = workspace + sh.partial_floats;
  const double c1 = (kK1 * (double)max_val) * (kK1 * (double)max_val), c2 = (kK2 * (double)max_val) * (kK2 * (double)max_val);
  const int cs = luma ? 1 : c;                           // channels SSIM is taken on
  const double count = (double)cs * sh.ho * sh.wo;
  const double gscale = -0.5 / count;                    // d((1 - mean) / 2) / d(one position's lum * cs)
  const dim3 grid(sh.tx, sh.ty, n), block(kThreads);
  if (luma) {
    hipLaunchKernelGGL((ssim_fwd_kernel<3, true, false>), grid, block, 0, s, img1, img2, h, w, c1, c2, gscale, partial, maps);
  } else if (c == 3) {
    if (grad) hipLaunchKernelGGL((ssim_fwd_kernel<3, false, true>), grid, block, 0, s, img1, img2, h, w, c1, c2, gscale, partial, maps);
    else hipLaunchKernelGGL((ssim_fwd_kernel<3, false, false>), grid, block, 0, s, img1, img2, h, w, c1, c2, gscale, partial, maps);
  } else {
    if (grad) hipLaunchKernelGGL((ssim_fwd_kernel<1, false, true>), grid, block, 0, s, img1, img2, h, w, c1, c2, gscale, partial, maps);
    else hipLaunchKernelGGL((ssim_fwd_kernel<1, false, false>), grid, block, 0, s, img1, img2, h, w, c1, c2, gscale, partial, maps);
  }
  hipLaunchKernelGGL(ssim_final_kernel, dim3(n), dim3(64), 0, s, partial, (int)sh.tiles, count, loss, values);
  if (grad) {
    const dim3 agrid(tiles_of(w, kTileW), tiles_of(h, kTileH), n);
    if (c == 3) hipLaunchKernelGGL((ssim_adj_kernel<3>), agrid, block, 0, s, img1, img2, h, w, maps, dunit);
    else hipLaunchKernelGGL((ssim_adj_kernel<1>), agrid, block, 0, s, img1, img2, h, w, maps, dunit);
  }
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

}  // namespace

extern "C" long nlt_ssim_workspace_floats(int n, int h, int w, int c, int want_grad) {
  Shape sh;
  if (!shape_of(n, h, w, c, &sh)) return -1;
  return sh.partial_floats + (want_grad ? sh.map_floats : 0);
}

extern "C" int nlt_ssim_loss(const float* pred, const float* gt, int n, int h, int w, int c, float max_val, float* workspace,
                             long workspace_floats, float* loss, float* dunit, void* stream) {
  if (!loss) return NLT_ERR_BAD_ARG;
  return ssim_impl(gt, pred, n, h, w, c, false, max_val, workspace, workspace_floats, loss, dunit, nullptr, stream);
}

extern "C" int nlt_ssim_values(const float* im1, const float* im2, int n, int h, int w, int c, float max_val, float* workspace,
                               long workspace_floats, double* values, void* stream) {
  if (!values) return NLT_ERR_BAD_ARG;
  return ssim_impl(im1, im2, n, h, w, c, c == 3, max_val, workspace, workspace_floats, nullptr, nullptr, values, stream);
}
