// 3x3 Conv2D / Conv2DTranspose with TF 'SAME' padding, stride 1 and 2: forward, backward-data and weight / bias gradient
// (nlt/networks/elements.py:26-39 with kernel = 3).  Exact fp32 throughout.
//
// One index scheme serves the four families.  Work is laid out on a ROW GRID of gh x gw texels per frame:
//   CONV_K3S1    grid = output (h, w)        in = g + a - 1        out = g
//   CONV_K3S2    grid = output (h/2, w/2)    in = 2 g + a          out = g
//   DECONV_K3S1  grid = output (h, w)        in = g + 1 - a        out = g
//   DECONV_K3S2  grid = INPUT (h, w), once per output parity class (pm, pn):   in = g - (a == 2)   out = 2 g + parity,
//                with the live taps a in {0, 2} for parity 0 and a = 1 for parity 1 (4, 2, 2, 1 taps per class).
// All of them read   in = g * S + OFF + k3_dy(a)   and write   out = g * US + parity;  a read outside [0, h) x [0, w) is zero.
// The weight array is Keras': (3,3,Cin,Cout) for the conv modes, (3,3,Cout,Cin) for the transposed ones, so backward-data
// of a layer is the opposite family's forward on the layer's own array, channel counts swapped, without bias.
//
// Forward, fast path (Cin % 4 == 0, Cout % 4 == 0): implicit GEMM on v_mfma_f32_16x16x4_f32.  A workgroup (4 waves) owns
// 8 x 8 grid texels x TN = 16 NB output channels.  Per 16-channel slice of Cin it stages the input tile with its halo and
// the live taps' weights in LDS (16-byte global loads along the channel axis) and loops the taps over that image.  Both
// operands are read with one 16-byte LDS load per lane: lane (i, kg) holds channels 4 kg + r, r = 0..3, of its texel / its
// output channel, and MFMA step r contracts them -- a permutation of k shared by A and B.
// Forward, any channel count: one thread per output element.
// Weight gradient: stage one gives every wave a (tap, 16 Cin, <= 64 Cout) block and a slice of the grid rows and writes its
// partial sums to the workspace; stage two adds the slices in index order onto the destination.  No float atomics.
#include "nlt_common.h"

namespace {

constexpr int K3_T = 8;             // grid texels per tile edge
constexpr int K3_KC = 16;           // input channels staged per pass
constexpr int K3_XS = K3_KC + 4;    // LDS floats per staged texel (80 B: 16-byte aligned, 5 slots apart)

struct K3P {
  const float* x; const float* wgt; const float* bias; float* y;
  const float* g;               // weight gradient: dpre [n, oh, ow, cout]
  int mode, deconv;             // deconv: the array is (3,3,Cout,Cin)
  int n, h, w, cin, cout;       // input dims
  int gh, gw, oh, ow;
  int S, OFF, US;
  int it;                       // staged tile edge: (K3_T - 1) * S + max dy + 1
  int tiles_y, tiles_x;
  int act; float alpha;
};

__host__ __device__ __forceinline__ int k3_ntaps(int mode, int par) { return mode == NLT_DECONV_K3S2 ? (par ? 1 : 2) : 3; }
__host__ __device__ __forceinline__ int k3_tap(int mode, int par, int t) { return mode == NLT_DECONV_K3S2 ? (par ? 1 : 2 * t) : t; }
__host__ __device__ __forceinline__ int k3_dy(int mode, int a) {
  if (mode == NLT_DECONV_K3S2) return a == 2 ? 0 : 1;
  if (mode == NLT_DECONV_K3S1) return 2 - a;
  return a;
}

__device__ __forceinline__ long k3_widx(const K3P& p, int tap, int c, int o) {
  return p.deconv ? ((long)tap * p.cout + o) * p.cin + c : ((long)tap * p.cin + c) * p.cout + o;
}

template <int NB>
__global__ __launch_bounds__(256) void k3_mfma_kernel(const K3P p) {
  extern __shared__ __attribute__((aligned(16))) char k3_smem[];
  constexpr int TN = 16 * NB;
  float* xs = reinterpret_cast<float*>(k3_smem);                 // [it * it texels][K3_XS]
  float* ws = xs + p.it * p.it * K3_XS;                          // [live tap][4 k groups][TN][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kg = lane >> 4;

  int t = blockIdx.x;
  const int tx = t % p.tiles_x; t /= p.tiles_x;
  const int ty = t % p.tiles_y; t /= p.tiles_y;
  const int cls = p.mode == NLT_DECONV_K3S2 ? (t & 3) : 0;
  const int f = p.mode == NLT_DECONV_K3S2 ? (t >> 2) : t;
  const int pm = cls >> 1, pn = cls & 1;
  const int nty = k3_ntaps(p.mode, pm), ntx = k3_ntaps(p.mode, pn);
  const int gy0 = ty * K3_T, gx0 = tx * K3_T;
  const int iy0 = gy0 * p.S + p.OFF, ix0 = gx0 * p.S + p.OFF;
  const int o0 = blockIdx.y * TN;

  f32x4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lr = 2 * wave + (li >> 3), lc = li & 7;              // this lane's A row: a texel of the tile
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < p.cin; c0 += K3_KC) {
    __syncthreads();
    for (int idx = tid; idx < p.it * p.it * 4; idx += 256) {     // input tile + halo, one channel quad per thread
      const int tex = idx >> 2, q = idx & 3;
      const int iy = iy0 + tex / p.it, ix = ix0 + tex % p.it, c = c0 + 4 * q;
      f32x4 v = zero4;
      if (iy >= 0 && iy < p.h && ix >= 0 && ix < p.w && c < p.cin)
        v = *reinterpret_cast<const f32x4*>(p.x + (((long)f * p.h + iy) * p.w + ix) * p.cin + c);
      *reinterpret_cast<f32x4*>(xs + tex * K3_XS + 4 * q) = v;
    }
    const int nw = nty * ntx * 4 * TN;                           // float4s of the live taps' weight slice
    for (int idx = tid; idx < nw; idx += 256) {
      if (p.deconv) {                                            // (3,3,Cout,Cin): the vector runs along Cin
        const int c4 = idx & 3, ol = (idx >> 2) % TN, tapi = idx / (4 * TN);
        const int tap = k3_tap(p.mode, pm, tapi / ntx) * 3 + k3_tap(p.mode, pn, tapi % ntx);
        const int c = c0 + 4 * c4, o = o0 + ol;
        f32x4 v = zero4;
        if (c < p.cin && o < p.cout) v = *reinterpret_cast<const f32x4*>(p.wgt + ((long)tap * p.cout + o) * p.cin + c);
        *reinterpret_cast<f32x4*>(ws + ((tapi * 4 + c4) * TN + ol) * 4) = v;
      } else {                                                   // (3,3,Cin,Cout): the vector runs along Cout
        const int o4 = idx % (TN / 4), cl = (idx / (TN / 4)) & 15, tapi = idx / (4 * TN);
        const int tap = k3_tap(p.mode, pm, tapi / ntx) * 3 + k3_tap(p.mode, pn, tapi % ntx);
        const int c = c0 + cl, o = o0 + 4 * o4;
        f32x4 v = zero4;
        if (c < p.cin && o < p.cout) v = *reinterpret_cast<const f32x4*>(p.wgt + ((long)tap * p.cin + c) * p.cout + o);
        float* d = ws + ((tapi * 4 + (cl >> 2)) * TN + 4 * o4) * 4 + (cl & 3);
        d[0] = v[0]; d[4] = v[1]; d[8] = v[2]; d[12] = v[3];
      }
    }
    __syncthreads();
    for (int ity = 0; ity < nty; ++ity) {
      const int dy = k3_dy(p.mode, k3_tap(p.mode, pm, ity));
      for (int itx = 0; itx < ntx; ++itx) {
        const int dx = k3_dy(p.mode, k3_tap(p.mode, pn, itx));
        const int tex = (lr * p.S + dy) * p.it + lc * p.S + dx;
        const f32x4 a = *reinterpret_cast<const f32x4*>(xs + tex * K3_XS + 4 * kg);
        const float* wt = ws + (((ity * ntx + itx) * 4 + kg) * TN + li) * 4;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const f32x4 b = *reinterpret_cast<const f32x4*>(wt + nb * 64);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], b[r], acc[nb], 0, 0, 0);
        }
      }
    }
  }

#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int o = o0 + nb * 16 + li;
    if (o >= p.cout) continue;
    const float bv = p.bias ? p.bias[o] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * kg + r;                                // D: row = 4 (lane >> 4) + r, column = lane & 15
      const int gy = gy0 + 2 * wave + (row >> 3), gx = gx0 + (row & 7);
      if (gy >= p.gh || gx >= p.gw) continue;
      float v = acc[nb][r] + bv;
      if (p.act) v = v > 0.f ? v : p.alpha * v;
      p.y[(((long)f * p.oh + gy * p.US + pm) * p.ow + gx * p.US + pn) * p.cout + o] = v;
    }
  }
}

__global__ __launch_bounds__(256) void k3_direct_kernel(const K3P p, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int o = (int)(idx % p.cout);
  long t = idx / p.cout;
  const int ox = (int)(t % p.ow); t /= p.ow;
  const int oy = (int)(t % p.oh);
  const int f = (int)(t / p.oh);
  const int pm = p.US == 2 ? (oy & 1) : 0, pn = p.US == 2 ? (ox & 1) : 0;
  const int gy = oy / p.US, gx = ox / p.US;
  float v = p.bias ? p.bias[o] : 0.f;
  const int nty = k3_ntaps(p.mode, pm), ntx = k3_ntaps(p.mode, pn);
  for (int ity = 0; ity < nty; ++ity) {
    const int a = k3_tap(p.mode, pm, ity);
    const int iy = gy * p.S + p.OFF + k3_dy(p.mode, a);
    if (iy < 0 || iy >= p.h) continue;
    for (int itx = 0; itx < ntx; ++itx) {
      const int b = k3_tap(p.mode, pn, itx);
      const int ix = gx * p.S + p.OFF + k3_dy(p.mode, b);
      if (ix < 0 || ix >= p.w) continue;
      const float* xp = p.x + (((long)f * p.h + iy) * p.w + ix) * p.cin;
      for (int c = 0; c < p.cin; ++c) v = fmaf(xp[c], p.wgt[k3_widx(p, a * 3 + b, c, o)], v);
    }
  }
  if (p.act) v = v > 0.f ? v : p.alpha * v;
  p.y[idx] = v;
}

// Stage one of the weight gradient: one wave per (tap, 16 input channels, <= 64 output channels) x slice of grid rows.
// A[i = input channel][k = row], B[k = row][j = output channel]; partial[slice][tap][c][o] in the workspace.
__global__ __launch_bounds__(64) void k3_wgrad_partial_kernel(const K3P p, float* ws, int rows, int chunk, int cblocks, int ogroups) {
  const int lane = threadIdx.x, li = lane & 15, kg = lane >> 4;
  int t = blockIdx.x;
  const int og = t % ogroups; t /= ogroups;
  const int cb = t % cblocks;
  const int tap = t / cblocks;
  const int a = tap / 3, b = tap % 3;
  const int dy = k3_dy(p.mode, a), dx = k3_dy(p.mode, b);
  const int pm = p.US == 2 ? (a & 1) : 0, pn = p.US == 2 ? (b & 1) : 0;
  const int r_begin = blockIdx.y * chunk, r_end = min(rows, r_begin + chunk);
  const int c = cb * 16 + li;
  const int oblocks = (p.cout + 15) >> 4;
  const int nbv = min(4, oblocks - og * 4);
  f32x4 acc[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int r0 = r_begin; r0 < r_end; r0 += 4) {
    const int r = r0 + kg;
    const bool live = r < r_end;
    const int gx = r % p.gw, gy = (r / p.gw) % p.gh, f = r / (p.gw * p.gh);
    const int iy = gy * p.S + p.OFF + dy, ix = gx * p.S + p.OFF + dx;
    float av = 0.f;
    if (live && c < p.cin && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w)
      av = p.x[(((long)f * p.h + iy) * p.w + ix) * p.cin + c];
    const float* gp = p.g + (((long)f * p.oh + gy * p.US + pm) * p.ow + gx * p.US + pn) * p.cout;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      if (nb < nbv) {
        const int o = (og * 4 + nb) * 16 + li;
        const float bv = (live && o < p.cout) ? gp[o] : 0.f;
        acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[nb], 0, 0, 0);
      }
    }
  }
  float* part = ws + ((long)blockIdx.y * 9 + tap) * p.cin * p.cout;
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    if (nb >= nbv) continue;
    const int o = (og * 4 + nb) * 16 + li;
    if (o >= p.cout) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cc = cb * 16 + 4 * kg + r;
      if (cc < p.cin) part[(long)cc * p.cout + o] = acc[nb][r];
    }
  }
}

// Bias partials: workgroup `s` sums its slice of dpre's texels per channel, four strided runs met in LDS in a fixed order.
__global__ __launch_bounds__(256) void k3_bgrad_partial_kernel(const float* g, long texels, long chunk, int cout, float* wsb) {
  __shared__ float part[256];
  const int sub = threadIdx.x >> 6, ol = threadIdx.x & 63;
  const long t_begin = blockIdx.x * chunk, t_end = min(texels, t_begin + chunk);
  for (int o0 = 0; o0 < cout; o0 += 64) {
    const int o = o0 + ol;
    float s = 0.f;
    if (o < cout)
      for (long tx = t_begin + sub; tx < t_end; tx += 4) s += g[tx * cout + o];
    __syncthreads();
    part[threadIdx.x] = s;
    __syncthreads();
    if (sub == 0 && o < cout) wsb[(long)blockIdx.x * cout + o] = ((part[ol] + part[64 + ol]) + part[128 + ol]) + part[192 + ol];
  }
}

// Stage two: slices added in index order, then onto the destination (Keras layout of the layer's family).
__global__ __launch_bounds__(256) void k3_wgrad_reduce_kernel(const float* ws, const float* wsb, int slices, int bslices, int cin, int cout,
                                                              int deconv, float* dw, float* db) {
  const long per = 9l * cin * cout;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < per) {
    float s = 0.f;
    for (int i = 0; i < slices; ++i) s += ws[i * per + e];
    long dst = e;
    if (deconv) {
      const int o = (int)(e % cout), c = (int)((e / cout) % cin), tap = (int)(e / ((long)cin * cout));
      dst = ((long)tap * cout + o) * cin + c;
    }
    dw[dst] += s;
  } else if (e < per + cout && db) {
    const int o = (int)(e - per);
    float s = 0.f;
    for (int i = 0; i < bslices; ++i) s += wsb[(long)i * cout + o];
    db[o] += s;
  }
}

bool k3_is_mode(int mode) { return mode >= NLT_CONV_K3S1 && mode <= NLT_DECONV_K3S2; }

// Geometry of `mode` on an [n, h, w, cin] input; no pointer is looked at.
int k3_fill(K3P& p, int mode, int n, int h, int w, int cin, int cout) {
  if (!k3_is_mode(mode)) return NLT_ERR_BAD_ARG;
  if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0) return NLT_ERR_BAD_ARG;
  p = K3P{};
  p.mode = mode; p.deconv = mode == NLT_DECONV_K3S1 || mode == NLT_DECONV_K3S2;
  p.n = n; p.h = h; p.w = w; p.cin = cin; p.cout = cout;
  p.gh = p.oh = h; p.gw = p.ow = w; p.S = 1; p.OFF = -1; p.US = 1;
  int dmax = 2;
  if (mode == NLT_CONV_K3S2) {
    if ((h | w) & 1) return NLT_ERR_UNSUPPORTED;
    p.gh = p.oh = h / 2; p.gw = p.ow = w / 2; p.S = 2; p.OFF = 0;
  } else if (mode == NLT_DECONV_K3S2) {
    p.oh = 2 * h; p.ow = 2 * w; p.US = 2; dmax = 1;
  }
  p.it = (K3_T - 1) * p.S + dmax + 1;
  p.tiles_y = (p.gh + K3_T - 1) / K3_T; p.tiles_x = (p.gw + K3_T - 1) / K3_T;
  const long long lim = 1ll << 31;
  if ((long long)n * h * w * cin >= lim || (long long)n * p.oh * p.ow * cout >= lim || 9ll * cin * cout >= lim) return NLT_ERR_UNSUPPORTED;
  return NLT_OK;
}

template <int NB>
int k3_launch_mfma(const K3P& p, hipStream_t s) {
  const int TN = 16 * NB;
  const size_t lds = sizeof(float) * ((size_t)p.it * p.it * K3_XS + 9 * 4 * TN * 4);
  const long tiles = (long)p.n * (p.mode == NLT_DECONV_K3S2 ? 4 : 1) * p.tiles_y * p.tiles_x;
  if (tiles >= (1l << 31) || lds > 64 * 1024) return NLT_ERR_UNSUPPORTED;
  dim3 grid((unsigned)tiles, (unsigned)((p.cout + TN - 1) / TN));
  hipLaunchKernelGGL(k3_mfma_kernel<NB>, grid, dim3(256), lds, s, p);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

int k3_forward(K3P& p, int algo, hipStream_t s) {
  const bool can_mfma = p.cin % 4 == 0 && p.cout % 4 == 0 && nlt_aligned16(p.x) && nlt_aligned16(p.wgt);
  if (algo == NLT_ALGO_AUTO) algo = can_mfma ? NLT_ALGO_MFMA : NLT_ALGO_DIRECT;
  if (algo == NLT_ALGO_MFMA) {
    if (!can_mfma) return NLT_ERR_UNSUPPORTED;
    if (p.cout > 32) return k3_launch_mfma<4>(p, s);
    if (p.cout > 16) return k3_launch_mfma<2>(p, s);
    return k3_launch_mfma<1>(p, s);
  }
  if (algo != NLT_ALGO_DIRECT) return NLT_ERR_BAD_ARG;
  const long total = (long)p.n * p.oh * p.ow * p.cout;
  hipLaunchKernelGGL(k3_direct_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, total);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

// Slices of the weight-gradient sums: a function of the shapes alone (the order of every sum is fixed by it).
struct K3Slices { int rows, chunk, slices, cblocks, ogroups; long btexels, bchunk; };

K3Slices k3_slices(const K3P& p) {
  K3Slices q;
  q.rows = p.n * p.gh * p.gw;
  q.cblocks = (p.cin + 15) / 16;
  q.ogroups = ((p.cout + 15) / 16 + 3) / 4;
  const long tiles = 9l * q.cblocks * q.ogroups;
  long want = (4096 + tiles - 1) / tiles;
  const long most = (q.rows + 63) / 64;
  if (want > most) want = most;
  if (want < 1) want = 1;
  q.chunk = (int)(((q.rows + want - 1) / want + 3) / 4 * 4);
  q.slices = (q.rows + q.chunk - 1) / q.chunk;
  q.btexels = (long)p.n * p.oh * p.ow;
  q.bchunk = (q.btexels + q.slices - 1) / q.slices;
  return q;
}

}  // namespace

extern "C" int nlt_conv_k3_forward(int mode, int algo, const float* x, int n, int h, int w, int cin,
                                   const float* w_keras, const float* bias, int cout, float* y,
                                   int act, float alpha, void* stream) {
  if (!x || !w_keras || !bias || !y) return NLT_ERR_BAD_ARG;
  K3P p;
  const int st = k3_fill(p, mode, n, h, w, cin, cout);
  if (st != NLT_OK) return st;
  p.x = x; p.wgt = w_keras; p.bias = bias; p.y = y; p.act = act; p.alpha = alpha;
  return k3_forward(p, algo, static_cast<hipStream_t>(stream));
}

extern "C" int nlt_conv_k3_backward_data(int mode, int algo, const float* dpre, int n, int h, int w, int cin,
                                         const float* w_keras, int cout, float* dx, void* stream) {
  if (!dpre || !w_keras || !dx) return NLT_ERR_BAD_ARG;
  K3P fwd;
  int st = k3_fill(fwd, mode, n, h, w, cin, cout);                // the layer itself: validates (h, w) and gives dpre's dims
  if (st != NLT_OK) return st;
  const int adj = mode == NLT_CONV_K3S1 ? NLT_DECONV_K3S1 : mode == NLT_CONV_K3S2 ? NLT_DECONV_K3S2
                : mode == NLT_DECONV_K3S1 ? NLT_CONV_K3S1 : NLT_CONV_K3S2;
  K3P p;
  st = k3_fill(p, adj, n, fwd.oh, fwd.ow, cout, cin);              // the opposite family on dpre, channel axes swapped
  if (st != NLT_OK) return st;
  if (p.oh != h || p.ow != w) return NLT_ERR_BAD_ARG;
  p.x = dpre; p.wgt = w_keras; p.bias = nullptr; p.y = dx; p.act = 0; p.alpha = 0.f;
  return k3_forward(p, algo, static_cast<hipStream_t>(stream));
}

extern "C" long nlt_conv_k3_wgrad_workspace_floats(int mode, int n, int h, int w, int cin, int cout) {
  K3P p;
  if (k3_fill(p, mode, n, h, w, cin, cout) != NLT_OK) return -1;
  const K3Slices q = k3_slices(p);
  return (long)q.slices * (9l * cin * cout + cout);
}

extern "C" int nlt_conv_k3_backward_weights(int mode, const float* x, int n, int h, int w, int cin,
                                            const float* dpre, int cout, float* dw_keras, float* dbias,
                                            float* workspace, long workspace_floats, void* stream) {
  if (!x || !dpre || !dw_keras || !workspace) return NLT_ERR_BAD_ARG;
  K3P p;
  const int st = k3_fill(p, mode, n, h, w, cin, cout);
  if (st != NLT_OK) return st;
  const K3Slices q = k3_slices(p);
  const long per = 9l * cin * cout;
  if (workspace_floats < (long)q.slices * (per + cout)) return NLT_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  p.x = x; p.g = dpre;
  float* wsb = workspace + (long)q.slices * per;
  hipLaunchKernelGGL(k3_wgrad_partial_kernel, dim3(9u * q.cblocks * q.ogroups, (unsigned)q.slices), dim3(64), 0, s,
                     p, workspace, q.rows, q.chunk, q.cblocks, q.ogroups);
  NLT_CHECK_LAUNCH();
  if (dbias) {
    hipLaunchKernelGGL(k3_bgrad_partial_kernel, dim3((unsigned)q.slices), dim3(256), 0, s, dpre, q.btexels, q.bchunk, cout, wsb);
    NLT_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k3_wgrad_reduce_kernel, dim3((unsigned)((per + cout + 255) / 256)), dim3(256), 0, s,
                     workspace, wsb, q.slices, q.slices, cin, cout, p.deconv, dw_keras, dbias);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}
