// Weight / bias gradients of the NARROW layers (few output columns):  dW[k][n] = sum_rows X[row][k] * dP[row][n]
// with N = cout (4 * cout for Conv2DTranspose k2s2) <= 32 and K = taps * cin <= 128.
//
// wgrad_tile.hip feeds 16 MFMAs from two 16-byte loads, but its 64 x 64 block of dW is mostly padding when the layer
// has 8 / 16 / 32 output channels (16 -> 16: a quarter of the matrix-core work is useful, and that work was the
// kernel's time).  Here the MFMA tile is matched to the layer instead: rows of dW = K index (tap, channel), 16 per
// M tile; columns = output channel, 16 per N tile; the reduction (MFMA K dimension) runs over texel rows, 4 per
// v_mfma_f32_16x16x4_f32.  Operands are 4-byte loads -- lane (i, kk) reads X[row kk][k = 16 mt + i] and
// dP[row kk][n = 16 nt + i], 16 consecutive floats per row -- MT + NT loads feed MT * NT MFMAs, all of them useful.
// Any channel count works (no quad alignment).  Row slices -> workspace -> fixed-order reduction, as in wgrad_tile.
#include "wgrad_common.h"
#include <type_traits>

namespace {

struct WN {
  ConvP c;
  const float* dp; int ldp;
  float* dw; float* db; float* ws;
  const float* zeros;           // zero page (walk form) or nullptr (index-deriving form)
  int K, N;                     // taps * (c0 + c1), GEMM columns
  int msplits, rows_per_split;
};

// One slice's workspace block: [K padded to MT * 16][NC] floats + NC column sums of dP.
template <int MT, int NT>
struct NarrowBlock { static constexpr int NC = NT * 16, KN = MT * 16 * NC, PER = KN + NC; };

// Scalar-A form: any channel count and leading dimension; the rows re-derived per step (RowCursor).
template <int MODE, int MT, int NT>
__global__ __launch_bounds__(256) void wgrad_narrow_kernel(WN w) {
  extern __shared__ float xch[];                                       // one wave's block: [MT*16][NT*16] + [NT*16] column sums
  const ConvP& p = w.c;
  constexpr int TAPS = MODE == NLT_DECONV_K2S2 ? 1 : 4;
  constexpr int S = MODE == NLT_CONV_K2S2 ? 2 : 1;                     // input rows per GEMM-grid row
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, kk = lane >> 4;
  const int ms = blockIdx.x;

  // A role per M tile: K index 16 mt + i, input texel of a row = (S * y + oy, S * x + ox); B role per N tile
  ARole<1> ar[MT]; int oy[MT], ox[MT], tdelta[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    ar[mt] = ARole<1>(mt * 16 + i, w.K, p);
    const int a = TAPS == 4 ? ar[mt].ta() : 0, b = TAPS == 4 ? ar[mt].tb() : 0;
    oy[mt] = MODE == NLT_DECONV_K2S1 ? -a : a;
    ox[mt] = MODE == NLT_DECONV_K2S1 ? -b : b;
    tdelta[mt] = oy[mt] * p.w + ox[mt];
  }
  BRole<MODE> br[NT]; int bdelta[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    br[nt] = BRole<MODE>(nt * 16 + i, w.N, p);
    bdelta[nt] = (br[nt].ab >> 1) * p.ow + (br[nt].ab & 1);
  }

  f32x4 acc[MT * NT];
  float bsum[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    bsum[nt] = 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt * NT + nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  RowCursor c;
  c.init(ms * w.rows_per_split, w.rows_per_split, wv, kk, p);
  auto issue = [&](float (&av)[MT], float (&bv)[NT]) {
    const bool rv = c.valid();
    const int ys = S * c.ry, xs = S * c.rx;
    const int rowtex = (c.rf * p.h + ys) * p.w + xs;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const bool ok = rv && ar[mt].ok && (unsigned)(ys + oy[mt]) < (unsigned)p.h && (unsigned)(xs + ox[mt]) < (unsigned)p.w;
      const int tex = ok ? rowtex + tdelta[mt] : 0;
      const float v = ar[mt].src[(size_t)tex * ar[mt].ld];                // unconditional, clamped address
      av[mt] = ok ? v : 0.f;
    }
    const int rowo = MODE == NLT_DECONV_K2S2 ? (c.rf * p.oh + 2 * c.ry) * p.ow + 2 * c.rx : c.m;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const bool ok = rv && br[nt].ok;
      const int otex = ok ? rowo + bdelta[nt] : 0;
      const float v = w.dp[(size_t)otex * w.ldp + br[nt].off];
      bv[nt] = ok ? v : 0.f;
    }
    c.advance16(p);
  };
  auto compute = [&](const float (&av)[MT], const float (&bv)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      bsum[nt] += bv[nt];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt * NT + nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[nt], acc[mt * NT + nt], 0, 0, 0);
    }
  };
  // (RowCursor::rotate3 written out: through the function, wgrad_narrow_kernel<NLT_DECONV_K2S2, 8, 1> loses a wave of occupancy)
  float a0[MT], b0[NT], a1[MT], b1[NT], a2[MT], b2[NT];
  issue(a0, b0);
  issue(a1, b1);
  for (int s3 = 0; s3 < c.nsteps; s3 += 3) {                           // steps past nsteps carry zero operands
    issue(a2, b2); compute(a0, b0);
    issue(a0, b0); compute(a1, b1);
    issue(a1, b1); compute(a2, b2);
  }

  // waves 1..3 hand their blocks to wave 0 one after the other; accumulator (mt, nt), D row 4 kk + r: K index 16 mt + 4 kk + r
  using Blk = NarrowBlock<MT, NT>;
  ColumnSums<NT> cols{bsum, Blk::KN + i, kk == 0};
  cols.across_row_groups();
  auto slot = [i, kk](int j, int r) { return (16 * (j / NT) + 4 * kk + r) * Blk::NC + (j % NT) * 16 + i; };
  wave_order_sum(xch, wv, acc, slot, cols);
  if (wv) return;
  float* dst = w.ws + (size_t)ms * Blk::PER;
  store_block(dst, acc, slot);
  cols.put(dst);
}

// Quad-A form (channel counts and leading dimensions multiples of 4, 16-byte aligned sources): ONE 16-byte load per lane brings the
// four K values of a channel quad, so a 64-entry slice of K (= all four taps of a 16-channel layer) costs one load + one address
// computation instead of four; tile e of the four MFMA row tiles it feeds holds K indices 4 * quad + e, i.e. the same [K][N]
// workspace layout as the scalar form above.  B stays one 4-byte load per 16 columns.
// WALK (row grid a multiple of 4 texels wide -- every released shape): the rows are walked (RowWalk) instead of re-derived
// (RowCursor), and the loads run PF - 1 steps ahead.  The re-deriving form's ~70 VALU instructions of index arithmetic per step
// (for 4 to 16 MFMAs) were this kernel's time.
template <int MQ, int NT> struct NarrowPF { static constexpr int value = MQ * NT >= 4 ? 6 : 8; };

template <int MODE, int MQ, int NT, bool WALK>
__global__ __launch_bounds__(256) void wgrad_narrowq_kernel(WN w) {
  extern __shared__ float xch[];
  const ConvP& p = w.c;
  constexpr int TAPS = MODE == NLT_DECONV_K2S2 ? 1 : 4;
  constexpr int S = MODE == NLT_CONV_K2S2 ? 2 : 1;                     // input rows per GEMM-grid row
  using Blk = NarrowBlock<4 * MQ, NT>;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, kk = lane >> 4;
  const int ms = blockIdx.x;

  // A role per M tile: input texel of a row = (S * y + oy, S * x + ox); B role per N tile
  ARole<4> ar[MQ]; int oy[MQ], ox[MQ], tdelta[MQ];
#pragma unroll
  for (int mq = 0; mq < MQ; ++mq) {
    ar[mq] = ARole<4>(mq * 16 + i, w.K >> 2, p);
    const int a = TAPS == 4 ? ar[mq].ta() : 0, b = TAPS == 4 ? ar[mq].tb() : 0;
    oy[mq] = MODE == NLT_DECONV_K2S1 ? -a : a;
    ox[mq] = MODE == NLT_DECONV_K2S1 ? -b : b;
    tdelta[mq] = oy[mq] * p.w + ox[mq];
  }
  BRole<MODE> br[NT]; int bdelta[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    br[nt] = BRole<MODE>(nt * 16 + i, w.N, p);
    bdelta[nt] = (br[nt].ab >> 1) * p.ow + (br[nt].ab & 1);
  }

  f32x4 acc[MQ * 4 * NT];                                              // [mq][e][nt]
  float bsum[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) bsum[nt] = 0.f;
#pragma unroll
  for (int j = 0; j < MQ * 4 * NT; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto compute = [&](const f32x4 (&av)[MQ], const float (&bv)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      bsum[nt] += bv[nt];
#pragma unroll
      for (int mq = 0; mq < MQ; ++mq)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          acc[(mq * 4 + e) * NT + nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mq][e], bv[nt], acc[(mq * 4 + e) * NT + nt], 0, 0, 0);
    }
  };

  if constexpr (WALK) {
    using Walk = RowWalk<MODE>;
    Walk k;
    k.start(ms, __builtin_amdgcn_readfirstlane(wv), w.rows_per_split, p);   // (rows_per_split: a multiple of 16 * PF rows)
    const float* pa[MQ]; int ainc[MQ], aincw[MQ]; typename Walk::TapBounds tb[MQ];
#pragma unroll
    for (int mq = 0; mq < MQ; ++mq) {
      const int a = oy[mq] < 0 ? -oy[mq] : oy[mq], b = ox[mq] < 0 ? -ox[mq] : ox[mq];
      // an empty run (slice past M) must not form an address past the buffer
      pa[mq] = k.nsteps > 0 ? ar[mq].src + k.a_start_texel(a, b, kk, p) * ar[mq].ld : ar[mq].src;
      ainc[mq] = Walk::a_inc(ar[mq].ld);
      aincw[mq] = Walk::a_inc_wrap(ar[mq].ld, p);
      tb[mq] = Walk::tap_bounds(a, b, kk, p);
    }
    const float* pb[NT]; int binc[NT], bincw[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      pb[nt] = k.nsteps > 0 ? w.dp + k.b_start_texel(br[nt].ab, kk, p) * w.ldp + br[nt].off : w.zeros;
      binc[nt] = Walk::b_inc(w.ldp);
      bincw[nt] = Walk::b_inc_wrap(w.ldp, p);
    }
    const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto issue = [&](f32x4 (&av)[MQ], float (&bv)[NT]) {
#pragma unroll
      for (int mq = 0; mq < MQ; ++mq) {
        if (Walk::PADS) {
          const bool ok = MODE == NLT_CONV_K2S1 ? (k.x0 < tb[mq].xlim && k.y < tb[mq].ylim) : (k.x0 >= tb[mq].xlo && k.y >= tb[mq].ylo);
          const f32x4 v = *reinterpret_cast<const f32x4*>(ok ? pa[mq] : ar[mq].src);   // a padded tap must not be dereferenced
          av[mq] = ok ? v : zero4;
        } else {
          av[mq] = *reinterpret_cast<const f32x4*>(pa[mq]);
        }
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bv[nt] = *pb[nt];
      const bool adv = k.advances(), wrap = k.wraps(p);
#pragma unroll
      for (int mq = 0; mq < MQ; ++mq) {
        const float* nx = pa[mq] + (wrap ? aincw[mq] : ainc[mq]);
        pa[mq] = adv ? nx : pa[mq];
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float* nx = pb[nt] + (wrap ? bincw[nt] : binc[nt]);
        pb[nt] = adv ? nx : w.zeros;
      }
      k.move_on(adv, wrap, p);
    };
    k.template pipeline<NarrowPF<MQ, NT>::value, f32x4[MQ], float[NT]>(issue, compute);
  } else {
    RowCursor c;
    c.init(ms * w.rows_per_split, w.rows_per_split, wv, kk, p);
    auto issue = [&](f32x4 (&av)[MQ], float (&bv)[NT]) {
      const bool rv = c.valid();
      const int ys = S * c.ry, xs = S * c.rx;
      const int rowtex = (c.rf * p.h + ys) * p.w + xs;
#pragma unroll
      for (int mq = 0; mq < MQ; ++mq) {
        const bool ok = rv && ar[mq].ok && (unsigned)(ys + oy[mq]) < (unsigned)p.h && (unsigned)(xs + ox[mq]) < (unsigned)p.w;
        const int tex = ok ? rowtex + tdelta[mq] : 0;
        const f32x4 v = *reinterpret_cast<const f32x4*>(ar[mq].src + (size_t)tex * ar[mq].ld);   // unconditional, clamped address
        av[mq] = ok ? v : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
      const int rowo = MODE == NLT_DECONV_K2S2 ? (c.rf * p.oh + 2 * c.ry) * p.ow + 2 * c.rx : c.m;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const bool ok = rv && br[nt].ok;
        const int otex = ok ? rowo + bdelta[nt] : 0;
        const float v = w.dp[(size_t)otex * w.ldp + br[nt].off];
        bv[nt] = ok ? v : 0.f;
      }
      c.advance16(p);
    };
    c.template rotate3<f32x4[MQ], float[NT]>(issue, compute);
  }

  // waves 1..3 hand their blocks to wave 0 one after the other; K index of accumulator (mq, e), D row 4 kk + r:  4 * (16 mq + 4 kk + r) + e
  ColumnSums<NT> cols{bsum, Blk::KN + i, kk == 0};
  cols.across_row_groups();
  auto slot = [i, kk](int j, int r) {
    const int nt = j % NT, e = (j / NT) % 4, mq = j / (NT * 4);
    return (4 * (16 * mq + 4 * kk + r) + e) * Blk::NC + nt * 16 + i;
  };
  wave_order_sum(xch, wv, acc, slot, cols);
  if (wv) return;
  float* dst = w.ws + (size_t)ms * Blk::PER;
  store_block(dst, acc, slot);
  cols.put(dst);
}

// Pass 2: 32 entries of the [K pad][N pad] block (+ the column sums) per workgroup: thread (q, g) adds the slices g, g + 32, ...
// of the entry QUAD q with 16-byte loads, 8 in flight (whole 128-byte lines per slice; ~2000 slices of 16 KB are 34 MB -- the
// 4-byte, 4-stream form of round 2 took 15-23 us for them, pure latency), fixed order.
template <int MODE, int MT, int NT>
__global__ __launch_bounds__(256) void wgrad_narrow_reduce_kernel(WN w) {
  __shared__ __attribute__((aligned(16))) float part[32][32];
  using Blk = NarrowBlock<MT, NT>;
  constexpr int NC = Blk::NC, KN = Blk::KN, PER = Blk::PER;             // PER is a multiple of 16
  const ConvP& p = w.c;
  const int q = threadIdx.x & 7, g = threadIdx.x >> 3;
  const int base = blockIdx.x * 32 + 4 * q;
  const bool live = base < PER;
  const f32x4* src = reinterpret_cast<const f32x4*>(w.ws + (live ? base : 0));
  constexpr size_t stride = PER / 4;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
  int ms = g;
  for (; ms + 224 < w.msplits; ms += 256) {
    f32x4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[(size_t)(ms + 32 * j) * stride];
    s0 += (v[0] + v[1]) + (v[2] + v[3]);
    s1 += (v[4] + v[5]) + (v[6] + v[7]);
  }
  for (; ms < w.msplits; ms += 32) s0 += src[(size_t)ms * stride];
  reinterpret_cast<f32x4*>(&part[g][0])[q] = s0 + s1;
  __syncthreads();
  if (threadIdx.x >= 32) return;
  const int e = threadIdx.x;
  const int idx = blockIdx.x * 32 + e;
  if (idx >= PER) return;
  float t[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    t[a] = 0.f;
#pragma unroll
    for (int b = 0; b < 8; ++b) t[a] += part[8 * a + b][e];
  }
  const float s = (t[0] + t[1]) + (t[2] + t[3]);
  const int cin = p.c0 + p.c1;
  if (idx < KN) {
    const int kidx = idx / NC, n = idx - kidx * NC;
    if (kidx >= w.K || n >= w.N) return;
    const int tap = kidx / cin, c = kidx - tap * cin;
    w.dw[nlt_keras_widx<MODE>(tap, c, n, cin, p.cout, p.cout, 0)] += s;
  } else if (w.db) {
    const int n = idx - KN;
    if (n >= w.N) return;
    if (MODE != NLT_DECONV_K2S2) w.db[n] += s;
    else w.ws[(size_t)w.msplits * PER + n] = s;                        // 4 (a,b) column groups per output channel: next launch
  }
}

// Conv2DTranspose k2s2 bias: db[o] = sum_ab colsum[ab * cout + o]
template <int MT, int NT>
__global__ void wgrad_narrow_bias_k2s2_kernel(WN w) {
  const int o = threadIdx.x;
  if (o >= w.c.cout) return;
  const float* tot = w.ws + (size_t)w.msplits * NarrowBlock<MT, NT>::PER;
  w.db[o] += (tot[o] + tot[w.c.cout + o]) + (tot[2 * w.c.cout + o] + tot[3 * w.c.cout + o]);
}

// Pass 2 and what follows it, after any of the slice kernels
template <int MODE, int MT, int NT>
int narrow_tail(WN& w, hipStream_t s) {
  hipLaunchKernelGGL((wgrad_narrow_reduce_kernel<MODE, MT, NT>), dim3((NarrowBlock<MT, NT>::PER + 31) / 32), dim3(256), 0, s, w);
  if (MODE == NLT_DECONV_K2S2 && w.db) hipLaunchKernelGGL((wgrad_narrow_bias_k2s2_kernel<MT, NT>), dim3(1), dim3(64), 0, s, w);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

template <int MODE, int MT, int NT>
int run_narrow(WN& w, hipStream_t s) {
  constexpr size_t lds = NarrowBlock<MT, NT>::PER * sizeof(float);
  hipLaunchKernelGGL((wgrad_narrow_kernel<MODE, MT, NT>), dim3((unsigned)w.msplits), dim3(256), lds, s, w);
  return narrow_tail<MODE, MT, NT>(w, s);
}

// The row-walking loop pays for every shape except the k2s1 families at K = 128, N = 32 (two A quads x two column tiles: 260 VALU
// instructions of padding checks per 6 steps at 2 waves per SIMD -- measured 55-57 us against 44-45 for the index-deriving loop).
inline bool narrow_walks(int mode, int K, int N, int gw) {
  if (gw % 4 || nlt_wgrad_generic_only()) return false;
  return !((mode == NLT_CONV_K2S1 || mode == NLT_DECONV_K2S1) && K > 64 && N > 16);
}

template <int MODE, int MQ, int NT>
int run_narrowq(WN& w, hipStream_t s) {
  constexpr size_t lds = NarrowBlock<4 * MQ, NT>::PER * sizeof(float);
  w.zeros = narrow_walks(MODE, w.K, w.N, w.c.gw) ? nlt_zero_page() : nullptr;
  if (w.zeros)
    hipLaunchKernelGGL((wgrad_narrowq_kernel<MODE, MQ, NT, true>), dim3((unsigned)w.msplits), dim3(256), lds, s, w);
  else
    hipLaunchKernelGGL((wgrad_narrowq_kernel<MODE, MQ, NT, false>), dim3((unsigned)w.msplits), dim3(256), lds, s, w);
  return narrow_tail<MODE, 4 * MQ, NT>(w, s);
}

template <int MODE>
int dispatchq(WN& w, int mq, int nt, hipStream_t s) {
  if (mq == 1) return nt == 1 ? run_narrowq<MODE, 1, 1>(w, s) : run_narrowq<MODE, 1, 2>(w, s);
  return nt == 1 ? run_narrowq<MODE, 2, 1>(w, s) : run_narrowq<MODE, 2, 2>(w, s);
}

template <int MODE>
int dispatch(WN& w, int mt, int nt, hipStream_t s) {
  if (nt == 1) {
    if (mt == 2) return run_narrow<MODE, 2, 1>(w, s);
    if (mt == 4) return run_narrow<MODE, 4, 1>(w, s);
    if (mt == 8) return run_narrow<MODE, 8, 1>(w, s);
  } else if (nt == 2) {
    if (mt == 2) return run_narrow<MODE, 2, 2>(w, s);
    if (mt == 4) return run_narrow<MODE, 4, 2>(w, s);
    if (mt == 8) return run_narrow<MODE, 8, 2>(w, s);
  }
  return NLT_ERR_UNSUPPORTED;
}

// ---------------------------------------------------------------------------------------------------------------------------
// r05: the stride-1 k2 layers with 16 / 32 channels in and out (levels 1 and 2 of both paths, the 16- and 32-channel expanding
// blocks: the five weight gradients that stream 134 MB each) as an LDS-TILED kernel.  The walking kernel above forms the four
// tap-shifted A operands with four overlapping global reads per texel (L1 / L2 traffic 4x the unique bytes, B from 64-byte
// halves of 128-byte lines): 72-84 us per launch against a 27 us HBM floor.  Here a workgroup stages a 4 x 64 (32 channels: 4 x 32)
// texel tile of dP and the haloed (+1 row, +1 column) tile of X in LDS ONCE (16-byte coalesced loads, every HBM byte read 1.0x / 1.27x), the next tile's loads
// are in flight in registers while the current tile's MFMAs read their operands from LDS, and the weight-gradient block stays in
// registers across the workgroup's tiles.  Wave r owns tile row r; per 4-texel step and tap: A[cin][texel] = X(y + a, x + b)
// (transposed family: X(y - a, x - b)), B[texel][cout] = dP(y, x); rows of D = cin, columns = cout.  Same [K][N] workspace
// block per workgroup, same fixed-order reduce pass (wgrad_narrow_reduce_kernel) as the kernels above: deterministic.
// 32 channels: texel pitch 32 floats would put lanes kk and kk + 1 of a ds_read_b32 on the same banks, so odd texels store
// their channel halves swapped (c ^ 16).
constexpr int S1_TH = 4, S1_XR = S1_TH + 1;

template <int C> struct S1T {
  static constexpr int TW = C == 16 ? 64 : 32;                          // tile width: 10 float4 of prefetch per thread either way
  static constexpr int XW = TW + 1;                                     // (32 channels x 64 texels: 241 registers, one wave per SIMD)
  static constexpr int Q = C / 4;                                       // float4 per texel
  static constexpr int NX = (S1_XR * XW * Q + 255) / 256;               // X-tile float4 per thread: 6
  static constexpr int ND = S1_TH * TW * Q / 256;                       // dP-tile float4 per thread: 4
  static constexpr int XF = S1_XR * XW * C, DF = S1_TH * TW * C;        // floats: 37 KB of LDS per workgroup
  static constexpr int T = C / 16;                                      // 16-row / 16-column MFMA tiles
};

template <int MODE, int C>
__global__ __launch_bounds__(256) void wgrad_s1t_kernel(WN w, int tiles_x, int tiles_y, int ntiles) {
  using TT = S1T<C>;
  constexpr int Q = TT::Q, NX = TT::NX, ND = TT::ND, T = TT::T, S1_TW = TT::TW, S1_XW = TT::XW;
  using Blk = NarrowBlock<4 * T, T>;
  constexpr int NC = Blk::NC, KN = Blk::KN;
  extern __shared__ __attribute__((aligned(16))) float s1_lds[];
  float* const xs = s1_lds;
  float* const ds = s1_lds + TT::XF;
  const ConvP& p = w.c;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int i = lane & 15, kk = lane >> 4;
  constexpr int OFF = MODE == NLT_DECONV_K2S1 ? -1 : 0;                 // tile origin of X relative to the dP tile
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- per-thread staging geometry (tile independent): float4 q -> (row, column, channel quad)
  int xr[NX], xc[NX], xg[NX], xl[NX];
#pragma unroll
  for (int it = 0; it < NX; ++it) {
    const int q = tid + 256 * it;
    const bool live = q < S1_XR * S1_XW * Q;
    const int tex = live ? q / Q : 0, cq = q - tex * Q;
    xr[it] = live ? tex / S1_XW : -4096;                               // (a dead slot never passes the bounds test)
    xc[it] = tex - (live ? tex / S1_XW : 0) * S1_XW;
    xg[it] = (xr[it] * p.w + xc[it]) * p.ld0 + 4 * cq;
    const int c0 = 4 * cq;
    xl[it] = tex * C + (C == 32 ? (c0 ^ ((tex & 1) << 4)) : c0);
  }
  int dr[ND], dc[ND], dg[ND], dl[ND];
#pragma unroll
  for (int it = 0; it < ND; ++it) {
    const int q = tid + 256 * it;
    const int tex = q / Q, cq = q - tex * Q;
    dr[it] = tex / S1_TW; dc[it] = tex - dr[it] * S1_TW;
    dg[it] = (dr[it] * p.w + dc[it]) * w.ldp + 4 * cq;
    const int c0 = 4 * cq;
    dl[it] = tex * C + (C == 32 ? (c0 ^ ((tex & 1) << 4)) : c0);
  }
  f32x4 px[NX], pd[ND];
  auto request = [&](int tile) {
    const int tx = tile % tiles_x, r2 = tile / tiles_x;
    const int ty = r2 % tiles_y, f = r2 / tiles_y;
    const int y0 = ty * S1_TH, x0 = tx * S1_TW;
    const long xbase = ((long)(f * p.h + y0 + OFF) * p.w + x0 + OFF) * p.ld0;
    const long dbase = ((long)(f * p.h + y0) * p.w + x0) * w.ldp;
#pragma unroll
    for (int it = 0; it < NX; ++it) {
      const int gy = y0 + OFF + xr[it], gx = x0 + OFF + xc[it];
      const bool ok = (unsigned)gy < (unsigned)p.h && (unsigned)gx < (unsigned)p.w;
      const f32x4 v = *reinterpret_cast<const f32x4*>(p.src0 + (ok ? xbase + xg[it] : 0));
      px[it] = ok ? v : zero4;
    }
#pragma unroll
    for (int it = 0; it < ND; ++it) {
      const bool ok = y0 + dr[it] < p.h && x0 + dc[it] < p.w;
      const f32x4 v = *reinterpret_cast<const f32x4*>(w.dp + (ok ? dbase + dg[it] : 0));
      pd[it] = ok ? v : zero4;
    }
  };

  f32x4 acc[4 * T * T];                                                 // [tap][mt][nt]
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int mt = 0; mt < T; ++mt)
#pragma unroll
      for (int nt = 0; nt < T; ++nt) acc[(t * T + mt) * T + nt] = zero4;
  f32x4 bsum = zero4;                                                   // column sums of dP: this thread's channel quad (tid % Q)

  // LDS read offsets of this lane (texel = step * 4 + kk of row wv)
  int a_off[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int a = t >> 1, b = t & 1;
    const int ry = MODE == NLT_DECONV_K2S1 ? wv + 1 - a : wv + a, cx = MODE == NLT_DECONV_K2S1 ? kk + 1 - b : kk + b;
    a_off[t] = ry * S1_XW + cx;                                        // texel index inside the X tile at step 0
  }
  const int b_tex = wv * S1_TW + kk;

  int tile = blockIdx.x;
  if (tile < ntiles) request(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    // ---- registers -> LDS
#pragma unroll
    for (int it = 0; it < NX; ++it)
      if (xr[it] >= 0) *reinterpret_cast<f32x4*>(xs + xl[it]) = px[it];
#pragma unroll
    for (int it = 0; it < ND; ++it) {
      *reinterpret_cast<f32x4*>(ds + dl[it]) = pd[it];
      bsum += pd[it];
    }
    __syncthreads();
    const int next = tile + gridDim.x;
    if (next < ntiles) request(next);                                  // in flight under this tile's MFMAs
    // ---- 16 steps of 4 texels
#pragma unroll 4
    for (int st = 0; st < S1_TW / 4; ++st) {
      float bv[T];
      const int bt = b_tex + 4 * st;
#pragma unroll
      for (int nt = 0; nt < T; ++nt) {
        const int c = 16 * nt + i;
        bv[nt] = ds[bt * C + (C == 32 ? (c ^ ((bt & 1) << 4)) : c)];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int at = a_off[t] + 4 * st;
#pragma unroll
        for (int mt = 0; mt < T; ++mt) {
          const int c = 16 * mt + i;
          const float av = xs[at * C + (C == 32 ? (c ^ ((at & 1) << 4)) : c)];
#pragma unroll
          for (int nt = 0; nt < T; ++nt) acc[(t * T + mt) * T + nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[nt], acc[(t * T + mt) * T + nt], 0, 0, 0);
        }
      }
    }
    __syncthreads();                                                   // the tile is consumed: LDS may be overwritten
  }

  // ---- the four waves' blocks, added in wave order (fixed -> deterministic), then the workgroup's block to the workspace
  float* const xch = s1_lds;                                           // [K][NC] + column sums
  auto slot = [i, kk](int j, int r) {                                  // accumulator (t, mt, nt), D row 4 kk + r
    const int nt = j % T, mt = (j / T) % T, t = j / (T * T);
    return (t * C + 16 * mt + 4 * kk + r) * NC + 16 * nt + i;
  };
  wave_order_sum(xch, wv, acc, slot, NoColumnSums{});
  float* dst = w.ws + (size_t)blockIdx.x * Blk::PER;
  if (wv == 0) store_block(dst, acc, slot);
  // column sums: thread t holds the sums of channel quad t % Q over its texels; added over the 256 / Q threads of a quad in thread order
  *reinterpret_cast<f32x4*>(xch + KN + 4 * tid) = bsum;                 // (K * NC <= the X tile: room for 1024 floats behind it)
  __syncthreads();
  if (tid < C) {
    const int quad = tid >> 2, e = tid & 3;
    float s = 0.f;
    for (int t = quad; t < 256; t += Q) s += xch[KN + 4 * t + e];
    dst[KN + tid] = s;
  }
}

// which launches the LDS-tiled form takes, and with how many (persistent) workgroups = slices of the reduce pass
inline bool s1t_ok(int mode, int c0, int c1, int ld0, int ldp, int cout, int h, int wd, const float* src0, const float* dpre) {
  const char* e = getenv("NLT_WGRAD_S1T");                              // (read per call: A/B runs and the parity test flip it in-process)
  if ((e && e[0] == '0') || nlt_wgrad_generic_only()) return false;
  if (mode != NLT_CONV_K2S1 && mode != NLT_DECONV_K2S1) return false;
  if (c1 != 0 || c0 != cout || (cout != 16 && cout != 32)) return false;
  if ((ld0 & 3) || (ldp & 3) || h < S1_TH || wd < 8) return false;
  if (src0 && (!nlt_aligned16(src0) || !nlt_aligned16(dpre))) return false;
  return true;
}

inline int s1t_blocks(int n, int h, int wd, int cout) {
  const int tw = cout == 16 ? S1T<16>::TW : S1T<32>::TW;
  const long tiles = (long)n * ((h + S1_TH - 1) / S1_TH) * ((wd + tw - 1) / tw);
  const long cap = cout == 16 ? 768 : 512;                            // what is resident at once: 3 / 2 workgroups per CU (148 / 216 registers)
  return (int)(tiles < cap ? tiles : cap);
}

template <int MODE, int C>
int run_s1t(WN& w, hipStream_t s) {
  using TT = S1T<C>;
  constexpr int MT = 4 * C / 16, NT = C / 16;
  const int ty = (w.c.h + S1_TH - 1) / S1_TH, tx = (w.c.w + TT::TW - 1) / TT::TW;
  const int ntiles = w.c.n * ty * tx;
  const size_t lds = (size_t)(TT::XF + TT::DF) * sizeof(float);
  static bool attr = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(wgrad_s1t_kernel<MODE, C>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)((TT::XF + TT::DF) * sizeof(float))) == hipSuccess;
  }();
  if (!attr) return NLT_ERR_LAUNCH;
  hipLaunchKernelGGL((wgrad_s1t_kernel<MODE, C>), dim3((unsigned)w.msplits), dim3(256), lds, s, w, tx, ty, ntiles);
  return narrow_tail<MODE, MT, NT>(w, s);
}

int tiles_m(int K) { return K <= 32 ? 2 : (K <= 64 ? 4 : 8); }

// f(std::integral_constant<int, MODE>) for the four families of the narrow entry point
template <class F>
int with_mode(int mode, F&& f) {
  switch (mode) {
    case NLT_CONV_K2S2: return f(std::integral_constant<int, NLT_CONV_K2S2>{});
    case NLT_CONV_K2S1: return f(std::integral_constant<int, NLT_CONV_K2S1>{});
    case NLT_DECONV_K2S2: return f(std::integral_constant<int, NLT_DECONV_K2S2>{});
    case NLT_DECONV_K2S1: return f(std::integral_constant<int, NLT_DECONV_K2S1>{});
  }
  return NLT_ERR_BAD_ARG;
}

int prepare_narrow(WN& w, int mode, const float* src0, int ld0, int c0, const float* src1, int ld1, int c1, int n, int h, int wd,
                   const float* dpre, int ldp, int cout, float* dw, float* db, long* ws_floats) {
  if (mode != NLT_CONV_K2S2 && mode != NLT_CONV_K2S1 && mode != NLT_DECONV_K2S2 && mode != NLT_DECONV_K2S1) return NLT_ERR_UNSUPPORTED;
  float* dummy = dw ? dw : reinterpret_cast<float*>(16);
  const float* d0 = src0 ? src0 : dummy;
  const int st = nlt_fill_conv_params(w.c, mode, d0, ld0, c0, c1 ? (src1 ? src1 : dummy) : nullptr, ld1, c1, n, h, wd, dummy, dummy,
                                      cout, dummy, cout, 0, 0.f, nullptr, 0, 0);
  if (st != NLT_OK) return st;
  if (ldp < cout) return NLT_ERR_BAD_ARG;
  const int taps = mode == NLT_DECONV_K2S2 ? 1 : 4;
  w.K = taps * (c0 + c1);
  w.N = w.c.N;
  if (w.K > 128 || w.N > 32) return NLT_ERR_UNSUPPORTED;
  if (w.c.gw < 4) return NLT_ERR_UNSUPPORTED;                          // the incremental row walk assumes >= 4 texels per grid row
  w.dp = dpre; w.ldp = ldp; w.dw = dw; w.db = db;
  const bool walk = narrow_walks(mode, w.K, w.N, w.c.gw);
  static const long nwant = [] { const char* e = getenv("NLT_WGRAD_NARROW_WANT"); return e ? atol(e) : 2048l; }();
  long rows = walk ? (w.c.M + nwant - 1) / nwant : (w.c.M + 511) / 512;   // walk: ~2048 workgroups (the loads run 5-7 steps ahead;
  if (rows < 256) rows = 256;                                          //  HBM-bound layers want many of them in flight)
  const long unit = walk ? 384 : 16;                                   // walk: every wave's run a whole number of pipeline rounds (6 or 8 steps)
  rows = (rows + unit - 1) / unit * unit;
  w.msplits = (int)((w.c.M + rows - 1) / rows);
  w.rows_per_split = (int)rows;
  long slices = w.msplits;
  if (s1t_ok(mode, c0, c1, ld0, ldp, cout, h, wd, src0, dpre)) {          // LDS-tiled form: one slice per persistent workgroup
    w.msplits = s1t_blocks(n, h, wd, cout);
    w.rows_per_split = 0;
    if (w.msplits > slices || src0) slices = w.msplits;                  // (the size query has no pointers to check: room for either form)
  }
  const int mt = w.K <= 64 ? 4 : 8, nt = w.N <= 16 ? 1 : 2;               // (the quad-A form pads K to 64 / 128)
  *ws_floats = (slices + 1) * (mt * 16 * nt * 16 + nt * 16);
  return NLT_OK;
}

}  // namespace

extern "C" long nlt_wgrad_narrow_workspace_floats(int mode, int c0, int c1, int n, int h, int w, int cout) {
  WN t;
  long need = -1;
  if (prepare_narrow(t, mode, nullptr, c0, c0, nullptr, c1, c1, n, h, w, nullptr, cout, cout, nullptr, nullptr, &need) != NLT_OK)
    return -1;
  return need;
}

extern "C" int nlt_conv_backward_weights_narrow(int mode,
                                                const float* src0, int ld0, int c0, const float* src1, int ld1, int c1,
                                                int n, int h, int w, const float* dpre, int ldp, int cout,
                                                float* dw_keras, float* dbias, float* workspace, long workspace_floats,
                                                void* stream) {
  if (!src0 || !dpre || !dw_keras || !workspace) return NLT_ERR_BAD_ARG;
  if (c1 > 0 && !src1) return NLT_ERR_BAD_ARG;
  WN t;
  long need = 0;
  const int st = prepare_narrow(t, mode, src0, ld0, c0, src1, ld1, c1, n, h, w, dpre, ldp, cout, dw_keras, dbias, &need);
  if (st != NLT_OK) return st;
  if (workspace_floats < need || !nlt_aligned16(workspace)) return NLT_ERR_BAD_ARG;
  t.ws = workspace;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int mt = tiles_m(t.K), nt = t.N <= 16 ? 1 : 2;
  const bool quads = !(c0 & 3) && !(c1 & 3) && !(ld0 & 3) && (c1 == 0 || !(ld1 & 3)) && nlt_aligned16(src0) &&
                     (c1 == 0 || nlt_aligned16(src1));
  return with_mode(mode, [&](auto m) {
    constexpr int MODE = decltype(m)::value;
    if constexpr (MODE == NLT_CONV_K2S1 || MODE == NLT_DECONV_K2S1)
      if (t.rows_per_split == 0)                                         // (prepare_narrow chose the LDS-tiled form)
        return cout == 16 ? run_s1t<MODE, 16>(t, s) : run_s1t<MODE, 32>(t, s);
    if (quads && t.K > 32) return dispatchq<MODE>(t, t.K <= 64 ? 1 : 2, nt, s);   // (K <= 32: two scalar row tiles beat four half-empty quad tiles)
    return dispatch<MODE>(t, mt, nt, s);
  });
}
