// Weight / bias gradients, second generation:  dW[k][n] = sum_rows X[row][k] * dP[row][n].
//
// The reduction runs over texel rows, 4 per v_mfma_f32_16x16x4_f32 step, so operand traffic decides the speed.
// Here both operands are fetched with ONE 16-byte NHWC load per lane per step and feed 16 MFMAs:
//   lane (i = l & 15, kk = l >> 4) loads the channel QUAD i of row kk of X  -> A_e[i][kk] = quad[e], e = 0..3
//   lane (j = l & 15, kk = l >> 4) loads the output  QUAD j of row kk of dP -> B_f[kk][j] = quad[f], f = 0..3
//   D_{e,f} = A_e * B_f accumulates dW[channel 4*quad_i + e][output 4*quad_j + f]
// i.e. a wave owns a 64 x 64 block of dW (16 k-quads x 16 n-quads; k-quads run over tap x virtual-concat channel
// quads, n-quads over output channels or, for Conv2DTranspose k2s2, over (a,b,o)) for one slice of the rows.
// Row slices write their partial blocks to a workspace with 16-byte stores; a second launch adds the slices in
// order and accumulates into the Keras-layout gradient -- deterministic, and no atomics (the first-generation
// kernel's thousands of waves adding into the 64 addresses of a 4 -> 4 layer were its bottleneck).
#include "wgrad_common.h"
#include <cstdlib>

namespace {

struct WT {
  ConvP c;            // geometry + X sources
  const float* dp; int ldp;
  float* dw; float* db;
  float* ws; float* wsb;
  const float* zeros;  // 16 zero bytes in device memory (the walk kernel's operand source past the end of a run)
  int kq, nq;         // k-quads (taps * (c0 + c1) / 4), n-quads (N / 4)
  int kblocks, nblocks, msplits, rows_per_split;
  int xcd_order;      // slice ms pinned to XCD ms % 8, its tiles consecutive there (wgrad_block)
};

// Workgroup -> (row slice, k-block, n-block).  Every tile of dW re-reads the slice's X rows (once per n-block and tap) and dP
// rows (once per k-block): 134 MB of L2 misses for 17 MB of operands at level 4 when those workgroups are dealt round-robin
// over the 8 XCDs (measured: FETCH_SIZE, TCC_MISS; that traffic, not the matrix pipe, was the kernel's time).  Workgroup ids go
// to XCDs modulo 8, so slice ms is pinned to XCD ms % 8 and its tiles are consecutive there: the slice is fetched into ONE L2 once.
__device__ __forceinline__ bool wgrad_block(const WT& w, int& ms, int& kb, int& nb) {
  const int tiles = w.kblocks * w.nblocks;
  if (!w.xcd_order) {                                                // few slices (deep levels): slices fastest, every XCD busy
    int blk = blockIdx.x;
    ms = blk % w.msplits; blk /= w.msplits;
    nb = blk % w.nblocks;
    kb = blk / w.nblocks;
    return true;
  }
  const int xcd = blockIdx.x & 7, r = blockIdx.x >> 3;
  const int tile = r % tiles;
  ms = (r / tiles) * 8 + xcd;
  nb = tile % w.nblocks;
  kb = tile / w.nblocks;
  return ms < w.msplits;
}

// What both kernels of a block share: 16 accumulators acc[e * 4 + f] + bias sums per lane, the MFMA step, and the way out
// (waves 1..3 -> wave 0 in wave order -> workspace [ms][kb][nb][e][f][lane], f32x4 = the 4 D rows this lane holds).
__device__ __forceinline__ void tile_mfma(f32x4 (&acc)[16], f32x4& bsum, const f32x4& av, const f32x4& bv) {
  bsum += bv;
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int f4 = 0; f4 < 4; ++f4)
      acc[e * 4 + f4] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[f4], acc[e * 4 + f4], 0, 0, 0);
}

__device__ __forceinline__ void tile_finish(const WT& w, f32x4* part, int wv, int lane, int ms, int kb, int nb, f32x4 (&acc)[16],
                                            f32x4& bsum) {
  auto slot = [lane](int j) { return j * 64 + lane; };
  wave_order_sum(part, wv, lane, acc, bsum, slot);
  if (wv > 0) return;
  store_block(reinterpret_cast<f32x4*>(w.ws) + (((size_t)ms * w.kblocks + kb) * w.nblocks + nb) * 16 * 64, acc, slot);
  if (w.wsb && kb == 0) {                                                       // column sums of dP for the bias
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      bsum[f] += __shfl_xor(bsum[f], 16);
      bsum[f] += __shfl_xor(bsum[f], 32);
    }
    if ((lane >> 4) == 0) reinterpret_cast<f32x4*>(w.wsb)[((size_t)ms * w.nblocks + nb) * 16 + (lane & 15)] = bsum;
  }
}

// The rows re-derived per step (RowCursor): any row grid at least 4 texels wide.
template <int MODE>
__global__ __launch_bounds__(256) void wgrad_tile_kernel(WT w) {
  __shared__ __attribute__((aligned(16))) f32x4 part[3 * 17 * 64];   // waves 1..3 -> wave 0 (16 blocks + bias sums)
  const ConvP& p = w.c;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int ms, kb, nb;                                                    // one workgroup = one (row slice, kb, nb)
  if (!wgrad_block(w, ms, kb, nb)) return;
  const int i = lane & 15, kk = lane >> 4;
  const ARole<4> ar(kb * 16 + i, w.kq, p);                           // this lane's k-quad = (tap, channel quad of the virtual concat)
  const BRole<MODE> br(4 * (nb * 16 + i), p.N, p);                   // this lane's n-quad

  f32x4 acc[16], bsum = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  RowCursor c;
  c.init(ms * w.rows_per_split, w.rows_per_split, wv, kk, p);
  auto issue = [&](f32x4& av, f32x4& bv) {
    const bool rv = c.valid();
    const int tex = conv_tap_texel<MODE>(p, c.rf, c.ry, c.rx, ar.tap);
    const size_t tx = (rv && tex >= 0) ? (size_t)tex : 0;
    av = *reinterpret_cast<const f32x4*>(ar.src + tx * ar.ld);                 // unconditional, clamped address
    if (!(rv && ar.ok && tex >= 0)) av = (f32x4){0.f, 0.f, 0.f, 0.f};
    size_t otex = rv ? ((size_t)c.rf * p.gh + c.ry) * p.gw + c.rx : 0;
    if (MODE == NLT_DECONV_K2S2) otex = rv ? ((size_t)c.rf * p.oh + 2 * c.ry + (br.ab >> 1)) * p.ow + 2 * c.rx + (br.ab & 1) : 0;
    bv = *reinterpret_cast<const f32x4*>(w.dp + otex * w.ldp + br.off);
    if (!(rv && br.ok)) bv = (f32x4){0.f, 0.f, 0.f, 0.f};
    c.advance16(p);
  };
  c.rotate3<f32x4, f32x4>(issue, [&](const f32x4& av, const f32x4& bv) { tile_mfma(acc, bsum, av, bv); });
  tile_finish(w, part, wv, lane, ms, kb, nb, acc, bsum);
}

// The same block, with the rows WALKED (RowWalk) instead of re-derived: the form used whenever the row grid is a multiple of 4
// texels wide -- every released shape.  The kernel above spends ~70 VALU instructions per 16-MFMA step on (frame, y, x)
// bookkeeping, 64-bit multiplies for two addresses and exec-masked loads; with two waves per SIMD that address arithmetic, not
// the matrix pipe, set its speed.  Here the loads are unconditional and a step's bookkeeping is scalar.
constexpr int WALK_PF = 6;

template <int MODE>
__global__ __launch_bounds__(256) void wgrad_walk_kernel(WT w) {
  __shared__ __attribute__((aligned(16))) f32x4 part[3 * 17 * 64];
  const ConvP& p = w.c;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int ms, kb, nb;                                                    // one workgroup = one (row slice, kb, nb)
  if (!wgrad_block(w, ms, kb, nb)) return;
  const int i = lane & 15, kk = lane >> 4;
  const ARole<4> ar(kb * 16 + i, w.kq, p);
  const BRole<MODE> br(4 * (nb * 16 + i), p.N, p);
  using Walk = RowWalk<MODE>;

  Walk k;
  k.start(ms, wv, w.rows_per_split, p);                              // (rows_per_split % 16 == 0, M % 4 == 0: runs of whole steps)
  const float* const zpage = w.zeros;
  // an empty run (slice past M) must not form an address past the buffer
  const float* pa = k.nsteps > 0 ? ar.src + k.a_start_texel(ar.ta(), ar.tb(), kk, p) * ar.ld : ar.src;
  const float* pb = k.nsteps > 0 ? w.dp + k.b_start_texel(br.ab, kk, p) * w.ldp + br.off : zpage;
  const int a_inc = Walk::a_inc(ar.ld), a_inc_wrap = Walk::a_inc_wrap(ar.ld, p);
  const int b_inc = Walk::b_inc(w.ldp), b_inc_wrap = Walk::b_inc_wrap(w.ldp, p);
  const typename Walk::TapBounds tb = Walk::tap_bounds(ar.ta(), ar.tb(), kk, p);
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};

  f32x4 acc[16], bsum = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto issue = [&](f32x4& av, f32x4& bv) {
    bool ok = ar.ok;
    if (MODE == NLT_CONV_K2S1) ok = ok && k.x0 < tb.xlim && k.y < tb.ylim;
    if (MODE == NLT_DECONV_K2S1) ok = ok && k.x0 >= tb.xlo && k.y >= tb.ylo;
    const float* la = pa;
    if (Walk::PADS) la = ok ? pa : ar.src;                                       // a padded tap must not be dereferenced
    av = *reinterpret_cast<const f32x4*>(la);
    bv = *reinterpret_cast<const f32x4*>(pb);
    if (Walk::PADS) av = ok ? av : zero4;
    const bool adv = k.advances(), wrap = k.wraps(p);
    const float* pan = pa + (wrap ? a_inc_wrap : a_inc);
    const float* pbn = pb + (wrap ? b_inc_wrap : b_inc);
    pa = adv ? pan : pa;
    pb = adv ? pbn : zpage;
    k.move_on(adv, wrap, p);
  };
  k.template pipeline<WALK_PF, f32x4, f32x4>(issue, [&](const f32x4& av, const f32x4& bv) { tile_mfma(acc, bsum, av, bv); });
  // lanes whose k-quad / n-quad is padding carry garbage operands (their loads are unconditional): the rows / columns
  // they produce are dropped by the reduce pass (kq >= w.kq || nq >= w.nq), but the bias sums need real zeros
  if (!br.ok) bsum = zero4;
  tile_finish(w, part, wv, lane, ms, kb, nb, acc, bsum);
}

// Pass 2: 64 dW elements of the block layout per workgroup; the slices are dealt to 16 thread groups (16-byte loads, 8 in
// flight per thread) and combined in a fixed order.
template <int MODE> __device__ void wgrad_bias_block(const WT& w, int ocq);

template <int MODE>
__device__ __forceinline__ void wgrad_scatter(const WT& w, long idx, float s) {
  const ConvP& p = w.c;
  const int r = idx & 3, ln = (idx >> 2) & 63, ef = (idx >> 8) & 15;
  const long blk = idx >> 12;
  const int nb = blk % w.nblocks, kb = blk / w.nblocks;
  const int kq = kb * 16 + 4 * (ln >> 4) + r;           // D row = k-quad inside the block
  const int nq = nb * 16 + (ln & 15);                   // D col = n-quad
  if (kq >= w.kq || nq >= w.nq) return;
  const int qpt = (p.c0 + p.c1) >> 2;
  const int tap = kq / qpt;
  const int c = 4 * (kq - tap * qpt) + (ef >> 2);
  const int ncol = 4 * nq + (ef & 3);
  w.dw[nlt_keras_widx<MODE>(tap, c, ncol, p.c0 + p.c1, p.cout, p.cout, 0)] += s;
}

// FEW = true (<= 8 slices: the mid-network layers, whose 64 x 64 blocks of dW are many and whose slices are few): one
// thread adds the slices of FOUR consecutive block entries with 16-byte loads, all of them in flight at once -- 1024
// entries per workgroup.  (The wave-per-slice-group form below gives such a launch 16 384 workgroups of one 4-byte
// load per thread: 16 us for 12 MB.)  Fixed order: ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)).
template <int MODE, bool FEW>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(WT w) {
  __shared__ __attribute__((aligned(16))) float part[16][64];
  const long per_slice = (long)w.kblocks * w.nblocks * 4096;
  const long dw_blocks = per_slice / (FEW ? 1024 : 64);
  if ((long)blockIdx.x >= dw_blocks) {                                // the trailing cout / 4 workgroups: the bias (no extra launch)
    wgrad_bias_block<MODE>(w, (int)(blockIdx.x - dw_blocks));
    return;
  }
  if (FEW) {
    const long idx = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 v[8];
#pragma unroll
    for (int ms = 0; ms < 8; ++ms)
      v[ms] = ms < w.msplits ? *reinterpret_cast<const f32x4*>(w.ws + (size_t)ms * per_slice + idx) : z;
    const f32x4 s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
#pragma unroll
    for (int r = 0; r < 4; ++r) wgrad_scatter<MODE>(w, idx + r, s[r]);
    return;
  }
  // many slices (the shallow levels: few blocks of dW, hundreds of slices): thread (q, g) adds the slices g, g + 16, ... of the
  // entry QUAD q with 16-byte loads, 8 of them in flight (the 4-byte, 4-stream form of round 2 was pure latency: 23 us for 8 MB)
  const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
  const long idx = (long)blockIdx.x * 64 + 4 * q;
  const f32x4* src = reinterpret_cast<const f32x4*>(w.ws + idx);
  const size_t stride = (size_t)per_slice / 4;                         // f32x4 per slice
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
  int ms = g;
  for (; ms + 112 < w.msplits; ms += 128) {
    f32x4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[(size_t)(ms + 16 * j) * stride];
    s0 += (v[0] + v[1]) + (v[2] + v[3]);
    s1 += (v[4] + v[5]) + (v[6] + v[7]);
  }
  for (; ms < w.msplits; ms += 16) s0 += src[(size_t)ms * stride];
  reinterpret_cast<f32x4*>(&part[g][0])[q] = s0 + s1;
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int e = threadIdx.x;
  float t[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) t[a] = (part[4 * a][e] + part[4 * a + 1][e]) + (part[4 * a + 2][e] + part[4 * a + 3][e]);
  wgrad_scatter<MODE>(w, (long)blockIdx.x * 64 + e, (t[0] + t[1]) + (t[2] + t[3]));
}

// Bias: one workgroup (of the reduce launch) per quad of output channels; 256 threads share the (slice, ab) terms,
// fixed-order LDS tree.
template <int MODE>
__device__ void wgrad_bias_block(const WT& w, int ocq) {
  __shared__ f32x4 part[256];
  const ConvP& p = w.c;
  const int t = threadIdx.x;
  const int nab = MODE == NLT_DECONV_K2S2 ? 4 : 1;
  const f32x4* wsb4 = reinterpret_cast<const f32x4*>(w.wsb);
  f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int it = t; it < nab * w.msplits; it += 256) {
    const int ab = it % nab, ms = it / nab;
    const int nq = ((ab * p.cout) >> 2) + ocq;                       // n-quad of column ab*cout + 4*ocq
    s += wsb4[((size_t)ms * w.nblocks + nq / 16) * 16 + nq % 16];
  }
  part[t] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) part[t] += part[t + off];
    __syncthreads();
  }
  if (t == 0) {
    const f32x4 v = part[0];
    w.db[4 * ocq] += v[0]; w.db[4 * ocq + 1] += v[1]; w.db[4 * ocq + 2] += v[2]; w.db[4 * ocq + 3] += v[3];
  }
}

inline bool tile_walks(const ConvP& p) { return p.gw % 4 == 0 && !nlt_wgrad_generic_only(); }

bool fill(WT& w, int mode, long* ws_floats) {
  const ConvP& p = w.c;
  const int taps = (mode == NLT_CONV1X1 || mode == NLT_DECONV_K2S2) ? 1 : 4;
  w.kq = taps * ((p.c0 + p.c1) >> 2);
  w.nq = p.N >> 2;
  w.kblocks = (w.kq + 15) / 16;
  w.nblocks = (w.nq + 15) / 16;
  static const long target = [] { const char* e = getenv("NLT_WGRAD_WANT"); return e ? atol(e) : 512l; }();
  long want = target / ((long)w.kblocks * w.nblocks);        // ~512 workgroups = the 2 per CU that are resident at once (measured:
                                                             // 1024 -> 512 takes 4 us off a 35 us mid-network launch: half the slices to reduce)
  if (want < 1) want = 1;
  long rows = (p.M + want - 1) / want;
  if (rows < 256) rows = 256;                                 // >= 16 MFMA steps per wave
  const bool walk = tile_walks(p);
  const long unit = walk ? 16 * WALK_PF : 16;                 // the walk kernel's runs: whole pipeline rounds
  rows = (rows + unit - 1) / unit * unit;
  w.msplits = (int)((p.M + rows - 1) / rows);
  if (w.msplits >= 8 && w.msplits % 8) {                      // whole XCD rounds if a slightly shorter slice gives them
    const long target = (w.msplits + 7) / 8 * 8;
    const long r2 = ((p.M + target - 1) / target + unit - 1) / unit * unit;
    if (r2 >= 16 * unit / 16 && (p.M + r2 - 1) / r2 == target) { rows = r2; w.msplits = (int)target; }
  }
  w.rows_per_split = (int)rows;
  w.xcd_order = w.msplits >= 8 && (w.msplits % 8 == 0 || w.msplits >= 24);
  *ws_floats = (long)w.msplits * w.kblocks * w.nblocks * 4096 + (long)w.msplits * w.nblocks * 64;
  return true;
}

template <int MODE>
int run(WT& w, hipStream_t s) {
  const long groups = (long)w.kblocks * w.nblocks * (w.xcd_order ? (w.msplits + 7) / 8 * 8 : w.msplits);   // (whole XCD rounds)
  w.zeros = tile_walks(w.c) ? nlt_zero_page() : nullptr;
  if (w.zeros)
    hipLaunchKernelGGL(wgrad_walk_kernel<MODE>, dim3((unsigned)groups), dim3(256), 0, s, w);
  else
    hipLaunchKernelGGL(wgrad_tile_kernel<MODE>, dim3((unsigned)groups), dim3(256), 0, s, w);
  const long items = (long)w.kblocks * w.nblocks * 4096;
  static const bool few_ok = [] { const char* e = getenv("NLT_WGRAD_REDUCE_FEW"); return !(e && e[0] == '0'); }();   // A/B switch
  if (w.msplits <= 8 && few_ok)
    hipLaunchKernelGGL((wgrad_reduce_kernel<MODE, true>), dim3((unsigned)(items / 1024 + (w.db ? w.c.cout / 4 : 0))), dim3(256), 0, s, w);
  else
    hipLaunchKernelGGL((wgrad_reduce_kernel<MODE, false>), dim3((unsigned)(items / 64 + (w.db ? w.c.cout / 4 : 0))), dim3(256), 0, s, w);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

int prepare(WT& w, int mode, const float* src0, int ld0, int c0, const float* src1, int ld1, int c1, int n, int h, int wd,
            const float* dpre, int ldp, int cout, float* dw, float* db, long* ws_floats) {
  float* dummy = dw ? dw : reinterpret_cast<float*>(16);
  const float* d0 = src0 ? src0 : dummy;
  const int st = nlt_fill_conv_params(w.c, mode, d0, ld0, c0, c1 ? (src1 ? src1 : dummy) : nullptr, ld1, c1, n, h, wd, dummy, dummy,
                                      cout, dummy, cout, 0, 0.f, nullptr, 0, 0);
  if (st != NLT_OK) return st;
  if ((c0 & 3) || (c1 & 3) || (cout & 3) || (ld0 & 3) || (c1 && (ld1 & 3)) || (ldp & 3) || ldp < cout) return NLT_ERR_UNSUPPORTED;
  if (w.c.gw < 4) return NLT_ERR_UNSUPPORTED;                      // the incremental row walk assumes >= 4 texels per grid row
  w.dp = dpre; w.ldp = ldp; w.dw = dw; w.db = db;
  fill(w, mode, ws_floats);
  return NLT_OK;
}

}  // namespace

extern "C" long nlt_wgrad_workspace_floats(int mode, int c0, int c1, int n, int h, int w, int cout) {
  WT t;
  long need = -1;
  if (prepare(t, mode, nullptr, c0 > 4 ? c0 : 4, c0, nullptr, c1 > 4 ? c1 : 4, c1, n, h, w, nullptr, cout, cout, nullptr, nullptr, &need) != NLT_OK)
    return -1;
  return need;
}

extern "C" int nlt_conv_backward_weights_tiled(int mode,
                                               const float* src0, int ld0, int c0, const float* src1, int ld1, int c1,
                                               int n, int h, int w, const float* dpre, int ldp, int cout,
                                               float* dw_keras, float* dbias, float* workspace, long workspace_floats,
                                               void* stream) {
  if (!src0 || !dpre || !dw_keras || !workspace) return NLT_ERR_BAD_ARG;
  if (c1 > 0 && !src1) return NLT_ERR_BAD_ARG;
  WT t;
  long need = 0;
  const int st = prepare(t, mode, src0, ld0, c0, src1, ld1, c1, n, h, w, dpre, ldp, cout, dw_keras, dbias, &need);
  if (st != NLT_OK) return st;
  if (workspace_floats < need) return NLT_ERR_BAD_ARG;
  if (!nlt_aligned16(src0) || (c1 && !nlt_aligned16(src1)) || !nlt_aligned16(dpre) || !nlt_aligned16(workspace)) return NLT_ERR_BAD_ARG;
  t.ws = workspace;
  t.wsb = dbias ? workspace + (long)t.msplits * t.kblocks * t.nblocks * 4096 : nullptr;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (mode) {
    case NLT_CONV1X1: return run<NLT_CONV1X1>(t, s);
    case NLT_CONV_K2S2: return run<NLT_CONV_K2S2>(t, s);
    case NLT_CONV_K2S1: return run<NLT_CONV_K2S1>(t, s);
    case NLT_DECONV_K2S2: return run<NLT_DECONV_K2S2>(t, s);
    case NLT_DECONV_K2S1: return run<NLT_DECONV_K2S1>(t, s);
  }
  return NLT_ERR_BAD_ARG;
}
