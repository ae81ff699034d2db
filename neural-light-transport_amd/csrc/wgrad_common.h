// The pieces the second-generation weight-gradient kernels share (wgrad_tile.hip: 64 x 64 blocks of dW from 16-byte operands;
// wgrad_narrow.hip: MFMA tiles matched to a narrow layer).  Every kernel there is  lane roles -> rows of its slice (re-derived
// per step: RowCursor, or walked: RowWalk) -> the four waves' blocks added in wave order -> the slice's block to the workspace.
// Each piece is written once here; the kernels keep their own operand ADDRESS expressions (they decide registers and speed).
#pragma once
#include "nlt_common.h"
#include "pack_common.h"

// ---- lane roles -------------------------------------------------------------------------------------------------------------
// A role: K entry k of the lane, in units of U channels (U = 1: K index; U = 4: channel quad) = (tap, channel of the virtual
// concat src0 | src1).  A padding entry (k >= count) reads tap 0, channel 0.
template <int U>
struct ARole {
  const float* src; int ld, tap; bool ok;
  __device__ __forceinline__ ARole(int k, int count, const ConvP& p) {
    const int per = U == 4 ? (p.c0 + p.c1) >> 2 : p.c0 + p.c1, n0 = U == 4 ? p.c0 >> 2 : p.c0;
    ok = k < count;
    tap = ok ? k / per : 0;
    const int c = ok ? k - tap * per : 0;
    const bool from1 = c >= n0;
    src = from1 ? p.src1 + U * (c - n0) : p.src0 + U * c;
    // (not `from1 ? p.ld1 : p.ld0`: where the kernel hands its argument struct on by reference, the compiler turns that into a
    // load through a selected address of a scratch copy -- 16 bytes of scratch in four of the walking kernels)
    ld = p.ld0 + (from1 ? p.ld1 - p.ld0 : 0);
  }
  ARole() = default;
  __device__ __forceinline__ int ta() const { return tap >> 1; }
  __device__ __forceinline__ int tb() const { return tap & 1; }
};

// B role: GEMM column ncol of the lane = output channel `off` (Conv2DTranspose k2s2: of output phase ab = a * 2 + b).  A padding
// column (ncol >= N) reads column 0.
template <int MODE>
struct BRole {
  int ab, off; bool ok;
  __device__ __forceinline__ BRole(int ncol, int N, const ConvP& p) {
    ok = ncol < N;
    const int nn = ok ? ncol : 0;
    ab = MODE == NLT_DECONV_K2S2 ? nn / p.cout : 0;
    off = MODE == NLT_DECONV_K2S2 ? nn - ab * p.cout : nn;
  }
  BRole() = default;
};

// ---- rows re-derived per step -----------------------------------------------------------------------------------------------
// The slice's rows [m_begin, m_end) are dealt to the 4 waves in steps of 4 rows (wave wv takes steps wv, wv + 4, ...); lane group
// kk holds row kk of a step.  (rf, ry, rx) = (frame, y, x) of the lane's row m of the NEXT step to be loaded, advanced
// incrementally instead of being re-derived by integer division every step.
struct RowCursor {
  int m, rx, ry, rf, m_end, nsteps;
  __device__ __forceinline__ void init(int m_begin, int rows, int wv, int kk, const ConvP& p) {
    m_end = m_begin + rows;
    if (m_end > p.M) m_end = p.M;
    m = m_begin + 4 * wv + kk;
    const int mc = m < p.M ? m : p.M - 1;
    rx = mc % p.gw; ry = (mc / p.gw) % p.gh; rf = mc / (p.gw * p.gh);
    const int first = m_begin + 4 * wv;
    nsteps = first < m_end ? (m_end - first + 15) / 16 : 0;
  }
  __device__ __forceinline__ bool valid() const { return m < m_end; }
  __device__ __forceinline__ void advance16(const ConvP& p) {           // the wave's next step is 16 rows further
    m += 16; rx += 16;
#pragma unroll
    for (int u = 0; u < 4; ++u) {                                      // gw >= 4 (checked by the host): at most 4 wraps, branch-free
      const bool wx = rx >= p.gw;
      rx -= wx ? p.gw : 0;
      ry += wx ? 1 : 0;
      const bool wy = ry >= p.gh;
      ry = wy ? 0 : ry;
      rf += wy ? 1 : 0;
    }
  }
  // Operand loads run two steps ahead of the MFMAs (three register sets of an A and a B operand, each a value or an array of
  // them); steps past nsteps carry zero operands.
  template <class A, class B, class Issue, class Compute>
  __device__ __forceinline__ void rotate3(Issue&& issue, Compute&& compute) const {
    A a0, a1, a2;
    B b0, b1, b2;
    issue(a0, b0);
    issue(a1, b1);
    for (int s3 = 0; s3 < nsteps; s3 += 3) {
      issue(a2, b2); compute(a0, b0);
      issue(a0, b0); compute(a1, b1);
      issue(a1, b1); compute(a2, b2);
    }
  }
};

// ---- rows walked (row grid a multiple of 4 texels wide) ---------------------------------------------------------------------
// A wave takes a contiguous run [m0, m1) of its slice (a quarter of it, a multiple of 4 rows), 4 rows per step; 4 | gw means the
// 4 rows of a step share one image row, so the position (x0, y) of a step's first row is WAVE-UNIFORM (scalar registers).  Each
// lane keeps operand POINTERS and advances them by lane-constant increments (a second constant on the steps that wrap to the
// next image row, where the stride-2 families jump); padding validity (k2s1 families only) is two compares against lane constants.
template <int MODE>
struct RowWalk {
  int m0, R0, x0, y, issued, nsteps;                                   // R0 = image row index of m0 over all frames
  __device__ __forceinline__ void start(int ms, int wv, int rows_per_split, const ConvP& p) {
    const int chunk = rows_per_split >> 2;
    m0 = __builtin_amdgcn_readfirstlane(ms * rows_per_split + wv * chunk);
    int m1 = m0 + chunk;
    if (m1 > p.M) m1 = p.M;
    nsteps = m1 > m0 ? (m1 - m0) >> 2 : 0;
    x0 = m0 % p.gw;
    R0 = m0 / p.gw;
    y = R0 % p.gh;
    issued = 0;
  }
  // texel of the lane's step-0 row m0 + kk: the tap (a, b) of source A (unclamped; validity is tracked separately), the output
  // phase ab of dP
  __device__ __forceinline__ long a_start_texel(int a, int b, int kk, const ConvP& p) const {
    if (MODE == NLT_CONV_K2S2) return ((long)(2 * R0 + a)) * p.w + 2 * (x0 + kk) + b;
    if (MODE == NLT_CONV_K2S1) return (long)m0 + kk + a * p.w + b;
    if (MODE == NLT_DECONV_K2S1) return (long)m0 + kk - a * p.w - b;
    return (long)m0 + kk;
  }
  __device__ __forceinline__ long b_start_texel(int ab, int kk, const ConvP& p) const {
    if (MODE == NLT_DECONV_K2S2) return ((long)(2 * R0 + (ab >> 1))) * p.ow + 2 * (x0 + kk) + (ab & 1);
    return (long)m0 + kk;
  }
  // per-step pointer increments (floats): plain step / step that wraps to the next image row (p.w = 2 gw, p.ow = 2 gw)
  static __device__ __forceinline__ int a_inc(int ald) { return (MODE == NLT_CONV_K2S2 ? 8 : 4) * ald; }
  static __device__ __forceinline__ int a_inc_wrap(int ald, const ConvP& p) { return MODE == NLT_CONV_K2S2 ? (8 + p.w) * ald : a_inc(ald); }
  static __device__ __forceinline__ int b_inc(int ldp) { return (MODE == NLT_DECONV_K2S2 ? 8 : 4) * ldp; }
  static __device__ __forceinline__ int b_inc_wrap(int ldp, const ConvP& p) { return MODE == NLT_DECONV_K2S2 ? (8 + p.ow) * ldp : b_inc(ldp); }
  // padding validity of the lane's tap (a, b), as bounds on the uniform (x0, y)
  //   k2s1:            x0 + kk + b < gw  and  y + a < gh           ->  x0 < xlim, y < ylim
  //   transposed k2s1: x0 + kk - b >= 0  and  y - a >= 0           ->  x0 >= xlo (only x0 = 0, kk = 0, b = 1 fails), y >= ylo
  // (the two compares themselves stay in each kernel's issue step: see profiles/README.md)
  struct TapBounds { int xlim, ylim, xlo, ylo; };
  static __device__ __forceinline__ TapBounds tap_bounds(int a, int b, int kk, const ConvP& p) {
    return TapBounds{p.gw - kk - b, p.gh - a, b - kk, a};
  }
  static constexpr bool PADS = MODE == NLT_CONV_K2S1 || MODE == NLT_DECONV_K2S1;
  // One step further (wave-uniform): adv = there is a next step in the run, wrap = it starts the next image row.  Call it once
  // per issue, advance the lane's pointers by (wrap ? inc_wrap : inc) where adv, then move_on().  Past the end of a run (the
  // pipeline issues ahead; a run clipped by M may not fill its last round) dP is read from the zero page, so the products vanish
  // without a select on the data, and X is re-read where the walk stopped.
  // (Two calls with the pointer arithmetic between them, not one function over the pointers or a returned {adv, wrap}: either
  // costs the narrow walking kernels 8 registers and a wave of occupancy -- profiles/README.md.)
  __device__ __forceinline__ bool advances() { return ++issued < nsteps; }
  __device__ __forceinline__ bool wraps(const ConvP& p) const { return x0 + 4 >= p.gw; }
  __device__ __forceinline__ void move_on(bool adv, bool wrap, const ConvP& p) {
    const int yn = y + 1 >= p.gh ? 0 : y + 1;
    y = (adv && wrap) ? yn : y;
    x0 = adv ? (wrap ? 0 : x0 + 4) : x0;
  }
  // Operand loads run PF - 1 steps ahead of the MFMAs (PF register sets; the host sizes the runs to multiples of PF steps).
  template <int PF, class A, class B, class Issue, class Compute>
  __device__ __forceinline__ void pipeline(Issue&& issue, Compute&& compute) const {
    A av[PF];
    B bv[PF];
#pragma unroll
    for (int j = 0; j < PF - 1; ++j) {
      issue(av[j], bv[j]);
      __builtin_amdgcn_sched_barrier(0);                               // (in order: the first round waits for the OLDEST loads only)
    }
    for (int s0 = 0; s0 < nsteps; s0 += PF) {
#pragma unroll
      for (int j = 0; j < PF; ++j) {
        // (the scheduler would otherwise hoist every load of the iteration to its top and drain them together)
        issue(av[(j + PF - 1) % PF], bv[(j + PF - 1) % PF]);
        __builtin_amdgcn_sched_barrier(0);
        compute(av[j], bv[j]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
};

// ---- the four waves' blocks, added in wave order ((w0 + w1) + w2) + w3 (fixed -> deterministic), and the workspace store -----
// `slot` maps an accumulator to where it lives in the exchange buffer AND in the slice's workspace block (the same layout).

// Tile family: NACC f32x4 accumulators + the bias sums of a lane, waves 1..3 each in a region of their own, ONE barrier; wave 0
// comes back with the sums.  part: [3][NACC + 1][64] f32x4, slot(j) in f32x4.
template <int NACC, class Slot>
__device__ __forceinline__ void wave_order_sum(f32x4* part, int wv, int lane, f32x4 (&acc)[NACC], f32x4& bsum, Slot&& slot) {
  constexpr int REGION = (NACC + 1) * 64;
  if (wv > 0) {
#pragma unroll
    for (int j = 0; j < NACC; ++j) part[(wv - 1) * REGION + slot(j)] = acc[j];
    part[(wv - 1) * REGION + NACC * 64 + lane] = bsum;
  }
  __syncthreads();
  if (wv == 0) {
#pragma unroll
    for (int o = 0; o < 3; ++o) {
#pragma unroll
      for (int j = 0; j < NACC; ++j) acc[j] += part[o * REGION + slot(j)];
      bsum += part[o * REGION + NACC * 64 + lane];
    }
  }
}
template <int NACC, class Slot>
__device__ __forceinline__ void store_block(f32x4* dst, const f32x4 (&acc)[NACC], Slot&& slot) {
#pragma unroll
  for (int j = 0; j < NACC; ++j) dst[slot(j)] = acc[j];
}

// Narrow family: ONE block [K][NC] of floats (+ NC column sums behind it) that waves 1..3 fill one after the other, a barrier
// pair per source wave; slot(j, r) = float index of D row r of accumulator j.  `cols` = the lane's column sums, handed over with
// the block (ColumnSums), or nothing (NoColumnSums: wgrad_s1t_kernel adds its column sums by thread, after the blocks).
template <int NT>
struct ColumnSums {
  float (&sum)[NT];
  int at;                                                              // KN + i: float index of the lane's column of tile 0
  bool writer;                                                         // kk == 0: the lane group that holds the wave's total
  __device__ __forceinline__ void across_row_groups() {                // rows kk = 0..3 of a step -> every group holds the total
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      sum[nt] += __shfl_xor(sum[nt], 16);
      sum[nt] += __shfl_xor(sum[nt], 32);
    }
  }
  __device__ __forceinline__ void put(float* blk) const {
    if (writer)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) blk[at + nt * 16] = sum[nt];
  }
  __device__ __forceinline__ void add(const float* blk) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) sum[nt] += blk[at + nt * 16];
  }
};
struct NoColumnSums {
  __device__ __forceinline__ void put(float*) const {}
  __device__ __forceinline__ void add(const float*) {}
};

template <int NACC, class Slot>
__device__ __forceinline__ void store_block(float* blk, const f32x4 (&acc)[NACC], Slot&& slot) {
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) blk[slot(j, r)] = acc[j][r];
}
template <int NACC, class Slot, class Cols>
__device__ __forceinline__ void wave_order_sum(float* xch, int wv, f32x4 (&acc)[NACC], Slot&& slot, Cols&& cols) {
  for (int src = 1; src < 4; ++src) {
    if (wv == src) {
      store_block(xch, acc, slot);
      cols.put(xch);
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
      for (int j = 0; j < NACC; ++j) {                                 // (the whole f32x4 at once: added element by element through
        f32x4 t;                                                       //  the reference, the 8-row-tile kernels lose 12 registers and a wave)
#pragma unroll
        for (int r = 0; r < 4; ++r) t[r] = xch[slot(j, r)];
        acc[j] += t;
      }
      cols.add(xch);
    }
    __syncthreads();
  }
}
