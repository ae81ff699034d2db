// `precision = f32x3`: the encoder's k2 convs (Conv2D k2s2 / k2s1, 'same') with fp32 operands SPLIT into three bf16 terms and
// multiplied on the bf16 matrix cores (v_mfma_f32_16x16x32_bf16, fp32 accumulate) -- 16x the rate of v_mfma_f32_16x16x4_f32.
//
//   x = hi + mid + lo exactly (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid): 8 + 8 + 8 significand bits = fp32's 24;
//   both subtractions are exact in fp32), so  a * b = sum over the nine term products, each EXACT in fp32 (8 x 8 bits).
//   NPROD = 9: all nine (what is lost is fp32 accumulation rounding only, as in the native fp32 MFMA);
//   NPROD = 6: the three products of order 2^-24 relative (mid*lo, lo*mid, lo*lo) are dropped: one extra fp32-rounding-sized
//              error per product.  Per fp32-equivalent K = 32 block that is 9 / 6 bf16 MFMAs of ~16 cycles against 8 fp32
//              MFMAs of 32 cycles: 0.56x / 0.375x the matrix-pipe time.
//   Small terms are accumulated first (lo-order products, then the mixed ones, hi*hi last).
//
// Structure = conv_tile.hip (8 x 16 output texels x TN output channels per 256-thread workgroup, 16-channel input slabs through a
// double-buffered LDS stage, one barrier per stage, observation mean in registers).  What differs:
//   * a K block of the bf16 MFMA is 32 = (2 taps) x (16 channels): lane group kk = lane >> 4 reads tap kk >> 1, channel half
//     kk & 1 -- 8 consecutive channels = one 16-byte LDS read per term plane;
//   * the texel slab is split when it is written to LDS (once per element per workgroup; every element is then used by
//     2-4 taps x TN output channels), into three planes [term][channel half][texel slot][8 bf16]; plane strides are multiples
//     of 16 slots, so the 16 lanes a ds_read_b128 services together (4 + 4 + 8 lanes of two lane groups) hit 16 different slots;
//   * the weights are split at pack time (nlt_pack_conv_tile3_weights): [g][cc][tap pair][ct][term][lane][8 bf16].
//
// Layout of this file: the STAGE PIECES, each defined once -- gather_unit (two 16-byte loads of a copy unit), split8 /
// split_store_unit (the three terms, and their LDS stores), read_a (A fragments), ORDER9 + term_products (the MFMAs of a K block),
// bias_act + epilogue (bias, LeakyReLU, out, observation mean), unit_slot / unit_source / stage_products (the shared 8 x 16 stage),
// wave_sync -- and FIVE SCHEDULES around them, which differ only in who stages what, when, and between which barriers:
//   conv_tile3_kernel      streaming: a tile per workgroup, weights and texels through the double-buffered stage;
//   conv_tile3d_kernel     streaming, texels direct (stride 2): gather_b_s2 / terms_b_s2 in place of the texel stage;
//   conv_tile3r_kernel     resident, shared stage: persistent workgroups, a group's weights stay in LDS;
//   conv_tile3w_kernel     resident, wave-private: every wave stages its own RT x 16 tile, no workgroup barrier;
//   conv_tile3w_s2_kernel  level hand-off: the wave-private schedule by tap class + the next level's stride-2 conv in registers.
// Per output element all five issue the same floating-point operations in the same order because they call the same pieces:
// slabs in order, tap pairs in order, ORDER9, bias, LeakyReLU, mean (tests/test_gpu_tile3_bits.py holds them to recorded bits,
// tests/test_gpu_tile3_s2direct.py the texels-direct schedule to the streaming kernel's).
#include "nlt_common.h"
#include "pack_common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef unsigned short u16;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int TH = 8, TW = 16;
constexpr int QS2 = 272, ODD2 = 132;        // k2s2 tap row: slots per (term, half) plane (2 x 128 + pad, = 0 mod 16); odd-x offset (= 4 mod 8)
constexpr int PL = 160;                      // k2s1 haloed tile: 9 x 17 = 153 texel slots, plane padded to 160

template <int MODE> struct T3;
template <> struct T3<NLT_CONV_K2S1> { static constexpr int PAIRS = 2, B_UNITS = 153 * 2, B_SLOTS = 6 * PL; };
template <> struct T3<NLT_CONV_K2S2> { static constexpr int PAIRS = 1, B_UNITS = 256 * 2, B_SLOTS = 6 * QS2; };

struct Tile3P {
  const float* src; const u16* packed; const float* bias;
  float* out; float* mean_out;
  int ld, cin, frames, kobs, h, w;
  int oh, ow, cout, ldo, ldm;
  int tiles_y, tiles_x, ncc;
  int act; float alpha;
};

__device__ __forceinline__ int xcd_tile3(int b, int nblocks) {
  return (nblocks & 7) ? b : (b & 7) * (nblocks >> 3) + (b >> 3);
}

// two floats -> their bf16 roundings (nearest even), packed (lo half = a)
__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {
  // (a conversion the compiler can see -- one v_cvt_pk_bf16_f32 -- not inline asm: the hazard recognizer pads MFMA -> VALU
  // read / write distances only for instructions it knows, r05)
  typedef float f32x2_ __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_){a, b}, bf16x2_));
}

// (a, b) -> packed (hi, mid, lo) terms
__device__ __forceinline__ void split2(float a, float b, unsigned& hi, unsigned& mid, unsigned& lo) {
  hi = cvt_pk_bf16(a, b);
  const float ra = a - __uint_as_float(hi << 16), rb = b - __uint_as_float(hi & 0xffff0000u);
  mid = cvt_pk_bf16(ra, rb);
  const float sa = ra - __uint_as_float(mid << 16), sb = rb - __uint_as_float(mid & 0xffff0000u);
  lo = cvt_pk_bf16(sa, sb);
}

// eight floats (a lane's two f32x4) -> the 16 bytes of each term: a B fragment of the bf16 MFMA, or one slot of each term plane
__device__ __forceinline__ void split8(const f32x4& v0, const f32x4& v1, u32x4& hi, u32x4& mid, u32x4& lo) {
  unsigned h[4], m[4], l[4];
  split2(v0[0], v0[1], h[0], m[0], l[0]);
  split2(v0[2], v0[3], h[1], m[1], l[1]);
  split2(v1[0], v1[1], h[2], m[2], l[2]);
  split2(v1[2], v1[3], h[3], m[3], l[3]);
  hi = (u32x4){h[0], h[1], h[2], h[3]};
  mid = (u32x4){m[0], m[1], m[2], m[3]};
  lo = (u32x4){l[0], l[1], l[2], l[3]};
}

// ---- the pieces every schedule below is made of: each is defined once, so "the forms give the same bits" is structural ----

// B copy unit u = (texel tx of the staged tile, channel half hf): 8 consecutive lanes take 8 consecutive texels of one half
// (conflict-free 16-byte LDS stores; the two halves of a texel are its 64 contiguous bytes in global memory)
__device__ __forceinline__ int unit_half(int u) { return (u >> 3) & 1; }
__device__ __forceinline__ int unit_texel(int u) { return (u >> 4) * 8 + (u & 7); }

// gather of a copy unit: channels [8 hf, 8 hf + 8) of texel `tex` of the slab at `sp`; zeros where the texel is outside the map
__device__ __forceinline__ void gather_unit(const float* sp, int ld, bool ok, long tex, int hf, f32x4& v0, f32x4& v1) {
  const float* q8 = sp + (ok ? tex : 0) * ld + 8 * hf;
  const f32x4 g0 = *reinterpret_cast<const f32x4*>(q8), g1 = *reinterpret_cast<const f32x4*>(q8 + 4);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  v0 = ok ? g0 : z;
  v1 = ok ? g1 : z;
}

// split of a copy unit and its three 16-byte LDS stores: slot `bb` of the hi plane pair, mid and lo one plane PAIR (2 x bpl) on
__device__ __forceinline__ void split_store_unit(u32x4* bb, int bpl, const f32x4& v0, const f32x4& v1) {
  u32x4 hi, mid, lo;
  split8(v0, v1, hi, mid, lo);
  bb[0] = hi;
  bb[2 * bpl] = mid;
  bb[4 * bpl] = lo;
}

// LDS written by one lane, read by another of the SAME wave (the wave-private stages: LDS operations of one wave execute in
// order; this only keeps the compiler from reordering them)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A fragments (three terms) of CT consecutive column tiles from tile `tile0` of a [tile][term][lane] block of packed weights
template <int CT>
__device__ __forceinline__ void read_a(const u32x4* A, int tile0, int lane, bf16x8 (&at)[3][CT]) {
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int t = 0; t < 3; ++t) at[t][ct] = __builtin_bit_cast(bf16x8, A[((tile0 + ct) * 3 + t) * 64 + lane]);
}

// (weight term, texel term), smallest products first
constexpr int ORDER9[9][2] = {{2, 2}, {2, 1}, {1, 2}, {2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}};

// the last NPROD term products of one K block into NR x CT accumulators: product outermost, then row (or tap class), then column
// tile, so consecutive MFMAs go to different accumulators.  bfrag(texel term, row) = the row's B fragment, wherever the caller keeps it
template <int NPROD, int NR, int CT, class BFrag>
__device__ __forceinline__ void term_products(const bf16x8 (&at)[3][CT], BFrag bfrag, f32x4 (&acc)[NR][CT]) {
#pragma unroll
  for (int pi = 9 - NPROD; pi < 9; ++pi)
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        acc[r][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at[ORDER9[pi][0]][ct], bfrag(ORDER9[pi][1], r), acc[r][ct], 0, 0, 0);
}

// accumulator + bias, LeakyReLU
__device__ __forceinline__ f32x4 bias_act(const f32x4& acc, const f32x4& bv, int act, float alpha) {
  f32x4 v = acc + bv;
  if (act) {
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) v[c4] = v[c4] > 0.f ? v[c4] : alpha * v[c4];
  }
  return v;
}

__host__ __device__ inline u16 bf16_rne_bits(float f) {
  union { float f; unsigned u; } x; x.f = f;
  x.u += 0x7fffu + ((x.u >> 16) & 1u);
  return (u16)(x.u >> 16);
}
__host__ __device__ inline float bf16_bits_float(u16 b) {
  union { float f; unsigned u; } x; x.u = (unsigned)b << 16;
  return x.f;
}

// packed weights: [g = cout / TN][cc = cin / 16][pair 2][ct TNT][term 3][lane 64][e 8] bf16; Keras (kh,kw,Cin,Cout), t = a*2+b
__global__ void pack_tile3_kernel(const float* __restrict__ wk, int cin, int cout, int tnt, long total, u16* __restrict__ wp) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int e = idx & 7, lane = (idx >> 3) & 63;
  long r = idx >> 9;
  const int term = r % 3; r /= 3;
  const int ct = r % tnt; r /= tnt;
  const int pair = r & 1; r >>= 1;
  const int ncc = cin >> 4;
  const int cc = r % ncc;
  const int g = r / ncc;
  const int kk = lane >> 4, i = lane & 15;
  const int t = pair * 2 + (kk >> 1);
  const int c = cc * 16 + (kk & 1) * 8 + e;
  const int o = (g * tnt + ct) * 16 + i;
  const float v = wk[((long)t * cin + c) * cout + o];
  const u16 hi = bf16_rne_bits(v);
  const float r1 = v - bf16_bits_float(hi);
  const u16 mid = bf16_rne_bits(r1);
  const float r2 = r1 - bf16_bits_float(mid);
  wp[idx] = term == 0 ? hi : (term == 1 ? mid : bf16_rne_bits(r2));
}

// one finished observation frame i of an NR x 16 texel tile: bias, LeakyReLU, `out`, the running observation mean and, with the
// last observation, `mean_out`.  Lane (kk, j) holds channels oc0 + 16 ct + [0, 4) of texel (gy0 + r, gx).  The accumulators are
// cleared for the next frame; NEXT_ITEM: the registers go on to another tile (persistent forms), which starts its own mean
template <bool NEXT_ITEM, int NR, int CT>
__device__ __forceinline__ void epilogue(const Tile3P& p, int f, int i, int oc0, int gy0, int gx, f32x4 (&acc)[NR][CT],
                                         f32x4 (&mean)[NR][CT]) {
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int oc = oc0 + 16 * ct;
    const f32x4 bv = *reinterpret_cast<const f32x4*>(p.bias + oc);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int gy = gy0 + r;
      const f32x4 v = bias_act(acc[r][ct], bv, p.act, p.alpha);
      acc[r][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
      mean[r][ct] += v;
      if (gy < p.oh && gx < p.ow) {
        const long ot = ((long)(f * p.kobs + i) * p.oh + gy) * p.ow + gx;
        if (p.out) *reinterpret_cast<f32x4*>(p.out + ot * p.ldo + oc) = v;
        if (p.mean_out && i == p.kobs - 1) {
          const long mt = ((long)f * p.oh + gy) * p.ow + gx;
          *reinterpret_cast<f32x4*>(p.mean_out + mt * p.ldm + oc) = mean[r][ct] * (1.f / (float)p.kobs);
        }
      }
      if (NEXT_ITEM && i == p.kobs - 1) mean[r][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
}

// The SHARED STAGE of a 8 x 16 output tile (conv_tile3_kernel, conv_tile3r_kernel): term planes [term][half][slot] of BPL slots.
// Copy unit u -> its channel half, its slot in the hi plane pair (+ term * 2 * BPL) and whether the unit exists at all ...
template <int MODE>
__device__ __forceinline__ void unit_slot(int u, int& hf, int& slot, bool& st) {
  const int tx = unit_texel(u);
  hf = unit_half(u);
  if (MODE == NLT_CONV_K2S1) {                                          // haloed 9 x 17 tile, row-major
    st = tx < 153;
    slot = hf * PL + tx;
  } else {                                                              // one tap row: 8 x 32 input texels, by x parity
    const int y = tx >> 5, xx = tx & 31;
    st = tx < 256;
    slot = hf * QS2 + (xx & 1) * ODD2 + y * 16 + (xx >> 1);
  }
}
// ... and, per tile (origin ty0, tx0 in output texels), texel tx of the staged tile in the input map and whether it lies inside.
// (k2s1: any haloed tile of 17 columns, so the wave-private RT x 16 tiles use it too)
template <int MODE>
__device__ __forceinline__ void unit_source(const Tile3P& p, int tx, bool st, int ty0, int tx0, bool& ok, long& tex) {
  if (MODE == NLT_CONV_K2S1) {
    const int gy = ty0 + tx / 17, gx = tx0 + tx % 17;
    ok = st && gy < p.h && gx < p.w;
    tex = (long)gy * p.w + gx;
  } else {
    const int y = tx >> 5, xx = tx & 31;
    const int gy = 2 * (ty0 + y), gx = 2 * tx0 + xx;
    ok = st && (ty0 + y) < p.oh && gx < p.w;
    tex = (long)gy * p.w + gx;
  }
}
// one slab's products of wave (wm, wn): per tap pair, the B fragments of its RT rows, the A fragments of its CT column tiles
template <int MODE, int TNT, int NPROD, int RT, int CT>
__device__ __forceinline__ void stage_products(const u32x4* A, const u32x4* B, int lane, int wm, int wn, f32x4 (&acc)[RT][CT]) {
  constexpr int BPL = MODE == NLT_CONV_K2S1 ? PL : QS2;
  const int kk = lane >> 4, j = lane & 15;
#pragma unroll
  for (int pl = 0; pl < T3<MODE>::PAIRS; ++pl) {
    bf16x8 bt[3][RT], at[3][CT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int y = wm * RT + rt;
      const int slot = MODE == NLT_CONV_K2S1 ? (kk & 1) * PL + (y + pl) * 17 + j + (kk >> 1)
                                             : (kk & 1) * QS2 + (kk >> 1) * ODD2 + y * 16 + j;
#pragma unroll
      for (int t = 0; t < 3; ++t) bt[t][rt] = __builtin_bit_cast(bf16x8, B[t * 2 * BPL + slot]);
    }
    read_a(A, pl * TNT + wn * CT, lane, at);
    term_products<NPROD>(at, [&](int t, int rt) { return bt[t][rt]; }, acc);
  }
}

// KO = observation frames of a tile that share ONE pass over the layer's weights (r04).  The weights are the larger half of what a
// stage moves (k2s1 at 64 channels: 24.6 KB of term fragments against 9.8 KB of texels; every workgroup of the chip streams them
// from L2), and the counter passes of r04 show the operand path, not the matrix pipe, bounding these launches.  With KO > 1 the
// stage order is (channel slab s, observation io) instead of (observation, slab): the slab's weight fragments are staged once and
// stay in LDS for KO micro-stages, each of which brings only the texel slab of its observation; every observation has its own
// accumulators (KO x RT x CT), and the frames' epilogues run together after the last slab.  kobs = groups x KO; the mean over
// all of them stays in registers as before.  KO = 1 is the r03 order.
template <int MODE, int TNT, int NPROD, int KO>
__global__ __launch_bounds__(256, 2) void conv_tile3_kernel(Tile3P p) {
  using TT = T3<MODE>;
  constexpr int WN = TNT == 4 ? 2 : 1, WM = 4 / WN, RT = TH / WM, CT = 2;
  constexpr int A_SLOTS = TT::PAIRS * TNT * 3 * 64;                    // 16-byte slots
  constexpr int NA = (A_SLOTS + 255) / 256, NB = (TT::B_UNITS + 255) / 256;      // (k2s2, TN = 32: 384 slots -> the last pass is half full)
  __shared__ u32x4 lds[2 * A_SLOTS + 2 * TT::B_SLOTS];                 // [A of slab parity 0 | 1][B of micro-stage parity 0 | 1]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kk = lane >> 4, j = lane & 15;
  const int wn = wave % WN, wm = wave / WN;
  int tile = xcd_tile3(blockIdx.x, gridDim.x);
  const int tx0 = (tile % p.tiles_x) * TW; tile /= p.tiles_x;
  const int ty0 = (tile % p.tiles_y) * TH;
  const int f = tile / p.tiles_y;
  const int g = blockIdx.y;
  const int spf = (MODE == NLT_CONV_K2S1 ? 1 : 2) * p.ncc;             // slabs (stages) per frame
  const int groups = p.kobs / KO;
  const int total = spf * p.kobs;                                      // micro-stages
  const long in_frame = (long)p.h * p.w;

  int b_lds[NB], b_hf[NB]; long b_tex[NB]; bool b_ok[NB], b_st[NB];    // B copy units
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    unit_slot<MODE>(tid + 256 * i, b_hf[i], b_lds[i], b_st[i]);
    unit_source<MODE>(p, unit_texel(tid + 256 * i), b_st[i], ty0, tx0, b_ok[i], b_tex[i]);
  }
  constexpr int BPL = MODE == NLT_CONV_K2S1 ? PL : QS2;

  u32x4 ra[NA];
  f32x4 rb[NB][2];
  // micro-stage (group gi, slab s, observation io): texel slab of frame gi * KO + io; weights of slab s (io == 0 only)
  auto load_a = [&](int s) {
    const int cc = MODE == NLT_CONV_K2S1 ? s : (s >> 1);
    const int a = MODE == NLT_CONV_K2S1 ? 0 : (s & 1);
    const u32x4* ap = reinterpret_cast<const u32x4*>(p.packed) + (((long)g * p.ncc + cc) * 2 + a) * (TNT * 3 * 64);
#pragma unroll
    for (int n = 0; n < NA; ++n) ra[n] = ap[(A_SLOTS % 256 == 0 || tid + 256 * n < A_SLOTS) ? tid + 256 * n : tid];
  };
  auto load_b = [&](int s, int frame) {
    const int cc = MODE == NLT_CONV_K2S1 ? s : (s >> 1);
    const int a = MODE == NLT_CONV_K2S1 ? 0 : (s & 1);
    const float* sp = p.src + ((long)(f * p.kobs + frame) * in_frame + (long)a * p.w) * p.ld + cc * 16;
#pragma unroll
    for (int n = 0; n < NB; ++n) gather_unit(sp, p.ld, b_ok[n], b_tex[n], b_hf[n], rb[n][0], rb[n][1]);
  };
  auto store_a = [&](int buf) {
    u32x4* base = lds + buf * A_SLOTS;
#pragma unroll
    for (int n = 0; n < NA; ++n)
      if (A_SLOTS % 256 == 0 || tid + 256 * n < A_SLOTS) base[tid + 256 * n] = ra[n];
  };
  auto store_b = [&](int buf) {
    u32x4* base = lds + 2 * A_SLOTS + buf * TT::B_SLOTS;
#pragma unroll
    for (int n = 0; n < NB; ++n)
      if (b_st[n]) split_store_unit(base + b_lds[n], BPL, rb[n][0], rb[n][1]);
  };

  f32x4 acc[KO][RT][CT], mean[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      mean[rt][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int io = 0; io < KO; ++io) acc[io][rt][ct] = mean[rt][ct];
    }

  load_a(0);
  load_b(0, 0);
  store_a(0);
  store_b(0);
  __syncthreads();
  int q = 0;                                                            // micro-stage counter (its parity = B buffer)
  for (int gi = 0; gi < groups; ++gi) {
    for (int s = 0; s < spf; ++s) {
      const int sa = (gi * spf + s) & 1;                                // A buffer of this slab
#pragma unroll
      for (int io = 0; io < KO; ++io, ++q) {
        // next micro-stage: (gi, s, io + 1), else (gi, s + 1, 0) -- with the next slab's weights --, else (gi + 1, 0, 0)
        const bool more = q + 1 < total;
        const bool new_slab = io + 1 == KO;
        int ns = s, ngi = gi;
        if (new_slab) { if (++ns == spf) { ns = 0; ++ngi; } }
        if (more) {
          if (new_slab) load_a(ns);
          load_b(ns, ngi * KO + (new_slab ? 0 : io + 1));
        }
        stage_products<MODE, TNT, NPROD>(lds + sa * A_SLOTS, lds + 2 * A_SLOTS + (q & 1) * TT::B_SLOTS, lane, wm, wn, acc[io]);
        if (s == spf - 1 && io == KO - 1) {                             // the group's KO observation frames are complete
#pragma unroll
          for (int e = 0; e < KO; ++e)
            epilogue<false>(p, f, gi * KO + e, (g * TNT + wn * CT) * 16 + 4 * kk, ty0 + wm * RT, tx0 + j, acc[e], mean);
        }
        if (more) {
          if (new_slab) store_a(sa ^ 1);
          store_b((q + 1) & 1);
        }
        __syncthreads();
      }
    }
  }
}

// B fragments of the stride-2 conv WITHOUT a texel stage: a 2 x 2 stride-2 conv on an even map has no halo and no tap overlap, so
// lane (kk, j)'s operand of output texel (y, x = x0 + j) in slab (cc, a) is channels 16 cc + 8 (kk & 1) ... + 8 of input texel
// (2y + a, 2x + (kk >> 1)): 32 contiguous bytes of global memory.  gather_b_s2 is the two 16-byte loads at `q8` (the caller's
// clamped address: always readable, so the loads are unconditional and can be issued slabs ahead of their use); terms_b_s2 runs
// when the values are needed: zeros where the output texel lies outside the map, split8 in registers, and the three terms ARE the
// B fragments term_products takes.
__device__ __forceinline__ void gather_b_s2(const float* q8, f32x4& v0, f32x4& v1) {
  v0 = *reinterpret_cast<const f32x4*>(q8);
  v1 = *reinterpret_cast<const f32x4*>(q8 + 4);
}
__device__ __forceinline__ void terms_b_s2(bool ok, const f32x4& v0, const f32x4& v1, bf16x8& hi, bf16x8& mid, bf16x8& lo) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  u32x4 t[3];
  split8(ok ? v0 : z, ok ? v1 : z, t[0], t[1], t[2]);
  hi = __builtin_bit_cast(bf16x8, t[0]);
  mid = __builtin_bit_cast(bf16x8, t[1]);
  lo = __builtin_bit_cast(bf16x8, t[2]);
}

// TEXELS DIRECT, streaming (stride 2 only): conv_tile3_kernel<NLT_CONV_K2S2> with gather_b_s2 in place of load_b / store_b / the B
// planes.  The weights still go through the double-buffered A stage, with ONE barrier per slab (not per micro-stage: nothing else
// is shared); LDS is the two A buffers (24.6 KB at TN = 64).  Every wave takes RT = 2 rows of the 8 x 16 tile and ALL of the group's
// TNT column tiles, so no two waves of a workgroup load the same texel.  A wave's texel loads sit in a register ring of two
// micro-stages: a slot is split into its terms, then refilled at once with the loads of micro-stage q + 2, so the loads of q + 1
// and q + 2 are in flight under the MFMAs of q, on the wave's own count and whatever the barrier does.  The slab's weight
// loads are issued BEFORE that refill: memory returns in order, and the wait before the LDS store of the weights then covers the
// loads issued earlier, not the ring's newest.  All loads are unconditional: past the last micro-stage the cursor stays on the
// last (group, slab) and the values are dropped.  Slabs s = 2 cc + a: the parity of s is the tap row a (and the A buffer), so the
// body unrolls over (a, io) and every ring slot and accumulator set has a static index.  Per output element: slabs in order,
// ORDER9, bias, LeakyReLU -- conv_tile3_kernel's bits.  No observation mean (the stride-2 launches have none).
// Launch bound = the workgroups per CU the registers allow without scratch (found by compiling): 3 (110-166 VGPRs), 2 where
// TNT x KO accumulator sets reach 8 (180-200 VGPRs).
template <int TNT, int NPROD, int KO>
__global__ __launch_bounds__(256, TNT * KO >= 8 ? 2 : 3) void conv_tile3d_kernel(Tile3P p) {
  constexpr int WM = 4, RT = TH / WM, CT = TNT;
  constexpr int A_SLOTS = TNT * 3 * 64;                                 // 16-byte slots of one slab's weights
  constexpr int NA = (A_SLOTS + 255) / 256;                             // (TN = 32: 384 slots -> the last pass is half full)
  constexpr int NM = 2 * KO;                                            // micro-stages of the unrolled body: (a, io)
  __shared__ u32x4 lds[2 * A_SLOTS];                                    // [A of tap row 0 | 1]
  p.mean_out = nullptr;                                                 // (known here: the shared epilogue's mean folds away)

  const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
  const int kk = lane >> 4, j = lane & 15;
  int tile = xcd_tile3(blockIdx.x, gridDim.x);
  const int tx0 = (tile % p.tiles_x) * TW; tile /= p.tiles_x;
  const int ty0 = (tile % p.tiles_y) * TH;
  const int f = tile / p.tiles_y;
  const int g = blockIdx.y;
  const int groups = p.kobs / KO;
  const int nouter = groups * p.ncc;                                    // (observation group gi, channel slab cc), gi outermost
  const long in_frame = (long)p.h * p.w;

  // the lane's texel of tap row 0 per output row, as an element offset from the slab's base (tile3_params bounds the whole map
  // below 2^31 elements); outside the map: texel (0, 0) of the frame
  int b_off[RT]; bool b_ok[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int y = ty0 + wm * RT + rt, x = tx0 + j;
    b_ok[rt] = y < p.oh && x < p.ow;
    b_off[rt] = (b_ok[rt] ? (2 * y * p.w + 2 * x + (kk >> 1)) * p.ld : 0) + 8 * (kk & 1);
  }

  u32x4 ra[NA];
  f32x4 rb[2][RT][2];                                                   // the ring: micro-stage parity
  auto load_a = [&](int cc, int a) {
    const u32x4* ap = reinterpret_cast<const u32x4*>(p.packed) + (((long)g * p.ncc + cc) * 2 + a) * A_SLOTS;
#pragma unroll
    for (int n = 0; n < NA; ++n) ra[n] = ap[(A_SLOTS % 256 == 0 || tid + 256 * n < A_SLOTS) ? tid + 256 * n : tid];
  };
  auto store_a = [&](int buf) {
    u32x4* base = lds + buf * A_SLOTS;
#pragma unroll
    for (int n = 0; n < NA; ++n)
      if (A_SLOTS % 256 == 0 || tid + 256 * n < A_SLOTS) base[tid + 256 * n] = ra[n];
  };
  auto load_b = [&](int u, int gi, int cc, int a, int io) {
    const float* sp = p.src + ((long)(f * p.kobs + gi * KO + io) * in_frame + (long)a * p.w) * p.ld + cc * 16;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) gather_b_s2(sp + b_off[rt], rb[u][rt][0], rb[u][rt][1]);
  };

  f32x4 acc[KO][RT][CT], mean[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      mean[rt][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int io = 0; io < KO; ++io) acc[io][rt][ct] = mean[rt][ct];
    }

  // peeled start: slab 0's weights, then the ring's two slots (micro-stages 0 and 1 of the first body)
  load_a(0, 0);
  load_b(0, 0, 0, 0, 0);
  load_b(1, 0, 0, 1 / KO, 1 % KO);
  store_a(0);
  __syncthreads();
  int gi = 0, cc = 0;
  for (int o = 0; o < nouter; ++o) {
    int ngi = gi, nc = cc + 1;                                          // the next (gi, cc); after the last one: itself again
    if (nc == p.ncc) { nc = 0; ++ngi; }
    if (o + 1 == nouter) { ngi = gi; nc = cc; }
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const int a = m / KO, io = m % KO, u = m & 1;
      bf16x8 bt[3][RT], at[3][CT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) terms_b_s2(b_ok[rt], rb[u][rt][0], rb[u][rt][1], bt[0][rt], bt[1][rt], bt[2][rt]);
      if (io == 0) {                                                    // the next slab's weights: tap row 1 of cc, else row 0 of the next
        if (a == 0) load_a(cc, 1);
        else load_a(nc, 0);
      }
      if (m + 2 < NM) load_b(u, gi, cc, (m + 2) / KO, (m + 2) % KO);    // micro-stage q + 2 into the slot just emptied
      else load_b(u, ngi, nc, (m + 2 - NM) / KO, (m + 2 - NM) % KO);
      // (the loads stay ABOVE the MFMAs: left alone, the scheduler sinks them to their uses to save registers, and the weight
      // store then waits out a whole memory latency behind the MFMAs instead of under them)
      __builtin_amdgcn_sched_barrier(0);
      read_a(lds + a * A_SLOTS, 0, lane, at);
      term_products<NPROD>(at, [&](int t, int rt) { return bt[t][rt]; }, acc[io]);
      if (m == NM - 1 && cc == p.ncc - 1) {                             // the group's KO observation frames are complete
#pragma unroll
        for (int e = 0; e < KO; ++e) epilogue<false>(p, f, gi * KO + e, g * TNT * 16 + 4 * kk, ty0 + wm * RT, tx0 + j, acc[e], mean);
      }
      if (io == KO - 1) {
        store_a(a ^ 1);
        __syncthreads();
      }
    }
    gi = ngi; cc = nc;
  }
}

template <int TNT, int KO>
int launch3d_k(const Tile3P& p, int nprod, hipStream_t s) {
  const dim3 grid((unsigned)((long)p.frames * p.tiles_y * p.tiles_x), (unsigned)(p.cout / (16 * TNT)));
  if (nprod == 9) hipLaunchKernelGGL((conv_tile3d_kernel<TNT, 9, KO>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((conv_tile3d_kernel<TNT, 6, KO>), grid, dim3(256), 0, s, p);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

// KO as the streaming kernel takes it: 4 at 32 channels per workgroup, 2 at 64, where kobs divides
template <int TNT>
int launch3d(const Tile3P& p, int nprod, hipStream_t s) {
  if (TNT == 2 && p.kobs % 4 == 0) return launch3d_k<TNT, (TNT == 2 ? 4 : 1)>(p, nprod, s);
  if (p.kobs % 2 == 0) return launch3d_k<TNT, 2>(p, nprod, s);
  return launch3d_k<TNT, 1>(p, nprod, s);
}

// RESIDENT form (stride 2, and 64 channels per group; the stride-1 conv at 32 channels per group: conv_tile3w_kernel below):
// persistent workgroups, each with the split weights of ONE output-channel group in LDS for as long as it works on
// that group (cin x TNT x 384 bytes, copied once), so a stage moves only its texel slab: load_a / store_a and their staging
// registers leave the loop.  The (group, frame, tile) items are cut into one contiguous run per workgroup (runs of one XCD are
// neighbours); the micro-stage sequence runs on across items as one software pipeline -- the first slab of the next item is in
// flight under the last stage of the current one -- and every global load of the loop is unconditional (after the last stage it
// re-reads a slab of the same tile and the value is dropped).  NWV = waves per workgroup: 4 (two workgroups per CU) or, where
// two do not fit the CU's 160 KB, 8 waves on the same 8 x 16 tile (twice the wave rows, RT halved).  Per output element the
// additions are those of conv_tile3_kernel in the same order: the two forms give the same bits.
extern __shared__ u32x4 tile3r_lds[];

template <int MODE, int TNT, int NPROD, int KO, int NWV>
__global__ __launch_bounds__(64 * NWV, 2) void conv_tile3r_kernel(Tile3P p, int ngroups) {
  using TT = T3<MODE>;
  constexpr int NT = 64 * NWV;
  constexpr int WN = TNT == 4 ? 2 : 1, WM = NWV / WN, RT = TH / WM, CT = 2;
  constexpr int A_SLOTS = TT::PAIRS * TNT * 3 * 64;                    // 16-byte slots of one slab's weights
  constexpr int NB = (TT::B_UNITS + NT - 1) / NT;
  constexpr int BPL = MODE == NLT_CONV_K2S1 ? PL : QS2;
  const int a_group = p.ncc * 2 * TNT * 3 * 64;                        // slots of a group's weights: [cc][pair][ct][term][lane]
  u32x4* const lds_b = tile3r_lds + a_group;                           // [A of the group][B of micro-stage parity 0 | 1]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kk = lane >> 4, j = lane & 15;
  const int wn = wave % WN, wm = wave / WN;
  const int spf = (MODE == NLT_CONV_K2S1 ? 1 : 2) * p.ncc;             // slabs (stages) per frame
  const int groups = p.kobs / KO;
  const long in_frame = (long)p.h * p.w;
  // this workgroup's items: item = g * tiles + (f * tiles_y + ty) * tiles_x + tx, run [it, it_end)
  const int tiles = p.frames * p.tiles_y * p.tiles_x;
  const long items = (long)tiles * ngroups;
  const int rank = xcd_tile3(blockIdx.x, gridDim.x);
  int it = (int)(rank * items / gridDim.x);
  const int it_end = (int)((rank + 1) * items / gridDim.x);
  if (it >= it_end) return;

  int b_lds[NB], b_hf[NB]; long b_tex[NB]; bool b_ok[NB], b_st[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) unit_slot<MODE>(tid + NT * i, b_hf[i], b_lds[i], b_st[i]);
  int ng = 0, nf = 0, nty0 = 0, ntx0 = 0;                               // the item whose slabs are being LOADED
  auto geom = [&](int item) {
    ng = item / tiles;
    int t = item - ng * tiles;
    ntx0 = (t % p.tiles_x) * TW; t /= p.tiles_x;
    nty0 = (t % p.tiles_y) * TH;
    nf = t / p.tiles_y;
#pragma unroll
    for (int i = 0; i < NB; ++i) unit_source<MODE>(p, unit_texel(tid + NT * i), b_st[i], nty0, ntx0, b_ok[i], b_tex[i]);
  };

  f32x4 rb[NB][2];
  auto load_b = [&](int s, int frame) {
    const int cc = MODE == NLT_CONV_K2S1 ? s : (s >> 1);
    const int a = MODE == NLT_CONV_K2S1 ? 0 : (s & 1);
    const float* sp = p.src + ((long)(nf * p.kobs + frame) * in_frame + (long)a * p.w) * p.ld + cc * 16;
#pragma unroll
    for (int n = 0; n < NB; ++n) gather_unit(sp, p.ld, b_ok[n], b_tex[n], b_hf[n], rb[n][0], rb[n][1]);
  };
  auto store_b = [&](int buf) {
    u32x4* base = lds_b + buf * TT::B_SLOTS;
#pragma unroll
    for (int n = 0; n < NB; ++n)
      if (b_st[n]) split_store_unit(base + b_lds[n], BPL, rb[n][0], rb[n][1]);
  };
  auto copy_a = [&](int grp) {                                          // the group's whole block, as it lies in `packed`
    const u32x4* ap = reinterpret_cast<const u32x4*>(p.packed) + (long)grp * a_group;
    for (int i = tid; i < a_group; i += NT) tile3r_lds[i] = ap[i];
  };

  f32x4 acc[KO][RT][CT], mean[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      mean[rt][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int io = 0; io < KO; ++io) acc[io][rt][ct] = mean[rt][ct];
    }

  geom(it);
  load_b(0, 0);
  copy_a(ng);
  store_b(0);
  __syncthreads();
  int q = 0;                                                            // micro-stage counter (its parity = B buffer)
  for (; it < it_end; ++it) {
    const int g = ng, f = nf, ty0 = nty0, tx0 = ntx0;                   // the item being COMPUTED
    const bool last_item = it + 1 == it_end;
    for (int gi = 0; gi < groups; ++gi) {
      for (int s = 0; s < spf; ++s) {
#pragma unroll
        for (int io = 0; io < KO; ++io, ++q) {
          // next micro-stage: (gi, s, io + 1), else (gi, s + 1, 0), else (gi + 1, 0, 0), else the first of the next item
          const bool new_slab = io + 1 == KO;
          int ns = s, ngi = gi;
          if (new_slab) { if (++ns == spf) { ns = 0; ++ngi; } }
          const bool item_end = ngi == groups;
          if (item_end) {
            ngi = 0;
            if (!last_item) geom(it + 1);
          }
          load_b(ns, ngi * KO + (new_slab ? 0 : io + 1));
          stage_products<MODE, TNT, NPROD>(tile3r_lds + s * A_SLOTS, lds_b + (q & 1) * TT::B_SLOTS, lane, wm, wn, acc[io]);
          if (s == spf - 1 && io == KO - 1) {                           // the group's KO observation frames are complete
#pragma unroll
            for (int e = 0; e < KO; ++e)
              epilogue<true>(p, f, gi * KO + e, (g * TNT + wn * CT) * 16 + 4 * kk, ty0 + wm * RT, tx0 + j, acc[e], mean);
          }
          if (!(item_end && last_item)) store_b((q + 1) & 1);
          __syncthreads();
        }
      }
    }
    if (!last_item && ng != g) {                                        // the run crosses into the next group: its weights
      copy_a(ng);
      __syncthreads();
    }
  }
}

constexpr size_t TILE3R_LDS_CU = 160 * 1024;                           // LDS of a CU (gfx950)

int tile3r_cus() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return v;
  }();
  return n;
}

// workgroups of a persistent launch: per_cu on every CU, at most max_wg (where > 0) and no more than there are items;
// 0 where the device cannot be asked
long tile3r_grid(int per_cu, int max_wg, long items) {
  long nwg = (long)tile3r_cus() * per_cu;
  if (max_wg > 0 && nwg > max_wg) nwg = max_wg;
  return nwg > items ? items : nwg;
}

// dynamic LDS above 64 KB needs the kernel's limit raised: once per device and kernel (`done`: the instantiation's largest size so far)
int tile3r_allow_lds(const void* kernel, size_t lds, size_t (&done)[8]) {
  int dev = 0;
  if (lds <= 64 * 1024) return NLT_OK;
  if (hipGetDevice(&dev) != hipSuccess) return NLT_ERR_LAUNCH;
  if (dev >= 0 && dev < 8 && done[dev] >= lds) return NLT_OK;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return NLT_ERR_LAUNCH;
  if (dev >= 0 && dev < 8) done[dev] = lds;
  return NLT_OK;
}

template <int MODE, int TNT, int NPROD, int KO, int NWV>
int launch3r_k(const Tile3P& p, size_t lds, int nwg, hipStream_t s) {
  auto* k = conv_tile3r_kernel<MODE, TNT, NPROD, KO, NWV>;
  static size_t done[8] = {};
  if (tile3r_allow_lds(reinterpret_cast<const void*>(k), lds, done) != NLT_OK) return NLT_ERR_LAUNCH;
  hipLaunchKernelGGL(k, dim3((unsigned)nwg), dim3(64 * NWV), lds, s, p, p.cout / (16 * TNT));
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

// WAVE-PRIVATE texel staging, the resident form of the stride-1 conv at 32 channels per group: one 8-wave workgroup per CU shares
// the group's resident weights, and every wave owns an RT x 16 output tile of its own -- it stages its (RT + 1) x 17 haloed texels
// in an LDS region nobody else touches, so the steady state has NO workgroup barrier (LDS operations of one wave execute in order;
// wave_sync() only keeps the compiler from reordering them) and the waves of a SIMD drift apart and fill each other's gaps.  A
// stage reads its RT + 1 row fragments to registers first (tap pair 1 of output row r uses the fragment pair 0 of row r + 1 uses:
// 15 reads instead of 24), which frees the region: the next slab is split and written between the MFMAs of the issuing wave,
// where bf16 MFMAs co-execute with VALU work (r05), with one buffer.  Price: (RT + 1) / RT times the texel loads and splits.
// A workgroup's run of items is cut at group changes (the only barriers: before and after the weights are replaced); inside a
// segment wave v takes items v, v + 8, ...  Per output element: slabs in order, tap pairs in order, ORDER9 -- conv_tile3_kernel's bits.
template <int RT, int NPROD>
__global__ __launch_bounds__(512, 2) void conv_tile3w_kernel(Tile3P p, int ngroups, int tiles_y) {
  constexpr int TNT = 2, CT = 2, NWV = 8;
  constexpr int ROWS = RT + 1, UNITS = ROWS * 17 * 2, NB = (UNITS + 63) / 64;
  constexpr int PLW = (ROWS * 17 + 15) / 16 * 16;                       // slots per (term, half) plane
  constexpr int A_SLOTS = 2 * TNT * 3 * 64;
  const int a_group = p.ncc * A_SLOTS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kk = lane >> 4, j = lane & 15;
  u32x4* const B = tile3r_lds + a_group + wave * (6 * PLW);
  const long in_frame = (long)p.h * p.w;
  const int tiles = p.frames * tiles_y * p.tiles_x;
  const long items = (long)tiles * ngroups;
  const int rank = xcd_tile3(blockIdx.x, gridDim.x);
  const int it0 = (int)(rank * items / gridDim.x), it1 = (int)((rank + 1) * items / gridDim.x);

  int b_lds[NB], b_hf[NB], b_tx[NB]; long b_tex[NB]; bool b_ok[NB], b_st[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    b_hf[i] = unit_half(lane + 64 * i);
    b_tx[i] = unit_texel(lane + 64 * i);
    b_st[i] = b_tx[i] < ROWS * 17;
    b_lds[i] = b_hf[i] * PLW + b_tx[i];
  }
  int nf = 0, nty0 = 0, ntx0 = 0;
  auto geom = [&](int t) {
    ntx0 = (t % p.tiles_x) * TW; t /= p.tiles_x;
    nty0 = (t % tiles_y) * RT;
    nf = t / tiles_y;
#pragma unroll
    for (int i = 0; i < NB; ++i) unit_source<NLT_CONV_K2S1>(p, b_tx[i], b_st[i], nty0, ntx0, b_ok[i], b_tex[i]);
  };
  f32x4 rb[NB][2];
  auto load_b = [&](int cc, int frame) {
    const float* sp = p.src + (long)(nf * p.kobs + frame) * in_frame * p.ld + cc * 16;
#pragma unroll
    for (int n = 0; n < NB; ++n) gather_unit(sp, p.ld, b_ok[n], b_tex[n], b_hf[n], rb[n][0], rb[n][1]);
  };
  auto store_b = [&]() {
#pragma unroll
    for (int n = 0; n < NB; ++n)
      if (b_st[n]) split_store_unit(B + b_lds[n], PLW, rb[n][0], rb[n][1]);
  };

  int seg = it0;
  while (seg < it1) {                                                   // one segment per output-channel group of the run
    const int g = seg / tiles;
    const int seg_end = min(it1, (g + 1) * tiles);
    {
      const u32x4* ap = reinterpret_cast<const u32x4*>(p.packed) + (long)g * a_group;
      for (int i = tid; i < a_group; i += 64 * NWV) tile3r_lds[i] = ap[i];
    }
    __syncthreads();
    int it = seg + wave;
    if (it < seg_end) {
      f32x4 acc[RT][CT], mean[RT][CT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = mean[rt][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
      geom(it - g * tiles);
      load_b(0, 0);
      store_b();
      wave_sync();
      for (; it < seg_end; it += NWV) {
        const int f = nf, ty0 = nty0, tx0 = ntx0;
        const bool last_item = it + NWV >= seg_end;
        for (int i = 0; i < p.kobs; ++i) {
          for (int s = 0; s < p.ncc; ++s) {
            int ns = s + 1, ni = i;
            if (ns == p.ncc) { ns = 0; ++ni; }
            const bool item_end = ni == p.kobs;
            if (item_end) {
              ni = 0;
              if (!last_item) geom(it + NWV - g * tiles);
            }
            load_b(ns, ni);
            bf16x8 bt[3][ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
#pragma unroll
              for (int t = 0; t < 3; ++t)
                bt[t][r] = __builtin_bit_cast(bf16x8, B[t * 2 * PLW + (kk & 1) * PLW + r * 17 + j + (kk >> 1)]);
            wave_sync();
            const u32x4* A = tile3r_lds + s * A_SLOTS;
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
              bf16x8 at[3][CT];
              read_a(A, pl * TNT, lane, at);
              term_products<NPROD>(at, [&](int t, int rt) { return bt[t][rt + pl]; }, acc);
            }
            if (!(item_end && last_item)) store_b();
            wave_sync();
            if (s == p.ncc - 1) epilogue<true>(p, f, i, g * TNT * 16 + 4 * kk, ty0, tx0 + j, acc, mean);
          }
        }
      }
    }
    seg = seg_end;
    if (seg < it1) __syncthreads();                                     // every wave is done with this group's weights
  }
}

// LDS = the group's weights + 8 single-buffered wave regions of 6 planes; refused where that exceeds the CU's 160 KB
template <int RT>
int launch3w(const Tile3P& p, int nprod, int max_wg, hipStream_t s) {
  constexpr int PLW = ((RT + 1) * 17 + 15) / 16 * 16;
  const size_t lds = (size_t)p.cin * 2 * 384 + 8 * 6 * PLW * sizeof(u32x4);
  if (lds > TILE3R_LDS_CU) return NLT_ERR_UNSUPPORTED;
  const int tiles_y = (p.oh + RT - 1) / RT;
  const long nwg = tile3r_grid(1, max_wg, (long)p.frames * tiles_y * p.tiles_x * (p.cout / 32));
  if (nwg <= 0) return NLT_ERR_LAUNCH;
  auto* k = nprod == 9 ? conv_tile3w_kernel<RT, 9> : conv_tile3w_kernel<RT, 6>;
  static size_t done[2][8] = {};
  if (tile3r_allow_lds(reinterpret_cast<const void*>(k), lds, done[nprod == 9]) != NLT_OK) return NLT_ERR_LAUNCH;
  hipLaunchKernelGGL(k, dim3((unsigned)nwg), dim3(512), lds, s, p, p.cout / 32, tiles_y);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

// resident form (other than wave-private): LDS = the group's weights + the double-buffered texel stage; two 4-wave workgroups per CU where two fit the
// CU's 160 KB, else one 8-wave workgroup (never fewer than 8 waves per CU); what does not fit at all is refused
template <int MODE, int TNT, int KO>
int launch3r(const Tile3P& p, int nprod, int max_wg, hipStream_t s) {
  if (nprod != 6 && nprod != 9) return NLT_ERR_UNSUPPORTED;
  if (MODE == NLT_CONV_K2S1 && TNT == 2) {                              // wave-private staging: 4-row tiles, 2-row where 4 do not fit
    int st = launch3w<4>(p, nprod, max_wg, s);
    if (st == NLT_ERR_UNSUPPORTED) st = launch3w<2>(p, nprod, max_wg, s);
    if (st != NLT_ERR_UNSUPPORTED) return st;
  }
  const size_t lds = (size_t)p.cin * TNT * 384 + 2 * T3<MODE>::B_SLOTS * sizeof(u32x4);
  if (lds > TILE3R_LDS_CU) return NLT_ERR_UNSUPPORTED;
  const bool wide = 2 * lds > TILE3R_LDS_CU;
  const long items = (long)p.frames * p.tiles_y * p.tiles_x * (p.cout / (16 * TNT));
  const int nwg = (int)tile3r_grid(wide ? 1 : 2, max_wg, items);
  if (nwg <= 0) return NLT_ERR_LAUNCH;
  if (items >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  if (wide) return nprod == 9 ? launch3r_k<MODE, TNT, 9, KO, 8>(p, lds, nwg, s) : launch3r_k<MODE, TNT, 6, KO, 8>(p, lds, nwg, s);
  return nprod == 9 ? launch3r_k<MODE, TNT, 9, KO, 4>(p, lds, nwg, s) : launch3r_k<MODE, TNT, 6, KO, 4>(p, lds, nwg, s);
}

// resident_wg < 0: the streaming kernel; >= 0: the resident form with at most that many workgroups (0 = sized from the device)
template <int MODE, int TNT, int KO>
int launch3k(const Tile3P& p, int nprod, hipStream_t s, int resident_wg) {
  if (resident_wg >= 0) return launch3r<MODE, TNT, KO>(p, nprod, resident_wg, s);
  const long tiles = (long)p.frames * p.tiles_y * p.tiles_x;
  const dim3 grid((unsigned)tiles, (unsigned)(p.cout / (16 * TNT)));
  if (nprod == 9) hipLaunchKernelGGL((conv_tile3_kernel<MODE, TNT, 9, KO>), grid, dim3(256), 0, s, p);
  else if (nprod == 6) hipLaunchKernelGGL((conv_tile3_kernel<MODE, TNT, 6, KO>), grid, dim3(256), 0, s, p);
  else if (KO > 1) return NLT_ERR_UNSUPPORTED;
  else if (nprod == 3) hipLaunchKernelGGL((conv_tile3_kernel<MODE, TNT, 3, 1>), grid, dim3(256), 0, s, p);   // hi*hi + hi*mid + mid*hi (~2^-16)
  else hipLaunchKernelGGL((conv_tile3_kernel<MODE, TNT, 1, 1>), grid, dim3(256), 0, s, p);                  // hi*hi: plain bf16 operands
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

// NLT_TILE3_KO: observation frames per pass over the weights (0 = the largest that fits the registers: 4 at 32 channels per
// workgroup, 2 at 64; 1 = the r03 order) -- A/B switch
template <int MODE, int TNT>
int launch3(const Tile3P& p, int nprod, hipStream_t s, int resident_wg) {
  static const int want = [] { const char* e = getenv("NLT_TILE3_KO"); return e ? atoi(e) : 0; }();
  // (stride-1 conv at 64 channels per workgroup: two sets of 4 x 2 accumulators beside the three-term fragments of 4 rows spill)
  // (the resident form has no weight stage to share: at 64 channels a second accumulator set only spills there)
  const int cap = want > 0 ? want : (TNT == 2 ? 4 : (MODE == NLT_CONV_K2S1 || resident_wg >= 0 ? 1 : 2));
  if (nprod >= 6) {
    if (TNT == 2 && cap >= 4 && p.kobs % 4 == 0) return launch3k<MODE, TNT, (TNT == 2 ? 4 : 1)>(p, nprod, s, resident_wg);
    if (cap >= 2 && p.kobs % 2 == 0) return launch3k<MODE, TNT, 2>(p, nprod, s, resident_wg);
  }
  return launch3k<MODE, TNT, 1>(p, nprod, s, resident_wg);
}

// LEVEL HAND-OFF: conv_tile3w_kernel<4, NPROD> at cin = cout = 32, plus the next level's stride-2 conv (32 -> 64, one K block of
// 32 per tap) per observation on the wave's own results, so the per-observation stride-1 map is never stored or read back.
// The stride-1 stage keeps its four MFMA column tiles by TAP CLASS (ty, tx) of the stride-2 conv instead of by output row:
// column j' = (y', x') = (j >> 3, j & 7) of tile (ty, tx) is texel (2y' + ty, 2x' + tx) of the wave's 4 x 16 tile, i.e. the
// input that output texel j' of the wave's 2 x 8 stride-2 tile reads through tap (ty, tx).  The D layout gives lane (kk, j')
// channels 4kk..4kk+3 of both 16-channel column tiles of that texel; the stride-2 weights are packed with exactly that channel
// order inside a K octet (nlt_tile3s2_fragment), so after bias + LeakyReLU the lane's eight values, split in registers, ARE its B
// fragment: no cross-lane move, no LDS hand-off region, no barrier.  Per output element of the stride-1 conv nothing changes
// (slabs in order, tap pairs in order, ORDER9, bias, LeakyReLU, mean): only the order in which a wave visits its texels does.
// The haloed 5 x 17 planes are stored by x parity, rows 20 slots apart (S2_PITCH): a B read takes columns 2x' + tx + b of rows
// r and r + 2 -- 8 consecutive slots of one parity, twice, 40 = 8 (mod 16) slots apart: 16 different slots mod 16 for every
// 16 lanes that share a b (and the plane stride is 0 mod 16, so the two channel halves of a lane group pair do not matter).
constexpr int S2_PITCH = 20, S2_ODD = 9, S2_PLW = 112;                  // row pitch; first odd-x slot of a row; slots per plane (97 used)
constexpr int S2_A1 = 2 * 2 * 2 * 3 * 64, S2_A2 = 4 * 4 * 3 * 64;      // 16-byte slots of the stride-1 / stride-2 weights
constexpr size_t S2_LDS = (size_t)(S2_A1 + S2_A2 + 8 * 6 * S2_PLW) * sizeof(u32x4) + 96 * sizeof(float);   // + both biases

struct Tile3S2P {
  Tile3P a;
  const u16* packed2; const float* bias2; float* out2;
  int ldo2, act2; float alpha2;
};

template <int NPROD>
__global__ __launch_bounds__(512, 2) void conv_tile3w_s2_kernel(Tile3S2P P, int tiles_y) {
  const Tile3P& p = P.a;
  constexpr int RT = 4, CT = 2, NWV = 8, NCL = 4, NC2 = 4;
  constexpr int UNITS = 5 * 17 * 2, NB = (UNITS + 63) / 64;
  constexpr int A_SLOTS = S2_A1 / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kk = lane >> 4, j = lane & 15, yq = j >> 3, xq = j & 7;
  const u32x4* const A2 = tile3r_lds + S2_A1;
  u32x4* const B = tile3r_lds + S2_A1 + S2_A2 + wave * (6 * S2_PLW);
  float* const biasl = reinterpret_cast<float*>(tile3r_lds + S2_A1 + S2_A2 + 8 * 6 * S2_PLW);    // [32 | 64]
  const long in_frame = (long)p.h * p.w;
  const int oh2 = p.h >> 1, ow2 = p.w >> 1;
  const long items = (long)p.frames * tiles_y * p.tiles_x;
  const int rank = xcd_tile3(blockIdx.x, gridDim.x);
  const int it0 = (int)(rank * items / gridDim.x), it1 = (int)((rank + 1) * items / gridDim.x);

  // B copy units in SLOT order: unit = (slot of the haloed tile, channel half); 8 consecutive lanes write 8 consecutive slots
  int b_lds[NB], b_hf[NB], b_row[NB], b_x[NB]; long b_tex[NB]; bool b_ok[NB], b_st[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int t = unit_texel(lane + 64 * i), q = t % 17;
    b_hf[i] = unit_half(lane + 64 * i);
    b_row[i] = t / 17;
    b_x[i] = q < S2_ODD ? 2 * q : 2 * (q - S2_ODD) + 1;
    b_st[i] = t < 5 * 17;
    b_lds[i] = b_hf[i] * S2_PLW + b_row[i] * S2_PITCH + q;
  }
  int nf = 0, nty0 = 0, ntx0 = 0;
  auto geom = [&](int t) {
    ntx0 = (t % p.tiles_x) * TW; t /= p.tiles_x;
    nty0 = (t % tiles_y) * RT;
    nf = t / tiles_y;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int gy = nty0 + b_row[i], gx = ntx0 + b_x[i];
      b_ok[i] = b_st[i] && gy < p.h && gx < p.w;
      b_tex[i] = (long)gy * p.w + gx;
    }
  };
  f32x4 rb[NB][2];
  auto load_b = [&](int cc, int frame) {
    const float* sp = p.src + (long)(nf * p.kobs + frame) * in_frame * p.ld + cc * 16;
#pragma unroll
    for (int n = 0; n < NB; ++n) gather_unit(sp, p.ld, b_ok[n], b_tex[n], b_hf[n], rb[n][0], rb[n][1]);
  };
  auto store_b = [&]() {
#pragma unroll
    for (int n = 0; n < NB; ++n)
      if (b_st[n]) split_store_unit(B + b_lds[n], S2_PLW, rb[n][0], rb[n][1]);
  };

  {                                                                     // both weight sets, once per workgroup
    const u32x4* a1 = reinterpret_cast<const u32x4*>(p.packed);
    const u32x4* a2 = reinterpret_cast<const u32x4*>(P.packed2);
    for (int i = tid; i < S2_A1; i += 64 * NWV) tile3r_lds[i] = a1[i];
    for (int i = tid; i < S2_A2; i += 64 * NWV) tile3r_lds[S2_A1 + i] = a2[i];
    // (the biases too: a global load in the epilogue would sit behind the next slab's loads in the in-order wait count)
    if (tid < 32) biasl[tid] = p.bias[tid];
    else if (tid < 96) biasl[tid] = P.bias2[tid - 32];
  }
  __syncthreads();
  int it = it0 + wave;
  if (it >= it1) return;
  // fragment (row set rs = ty + pair, tx) of the stride-1 stage: rows rs + 2y', columns 2x' + tx + b, b = kk >> 1
  const int bl0 = (kk & 1) * S2_PLW + 2 * yq * S2_PITCH + xq;
  int offx[2];
#pragma unroll
  for (int tx = 0; tx < 2; ++tx) {
    const int xx = tx + (kk >> 1);
    offx[tx] = (xx & 1) * S2_ODD + (xx >> 1);
  }
  f32x4 acc[NCL][CT], mean[NCL][CT];
#pragma unroll
  for (int c = 0; c < NCL; ++c)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[c][ct] = mean[c][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  geom(it);
  load_b(0, 0);
  store_b();
  wave_sync();
  for (; it < it1; it += NWV) {
    const int f = nf, ty0 = nty0, tx0 = ntx0;
    const bool last_item = it + NWV >= it1;
    for (int i = 0; i < p.kobs; ++i) {
      for (int s = 0; s < 2; ++s) {
        int ns = s + 1, ni = i;
        if (ns == 2) { ns = 0; ++ni; }
        const bool item_end = ni == p.kobs;
        if (item_end) {
          ni = 0;
          if (!last_item) geom(it + NWV);
        }
        load_b(ns, ni);                                                 // (in flight across the MFMAs and, after the last slab, the stride-2 stage)
        bf16x8 bt[3][6];
#pragma unroll
        for (int rs = 0; rs < 3; ++rs)
#pragma unroll
          for (int tx = 0; tx < 2; ++tx)
#pragma unroll
            for (int t = 0; t < 3; ++t)
              bt[t][rs * 2 + tx] = __builtin_bit_cast(bf16x8, B[t * 2 * S2_PLW + bl0 + rs * S2_PITCH + offx[tx]]);
        wave_sync();
        const u32x4* A = tile3r_lds + s * A_SLOTS;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
          bf16x8 at[3][CT];
          read_a(A, pl * 2, lane, at);
          term_products<NPROD>(at, [&](int t, int c) { return bt[t][((c >> 1) + pl) * 2 + (c & 1)]; }, acc);
        }
        if (s == 1) {
          // (its own epilogue: no `out`, tap classes instead of rows, biases from LDS -- and the values stay in registers)
          u32x4 bs[3][NCL];                                             // the stride-2 conv's B fragments: tap class c, three terms
#pragma unroll
          for (int c = 0; c < NCL; ++c) {
            const int gy = ty0 + 2 * yq + (c >> 1), gx = tx0 + 2 * xq + (c & 1);
            f32x4 v2[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
              const int oc = ct * 16 + 4 * kk;
              const f32x4 v = bias_act(acc[c][ct], *reinterpret_cast<const f32x4*>(biasl + oc), p.act, p.alpha);
              acc[c][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
              mean[c][ct] += v;
              if (p.mean_out && i == p.kobs - 1 && gy < p.oh && gx < p.ow) {
                const long mt = ((long)f * p.oh + gy) * p.ow + gx;
                *reinterpret_cast<f32x4*>(p.mean_out + mt * p.ldm + oc) = mean[c][ct] * (1.f / (float)p.kobs);
              }
              if (i == p.kobs - 1) mean[c][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
              v2[ct] = v;
            }
            split8(v2[0], v2[1], bs[0][c], bs[1][c], bs[2][c]);
          }
          f32x4 acc2[NC2 / 2][1][2];                                    // [pair of column tiles]: one row of two tiles per K block
#pragma unroll
          for (int c2 = 0; c2 < NC2; ++c2) acc2[c2 >> 1][0][c2 & 1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int c = 0; c < NCL; ++c) {                               // K block = tap (ty, tx) = c
#pragma unroll
            for (int ch = 0; ch < NC2; ch += 2) {                       // two column tiles at a time: 24 registers of A fragments
              bf16x8 a2[3][2];
              read_a(A2, c * NC2 + ch, lane, a2);
              term_products<NPROD>(a2, [&](int t, int) { return __builtin_bit_cast(bf16x8, bs[t][c]); }, acc2[ch >> 1]);
            }
          }
          const int oy = (ty0 >> 1) + yq, ox = (tx0 >> 1) + xq;
          if (oy < oh2 && ox < ow2) {
            const long ot = ((long)(f * p.kobs + i) * oh2 + oy) * ow2 + ox;
#pragma unroll
            for (int c2 = 0; c2 < NC2; ++c2) {
              const int oc = c2 * 16 + 4 * kk;
              *reinterpret_cast<f32x4*>(P.out2 + ot * P.ldo2 + oc) =
                  bias_act(acc2[c2 >> 1][0][c2 & 1], *reinterpret_cast<const f32x4*>(biasl + 32 + oc), P.act2, P.alpha2);
            }
          }
        }
        if (!(item_end && last_item)) store_b();
        wave_sync();
      }
    }
  }
}

int launch3w_s2(const Tile3S2P& P, int nprod, int max_wg, hipStream_t s) {
  if (S2_LDS > TILE3R_LDS_CU) return NLT_ERR_UNSUPPORTED;
  const int tiles_y = (P.a.oh + 3) / 4;
  const long items = (long)P.a.frames * tiles_y * P.a.tiles_x;
  const long nwg = tile3r_grid(1, max_wg, items);
  if (nwg <= 0) return NLT_ERR_LAUNCH;
  if (items >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  auto* k = nprod == 9 ? conv_tile3w_s2_kernel<9> : conv_tile3w_s2_kernel<6>;
  static size_t done[2][8] = {};
  if (tile3r_allow_lds(reinterpret_cast<const void*>(k), S2_LDS, done[nprod == 9]) != NLT_OK) return NLT_ERR_LAUNCH;
  hipLaunchKernelGGL(k, dim3((unsigned)nwg), dim3(512), S2_LDS, s, P, tiles_y);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

__global__ void pack_tile3s2_kernel(const float* __restrict__ wk, int cin, int cout, long total, u16* __restrict__ wp) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < total) wp[idx] = nlt_tile3s2_fragment(wk, idx, cin, cout);
}

// What every forward entry point checks, in the order its statuses rank (bad argument, unsupported shape, bad layout, too large),
// and the Tile3P of the conv.  The caller's own conditions come evaluated, one per rank: own_args, supported, own_layout;
// ld_other = the row length of the per-observation map it writes, for the 32-bit index bound.
int tile3_params(Tile3P& p, bool own_args, bool supported, bool own_layout, int ld_other, bool stride2,
                 const float* src, int ld, int cin, int frames, int kobs, int h, int w, const u16* packed, const float* bias, int cout,
                 float* out, int ldo, float* mean_out, int ldm, int act, float alpha) {
  if (!own_args || !src || !packed || !bias) return NLT_ERR_BAD_ARG;
  if (frames <= 0 || kobs <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0) return NLT_ERR_BAD_ARG;
  if (!supported) return NLT_ERR_UNSUPPORTED;
  if (!own_layout || ld < cin || (ld & 3) || (out && (ldo < cout || (ldo & 3))) || (mean_out && (ldm < cout || (ldm & 3))))
    return NLT_ERR_BAD_ARG;
  if (!nlt_aligned16(src) || !nlt_aligned16(packed) || !nlt_aligned16(bias) || (out && !nlt_aligned16(out)) ||
      (mean_out && !nlt_aligned16(mean_out))) return NLT_ERR_BAD_ARG;
  if ((long long)frames * kobs * h * w * (long long)(ld > ld_other ? ld : ld_other) >= (1ll << 31)) return NLT_ERR_UNSUPPORTED;
  p.src = src; p.packed = packed; p.bias = bias; p.out = out; p.mean_out = mean_out;
  p.ld = ld; p.cin = cin; p.frames = frames; p.kobs = kobs; p.h = h; p.w = w;
  p.oh = stride2 ? h / 2 : h; p.ow = stride2 ? w / 2 : w;
  p.cout = cout; p.ldo = ldo; p.ldm = ldm; p.ncc = cin / 16; p.act = act; p.alpha = alpha;
  p.tiles_y = (p.oh + TH - 1) / TH; p.tiles_x = (p.ow + TW - 1) / TW;
  return NLT_OK;
}

}  // namespace

extern "C" long nlt_conv_tile3_packed_elems(int mode, int cin, int cout, int tn) {
  if ((mode != NLT_CONV_K2S1 && mode != NLT_CONV_K2S2) || cin <= 0 || cout <= 0) return -1;
  if ((cin & 15) || (tn != 32 && tn != 64) || cout % tn) return -1;
  return (long)12 * cin * cout;                                       // 4 taps x 3 terms
}

extern "C" int nlt_pack_conv_tile3_weights(int mode, const float* w_keras, int cin, int cout, int tn, unsigned short* packed,
                                           void* stream) {
  const long total = nlt_conv_tile3_packed_elems(mode, cin, cout, tn);
  if (total <= 0) return NLT_ERR_UNSUPPORTED;
  if (!w_keras || !packed || !nlt_aligned16(packed)) return NLT_ERR_BAD_ARG;
  hipLaunchKernelGGL(pack_tile3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     w_keras, cin, cout, tn / 16, total, packed);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

static int tile3_forward(int mode, int nprod, const float* src, int ld, int cin, int frames, int kobs, int h, int w,
                         const unsigned short* packed, const float* bias, int cout, int tn,
                         float* out, int ldo, float* mean_out, int ldm, int act, float alpha, int resident_wg, void* stream) {
  const bool own_args = (out || mean_out) && (nprod == 1 || nprod == 3 || nprod == 6 || nprod == 9);
  const bool supported = nlt_conv_tile3_packed_elems(mode, cin, cout, tn) > 0 && !(mode == NLT_CONV_K2S2 && ((h | w) & 1));
  Tile3P p;
  const int st = tile3_params(p, own_args, supported, true, ldo, mode == NLT_CONV_K2S2, src, ld, cin, frames, kobs, h, w, packed, bias,
                              cout, out, ldo, mean_out, ldm, act, alpha);
  if (st != NLT_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode == NLT_CONV_K2S1)
    return tn == 64 ? launch3<NLT_CONV_K2S1, 4>(p, nprod, s, resident_wg) : launch3<NLT_CONV_K2S1, 2>(p, nprod, s, resident_wg);
  return tn == 64 ? launch3<NLT_CONV_K2S2, 4>(p, nprod, s, resident_wg) : launch3<NLT_CONV_K2S2, 2>(p, nprod, s, resident_wg);
}

extern "C" int nlt_conv_tile3_forward(int mode, int nprod, const float* src, int ld, int cin, int frames, int kobs, int h, int w,
                                      const unsigned short* packed, const float* bias, int cout, int tn,
                                      float* out, int ldo, float* mean_out, int ldm, int act, float alpha, void* stream) {
  return tile3_forward(mode, nprod, src, ld, cin, frames, kobs, h, w, packed, bias, cout, tn, out, ldo, mean_out, ldm, act, alpha,
                       -1, stream);
}

extern "C" int nlt_conv_tile3r_forward(int mode, int nprod, const float* src, int ld, int cin, int frames, int kobs, int h, int w,
                                       const unsigned short* packed, const float* bias, int cout, int tn,
                                       float* out, int ldo, float* mean_out, int ldm, int act, float alpha, int max_workgroups,
                                       void* stream) {
  if (max_workgroups < 0) return NLT_ERR_BAD_ARG;
  return tile3_forward(mode, nprod, src, ld, cin, frames, kobs, h, w, packed, bias, cout, tn, out, ldo, mean_out, ldm, act, alpha,
                       max_workgroups, stream);
}

extern "C" int nlt_conv_tile3d_forward(int mode, int nprod, const float* src, int ld, int cin, int frames, int kobs, int h, int w,
                                       const unsigned short* packed, const float* bias, int cout, int tn,
                                       float* out, int ldo, float* mean_out, int ldm, int act, float alpha, void* stream) {
  // (stride 2 on an even map only: that is what makes a lane's operand 32 contiguous bytes; the stride-2 launches have no mean)
  const bool supported = mode == NLT_CONV_K2S2 && nlt_conv_tile3_packed_elems(mode, cin, cout, tn) > 0 && !((h | w) & 1) &&
                         (nprod == 6 || nprod == 9) && !mean_out;
  Tile3P p;
  const int st = tile3_params(p, out != nullptr, supported, true, ldo, true, src, ld, cin, frames, kobs, h, w, packed, bias, cout,
                              out, ldo, mean_out, ldm, act, alpha);
  if (st != NLT_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return tn == 64 ? launch3d<4>(p, nprod, s) : launch3d<2>(p, nprod, s);
}

extern "C" long nlt_conv_tile3w_s2_packed_elems(int cin2, int cout2) {
  return (cin2 == 32 && cout2 == 64) ? (long)12 * cin2 * cout2 : -1;   // 4 taps x 3 terms
}

extern "C" int nlt_pack_conv_tile3w_s2_weights(const float* w_keras, int cin2, int cout2, unsigned short* packed, void* stream) {
  const long total = nlt_conv_tile3w_s2_packed_elems(cin2, cout2);
  if (total <= 0) return NLT_ERR_UNSUPPORTED;
  if (!w_keras || !packed || !nlt_aligned16(packed)) return NLT_ERR_BAD_ARG;
  hipLaunchKernelGGL(pack_tile3s2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     w_keras, cin2, cout2, total, packed);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

// LDS bytes of a workgroup (both weight sets + 8 wave regions), or -1 where the kernel does not exist
extern "C" long nlt_conv_tile3w_s2_lds_bytes(int cin, int cout, int cout2) {
  return (cin == 32 && cout == 32 && cout2 == 64 && S2_LDS <= TILE3R_LDS_CU) ? (long)S2_LDS : -1;
}

extern "C" int nlt_conv_tile3w_s2_forward(int nprod, const float* src, int ld, int cin, int frames, int kobs, int h, int w,
                                          const unsigned short* packed, const float* bias, int cout, float* out, int ldo,
                                          float* mean_out, int ldm, int act, float alpha,
                                          const unsigned short* packed2, const float* bias2, int cout2, float* out2, int ldo2,
                                          int act2, float alpha2, int max_workgroups, void* stream) {
  const bool own_args = packed2 && bias2 && out2 && max_workgroups >= 0 && cout2 > 0;
  // (the stride-1 map is not stored: a caller that wants `out` is refused)
  const bool supported = nlt_conv_tile3w_s2_lds_bytes(cin, cout, cout2) > 0 && (nprod == 6 || nprod == 9) && !((h | w) & 1) && !out;
  const bool own_layout = ldo2 >= cout2 && !(ldo2 & 3) && nlt_aligned16(packed2) && nlt_aligned16(bias2) && nlt_aligned16(out2);
  Tile3S2P P;
  const int st = tile3_params(P.a, own_args, supported, own_layout, ldo2, false, src, ld, cin, frames, kobs, h, w, packed, bias, cout,
                              out, ldo, mean_out, ldm, act, alpha);
  if (st != NLT_OK) return st;
  P.packed2 = packed2; P.bias2 = bias2; P.out2 = out2; P.ldo2 = ldo2; P.act2 = act2; P.alpha2 = alpha2;
  return launch3w_s2(P, nprod, max_workgroups, static_cast<hipStream_t>(stream));
}
