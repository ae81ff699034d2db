// The pieces the wave-per-strip front kernels share (front4.hip: both paths from observations; front_ovr.hip: the query half over
// given override maps).  Both are  persistent 8-wave workgroups -> a wave walks its run of strips -> per strip: raw rows staged
// through wave-private LDS -> stage 1 (folded L0 + L1 stride-2) -> stage 2 (L1 stride-1) -> stage 3 (level 2's stride-2 conv).
// Each piece is written once here; a kernel keeps what only it does (its item sequence, its loads, its loop) and every choice
// that decides its registers: whether lane-only index arithmetic is hoisted (front_ovr) or recomputed per strip behind opaque()
// (front4, which has no register to spare) is the CALLER's -- the pieces take the lane index as an argument.
//
// NO inline-asm VALU in these kernels: the hazard recognizer pads MFMA -> VALU read / write distances with s_nop only for
// instructions it can see, and a v_max_f32 / v_pk_add_f32 written as asm landed inside an MFMA's write-back window in one
// build of front4's uint8 variant (obs texels wrong by 1e-1; which build depends on register allocation).
#pragma once
#include <type_traits>
#include "front_common.h"

namespace {

// ---- strip geometry -----------------------------------------------------------------------------------------------------------
constexpr int SH = 4, SW = 16;             // level-1 strip of one wave
constexpr int AH = SH + 1, AW = SW + 1;    // haloed: 5 x 17 = 85 texels
constexpr int AT = AH * AW;
constexpr int NC = (AT + 15) / 16;         // 6 column tiles (96 slots)
constexpr int SLOTS = NC * 16;
constexpr int XH = 2 * AH;                 // raw rows: 10
constexpr int R3 = 104;                    // floats per staged 3-channel raw row (34 texels = 102, 26 float4)
constexpr int R1 = 40;                     // floats per staged 1-channel raw row (34 -> 5 x 8)
constexpr int NWAVES = 8;                  // waves of a workgroup = of a CU (two per SIMD)

// LDS plan (floats).  Per wave: the raw tiles and the stage-1 tile; per workgroup: the query path's fragments and biases.
// OBS = the kernel also runs the observation path: a raw observation tile, both slabs of level 2's query fragments, every bias.
template <bool OBS>
struct StripLds {
  static constexpr int W_RO = 0;                                   // raw observation (nn_rgb - nn_base); OBS only
  static constexpr int W_RQ = OBS ? XH * R3 : 0;                   // raw base
  static constexpr int W_RC = W_RQ + XH * R3;                      // raw cvis
  static constexpr int W_RL = W_RC + XH * R1;                      // raw lvis
  static constexpr int W_OT = W_RL + XH * R1;                      // stage-1 tile [4 channel quads][96 slots][4]; then the level-1 tile of stage 3
  static constexpr int W_END = W_OT + 4 * SLOTS * 4;               // 4416 (OBS) / 3376 floats per wave
  static constexpr int C8 = OBS ? 8 : 4;                           // channel quads of level 2's query fragments (slab 0 = q1, 1 = mean o1)
  static constexpr int W_AQ3 = 0;                                  // level-2 fragments [rt 2][c8][lane 64][4]
  static constexpr int W_AQ1 = W_AQ3 + 2 * C8 * 64 * 4;            // stride-1 fragments [tap 4][lane 64][4]
  static constexpr int W_BIAS = W_AQ1 + 4 * 64 * 4;                // OBS: [bq2 | bo2 | bq1 | bo1] (16 each), [bq3 | bo3] (32 each); else bq1
  static constexpr int W_WAVES = W_BIAS + (OBS ? 128 : 16);
  static constexpr int FLOATS = W_WAVES + NWAVES * W_END;          // 162 304 B (OBS) / 120 384 B of the CU's 163 840
};

// ---- small helpers ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_sync() {       // orders this wave's LDS traffic for the compiler; no instruction
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// hides a lane-only value from loop-invariant code motion: what is derived from it is recomputed where it is used (no instruction)
__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+v"(v)); return v; }

// LeakyReLU for 0 <= alpha <= 1 (checked by the launcher): max(v, alpha * v), bit-identical to the select form.  r05: the
// products as <2 x float> multiplies (v_pk_mul_f32) and the maximum as v_med3_f32(v, alpha v, FLT_MAX) (= max for every finite value): 1.5 instead of 2 VALU
// instructions per value (fmaxf() on an MFMA result costs a third: the compiler quiets the operand first).
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x4 lrelu4m(f32x4 v, f32x2 alpha2) {
  const f32x2 plo = (f32x2){v[0], v[1]} * alpha2, phi = (f32x2){v[2], v[3]} * alpha2;
  const float top = 3.4028234663852886e38f;   // FLT_MAX, not +inf: med3 with an infinity is folded back into the quieting max
  return (f32x4){__builtin_amdgcn_fmed3f(v[0], plo[0], top), __builtin_amdgcn_fmed3f(v[1], plo[1], top),
                 __builtin_amdgcn_fmed3f(v[2], phi[0], top), __builtin_amdgcn_fmed3f(v[3], phi[1], top)};
}

// r05 (r04 review item 5): the uint8-store variants stage the raw BYTE values (v_cvt_f32_ubyteN: one instruction, exact) instead of
// `_load_data`'s float32(float64(u) / 255) (u8_unit: four instructions per byte, 192 per observation), and the 1 / 255 moves into
// the operands the raw values meet: the stage-1 A operands (the folded L0 + L1 stride-2 weights) and the head's skip rows are
// multiplied by fl(1 / 255) -- the first in registers, once per wave; the second at pack time (OFF_WSK8) -- and `+ base` becomes
// fma(byte, fl(1 / 255), .).  nn_rgb - nn_base is an exact integer in [-255, 255].  fl(W / 255) . u instead of W . fl(u / 255):
// a uint8 variant is not bit-identical to its float kernel on the assembled batch, it is <= 3e-7 rel-L2 from it
// (tests/test_gpu_front4.py, tests/test_gpu_infer.py).
constexpr float INV255 = 1.0f / 255.0f;
__device__ __forceinline__ f32x4 u8x4_unit(unsigned v) {
  return (f32x4){(float)(v & 255u), (float)((v >> 8) & 255u), (float)((v >> 16) & 255u), (float)(v >> 24)};
}

// ---- strip walk ---------------------------------------------------------------------------------------------------------------
// XCD x = blockIdx & 7 owns a contiguous run of tiles (neighbours share halo lines in its L2); its waves take them round-robin
// (slot = wave * workgroups-per-XCD + workgroup: consecutive slots = consecutive strips; wave-major: a small input still puts a
// wave on every CU).  This wave's strips are tile, tile + stride, ... below t_hi.  (Whether a strip's haloed tile lies inside the
// image -- ty0 + AH <= h2 && tx0 + AW <= w2 -- is spelled in each kernel, not here: front_ovr.hip says why.)
struct Strip {
  int tx0, ty0, f;                          // first level-1 texel of the strip, frame of the batch
};
struct StripWalk {
  int tiles_y, tiles_x, t_hi, stride, tile;
  __device__ __forceinline__ StripWalk(int ntiles, int tiles_y_, int tiles_x_, int wv) : tiles_y(tiles_y_), tiles_x(tiles_x_) {
    const int per_xcd = (ntiles + 7) >> 3;
    const int t_lo = (blockIdx.x & 7) * per_xcd;
    t_hi = min(t_lo + per_xcd, ntiles);
    stride = (gridDim.x >> 3) * NWAVES;
    tile = t_lo + wv * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
  }
  __device__ __forceinline__ bool done() const { return tile >= t_hi; }
  __device__ __forceinline__ Strip decode(int t) const {
    Strip s;
    s.tx0 = (t % tiles_x) * SW; t /= tiles_x;
    s.ty0 = (t % tiles_y) * SH;
    s.f = t / tiles_y;
    return s;
  }
};

// ---- staging ------------------------------------------------------------------------------------------------------------------
// A raw tile (10 rows of 34 texels) travels global -> registers -> LDS in row-contiguous pieces: item = pass * 64 + lane ->
// (raw row, piece of the row).  Float inputs: 16-byte pieces; the uint8 stores: 8-byte pieces that become 8 floats in LDS.
template <bool U8>
struct Pieces {
  static constexpr int N3 = U8 ? 13 : 26, P3 = U8 ? 3 : 5, E3 = U8 ? 8 : 4;   // 3-channel rows: pieces per row, passes, floats per piece
  static constexpr int N1 = U8 ? 5 : 9, P1 = U8 ? 1 : 2, E1 = U8 ? 8 : 4;     // 1-channel rows
  static constexpr unsigned BPE = U8 ? 1u : 4u;                               // bytes per stored element
  using Piece = typename std::conditional<U8, uint2, f32x4>::type;

  // Byte offsets inside a frame of the lane's pieces of strip s (32 bits: the load takes them as the VGPR offset of an SGPR base
  // -- no address VALU), clamped: a piece that lies beyond the image's bottom / right edge (or a lane without a piece) reads the
  // frame's first bytes instead.  So the loads are unconditional, and whatever such a piece delivers only reaches stage-1 texels
  // outside the image, whose outputs are forced to zero (`inside_m`): no select is needed.
  static __device__ __forceinline__ void stage_geom(Strip s, int ln, int h, int w, unsigned (&g3)[P3], unsigned (&g1)[P1]) {
#pragma unroll
    for (int p = 0; p < P3; ++p) {
      const int item = p * 64 + ln;
      const int r = item / N3, i = item - r * N3;
      const int gy = 2 * s.ty0 + r;
      const bool ok = item < XH * N3 && gy < h && 3 * (2 * s.tx0) + E3 * i < 3 * w;
      g3[p] = ok ? (unsigned)((gy * w + 2 * s.tx0) * 3 + E3 * i) * BPE : 0u;
    }
#pragma unroll
    for (int p = 0; p < P1; ++p) {
      const int item = p * 64 + ln;
      const int r = item / N1, i = item - r * N1;
      const int gy = 2 * s.ty0 + r;
      const bool ok = item < XH * N1 && gy < h && 2 * s.tx0 + E1 * i < w;
      g1[p] = ok ? (unsigned)(gy * w + 2 * s.tx0 + E1 * i) * BPE : 0u;
    }
  }
  // only the LAST pass can hold lanes without an item; spelled so that the full passes carry no lane-dependent branch
  // (the compiler does not derive lane < 64 here, and a branch per piece also makes its wait counts conservative)
  template <int N> static __device__ __forceinline__ bool no_item(int p, int ln) { return (p + 1) * 64 > XH * N && p * 64 + ln >= XH * N; }
  // LDS offset of the lane's 1-channel piece of pass p inside a tile of R1-float rows (3-channel tiles: item * E3)
  static __device__ __forceinline__ int off1(int p, int ln) {
    const int item = p * 64 + ln;
    const int r = item / N1, i = item - r * N1;
    return r * R1 + E1 * i;
  }
  // one staged piece -> its floats in LDS (bytes stay byte VALUES)
  static __device__ __forceinline__ void put(float* dst, Piece v) {
    if constexpr (U8) {
      *reinterpret_cast<f32x4*>(dst) = u8x4_unit(v.x);
      *reinterpret_cast<f32x4*>(dst + 4) = u8x4_unit(v.y);
    } else {
      *reinterpret_cast<f32x4*>(dst) = v;
    }
  }
  // the query inputs' three tiles (rq, rc, rl), registers -> LDS: st = [P3 of base | P1 of cvis | P1 of lvis], o1[p] = off1(p, .)
  static __device__ __forceinline__ void store_query(float* rq, float* rc, float* rl, const Piece* st, int lane, const int (&o1)[P1]) {
#pragma unroll
    for (int p = 0; p < P3; ++p) {
      if (no_item<N3>(p, lane)) continue;
      put(rq + (p * 64 + lane) * E3, st[p]);
    }
#pragma unroll
    for (int p = 0; p < P1; ++p) {
      if (no_item<N1>(p, lane)) continue;
      put(rc + o1[p], st[P3 + p]);
      put(rl + o1[p], st[P3 + P1 + p]);
    }
  }
};

// ---- lane positions -----------------------------------------------------------------------------------------------------------
// Stage 1 computes the haloed tile as six column tiles: the lane's slot of column tile c is haloed texel t = c * 16 + j, tap kk
// (a raw texel of its 2 x 2 footprint).  A dead slot (t >= AT) stands for texel 0; a slot with hy < SH && hx < SW is a texel of
// the strip itself ("owned").  (That test is written out where it is used: as a member returning `a && b` it turns front_ovr's
// clamped map loads of border strips into branches -- profiles/README.md r11_a.)
struct Slot {
  int hy, hx;
  __device__ __forceinline__ Slot(int t, bool live) : hy(live ? t / AW : 0), hx(live ? t % AW : 0) {}
  __device__ __forceinline__ int raw3(int kk) const { return (2 * hy + (kk >> 1)) * R3 + (2 * hx + (kk & 1)) * 3; }   // float offset of its raw
  __device__ __forceinline__ int raw1(int kk) const { return (2 * hy + (kk >> 1)) * R1 + 2 * hx + (kk & 1); }         // texel in a staged tile
};
// column tiles whose slot is a texel of the haloed tile / of the strip
__device__ __forceinline__ void lane_slots(int j, int kk, int (&rd3)[NC], unsigned& live_m, unsigned& own_m) {
  live_m = own_m = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int t = c * 16 + j;
    const bool live = t < AT;
    const Slot s(t, live);
    rd3[c] = s.raw3(kk);
    live_m |= (unsigned)live << c;
    own_m |= (unsigned)(live && s.hy < SH && s.hx < SW) << c;
  }
}
// ... of a border strip: and inside the image (beyond it: the stride-1 conv's zero padding, nothing kept or stored)
__device__ __forceinline__ void border_masks(unsigned live_m, int j, Strip s, int h2, int w2, unsigned& inside_m, unsigned& owned_m) {
  inside_m = owned_m = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const bool live = (live_m >> c) & 1;
    const Slot q(c * 16 + j, live);
    const bool inside = live && s.ty0 + q.hy < h2 && s.tx0 + q.hx < w2;
    inside_m |= (unsigned)inside << c;
    owned_m |= (unsigned)(inside && q.hy < SH && q.hx < SW) << c;
  }
}

// level-1 tile in LDS (stage 3's input, in place of the stage-1 tile): [channel quad][x parity][row 4][x / 2 8][4], parity plane 1
// xor-swizzled by 8 slots so that the 16 lanes a ds_read_b128 services (two taps x two rows) touch 16 different 16-byte slots.
// Written by lane = (channel quad kk, column j) row by row; read by lane = (tap kk, level-2 texel j = (Y, X) of the 2 x 8 tile).
struct L1Tile {
  int kk, j, Y, X, rd;
  __device__ __forceinline__ L1Tile(int kk_, int j_) : kk(kk_), j(j_), Y(j_ >> 3), X(j_ & 7) {
    rd = ((kk & 1) * 32 + ((((2 * Y + (kk >> 1)) * 8) + X) ^ ((kk & 1) * 8))) * 4;
  }
  __device__ __forceinline__ int wr(int row) const { return (kk * 64 + (j & 1) * 32 + (((row * 8) + (j >> 1)) ^ ((j & 1) * 8))) * 4; }
};

// ---- stages -------------------------------------------------------------------------------------------------------------------
// stage 1's MFMAs for three column tiles (three independent accumulators keep the matrix pipe issuing; six at once cost 21 more
// registers): ROWS raw channels, A operand a[m] per channel.  acc holds the chains' initial values: a bias, or an override map.
template <int ROWS>
__device__ __forceinline__ void stage1_chain(const float (&a)[ROWS], const float (&raw)[3][ROWS], f32x4 (&acc)[3]) {
#pragma unroll
  for (int m = 0; m < ROWS; ++m)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], raw[c][m], acc[c], 0, 0, 0);
}

// stage 2: L1 stride-1 conv of the haloed tile in `ot` (TF 'same': taps (y + a, x + b)), four rows side by side.  frag(t) = the
// lane's A fragment of tap t.  r05: the bias is the chain's initial value (no add).
template <class Frag>
__device__ __forceinline__ void stage2(const float* ot, int kk, int j, Frag&& frag, f32x4 bias, f32x2 alpha2, f32x4 (&out)[SH]) {
  const float* tilep = ot + kk * SLOTS * 4;
  f32x4 acc[SH] = {bias, bias, bias, bias};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const f32x4 a = frag(t);
    f32x4 b[SH];
#pragma unroll
    for (int r = 0; r < SH; ++r) b[r] = *reinterpret_cast<const f32x4*>(tilep + ((r + (t >> 1)) * AW + j + (t & 1)) * 4);
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
      for (int r = 0; r < SH; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s4], b[r][s4], acc[r], 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < SH; ++r) out[r] = lrelu4m(acc[r], alpha2);
}

// stage 3: level 2's stride-2 conv of the level-1 tile in `ot`, 16 channels (four quads) onto the two row-tile chains a3 (their
// initial values: the bias, an override map, or the chains of an earlier slab).  frag(rt, c4) = the lane's A fragment.
template <class Frag>
__device__ __forceinline__ void level2_chain(const float* ot, int l1_rd, Frag&& frag, f32x4 (&a3)[2]) {
#pragma unroll
  for (int c4 = 0; c4 < 4; ++c4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(ot + c4 * 256 + l1_rd);
    const f32x4 w0 = frag(0, c4), w1 = frag(1, c4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a3[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[e], v[e], a3[0], 0, 0, 0);
      a3[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[e], v[e], a3[1], 0, 0, 0);
    }
  }
}
__device__ __forceinline__ void level2_store(float* o, const f32x4 (&a3)[2], f32x2 alpha2) {      // 32 channels of one level-2 texel
  *reinterpret_cast<f32x4*>(o) = lrelu4m(a3[0], alpha2);
  *reinterpret_cast<f32x4*>(o + 16) = lrelu4m(a3[1], alpha2);
}

// the head's share of the L0 features of one raw texel: s += raw . wsk rows (+ base; uint8: base is a byte value, see u8x4_unit)
template <int ROWS, bool U8>
__device__ __forceinline__ void skip_sums(const float (&raw)[ROWS], const float (&wsk)[ROWS * 3], int add_base, float& s0, float& s1, float& s2) {
#pragma unroll
  for (int rr = 0; rr < ROWS; ++rr) {
    s0 = fmaf(raw[rr], wsk[rr * 3], s0);
    s1 = fmaf(raw[rr], wsk[rr * 3 + 1], s1);
    s2 = fmaf(raw[rr], wsk[rr * 3 + 2], s2);
  }
  if (add_base) {
    if constexpr (U8) { s0 = fmaf(raw[0], INV255, s0); s1 = fmaf(raw[1], INV255, s1); s2 = fmaf(raw[2], INV255, s2); }
    else { s0 += raw[0]; s1 += raw[1]; s2 += raw[2]; }
  }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
template <class... P> bool front_all_set(P... p) { return (... && (p != nullptr)); }
template <class... P> bool front_all_aligned16(P... p) { return (... && nlt_aligned16(p)); }

// The checks both launchers make, in the order that decides the status code, and the launch geometry.  set / sizes_ok: every
// pointer given, every count in range; bufs16: blobs, maps and the outputs stored 16 bytes at a time; in16: the raw inputs (row
// pieces are loaded 16 (8) bytes at a time); fits: every 32-bit offset of the kernel.
struct StripGrid { int ty, tx, tiles; unsigned blocks; };
inline int front_strip_check(bool set, bool sizes_ok, bool u8, int n, int h, int w, float alpha, bool bufs16, bool in16, bool fits, StripGrid& g) {
  if (!set || !sizes_ok) return NLT_ERR_BAD_ARG;
  if ((h | w) & 3) return NLT_ERR_UNSUPPORTED;                         // level 2 halves the half-resolution grid again
  if (u8 && (w & 7)) return NLT_ERR_UNSUPPORTED;                       // 8-byte pieces of a uint8 row
  if (!(alpha >= 0.f && alpha <= 1.f)) return NLT_ERR_UNSUPPORTED;     // LeakyReLU as max(v, alpha v)
  if (!bufs16) return NLT_ERR_BAD_ARG;
  if (!in16 || !fits) return NLT_ERR_UNSUPPORTED;
  g.ty = (h / 2 + SH - 1) / SH; g.tx = (w / 2 + SW - 1) / SW;
  const long tiles = (long)n * g.ty * g.tx;
  if (tiles >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  g.tiles = (int)tiles;
  // one workgroup per CU (always a multiple of 8: one run of tiles per XCD); with fewer than 2048 strips its waves share them out
  long groups = (tiles + 7) / 8;                                       // workgroups per XCD: one per CU, fewer only below 32 strips per XCD
  if (groups > 32) groups = 32;
  g.blocks = (unsigned)(8 * groups);
  return NLT_OK;
}

}  // namespace
