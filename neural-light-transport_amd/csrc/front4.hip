// Third-generation fused front kernel (inference): layers 0-1 of both paths, both observation means and level 2's
// stride-2 convs from the raw texel buffers (nlt/models/nlt.py:95-96,141-180) -- the arithmetic, weight blobs and
// results of front_kernel<true> (fused.hip), bit for bit -- organised so that NO workgroup barrier separates its stages:
//
//   one WAVE works on one 4 x 16 strip of level-1 (half-resolution) texels at a time, i.e. 8 x 32 raw texels plus the
//   halo, i.e. exactly ONE 16-texel MFMA column tile of level 2 (2 x 8).  Everything a strip needs is wave-private:
//   its raw rows (staged in LDS in their natural row layout by 16-byte loads, item by item), its haloed stage-1 tile
//   (5 x 17 -> 6 column tiles), its level-1 tile for the level-2 convs.  Eight such waves live on a CU (17.3 KB of LDS
//   and <= 256 registers each); they run independently, so one wave's staging / LDS traffic / stores run under another
//   wave's MFMAs instead of every workgroup of the chip marching through the same phases in lockstep (what the
//   barrier-separated stages of the first two generations did: their phases added up linearly -- profiles/README.md r02_a).
//
// Per observation (any k): stage 1 (folded L0 + L1 stride-2, 6 independent accumulators) -> stage 2 (L1 stride-1,
// 4 rows = 4 accumulators) -> stage 3 (level 2's stride-2 conv of that observation, 2 accumulators); only the running
// observation mean and the raw mean stay in registers.  The query path runs last.
//
// r04: the waves are PERSISTENT.  With one strip per one-wave workgroup (r02-r04_b) the k = 1 -> 4 sweep read 0.029 ms per
// observation and 0.144 ms for "everything else" -- the query path (1.5 observations' worth of MFMAs) plus, for every one of
// the 16 384 strips, a workgroup launch, the kernel-argument / weight / geometry prologue and an exposed HBM round trip for
// its first observation.  Now one workgroup = the eight waves of a CU, launched once; each wave walks its own sequence of
// strips and
//   * every weight and bias is fetched once per wave (the query path's level-2 fragments once per CU, into LDS) instead of
//     once per strip;
//   * the raw inputs of a strip are a sequence of staged items -- observation 0 .. k - 1, then the query inputs -- that
//     continues into the next strip: while item t is computed, item t + 1 is converted into LDS and item t + 2 is in flight
//     in registers, so no strip starts with a wait.
// The arithmetic of a strip was unchanged by r04's persistence (bit-identical to front_kernel<true> then).  r05: the biases became
// the initial values of the MFMA chains and the uint8 variant feeds raw bytes -- a re-association: <= 3.3e-7 max-abs from
// front_kernel<true>, float / uint8 forms <= 3e-7 rel-L2 apart (tests/test_gpu_front4.py: 5e-7 bars); float = train form bit for bit.
//
// U8 = true reads the resident uint8 capture store (nlt/datasets/nlt.py:131-136,173-181) and feeds the byte values themselves:
// see u8x4_unit.  The strip walk, the staging, the lane positions and the stages are front_strip.h's, shared with front_ovr.hip;
// this file keeps the item sequence, the observation loop with its running means and the TRAIN keeps.
#include "front_strip.h"

namespace {

using L = StripLds<true>;
constexpr int B_Q2 = 0, B_O2 = 16, B_Q1 = 32, B_O1 = 48, B_Q3 = 64, B_O3 = 96;   // inside L::W_BIAS

struct Front4In {
  const void *base, *cvis, *lvis, *nn_rgb, *nn_base;   // float buffers, or the uint8 stores (base = diffuse, nn_rgb = rgb store)
  const int *ids, *nn_ids;                              // U8 only: frame of each sample [n], of each observation [n,k] (-1: zeros)
};

// a - b as two packed operations
__device__ __forceinline__ f32x4 sub4(f32x4 a, f32x4 b) {
  const f32x2 m1 = (f32x2){-1.f, -1.f};                 // fma(b, -1, a) = a - b, one rounding: v_pk_fma_f32
  const f32x2 lo = __builtin_elementwise_fma((f32x2){b[0], b[1]}, m1, (f32x2){a[0], a[1]});
  const f32x2 hi = __builtin_elementwise_fma((f32x2){b[2], b[3]}, m1, (f32x2){a[2], a[3]});
  return (f32x4){lo[0], lo[1], hi[0], hi[1]};
}

// Two waves per SIMD (<= 256 registers).  A leaner variant (weights re-read per observation, query inputs fetched
// late, 10 KB of LDS, 168 registers, three waves per SIMD) measured SLOWER (0.27 vs 0.25 ms at k = 4, uint8): what
// limits the kernel is each wave's own MFMA duty cycle, not the number of waves (profiles/README.md r02_a; r04: fp32
// MFMAs and VALU instructions of a SIMD's waves do not overlap at all -- tools/micro/mfma_valu_overlap.hip).
// TRAIN = true additionally keeps what the backward pass reads (the maps nlt_front_forward_train keeps): the level-1
// stride-2 outputs of both paths (owned texels of the haloed stage-1 tile) and the per-observation level-1 maps.
struct Front4Keep { float *obs1, *qtmp1, *otmp1; };

template <bool U8, bool TRAIN>
__global__ __launch_bounds__(512, 1) void front4_kernel(
    Front4In in, int k, int h, int w, int tiles_y, int tiles_x, int ntiles, const float* __restrict__ blob, int add_base,
    float alpha, float* __restrict__ fm1, float* __restrict__ skip3, const float* __restrict__ blob3,
    float* __restrict__ qtmp2, float* __restrict__ otmp2, Front4Keep keep) {
  __shared__ __attribute__((aligned(16))) float lds_all[L::FLOATS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int kk = lane >> 4, j = lane & 15;
  const int h2 = h >> 1, w2 = w >> 1;
  const long hw = (long)h * w;
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  const f32x2 alpha2 = (f32x2){alpha, alpha};

  // ---- the query path's level-2 and stride-1 fragments and all biases: once per workgroup (128 registers of every wave otherwise)
#pragma unroll
  for (int u = tid; u < 2 * 8 * 64; u += 512)
    *reinterpret_cast<f32x4*>(lds_all + L::W_AQ3 + u * 4) = *reinterpret_cast<const f32x4*>(blob3 + OFF3_AQ + u * 4);
  if (tid < 256) *reinterpret_cast<f32x4*>(lds_all + L::W_AQ1 + tid * 4) = *reinterpret_cast<const f32x4*>(blob + OFF_AQ1 + tid * 4);
  else if (tid < 320) lds_all[L::W_BIAS + tid - 256] = blob[OFF_BQ2 + tid - 256];    // the four level-1 biases are contiguous in the blob
  else if (tid < 384) lds_all[L::W_BIAS + tid - 256] = blob3[OFF3_BQ + tid - 320];   // so are level 2's
  __syncthreads();

  // ---- this wave's strips
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  StripWalk walk(ntiles, tiles_y, tiles_x, wv);
  if (walk.done()) return;
  float* const lds = lds_all + L::W_WAVES + wv * L::W_END;

  // ---- staging geometry of the strip whose items are being LOADED (it runs ahead of the strip being computed)
  using P = Pieces<U8>;
  constexpr int P3 = P::P3, P1 = P::P1;
  unsigned g3[P3], g1[P1];                                               // BYTE offsets inside a frame (Pieces::stage_geom)
  int lf = 0;                                                            // sample (frame of the batch) of that strip
  // (`opaque`: the lane-only parts of these index computations are loop invariants; hoisted out of the strip loop they
  // would occupy ~40 registers of a kernel that has none to spare -- recomputing them per strip is ~100 VALU instructions)
  auto load_geom = [&](int t) {
    const Strip s = walk.decode(t);
    lf = s.f;
    P::stage_geom(s, opaque(lane), h, w, g3, g1);
  };
  // staged item in flight between its global loads and its LDS writes: float inputs = ten 16-byte pieces per lane (an
  // observation: 5 of nn_rgb + 5 of nn_base; the query inputs: 5 of base + 2 of cvis + 2 of lvis), uint8 stores = six 8-byte ones
  using Piece = typename P::Piece;
  Piece st[2 * P3];
  // loads are unconditional: wave-uniform frame pointer + 32-bit lane offset
  auto ld3 = [&](const void* arr, long frame, int at) {
#pragma unroll
    for (int p = 0; p < P3; ++p)
      st[at + p] = *reinterpret_cast<const Piece*>(static_cast<const unsigned char*>(arr) + frame * hw * (3 * P::BPE) + g3[p]);
  };
  auto ld1 = [&](const void* arr, long frame, int at) {
#pragma unroll
    for (int p = 0; p < P1; ++p)
      st[at + p] = *reinterpret_cast<const Piece*>(static_cast<const unsigned char*>(arr) + frame * hw * P::BPE + g1[p]);
  };
  auto load_obs = [&](int i) {                                           // observation i of the strip being loaded
    long fr;
    if constexpr (U8) fr = in.nn_ids[lf * k + i]; else fr = (long)lf * k + i;
    if constexpr (U8) {                                                  // (float batches have every neighbour: the assembler wrote zeros)
      if (fr < 0) {                                                      // a missing neighbour (wave-uniform): zeros
#pragma unroll
        for (int p = 0; p < 2 * P3; ++p) st[p] = make_uint2(0u, 0u);
        return;
      }
    }
    ld3(in.nn_rgb, fr, 0);
    ld3(in.nn_base, fr, P3);
  };
  auto load_query = [&]() {
    long fr;
    if constexpr (U8) fr = in.ids[lf]; else fr = lf;
    ld3(in.base, fr, 0);
    ld1(in.cvis, fr, P3);
    ld1(in.lvis, fr, P3 + P1);
  };
  // registers -> LDS, natural row layout: 16-byte stores at consecutive addresses.  An observation is nn_rgb - nn_base.
  auto store_obs = [&]() {
    float* const dst = lds + L::W_RO;
#pragma unroll
    for (int p = 0; p < P3; ++p) {
      if (P::template no_item<P::N3>(p, lane)) continue;
      const int item = p * 64 + lane;
      if constexpr (U8) {
        *reinterpret_cast<f32x4*>(dst + item * 8) = u8x4_unit(st[p].x) - u8x4_unit(st[P3 + p].x);
        *reinterpret_cast<f32x4*>(dst + item * 8 + 4) = u8x4_unit(st[p].y) - u8x4_unit(st[P3 + p].y);
      } else {
        *reinterpret_cast<f32x4*>(dst + item * 4) = sub4(st[p], st[P3 + p]);
      }
    }
  };
  auto store_query = [&]() {
    int o1[P1];
    const int ln = opaque(lane);
#pragma unroll
    for (int p = 0; p < P1; ++p) o1[p] = P::off1(p, ln);
    P::store_query(lds + L::W_RQ, lds + L::W_RC, lds + L::W_RL, st, lane, o1);
  };

  // ---- weights: held in registers for every strip of the wave
  float ao2[3], aq2[8];
#pragma unroll
  for (int m = 0; m < 3; ++m) ao2[m] = blob[OFF_AO2 + m * 64 + lane];
#pragma unroll
  for (int m = 0; m < 8; ++m) aq2[m] = blob[OFF_AQ2 + m * 64 + lane];
  if constexpr (U8) {                                                    // stage 1 multiplies byte values (see u8x4_unit)
#pragma unroll
    for (int m = 0; m < 3; ++m) ao2[m] *= INV255;
#pragma unroll
    for (int m = 0; m < 8; ++m) aq2[m] *= INV255;
  }
  const float* const bl = lds_all + L::W_BIAS + 4 * kk;                  // biases: read where they are added
  auto bias4 = [&](int off) { return *reinterpret_cast<const f32x4*>(bl + off); };
  f32x4 ao1[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) ao1[t] = *reinterpret_cast<const f32x4*>(blob + OFF_AO1 + (t * 64 + lane) * 4);
  f32x4 ao3[2][4];                                                       // level 2, obs (2,2,16,32): [row tile][channel quad]
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) ao3[rt][c4] = *reinterpret_cast<const f32x4*>(blob3 + OFF3_AO + ((rt * 4 + c4) * 64 + lane) * 4);
  const float s0b = blob[OFF_BSK], s1b = blob[OFF_BSK + 1], s2b = blob[OFF_BSK + 2];
  const float inv_k = 1.f / (float)k;

  int rd3[NC];                                                           // float offset of the lane's raw texel in a 3-channel raw tile
  unsigned live_m, own_m;
  lane_slots(j, kk, rd3, live_m, own_m);
  float* const ot = lds + L::W_OT;
  const L1Tile l1(kk, j);
  const int h4 = h2 >> 1, w4 = w2 >> 1;

  // ---- prologue: item 0 of the first strip into LDS, item 1 in flight
  load_geom(walk.tile);
  load_obs(0);
  store_obs();
  if (k > 1) load_obs(1); else load_query();
  wave_sync();

  for (;;) {
    // ---- geometry of the strip being computed
    const Strip s = walk.decode(walk.tile);
    const int tx0 = s.tx0, ty0 = s.ty0, f = s.f;
    const int next = walk.tile + walk.stride;
    const bool has_next = next < walk.t_hi;
    // a strip whose haloed tile lies inside the image needs no zero-padding masks (wave-uniform)
    const bool interior = ty0 + AH <= h2 && tx0 + AW <= w2;
    unsigned inside_m = live_m, owned_m = own_m;
    if (!interior) border_masks(live_m, opaque(j), s, h2, w2, inside_m, owned_m);
    const int gy2 = (ty0 >> 1) + l1.Y, gx2 = (tx0 >> 1) + l1.X;           // the lane's level-2 texel (stage 3)
    const bool in2 = gy2 < h4 && gx2 < w4;
    const long tex2 = (long)gy2 * w4 + gx2;

    float xs[NC][3];
#pragma unroll
    for (int c = 0; c < NC; ++c) xs[c][0] = xs[c][1] = xs[c][2] = 0.f;
    f32x4 mean[SH] = {zero4, zero4, zero4, zero4};

    for (int i = 0; i < k; ++i) {
      // ---- stage 1: folded L0 + L1 stride-2 conv of observation i, three column tiles at a time
      f32x4 sv[NC];
#pragma unroll
      for (int c0 = 0; c0 < NC; c0 += 3) {
        const f32x4 b2 = bias4(B_O2);
        f32x4 acc[3] = {b2, b2, b2};
        float d[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float* sp = lds + L::W_RO + rd3[c0 + c];
          d[c][0] = sp[0]; d[c][1] = sp[1]; d[c][2] = sp[2];
        }
        stage1_chain(ao2, d, acc);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          xs[c0 + c][0] += d[c][0]; xs[c0 + c][1] += d[c][1]; xs[c0 + c][2] += d[c][2];
          sv[c0 + c] = lrelu4m(acc[c], alpha2);
        }
      }
      if (!interior) {                                                     // beyond the image: the stride-1 conv's zero padding.
        asm volatile("" ::: "memory");                                     // A BRANCH (wave-uniform, border strips only), not 24 selects in every strip
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (!((inside_m >> c) & 1)) sv[c] = zero4;
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) *reinterpret_cast<f32x4*>(ot + (kk * SLOTS + c * 16 + j) * 4) = sv[c];
      if constexpr (TRAIN) {
        const int jt = opaque(j);
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if ((owned_m >> c) & 1) {
            const int t = c * 16 + jt;
            float* o = keep.otmp1 + ((((long)f * k + i) * h2 + ty0 + t / AW) * w2 + tx0 + t % AW) * 16 + 4 * kk;
            *reinterpret_cast<f32x4*>(o) = sv[c];
          }
      }
      wave_sync();                                                         // every lane has its raw values: the raw tile is free
      // item i + 1 (requested an iteration ago) is converted and stored NEXT TO stage 2's MFMAs (same scheduling region,
      // no fence between them), item i + 2 is requested: the next observation, the query inputs, or the next strip's first
      if (i + 1 < k) store_obs(); else store_query();
      if (i + 2 < k) load_obs(i + 2);
      else if (i + 2 == k) load_query();
      else if (has_next) { load_geom(next); load_obs(0); }
      // ---- stage 2
      f32x4 o1[SH];
      stage2(ot, kk, j, [&](int t) { return ao1[t]; }, bias4(B_O1), alpha2, o1);
#pragma unroll
      for (int r = 0; r < SH; ++r) mean[r] += o1[r];
      if constexpr (TRAIN) {
#pragma unroll
        for (int r = 0; r < SH; ++r)
          if (ty0 + r < h2 && tx0 + j < w2)
            *reinterpret_cast<f32x4*>(keep.obs1 + ((((long)f * k + i) * h2 + ty0 + r) * w2 + tx0 + j) * 16 + 4 * kk) = o1[r];
      }
      wave_sync();                                                         // stage-2 reads of `ot` are done: it becomes the level-1 tile
      // ---- stage 3: level 2's stride-2 conv of this observation's level-1 strip
#pragma unroll
      for (int r = 0; r < SH; ++r) *reinterpret_cast<f32x4*>(ot + l1.wr(r)) = o1[r];
      wave_sync();
      {
        f32x4 a3[2] = {bias4(B_O3), bias4(B_O3 + 16)};                     // the biases: initial values of the two chains
        level2_chain(ot, l1.rd, [&](int rt, int c4) { return ao3[rt][c4]; }, a3);
        if (in2) level2_store(otmp2 + (((long)f * k + i) * h4 * w4 + tex2) * 32 + 4 * kk, a3, alpha2);
      }
      wave_sync();                                                         // the level-1 tile is consumed: `ot` is free again
    }

    // ---- query path
    {
      float wsk[24];                                                       // wave-uniform: scalar loads
#pragma unroll
      for (int rr = 0; rr < 24; ++rr) wsk[rr] = blob[(U8 ? OFF_WSK8 : OFF_WSK) + rr];
      const int jq = opaque(j);
      // stage 1 (8 MFMAs per column tile): raw = (base r g b, cvis, lvis, mean raw observation r g b)
#pragma unroll
      for (int c0 = 0; c0 < NC; c0 += 3) {                                 // three column tiles at a time, as for the observations
        const f32x4 b2 = bias4(B_Q2);
        f32x4 acc[3] = {b2, b2, b2};
        float raw[3][8];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float* sp = lds + L::W_RQ + rd3[c0 + c];
          raw[c][0] = sp[0]; raw[c][1] = sp[1]; raw[c][2] = sp[2];
          const int o1c = Slot((c0 + c) * 16 + jq, (live_m >> (c0 + c)) & 1).raw1(kk);
          raw[c][3] = lds[L::W_RC + o1c]; raw[c][4] = lds[L::W_RL + o1c];
          raw[c][5] = xs[c0 + c][0] * inv_k; raw[c][6] = xs[c0 + c][1] * inv_k; raw[c][7] = xs[c0 + c][2] * inv_k;
        }
        stage1_chain(aq2, raw, acc);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          f32x4 v = lrelu4m(acc[c], alpha2);
          if (!interior) {
            asm volatile("" ::: "memory");
            if (!((inside_m >> (c0 + c)) & 1)) v = zero4;
          }
          *reinterpret_cast<f32x4*>(ot + (kk * SLOTS + (c0 + c) * 16 + j) * 4) = v;
          if constexpr (TRAIN) {
            if ((owned_m >> (c0 + c)) & 1) {
              const int t = (c0 + c) * 16 + jq;
              *reinterpret_cast<f32x4*>(keep.qtmp1 + (((long)f * h2 + ty0 + t / AW) * w2 + tx0 + t % AW) * 16 + 4 * kk) = v;
            }
          }
          if ((owned_m >> (c0 + c)) & 1) {                                 // the head's share of the L0 features (+ base)
            float s0 = s0b, s1 = s1b, s2 = s2b;
            skip_sums<8, U8>(raw[c], wsk, add_base, s0, s1, s2);
            const int t = (c0 + c) * 16 + jq;
            // (staging these rows through LDS for 16-byte stores was built and measured in r03: no change -- the stores are not
            // what the query path waits for)
            float* sk = skip3 + ((long)f * hw + (long)(2 * (ty0 + t / AW) + (kk >> 1)) * w + 2 * (tx0 + t % AW) + (kk & 1)) * 3;
            sk[0] = s0; sk[1] = s1; sk[2] = s2;
          }
        }
      }
      wave_sync();                                                         // the raw observation tile has long been free
      if (has_next) {                                                      // next strip: its observation 0 to LDS, its item 1 requested
        store_obs();
        if (k > 1) load_obs(1); else load_query();
      }
      f32x4 qv[SH];
      {
        f32x4 aq1[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) aq1[t] = *reinterpret_cast<const f32x4*>(lds_all + L::W_AQ1 + (t * 64 + lane) * 4);
        stage2(ot, kk, j, [&](int t) { return aq1[t]; }, bias4(B_Q1), alpha2, qv);
      }
#pragma unroll
      for (int r = 0; r < SH; ++r) mean[r] *= inv_k;
      {
        const long hw2 = (long)h2 * w2;
        const int gx = tx0 + j;
#pragma unroll
        for (int r = 0; r < SH; ++r)
          if (ty0 + r < h2 && gx < w2) {
            float* o = fm1 + ((long)f * hw2 + (long)(ty0 + r) * w2 + gx) * 32 + 4 * kk;
            *reinterpret_cast<f32x4*>(o) = qv[r];
            *reinterpret_cast<f32x4*>(o + 16) = mean[r];
          }
      }
      wave_sync();
      // stage 3, query (2,2,32,32): slab 0 = q1 (c8 0..3), slab 1 = mean o1 (c8 4..7), accumulated in this order; fragments
      // from the workgroup's LDS copy
      f32x4 a3[2] = {bias4(B_Q3), bias4(B_Q3 + 16)};
#pragma unroll
      for (int slab = 0; slab < 2; ++slab) {
#pragma unroll
        for (int r = 0; r < SH; ++r) *reinterpret_cast<f32x4*>(ot + l1.wr(r)) = slab ? mean[r] : qv[r];
        wave_sync();
        level2_chain(ot, l1.rd, [&](int rt, int c4) {
          return *reinterpret_cast<const f32x4*>(lds_all + L::W_AQ3 + ((rt * 8 + slab * 4 + c4) * 64 + lane) * 4);
        }, a3);
        wave_sync();
      }
      if (in2) level2_store(qtmp2 + ((long)f * h4 * w4 + tex2) * 32 + 4 * kk, a3, alpha2);
    }
    if (!has_next) break;
    walk.tile = next;
  }
}

template <bool U8, bool TRAIN = false>
int front4_launch(const Front4In& in, int n, int k, int h, int w, const float* packed, const float* packed_l2, int add_base,
                  float alpha, float* fm1, float* skip3, float* qtmp2, float* otmp2, int wps, void* stream,
                  Front4Keep keep = Front4Keep{nullptr, nullptr, nullptr}) {
  StripGrid g;
  const int rc = front_strip_check(
      front_all_set(in.base, in.cvis, in.lvis, in.nn_rgb, in.nn_base, packed, packed_l2, fm1, skip3, qtmp2, otmp2) &&
          (!U8 || (in.ids && in.nn_ids)),
      n > 0 && k > 0 && h > 0 && w > 0, U8, n, h, w, alpha, front_all_aligned16(packed, packed_l2, fm1, qtmp2, otmp2),
      front_all_aligned16(in.base, in.cvis, in.lvis, in.nn_rgb, in.nn_base), (long long)n * k * h * w * 3 < (1ll << 31), g);
  if (rc != NLT_OK) return rc;
  (void)wps;                                                           // one register allocation (2 waves per SIMD); kept in the ABI
  if (TRAIN && !(front_all_set(keep.obs1, keep.qtmp1, keep.otmp1) && front_all_aligned16(keep.obs1, keep.qtmp1, keep.otmp1)))
    return NLT_ERR_BAD_ARG;
  hipLaunchKernelGGL((front4_kernel<U8, TRAIN>), dim3(g.blocks), dim3(64 * NWAVES), 0, static_cast<hipStream_t>(stream),
                     in, k, h, w, g.ty, g.tx, g.tiles, packed, add_base, alpha, fm1, skip3, packed_l2, qtmp2, otmp2, keep);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

}  // namespace

extern "C" int nlt_front4_forward(const float* base, const float* cvis, const float* lvis, const float* nn_rgb,
                                  const float* nn_base, int n, int k, int h, int w, const float* packed,
                                  const float* packed_l2, int add_base, float alpha, float* fm1, float* skip3,
                                  float* qtmp2, float* otmp2, int waves_per_simd, void* stream) {
  Front4In in = {base, cvis, lvis, nn_rgb, nn_base, nullptr, nullptr};
  return front4_launch<false>(in, n, k, h, w, packed, packed_l2, add_base, alpha, fm1, skip3, qtmp2, otmp2, waves_per_simd, stream);
}

extern "C" int nlt_front4_forward_u8(const unsigned char* diffuse_store, const unsigned char* rgb_store,
                                     const unsigned char* cvis_store, const unsigned char* lvis_store,
                                     const int* ids, const int* nn_ids, int n, int k, int h, int w,
                                     const float* packed, const float* packed_l2, int add_base, float alpha,
                                     float* fm1, float* skip3, float* qtmp2, float* otmp2, int waves_per_simd,
                                     void* stream) {
  Front4In in = {diffuse_store, cvis_store, lvis_store, rgb_store, diffuse_store, ids, nn_ids};
  return front4_launch<true>(in, n, k, h, w, packed, packed_l2, add_base, alpha, fm1, skip3, qtmp2, otmp2, waves_per_simd, stream);
}

extern "C" int nlt_front4_forward_train(const float* base, const float* cvis, const float* lvis, const float* nn_rgb,
                                        const float* nn_base, int n, int k, int h, int w, const float* packed,
                                        const float* packed_l2, int add_base, float alpha, float* fm1, float* skip3,
                                        float* qtmp2, float* otmp2, float* obs1, float* qtmp1, float* otmp1, void* stream) {
  Front4In in = {base, cvis, lvis, nn_rgb, nn_base, nullptr, nullptr};
  return front4_launch<false, true>(in, n, k, h, w, packed, packed_l2, add_base, alpha, fm1, skip3, qtmp2, otmp2, 0, stream,
                                    Front4Keep{obs1, qtmp1, otmp1});
}
