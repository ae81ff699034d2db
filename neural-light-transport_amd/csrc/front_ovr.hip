// Fused front kernel of the reference's INFERENCE mode (nlt/nlt_test.py:78-94 -> Model.call(obs_override=feat_agg),
// nlt/models/nlt.py:154-155,172-173): the observation path is not run; every level's aggregated observation feature
// map is GIVEN, one [1,h,w,C] map shared by all frames of the batch (and by all batches of a video).
//
// What the given maps contribute to a conv's pre-activation is linear and frame-independent:
//   conv(concat(q, ovr)) = Wq * q + (Wo * ovr + b)
// so the plan evaluates the bracket ONCE per feat_agg ("override maps", engine.RenderPlan._prepare_override) and the
// per-frame pass reads it where a bias would be added.  This kernel is the query half of front4_kernel (front4.hip) with
// no observation items: layers 0-1 of the query path (L0 folded into L1's stride-2 conv) and level 2's stride-2 conv from
// the raw texel buffers,
//   stage 1  y1 = lrelu(Wfold * raw5 + P1[texel])            P1 [h/2,w/2,16] = W_L1s2[o rows] * ovr0 + folded bias
//   stage 2  q1 = lrelu(W_L1s1 * y1 + b)                     -> fm1[..., 0:16]  (the [16:32) half is the given ovr1)
//   stage 3  qtmp2 = lrelu(W_L2s2[q rows] * q1 + P2[texel])  P2 [h/4,w/4,32] = W_L2s2[o rows] * ovr1 + bias
//   skip3 = Wskip * raw5 + S0[texel] (+ base)                S0 [h,w,4]     = W_head[o rows] * ovr0 + folded bias
// with the maps as the INITIAL VALUES of the MFMA accumulator chains (no add).  The organisation is front4's, and its pieces are
// the same text (front_strip.h): persistent 8-wave workgroups, a wave owns a 4 x 16 strip of level-1 texels, raw rows staged
// through wave-private LDS by 16-byte row-contiguous loads, no workgroup barrier after the prologue.  This file keeps what
// front4 does not do: the split into interior and border strips, the map loads, the lane-constant geometry of interior
// strips and the software pipeline across them (the next strip's raw rows and map values in flight in registers under the
// current strip's MFMAs).
#include "front_strip.h"

namespace {

using L = StripLds<false>;

struct OvrMaps { const float *p1, *s0, *p2; };

// U8 = true reads the resident uint8 capture store (nlt/datasets/nlt.py:131-136,173-181: diffuse / cvis / lvis stores, frame id per
// sample) and stages the raw BYTE values, like front4_kernel<true> (see u8x4_unit).
template <int NW, bool U8>
__global__ __launch_bounds__(64 * NW, 1) void front_ovr_kernel(
    const void* __restrict__ base, const void* __restrict__ cvis, const void* __restrict__ lvis, const int* __restrict__ ids, int h, int w,
    int tiles_y, int tiles_x, int ntiles, const float* __restrict__ blob, const float* __restrict__ blob3, OvrMaps maps,
    int add_base, float alpha, float* __restrict__ q1, int ldq, float* __restrict__ skip3, float* __restrict__ qtmp2) {
  static_assert(NW == NWAVES, "the strip walk and the LDS plan are laid out for the eight waves of a CU");
  __shared__ __attribute__((aligned(16))) float lds_all[L::FLOATS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int kk = lane >> 4, j = lane & 15;
  const int h2 = h >> 1, w2 = w >> 1;
  const long hw = (long)h * w;
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  const f32x2 alpha2 = (f32x2){alpha, alpha};

  // ---- level 2's query-row fragments (slab 0 of OFF3_AQ), the stride-1 fragments and bias: once per workgroup
  for (int u = tid; u < 2 * 4 * 64; u += 64 * NW) {
    const int rt = u >> 8, r = u & 255;                                  // r = c4 * 64 + lane
    *reinterpret_cast<f32x4*>(lds_all + L::W_AQ3 + u * 4) = *reinterpret_cast<const f32x4*>(blob3 + OFF3_AQ + ((rt * 8) * 64 + r) * 4);
  }
  for (int u = tid; u < 256; u += 64 * NW)
    *reinterpret_cast<f32x4*>(lds_all + L::W_AQ1 + u * 4) = *reinterpret_cast<const f32x4*>(blob + OFF_AQ1 + u * 4);
  if (tid < 16) lds_all[L::W_BIAS + tid] = blob[OFF_BQ1 + tid];
  __syncthreads();

  // ---- this wave's strips
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const StripWalk walk(ntiles, tiles_y, tiles_x, wv);
  if (walk.done()) return;
  float* const lds = lds_all + L::W_WAVES + wv * L::W_END;

  // ---- staging of the raw rows.  This kernel has registers to spare (front4 has none): everything that depends on the lane
  // only is computed ONCE -- byte offsets of the lane's pieces inside a strip, LDS offsets, map offsets -- and a strip whose
  // haloed tile lies inside the image (all but the last row / column of strips) adds wave-uniform bases to them; border strips
  // re-derive with clamps (Pieces::stage_geom).
  using P = Pieces<U8>;
  using Piece = typename P::Piece;
  constexpr int P3 = P::P3, P1 = P::P1;
  unsigned g3[P3], g1[P1];                                               // byte offsets inside a frame, strip being loaded
  unsigned c3[P3], c1[P1];                                               // their lane-constant parts (interior strips)
  int l1o[P1];                                                           // LDS offset of the lane's 1-channel pieces
#pragma unroll
  for (int p = 0; p < P3; ++p) {
    const int item = p * 64 + lane;
    const int r = item / P::N3, i = item - r * P::N3;
    c3[p] = item < XH * P::N3 ? (unsigned)((r * w) * 3 + P::E3 * i) * P::BPE : 0u;
  }
#pragma unroll
  for (int p = 0; p < P1; ++p) {
    const int item = p * 64 + lane;
    const int r = item / P::N1, i = item - r * P::N1;
    c1[p] = item < XH * P::N1 ? (unsigned)(r * w + P::E1 * i) * P::BPE : 0u;
    l1o[p] = P::off1(p, lane);
  }
  int lf = 0;                                                            // sample (frame of the batch) of the strip being loaded
  Piece st[P3 + 2 * P1];     // the staged item: 16-byte (float) / 8-byte (uint8) pieces
  auto load_query = [&]() {
    long fr = lf;
    if constexpr (U8) fr = ids[lf];
    const unsigned char* pb = static_cast<const unsigned char*>(base) + fr * hw * (3 * P::BPE);
    const unsigned char* pc = static_cast<const unsigned char*>(cvis) + fr * hw * P::BPE;
    const unsigned char* pl = static_cast<const unsigned char*>(lvis) + fr * hw * P::BPE;
#pragma unroll
    for (int p = 0; p < P3; ++p) st[p] = *reinterpret_cast<const Piece*>(pb + g3[p]);
#pragma unroll
    for (int p = 0; p < P1; ++p) {
      st[P3 + p] = *reinterpret_cast<const Piece*>(pc + g1[p]);
      st[P3 + P1 + p] = *reinterpret_cast<const Piece*>(pl + g1[p]);
    }
  };
  auto store_query = [&]() { P::store_query(lds + L::W_RQ, lds + L::W_RC, lds + L::W_RL, st, lane, l1o); };

  // ---- weights held in registers: the folded stage-1 rows of the five query channels (the three observation rows of
  // the blob are zero: it was packed with a zero observation L0)
  float aq2[5];
#pragma unroll
  for (int m = 0; m < 5; ++m) aq2[m] = blob[OFF_AQ2 + m * 64 + lane] * (U8 ? INV255 : 1.0f);

  int rd3[NC], rd1[NC];                                                  // LDS offsets of the lane's raw texel (3- / 1-channel tiles)
  unsigned mo1[NC], tex0[NC];                                            // interior strips: P1 offset (floats), raw texel index, minus the strip's base
  unsigned live_m, own_m;
  lane_slots(j, kk, rd3, live_m, own_m);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const bool live = (live_m >> c) & 1;
    const Slot s(c * 16 + j, live);
    rd1[c] = s.raw1(kk);
    mo1[c] = live ? (unsigned)((s.hy * w2 + s.hx) * 16 + 4 * kk) : 0u;   // (dead slots read the strip's first texel: no select per strip)
    tex0[c] = (own_m >> c) & 1 ? (unsigned)((2 * s.hy + (kk >> 1)) * w + 2 * s.hx + (kk & 1)) : 0u;
  }
  float* const ot = lds + L::W_OT;
  const L1Tile l1(kk, j);
  const int h4 = h2 >> 1, w4 = w2 >> 1;

  // ---- the override maps of a strip: P1 at the lane's six haloed level-1 texels, S0 at its six raw texels, P2 at its
  // level-2 texel.  Texels beyond the image read the map's first texel: their results are masked / never stored.
  f32x4 mp1[NC], ms0[NC], mp2[2];
  const unsigned mo2 = (unsigned)((l1.Y * w4 + l1.X) * 32 + 4 * kk);
  auto maps_fast = [&](int t) {                                          // interior strips: wave-uniform bases + lane constants
    const Strip s = walk.decode(t);
    const float* b1 = maps.p1 + (size_t)(s.ty0 * w2 + s.tx0) * 16;
    const float* b0 = maps.s0 + (size_t)(2 * s.ty0 * w + 2 * s.tx0) * 4;
    const float* b2 = maps.p2 + (size_t)((s.ty0 >> 1) * w4 + (s.tx0 >> 1)) * 32;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      mp1[c] = *reinterpret_cast<const f32x4*>(b1 + mo1[c]);
      ms0[c] = *reinterpret_cast<const f32x4*>(b0 + tex0[c] * 4u);
    }
    mp2[0] = *reinterpret_cast<const f32x4*>(b2 + mo2);
    mp2[1] = *reinterpret_cast<const f32x4*>(b2 + mo2 + 16);
  };
  auto maps_slow = [&](Strip s) {
    const int jo = opaque(j);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const bool live = (live_m >> c) & 1;
      const Slot q(c * 16 + jo, live);
      const int y1 = s.ty0 + q.hy, x1 = s.tx0 + q.hx;
      const bool in1 = live && y1 < h2 && x1 < w2;
      const unsigned o1 = in1 ? (unsigned)((y1 * w2 + x1) * 16 + 4 * kk) : 0u;
      mp1[c] = *reinterpret_cast<const f32x4*>(maps.p1 + o1);
      const bool own = in1 && q.hy < SH && q.hx < SW;
      const unsigned o0 = own ? (unsigned)(((2 * y1 + (kk >> 1)) * w + 2 * x1 + (kk & 1)) * 4) : 0u;
      ms0[c] = *reinterpret_cast<const f32x4*>(maps.s0 + o0);
    }
    const int gy2 = (s.ty0 >> 1) + l1.Y, gx2 = (s.tx0 >> 1) + l1.X;
    const unsigned o2 = (gy2 < h4 && gx2 < w4) ? (unsigned)((gy2 * w4 + gx2) * 32 + 4 * kk) : 0u;
    mp2[0] = *reinterpret_cast<const f32x4*>(maps.p2 + o2);
    mp2[1] = *reinterpret_cast<const f32x4*>(maps.p2 + o2 + 16);
  };

  float wsk[15];                                                         // wave-uniform: scalar loads
#pragma unroll
  for (int rr = 0; rr < 15; ++rr) wsk[rr] = blob[(U8 ? OFF_WSK8 : OFF_WSK) + rr];

  // ---- one strip: stage 1 -> [`between`: the staging of later strips] -> stage 2 -> stage 3.  FAST = the strip's haloed tile
  // lies inside the image: no masks, and NO CONDITION AROUND A GLOBAL STORE OR LOAD (see the loop below for why that matters).
  auto strip = [&](auto fast_tag, Strip s, auto&& between) {
    constexpr bool FAST = decltype(fast_tag)::value;
    const int tx0 = s.tx0, ty0 = s.ty0, f = s.f;
    unsigned inside_m = live_m, owned_m = own_m;
    if constexpr (!FAST) border_masks(live_m, opaque(j), s, h2, w2, inside_m, owned_m);
    const int gy2 = (ty0 >> 1) + l1.Y, gx2 = (tx0 >> 1) + l1.X;
    const bool in2 = FAST || (gy2 < h4 && gx2 < w4);
    const long tex2 = (long)gy2 * w4 + gx2;
    const f32x4 p2a = mp2[0], p2b = mp2[1];                              // (mp2 is refilled for a later strip in `between`)

    // stage 1 (5 MFMAs per column tile) + the head's share of the L0 features
    float* const skbase = skip3 + ((long)f * hw + (long)(2 * ty0) * w + 2 * tx0) * 3;   // (owned texels are inside the image)
#pragma unroll
    for (int c0 = 0; c0 < NC; c0 += 3) {
      f32x4 acc[3] = {mp1[c0], mp1[c0 + 1], mp1[c0 + 2]};
      float raw[3][5];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* sp = lds + L::W_RQ + rd3[c0 + c];
        raw[c][0] = sp[0]; raw[c][1] = sp[1]; raw[c][2] = sp[2];
        raw[c][3] = lds[L::W_RC + rd1[c0 + c]]; raw[c][4] = lds[L::W_RL + rd1[c0 + c]];
      }
      stage1_chain(aq2, raw, acc);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        f32x4 v = lrelu4m(acc[c], alpha2);
        if constexpr (!FAST) {
          if (!((inside_m >> (c0 + c)) & 1)) v = zero4;
        }
        *reinterpret_cast<f32x4*>(ot + (kk * SLOTS + (c0 + c) * 16 + j) * 4) = v;
        // every lane forms its three sums (a lane that owns no texel wastes nothing: SIMD); only the 12-byte store is predicated
        float s0 = ms0[c0 + c][0], s1 = ms0[c0 + c][1], s2 = ms0[c0 + c][2];
        skip_sums<5, U8>(raw[c], wsk, add_base, s0, s1, s2);
        if ((owned_m >> (c0 + c)) & 1) {
          unsigned at;
          if constexpr (FAST) at = tex0[c0 + c];
          else {
            const int tt = (c0 + c) * 16 + opaque(j);
            at = (unsigned)((2 * (tt / AW) + (kk >> 1)) * w + 2 * (tt % AW) + (kk & 1));
          }
          float* sk = skbase + at * 3u;
          sk[0] = s0; sk[1] = s1; sk[2] = s2;
        }
      }
    }
    wave_sync();                                                         // every lane has its raw values: the raw tile is free
    between();
    f32x4 qv[SH];
    stage2(ot, kk, j, [&](int tp) { return *reinterpret_cast<const f32x4*>(lds_all + L::W_AQ1 + (tp * 64 + lane) * 4); },
           *reinterpret_cast<const f32x4*>(lds_all + L::W_BIAS + 4 * kk), alpha2, qv);
    {
      const long hw2 = (long)h2 * w2;
      const int gx = tx0 + j;
#pragma unroll
      for (int r = 0; r < SH; ++r)
        if (FAST || (ty0 + r < h2 && gx < w2))
          *reinterpret_cast<f32x4*>(q1 + ((long)f * hw2 + (long)(ty0 + r) * w2 + gx) * ldq + 4 * kk) = qv[r];
    }
    wave_sync();                                                         // stage-2 reads of `ot` are done: it becomes the level-1 tile
    // stage 3: level 2's stride-2 conv, query rows only
#pragma unroll
    for (int r = 0; r < SH; ++r) *reinterpret_cast<f32x4*>(ot + l1.wr(r)) = qv[r];
    wave_sync();
    {
      f32x4 a3[2] = {p2a, p2b};
      level2_chain(ot, l1.rd, [&](int rt, int c4) {
        return *reinterpret_cast<const f32x4*>(lds_all + L::W_AQ3 + ((rt * 4 + c4) * 64 + lane) * 4);
      }, a3);
      if (in2) level2_store(qtmp2 + ((long)f * h4 * w4 + tex2) * 32 + 4 * kk, a3, alpha2);
    }
    wave_sync();                                                         // the level-1 tile is consumed: `ot` is free again
  };

  // ---- INTERIOR strips (all but the last row / column of strips): a software pipeline across strips -- while strip s is
  // computed, strip s + 1's raw rows go registers -> LDS and its maps are requested, strip s + 2's raw rows are requested.
  //
  // r06 (PMC + ISA of the first version): the pipeline existed but the compiler's wait-count insertion defeated it -- at the top
  // of every strip and before the LDS staging it emitted `s_waitcnt vmcnt(0)`, draining EVERY outstanding memory operation, the
  // stores issued a moment earlier included (matrix pipe 0.37 busy, waves waiting 0.34 of their cycles).  Two causes, both
  // structural: (1) a global store / load behind a condition (`if (has_next)`, per-lane store predicates inside larger blocks)
  // makes the pass merge paths with different operation counts, and it keeps the smaller count; (2) the loop header merges the
  // back edge with the PROLOGUE's state, where nothing has been issued behind the first loads, so their allowed-outstanding
  // count is 0 for every iteration.  Hence: every memory operation of this loop body is unconditional (prefetches past the last
  // strip are clamped to a valid strip and simply unused; border strips run in the second loop), and the first iteration is
  // PEELED so that both predecessors of the loop header have issued the same sequence.
  // (the haloed tile lies inside the image.  Spelled here, not as a function of front_strip.h that front4 could share: through one,
  // forced inline or not, this loop comes out with other wait counts and twice the SGPR spills -- profiles/README.md r11_a)
  auto is_interior = [&](int t) { const Strip s = walk.decode(t); return s.ty0 + AH <= h2 && s.tx0 + AW <= w2; };
  auto next_interior = [&](int t) {
    do { t += walk.stride; } while (t < walk.t_hi && !is_interior(t));
    return t;
  };
  auto geom_fast = [&](int t) {
    const Strip s = walk.decode(t);
    lf = s.f;
    const unsigned b3 = (unsigned)((2 * s.ty0 * w + 2 * s.tx0) * 3) * P::BPE, b1 = (unsigned)(2 * s.ty0 * w + 2 * s.tx0) * P::BPE;
#pragma unroll
    for (int p = 0; p < P3; ++p) g3[p] = b3 + c3[p];                     // (lanes without a piece: c3 = 0, the strip's first bytes)
#pragma unroll
    for (int p = 0; p < P1; ++p) g1[p] = b1 + c1[p];
  };
  int cur = is_interior(walk.tile) ? walk.tile : next_interior(walk.tile);
  if (cur < walk.t_hi) {
    geom_fast(cur);
    load_query();
    maps_fast(cur);
    store_query();
    int nx = next_interior(cur);
    geom_fast(nx < walk.t_hi ? nx : cur);
    load_query();
    wave_sync();
    auto iteration = [&](int c_, int n_) {
      strip(std::true_type{}, walk.decode(c_), [&]() {
        store_query();                                                   // raw rows of the next strip: registers -> LDS
        const int pf = n_ < walk.t_hi ? n_ : c_;
        maps_fast(pf);                                                   // its maps
        const int n2 = next_interior(pf);
        geom_fast(n2 < walk.t_hi ? n2 : pf);                             // the raw rows of the strip after it
        load_query();
      });
    };
    iteration(cur, nx);                                                  // peeled (see above)
    while (nx < walk.t_hi) {
      cur = nx;
      nx = next_interior(cur);
      iteration(cur, nx);
    }
  }
  // ---- border strips (halo beyond the image): one at a time, masks and clamps, no pipelining across strips
  for (int t = walk.tile; t < walk.t_hi; t += walk.stride) {
    if (is_interior(t)) continue;
    const Strip s = walk.decode(t);
    lf = s.f;
    P::stage_geom(s, opaque(lane), h, w, g3, g1);
    load_query();
    maps_slow(s);
    store_query();
    wave_sync();
    strip(std::false_type{}, s, []() {});
  }
}

}  // namespace

static int front_ovr_launch(bool u8, const void* base, const void* cvis, const void* lvis, const int* ids, int n, int h, int w,
                            const float* packed, const float* packed_l2, const float* p1, const float* s0, const float* p2,
                            int add_base, float alpha, float* q1, int ldq, float* skip3, float* qtmp2, void* stream) {
  StripGrid g;
  const int rc = front_strip_check(
      front_all_set(base, cvis, lvis, packed, packed_l2, p1, s0, p2, q1, skip3, qtmp2) && (!u8 || ids),
      n > 0 && h > 0 && w > 0 && ldq >= 16 && !(ldq & 3), u8, n, h, w, alpha, front_all_aligned16(packed, packed_l2, q1, qtmp2, p1, s0, p2),
      front_all_aligned16(base, cvis, lvis), (long long)n * h * w * 3 < (1ll << 31) && (long long)h * w * 16 < (1ll << 31), g);
  if (rc != NLT_OK) return rc;
  OvrMaps maps = {p1, s0, p2};
  const dim3 grid(g.blocks), block(64 * NWAVES);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (u8)
    hipLaunchKernelGGL((front_ovr_kernel<NWAVES, true>), grid, block, 0, s, base, cvis, lvis, ids, h, w, g.ty, g.tx, g.tiles, packed, packed_l2,
                       maps, add_base, alpha, q1, ldq, skip3, qtmp2);
  else
    hipLaunchKernelGGL((front_ovr_kernel<NWAVES, false>), grid, block, 0, s, base, cvis, lvis, ids, h, w, g.ty, g.tx, g.tiles, packed, packed_l2,
                       maps, add_base, alpha, q1, ldq, skip3, qtmp2);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_front_ovr_forward(const float* base, const float* cvis, const float* lvis, int n, int h, int w,
                                     const float* packed, const float* packed_l2, const float* p1, const float* s0,
                                     const float* p2, int add_base, float alpha, float* q1, int ldq, float* skip3,
                                     float* qtmp2, void* stream) {
  return front_ovr_launch(false, base, cvis, lvis, nullptr, n, h, w, packed, packed_l2, p1, s0, p2, add_base, alpha, q1, ldq, skip3,
                          qtmp2, stream);
}

extern "C" int nlt_front_ovr_forward_u8(const unsigned char* diffuse_store, const unsigned char* cvis_store,
                                        const unsigned char* lvis_store, const int* ids, int n, int h, int w,
                                        const float* packed, const float* packed_l2, const float* p1, const float* s0,
                                        const float* p2, int add_base, float alpha, float* q1, int ldq, float* skip3,
                                        float* qtmp2, void* stream) {
  return front_ovr_launch(true, diffuse_store, cvis_store, lvis_store, ids, n, h, w, packed, packed_l2, p1, s0, p2, add_base, alpha, q1,
                          ldq, skip3, qtmp2, stream);
}
