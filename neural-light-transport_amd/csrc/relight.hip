// Relighting a view under an environment map from its one-light-at-a-time (OLAT) renders: per-light weights of a lat-long
// probe, the weighted sum of the per-light predictions, and the exposure / encode at the end.
//   replaces: nothing -- the reference has no call site for this step.  It is the HDRI relighting of the paper (Zhang et al.,
//             "Neural Light Transport for Relighting and View Synthesis", the environment-map results): the view's OLAT renders
//             combined linearly with the probe's per-light solid-angle integrals.
// Lat-long convention (ours, z-up as in the Blender scenes): pixel (i, j) of an [He, We] probe looks along
//   d = (sin t cos p, sin t sin p, cos t),  t = pi (i + 1/2) / He,  p = 2 pi (j + 1/2) / We - pi,
// and covers the solid angle dO = sin t * (pi / He) * (2 pi / We).  Rotation r turns d into rot[r] . d before the nearest light
// (largest dot product, ties to the lowest index) is looked up.
// Sums: no float atomics.  Weights: a workgroup owns one probe row of one rotation; every light's row sum is taken by ONE thread
// in pixel order (float64), and the rows are added in row order by a second launch (float64, rounded once to float32).  The
// accumulation is a per-element fmaf chain in light order that starts from the stored value, so cutting the lights into chunks
// changes nothing.  Equal inputs give equal bits.
#include "nlt_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLights = 1024;                // dirs in LDS, <= kLightSlots lights per thread
constexpr int kLightSlots = kMaxLights / kThreads;
constexpr int kPix = 1024;                      // pixels of a row staged at a time
constexpr long kWsBudgetFloats = 16l << 20;     // row partials of at most this many floats (64 MiB) per launch pair
constexpr double kPi = 3.14159265358979323846;

// ---------------------------------------------------------------- probe -> per-light weights
// Grid (He, rotations of this launch).  partial [rotation][row][l][3] float64 = dO(row) * sum of the row's pixels whose nearest
// light is l.
__global__ __launch_bounds__(kThreads) void envmap_rows_kernel(const float* __restrict__ envmap, const float* __restrict__ dirs,
                                                                const float* __restrict__ rot, int he, int we, int L,
                                                                double* __restrict__ partial) {
  __shared__ float s_dirs[kMaxLights * 3];
  __shared__ float s_e[kPix * 3];
  __shared__ int s_idx[kPix];
  const int tid = threadIdx.x, row = blockIdx.x, r = blockIdx.y;
  for (int i = tid; i < L * 3; i += kThreads) s_dirs[i] = dirs[i];
  const float* m = rot + (long)r * 9;
  const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
  const double theta = kPi * ((double)row + 0.5) / (double)he;
  const double st = sin(theta), ct = cos(theta);
  const double domega = st * (kPi / (double)he) * (2.0 * kPi / (double)we);
  const float* erow = envmap + (long)row * we * 3;

  double acc[kLightSlots][3];
#pragma unroll
  for (int g = 0; g < kLightSlots; ++g) acc[g][0] = acc[g][1] = acc[g][2] = 0.0;

  for (int p0 = 0; p0 < we; p0 += kPix) {
    const int np = min(kPix, we - p0);
    __syncthreads();                                  // s_dirs written (first pass); s_e / s_idx free again (later passes)
    for (int i = tid; i < np * 3; i += kThreads) s_e[i] = erow[(long)p0 * 3 + i];
    for (int p = tid; p < np; p += kThreads) {
      const double phi = 2.0 * kPi * ((double)(p0 + p) + 0.5) / (double)we - kPi;
      const double dx = st * cos(phi), dy = st * sin(phi), dz = ct;
      const float x = (float)(m00 * dx + m01 * dy + m02 * dz);
      const float y = (float)(m10 * dx + m11 * dy + m12 * dz);
      const float z = (float)(m20 * dx + m21 * dy + m22 * dz);
      float best = fmaf(x, s_dirs[0], fmaf(y, s_dirs[1], z * s_dirs[2]));
      int arg = 0;
      for (int l = 1; l < L; ++l) {
        const float d = fmaf(x, s_dirs[3 * l], fmaf(y, s_dirs[3 * l + 1], z * s_dirs[3 * l + 2]));
        if (d > best) { best = d; arg = l; }          // strict: a tie keeps the lower index
      }
      s_idx[p] = arg;
    }
    __syncthreads();
    for (int p = 0; p < np; ++p) {
      const int l = s_idx[p];
      if ((l & (kThreads - 1)) == tid) {               // the one thread that owns light l
        const double e0 = s_e[3 * p], e1 = s_e[3 * p + 1], e2 = s_e[3 * p + 2];
        const int g = l / kThreads;
#pragma unroll
        for (int gg = 0; gg < kLightSlots; ++gg)
          if (gg == g) { acc[gg][0] += e0; acc[gg][1] += e1; acc[gg][2] += e2; }
      }
    }
  }
  double* out = partial + ((long)r * he + row) * (long)L * 3;
#pragma unroll
  for (int g = 0; g < kLightSlots; ++g) {
    const int l = g * kThreads + tid;
    if (l < L) {
      out[3 * l] = acc[g][0] * domega;
      out[3 * l + 1] = acc[g][1] * domega;
      out[3 * l + 2] = acc[g][2] * domega;
    }
  }
}

// out[r][i] = float32(sum over rows, in row order, of partial[r][row][i]), i over L * 3
__global__ __launch_bounds__(kThreads) void envmap_reduce_kernel(const double* __restrict__ partial, int he, int L3,
                                                                  float* __restrict__ out) {
  const int i = blockIdx.x * kThreads + threadIdx.x, r = blockIdx.y;
  if (i >= L3) return;
  const double* p = partial + (long)r * he * L3 + i;
  double s = 0.0;
  for (int row = 0; row < he; ++row) s += p[(long)row * L3];
  out[(long)r * L3 + i] = (float)s;
}

long rows_floats(int he, int L) { return 2l * he * L * 3; }       // one rotation's float64 row partials, in floats

// rotations per launch pair: as many as the budget holds, at least one
int rot_tile(int he, int L, int R) {
  const long per = rows_floats(he, L);
  long t = kWsBudgetFloats / per;
  if (t < 1) t = 1;
  if (t > R) t = R;
  if (t > 65535) t = 65535;
  return (int)t;
}

int weights_shape_status(int he, int we, int L, int R) {
  if (he <= 0 || we <= 0 || L <= 0 || R <= 0) return NLT_ERR_BAD_ARG;
  if (L > kMaxLights) return NLT_ERR_UNSUPPORTED;
  if ((long)he * we * 3 >= (1l << 31) || (long)R * L * 3 >= (1l << 31) || rows_floats(he, L) >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  return NLT_OK;
}

// ---------------------------------------------------------------- sum of weighted OLAT renders
constexpr int kRTile = 8;                       // rotations per thread (registers): a prediction value is read once per tile
constexpr int kGroup = 4;                       // texels per thread: 12 floats = three 16-byte accesses, channel = element % 3

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__device__ __forceinline__ float srgb_decode(float v) {
  return v < 0.04045f ? v / 12.92f : powf((v + 0.055f) / 1.055f, 2.4f);
}

__device__ __forceinline__ float srgb_encode(float v) {
  return v > 0.0031308f ? 1.055f * powf(v, 1.f / 2.4f) - 0.055f : v * 12.92f;
}

// 12 consecutive floats at p.  VEC: p is 16-byte aligned and all 12 exist.  Else element i is touched only if i < n.
template <bool VEC>
__device__ __forceinline__ void load12(const float* __restrict__ p, int n, float (&v)[12]) {
  if (VEC) {
    const f32x4* q = reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const f32x4 t = q[k];
      v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i] = i < n ? p[i] : 0.f;
  }
}

template <bool VEC>
__device__ __forceinline__ void store12(float* __restrict__ p, int n, const float (&v)[12]) {
  if (VEC) {
    f32x4* q = reinterpret_cast<f32x4*>(p);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      f32x4 t;
      t.x = v[4 * k]; t.y = v[4 * k + 1]; t.z = v[4 * k + 2]; t.w = v[4 * k + 3];
      q[k] = t;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (i < n) p[i] = v[i];
  }
}

// Grid (groups of kGroup texels / kThreads, rotation tiles).  pred [lc][t3], weights [R][L][3], acc [R][t3]; t3 = texels * 3.
// VEC: texels % 4 == 0 and both arrays 16-byte aligned, so every row of pred and acc starts aligned too.
template <bool VEC, bool LINEAR>
__global__ __launch_bounds__(kThreads) void relight_accumulate_kernel(const float* __restrict__ pred,
                                                                       const float* __restrict__ weights, int lc, int l0, int L,
                                                                       int R, long t3, long groups, float* __restrict__ acc) {
  const long g = (long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= groups) return;
  const long e0 = g * (kGroup * 3);
  const int n = (int)min((long)(kGroup * 3), t3 - e0);          // floats of this group that exist (VEC: always 12)
  const int r0 = blockIdx.y * kRTile;

  float a[kRTile][12];
#pragma unroll
  for (int rr = 0; rr < kRTile; ++rr)
    if (r0 + rr < R) load12<VEC>(acc + (long)(r0 + rr) * t3 + e0, n, a[rr]);

  for (int l = 0; l < lc; ++l) {
    float v[12];
    load12<VEC>(pred + (long)l * t3 + e0, n, v);
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      v[i] = clip01(v[i]);
      if (!LINEAR) v[i] = srgb_decode(v[i]);
    }
#pragma unroll
    for (int rr = 0; rr < kRTile; ++rr) {
      if (r0 + rr < R) {                                          // (uniform over the workgroup)
        const float* w = weights + ((long)(r0 + rr) * L + (l0 + l)) * 3;
        const float w0 = w[0], w1 = w[1], w2 = w[2];
#pragma unroll
        for (int t = 0; t < kGroup; ++t) {
          a[rr][3 * t] = fmaf(w0, v[3 * t], a[rr][3 * t]);
          a[rr][3 * t + 1] = fmaf(w1, v[3 * t + 1], a[rr][3 * t + 1]);
          a[rr][3 * t + 2] = fmaf(w2, v[3 * t + 2], a[rr][3 * t + 2]);
        }
      }
    }
  }
#pragma unroll
  for (int rr = 0; rr < kRTile; ++rr)
    if (r0 + rr < R) store12<VEC>(acc + (long)(r0 + rr) * t3 + e0, n, a[rr]);
}

// out = enc(clip01(exposure * acc)) over n floats; VEC: both 16-byte aligned, four per thread, the last n % 4 one by one
template <bool SRGB>
__device__ __forceinline__ float finish_one(float v, float exposure) {
  v = clip01(exposure * v);
  return SRGB ? srgb_encode(v) : v;
}

template <bool VEC, bool SRGB>
__global__ __launch_bounds__(kThreads) void relight_finish_kernel(const float* __restrict__ acc, float exposure, long n,
                                                                   float* __restrict__ out) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (VEC) {
    const long n4 = n >> 2;
    if (i < n4) {
      const f32x4 t = reinterpret_cast<const f32x4*>(acc)[i];
      f32x4 o;
      o.x = finish_one<SRGB>(t.x, exposure); o.y = finish_one<SRGB>(t.y, exposure);
      o.z = finish_one<SRGB>(t.z, exposure); o.w = finish_one<SRGB>(t.w, exposure);
      reinterpret_cast<f32x4*>(out)[i] = o;
    } else if (i - n4 < (n & 3)) {
      const long e = (n4 << 2) + (i - n4);
      out[e] = finish_one<SRGB>(acc[e], exposure);
    }
  } else if (i < n) {
    out[i] = finish_one<SRGB>(acc[i], exposure);
  }
}

}  // namespace

extern "C" long nlt_envmap_light_weights_workspace_floats(int he, int we, int n_lights, int n_rot) {
  if (weights_shape_status(he, we, n_lights, n_rot) != NLT_OK) return -1;
  return rows_floats(he, n_lights) * rot_tile(he, n_lights, n_rot);
}

extern "C" int nlt_envmap_light_weights(const float* envmap, int he, int we, const float* dirs, int n_lights, const float* rot,
                                        int n_rot, float* workspace, long workspace_floats, float* out, void* stream) {
  if (!envmap || !dirs || !rot || !workspace || !out) return NLT_ERR_BAD_ARG;
  const int st = weights_shape_status(he, we, n_lights, n_rot);
  if (st != NLT_OK) return st;
  const int rt = rot_tile(he, n_lights, n_rot);
  if (workspace_floats < rows_floats(he, n_lights) * rt) return NLT_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 7u) return NLT_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* partial = reinterpret_cast<double*>(workspace);
  const int L3 = n_lights * 3;
  for (int r0 = 0; r0 < n_rot; r0 += rt) {                      // (one stream: the next pair waits for this pair's reduce)
    const int nr = n_rot - r0 < rt ? n_rot - r0 : rt;
    hipLaunchKernelGGL(envmap_rows_kernel, dim3(he, nr), dim3(kThreads), 0, s, envmap, dirs, rot + (long)r0 * 9, he, we, n_lights,
                       partial);
    hipLaunchKernelGGL(envmap_reduce_kernel, dim3((L3 + kThreads - 1) / kThreads, nr), dim3(kThreads), 0, s, partial, he, L3,
                       out + (long)r0 * L3);
  }
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_relight_accumulate(const float* pred, int n_chunk, long texels, const float* weights, int n_rot, int n_lights,
                                      int l0, int is_linear, float* acc, void* stream) {
  if (!pred || !weights || !acc) return NLT_ERR_BAD_ARG;
  if (n_chunk <= 0 || texels <= 0 || n_rot <= 0 || n_lights <= 0 || l0 < 0 || (long)l0 + n_chunk > n_lights) return NLT_ERR_BAD_ARG;
  if (texels >= (1l << 31) / 3) return NLT_ERR_UNSUPPORTED;
  const long t3 = texels * 3;
  if (t3 * n_chunk >= (1l << 31) || t3 * n_rot >= (1l << 31) || (long)n_rot * n_lights * 3 >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  const long groups = (texels + kGroup - 1) / kGroup;
  const dim3 grid((unsigned)((groups + kThreads - 1) / kThreads), (n_rot + kRTile - 1) / kRTile), block(kThreads);
  if (grid.y > 65535) return NLT_ERR_UNSUPPORTED;
  const bool vec = texels % kGroup == 0 && nlt_aligned16(pred) && nlt_aligned16(acc);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define NLT_RELIGHT_ACC(V, LIN)                                                                                                \
  hipLaunchKernelGGL((relight_accumulate_kernel<V, LIN>), grid, block, 0, s, pred, weights, n_chunk, l0, n_lights, n_rot, t3, \
                     groups, acc)
  if (vec) { if (is_linear) NLT_RELIGHT_ACC(true, true); else NLT_RELIGHT_ACC(true, false); }
  else { if (is_linear) NLT_RELIGHT_ACC(false, true); else NLT_RELIGHT_ACC(false, false); }
#undef NLT_RELIGHT_ACC
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_relight_finish(const float* acc, int n_rot, long texels, float exposure, int to_srgb, float* out, void* stream) {
  if (!acc || !out || n_rot <= 0 || texels <= 0) return NLT_ERR_BAD_ARG;
  if (texels >= (1l << 31) / 3 || texels * 3 * n_rot >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  const long n = texels * 3 * n_rot;
  const bool vec = nlt_aligned16(acc) && nlt_aligned16(out);
  const long threads = vec ? (n >> 2) + (n & 3) : n;
  const dim3 grid((unsigned)((threads + kThreads - 1) / kThreads)), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec) {
    if (to_srgb) hipLaunchKernelGGL((relight_finish_kernel<true, true>), grid, block, 0, s, acc, exposure, n, out);
    else hipLaunchKernelGGL((relight_finish_kernel<true, false>), grid, block, 0, s, acc, exposure, n, out);
  } else {
    if (to_srgb) hipLaunchKernelGGL((relight_finish_kernel<false, true>), grid, block, 0, s, acc, exposure, n, out);
    else hipLaunchKernelGGL((relight_finish_kernel<false, false>), grid, block, 0, s, acc, exposure, n, out);
  }
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}
