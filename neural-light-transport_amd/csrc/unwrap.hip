// Smart-UV-style mesh unwrapping: the projection groups, islands, island boxes and loop UVs behind the {face: [loop, vert, u, v]}
// table that data_gen/render.py's `calc_bidir_mapping` takes, without Blender.
//   replaces: xm.blender.object.smart_uv_unwrap (third_party/xiuminglib/xiuminglib/blender/object.py:835-893), that is
//             bpy.ops.uv.smart_project inside Blender 2.78c, as data_gen/uv_unwrap.py calls it.  The greedy rule for the
//             projection vectors is restated from Blender's published script; parity with Blender is not claimed.
// Built with -ffp-contract=off (csrc/Makefile): every output is compared bit for bit with NumPy (tests/unwrap_ref.py).
//
// ARITHMETIC: float64, only + - * / sqrt and comparisons, no fused operation.  a . b = (ax*bx + ay*by) + az*bz;
// a x b = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx).  No sine or cosine: the two cosines of the angle limit come from the
// host.  No float atomics; the only atomics are integer min / max, whose result no arrival order changes.  Equal inputs give
// equal bits; every output element is written.
//
// MESH: verts [V][3]; loop_verts [L], the faces' vertex indices end to end; face_off [F + 1] (non-decreasing, face_off[0] = 0,
// face_off[F] = L; the host checks that).  A polygon is the fan (0, i, i + 1).  Per-face vectors are stored by component,
// n [3][F] and unit [3][F], so that a wave reads 64 consecutive doubles.
//
// a. FRAMES (`frames_kernel`, one face per lane): n = the sum over the fan, in order, of (v_i - v_0) x (v_{i+1} - v_0), starting
//    from +0; len = sqrt((nx*nx + ny*ny) + nz*nz); area = 0.5 * len; unit = n / len per component.  A face with fewer than three
//    loops, a vertex index outside 0 .. V-1, or a len that is zero or not finite is DEGENERATE: ok = 0, n as summed (0 when an
//    index is bad), unit = 0, area = 0.
// b. PROJECTION VECTORS, one round per vector:
//    seed (`argext_kernel<true>`): the ok face of largest area, ties to the lowest index; it also sets remaining = ok.
//    gather (`gather_kernel`): a remaining face f with f == seed or unit_f . unit_seed > cos_half leaves `remaining` and
//      contributes unit_f * ((area_f * aw) + omw) per component; every other face, and the padding, contributes +0.0.
//      THE SUM IS A FIXED TREE: faces in index order in blocks of 256; inside a block x[i] += x[i + s] for s = 128, 64 .. 1; the
//      block results are reduced by the same rule (`tree_kernel`), level after level, until one value is left.
//      vec = sum / sqrt(sum . sum) per component (`normalize_kernel`).
//    farthest (`farthest_kernel`): best_f = d (first round) or (d > best_f ? d : best_f) with d = unit_f . vec for every ok face
//      (0 for a degenerate one); then the remaining face of smallest best, ties to the lowest index.
//    The host reads one (index, value) pair per round and stops when no face remains or the value is >= cos_full.
// c. ASSIGNMENT (`assign_kernel`): group_f = the k of largest unit_f . vec_k, ties to the lowest k; -1 for a degenerate face.
// d. ISLANDS: `edge_keys_kernel` (one loop per lane) finds the loop's face by bisection of face_off and writes
//    key = min(a, b) * V + max(a, b) for the edge from this loop's vertex to the next loop's of the same face.  The host sorts
//    the keys (stable).  `hook_kernel`, one sorted position per lane: equal neighbouring keys link their two faces when both
//    groups are the same and >= 0.  label is a parent array with label[f] <= f: the larger of the two roots is hooked under the
//    smaller by an integer atomicMin, then `jump_kernel` points every face at its root.  A round that hooks nothing sets no flag.
//    When no round changes anything, label[f] is the smallest face index of f's component, whatever the schedule was: parents
//    only ever decrease, a root is the smallest index of its tree, and two linked faces have the same root.  -1: degenerate.
// e. ISLAND BOXES (`project_kernel`, one loop per lane): pu = (p . U_k) + 0.0, pv = (p . V_k) + 0.0 (the + 0.0 turns -0.0 into
//    +0.0, so that min / max have one answer), k = the face's group; per island the exact min / max through order-preserving
//    64-bit keys (sign bit flipped for positives, all bits for negatives) and integer atomicMin / atomicMax, in the box buffer
//    itself: `box_init_kernel` before, `box_decode_kernel` after.  Loops of degenerate faces get (0, 0) and touch no box.
// g. UVS (`uv_kernel`, one slot of the dense [F][vmax][2] table per lane): local = (pu - umin, pv - vmin), or for a turned
//    island (pv - vmin, umax - pu); uv = local * scale + offset (a multiply, then an add).  Pads and degenerate faces: (0, 0).
//    (f. the packing is host code: data_gen/unwrap.py.)
// Every store is a plain vector store; there is no dynamically indexed private array.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "nlt_common.h"
#include "../../include/nlt_hip.h"

namespace {

constexpr int kT = 256;
constexpr long kNone = 0x7fffffffffffffffl;

struct V3 { double x, y, z; };
__device__ inline double dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline V3 sub3(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline V3 cross3(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline V3 load3(const double* p, long i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ inline V3 load3s(const double* p, long i, long n) { return {p[i], p[n + i], p[2 * n + i]}; }

inline unsigned nblocks(long n) { return (unsigned)((n + kT - 1) / kT); }

int count_status(long n) {
  if (n <= 0) return NLT_ERR_BAD_ARG;
  if (n >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  return NLT_OK;
}

// ---------------------------------------------------------------------------------------------------- a. frames
__global__ __launch_bounds__(kT) void frames_kernel(const double* __restrict__ verts, int n_verts, const int* __restrict__ loop_verts,
                                                    const int* __restrict__ face_off, int n_faces, double* __restrict__ n_out,
                                                    double* __restrict__ unit, double* __restrict__ area, unsigned char* __restrict__ ok) {
  const long f = (long)blockIdx.x * kT + threadIdx.x;
  if (f >= n_faces) return;
  const int o0 = face_off[f], o1 = face_off[f + 1];
  bool good = o1 - o0 >= 3;
  for (int l = o0; l < o1; ++l) {
    const int v = loop_verts[l];
    good = good && v >= 0 && v < n_verts;
  }
  V3 n = {0.0, 0.0, 0.0};
  if (good) {
    const V3 v0 = load3(verts, loop_verts[o0]);
    V3 a = sub3(load3(verts, loop_verts[o0 + 1]), v0);
    for (int l = o0 + 2; l < o1; ++l) {
      const V3 b = sub3(load3(verts, loop_verts[l]), v0);
      const V3 c = cross3(a, b);
      n = {n.x + c.x, n.y + c.y, n.z + c.z};
      a = b;
    }
  }
  const double len = sqrt((n.x * n.x + n.y * n.y) + n.z * n.z);
  good = good && isfinite(len) && len > 0.0;
  const long F = n_faces;
  n_out[f] = n.x; n_out[F + f] = n.y; n_out[2 * F + f] = n.z;
  unit[f] = good ? n.x / len : 0.0; unit[F + f] = good ? n.y / len : 0.0; unit[2 * F + f] = good ? n.z / len : 0.0;
  area[f] = good ? 0.5 * len : 0.0;
  ok[f] = good ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------- b. the arg-extremum
template <bool kMax>
__device__ inline bool better(double v, long i, double bv, long bi) {
  if (i == kNone) return false;
  if (bi == kNone) return true;
  return (kMax ? v > bv : v < bv) || (v == bv && i < bi);
}

// the block's best candidate lands in (val[0], idx[0]); the rule is associative and commutative, so any pairing gives one answer
template <bool kMax>
__device__ inline void block_best(double v, long i, double* val, long* idx) {
  const int t = threadIdx.x;
  val[t] = v; idx[t] = i;
  __syncthreads();
  for (int s = kT / 2; s >= 1; s >>= 1) {
    if (t < s && better<kMax>(val[t + s], idx[t + s], val[t], idx[t])) { val[t] = val[t + s]; idx[t] = idx[t + s]; }
    __syncthreads();
  }
}

// one block: partial candidates [n] -> pair = (index or -1, the value's bits)
template <bool kMax>
__global__ __launch_bounds__(kT) void argext_final_kernel(const double* __restrict__ pval, const long* __restrict__ pidx, int n,
                                                          long* __restrict__ pair) {
  __shared__ double val[kT];
  __shared__ long idx[kT];
  double bv = 0.0;
  long bi = kNone;
  for (int j = threadIdx.x; j < n; j += kT)
    if (better<kMax>(pval[j], pidx[j], bv, bi)) { bv = pval[j]; bi = pidx[j]; }
  block_best<kMax>(bv, bi, val, idx);
  if (threadIdx.x == 0) {
    pair[0] = idx[0] == kNone ? -1 : idx[0];
    pair[1] = idx[0] == kNone ? 0 : __double_as_longlong(val[0]);
  }
}

__global__ __launch_bounds__(kT) void seed_kernel(const double* __restrict__ area, const unsigned char* __restrict__ ok, int n_faces,
                                                  unsigned char* __restrict__ remaining, double* __restrict__ pval, long* __restrict__ pidx) {
  __shared__ double val[kT];
  __shared__ long idx[kT];
  const long f = (long)blockIdx.x * kT + threadIdx.x;
  double v = 0.0;
  long i = kNone;
  if (f < n_faces) {
    const unsigned char o = ok[f];
    remaining[f] = o;
    if (o) { v = area[f]; i = f; }
  }
  block_best<true>(v, i, val, idx);
  if (threadIdx.x == 0) { pval[blockIdx.x] = val[0]; pidx[blockIdx.x] = idx[0]; }
}

__global__ __launch_bounds__(kT) void farthest_kernel(const double* __restrict__ unit, const unsigned char* __restrict__ ok,
                                                      const unsigned char* __restrict__ remaining, double* __restrict__ best, int n_faces,
                                                      const double* __restrict__ vec, int first, double* __restrict__ pval,
                                                      long* __restrict__ pidx) {
  __shared__ double val[kT];
  __shared__ long idx[kT];
  const long f = (long)blockIdx.x * kT + threadIdx.x;
  double v = 0.0;
  long i = kNone;
  if (f < n_faces) {
    double b = 0.0;
    if (ok[f]) {
      const double d = dot3(load3s(unit, f, n_faces), V3{vec[0], vec[1], vec[2]});
      b = d;
      if (!first) { const double old = best[f]; b = d > old ? d : old; }
    }
    best[f] = b;
    if (remaining[f]) { v = b; i = f; }
  }
  block_best<false>(v, i, val, idx);
  if (threadIdx.x == 0) { pval[blockIdx.x] = val[0]; pidx[blockIdx.x] = idx[0]; }
}

// ---------------------------------------------------------------------------------------------------- b. the tree sum
// x[i] += x[i + s], s = 128 .. 1, on three components at once; the block's sums land in x*[0]
__device__ inline void block_tree(double* x, double* y, double* z) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int s = kT / 2; s >= 1; s >>= 1) {
    if (t < s) { x[t] = x[t] + x[t + s]; y[t] = y[t] + y[t + s]; z[t] = z[t] + z[t + s]; }
    __syncthreads();
  }
}

// out [3][n_blocks] by component
__global__ __launch_bounds__(kT) void gather_kernel(const double* __restrict__ unit, const double* __restrict__ area,
                                                    unsigned char* __restrict__ remaining, int n_faces, int seed, double cos_half,
                                                    double aw, double omw, double* __restrict__ out) {
  __shared__ double x[kT], y[kT], z[kT];
  const long f = (long)blockIdx.x * kT + threadIdx.x;
  V3 c = {0.0, 0.0, 0.0};
  if (f < n_faces && remaining[f]) {
    const V3 u = load3s(unit, f, n_faces);
    if (f == seed || dot3(u, load3s(unit, seed, n_faces)) > cos_half) {
      const double w = (area[f] * aw) + omw;
      c = {u.x * w, u.y * w, u.z * w};
      remaining[f] = 0;
    }
  }
  x[threadIdx.x] = c.x; y[threadIdx.x] = c.y; z[threadIdx.x] = c.z;
  block_tree(x, y, z);
  if (threadIdx.x == 0) {
    const long nb = gridDim.x;
    out[blockIdx.x] = x[0]; out[nb + blockIdx.x] = y[0]; out[2 * nb + blockIdx.x] = z[0];
  }
}

// in [3][n_in] -> out [3][ceil(n_in / 256)]
__global__ __launch_bounds__(kT) void tree_kernel(const double* __restrict__ in, int n_in, double* __restrict__ out) {
  __shared__ double x[kT], y[kT], z[kT];
  const long j = (long)blockIdx.x * kT + threadIdx.x;
  const bool has = j < n_in;
  x[threadIdx.x] = has ? in[j] : 0.0; y[threadIdx.x] = has ? in[(long)n_in + j] : 0.0; z[threadIdx.x] = has ? in[2l * n_in + j] : 0.0;
  block_tree(x, y, z);
  if (threadIdx.x == 0) {
    const long nb = gridDim.x;
    out[blockIdx.x] = x[0]; out[nb + blockIdx.x] = y[0]; out[2 * nb + blockIdx.x] = z[0];
  }
}

__global__ void normalize_kernel(const double* __restrict__ sum, double* __restrict__ vec) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const V3 s = {sum[0], sum[1], sum[2]};
  const double len = sqrt(dot3(s, s));
  vec[0] = s.x / len; vec[1] = s.y / len; vec[2] = s.z / len;
}

// ---------------------------------------------------------------------------------------------------- c. assignment
__global__ __launch_bounds__(kT) void assign_kernel(const double* __restrict__ unit, const unsigned char* __restrict__ ok, int n_faces,
                                                    const double* __restrict__ vectors, int n_vectors, int* __restrict__ group) {
  const long f = (long)blockIdx.x * kT + threadIdx.x;
  if (f >= n_faces) return;
  int g = -1;
  if (ok[f]) {
    const V3 u = load3s(unit, f, n_faces);
    double bd = dot3(u, load3(vectors, 0));
    g = 0;
    for (int k = 1; k < n_vectors; ++k) {
      const double d = dot3(u, load3(vectors, k));
      if (d > bd) { bd = d; g = k; }
    }
  }
  group[f] = g;
}

// ---------------------------------------------------------------------------------------------------- d. islands
__global__ __launch_bounds__(kT) void edge_keys_kernel(const int* __restrict__ loop_verts, int n_loops, const int* __restrict__ face_off,
                                                       int n_faces, long n_verts, long* __restrict__ keys, int* __restrict__ loop_face) {
  const long l = (long)blockIdx.x * kT + threadIdx.x;
  if (l >= n_loops) return;
  int lo = 0, hi = n_faces - 1;                         // the first face whose end is past l (face_off[n_faces] = n_loops > l)
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (face_off[mid + 1] <= l) lo = mid + 1; else hi = mid;
  }
  const int next = l + 1 < face_off[lo + 1] ? (int)l + 1 : face_off[lo];
  const long a = loop_verts[l], b = loop_verts[next];
  keys[l] = (a < b ? a : b) * n_verts + (a < b ? b : a);
  loop_face[l] = lo;
}

__global__ __launch_bounds__(kT) void label_init_kernel(const int* __restrict__ group, int n_faces, int* __restrict__ label) {
  const long f = (long)blockIdx.x * kT + threadIdx.x;
  if (f < n_faces) label[f] = group[f] >= 0 ? (int)f : -1;
}

__device__ inline int peek(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// label[] holds roots on entry (label_init_kernel or jump_kernel wrote it), so label[label[f]] == label[f] for what is read here
__global__ __launch_bounds__(kT) void hook_kernel(const long* __restrict__ keys, const long* __restrict__ order,
                                                  const int* __restrict__ loop_face, int n_loops, const int* __restrict__ group,
                                                  int* __restrict__ label, int* __restrict__ changed) {
  const long i = (long)blockIdx.x * kT + threadIdx.x + 1;
  if (i >= n_loops || keys[i] != keys[i - 1]) return;
  const int fa = loop_face[order[i - 1]], fb = loop_face[order[i]];
  const int g = group[fa];
  if (g < 0 || g != group[fb]) return;
  const int ra = peek(label + fa), rb = peek(label + fb);
  if (ra == rb) return;
  atomicMin(label + (ra > rb ? ra : rb), ra > rb ? rb : ra);
  *changed = 1;                                         // (every writer stores the same word)
}

// parents only decrease and nothing hooks while this runs: the walk ends at a root, whatever the other lanes have stored so far
__global__ __launch_bounds__(kT) void jump_kernel(int n_faces, int* __restrict__ label) {
  const long f = (long)blockIdx.x * kT + threadIdx.x;
  if (f >= n_faces) return;
  int p = peek(label + f);
  if (p < 0) return;
  for (int pp = peek(label + p); pp != p; pp = peek(label + p)) p = pp;
  __hip_atomic_store(label + f, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------- e. island boxes
__device__ inline unsigned long long order_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ inline double order_value(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? k & 0x7fffffffffffffffull : ~k));
}

// boxes [I][4] = (umin, vmin, umax, vmax), here still as keys: the mins start at the largest key, the maxes at the smallest
__global__ __launch_bounds__(kT) void box_init_kernel(unsigned long long* __restrict__ boxes, long n) {
  const long i = (long)blockIdx.x * kT + threadIdx.x;
  if (i < n) boxes[i] = (i & 2) ? 0ull : ~0ull;
}

__global__ __launch_bounds__(kT) void project_kernel(const double* __restrict__ verts, const int* __restrict__ loop_verts,
                                                     const int* __restrict__ loop_face, int n_loops, const int* __restrict__ group,
                                                     const int* __restrict__ island, const double* __restrict__ frames,
                                                     int n_vectors, int n_islands, double2* __restrict__ puv,
                                                     unsigned long long* __restrict__ boxes) {
  const long l = (long)blockIdx.x * kT + threadIdx.x;
  if (l >= n_loops) return;
  const int f = loop_face[l];
  const int isl = island[f], g = group[f];
  double pu = 0.0, pv = 0.0;
  if (isl >= 0 && isl < n_islands && g >= 0 && g < n_vectors) {      // (a face of an island is ok: its vertex indices are in range)
    const V3 p = load3(verts, loop_verts[l]);
    pu = dot3(p, load3(frames, 2l * g)) + 0.0;
    pv = dot3(p, load3(frames, 2l * g + 1)) + 0.0;
    unsigned long long* b = boxes + 4l * isl;
    const unsigned long long ku = order_key(pu), kv = order_key(pv);
    atomicMin(b, ku); atomicMin(b + 1, kv); atomicMax(b + 2, ku); atomicMax(b + 3, kv);
  }
  puv[l] = make_double2(pu, pv);
}

__global__ __launch_bounds__(kT) void box_decode_kernel(unsigned long long* __restrict__ boxes, long n) {
  const long i = (long)blockIdx.x * kT + threadIdx.x;
  if (i < n) reinterpret_cast<double*>(boxes)[i] = order_value(boxes[i]);
}

// ---------------------------------------------------------------------------------------------------- g. UVs
__global__ __launch_bounds__(kT) void uv_kernel(const double2* __restrict__ puv, const int* __restrict__ face_off,
                                                const int* __restrict__ island, long n_slots, int vmax, const double* __restrict__ boxes,
                                                const unsigned char* __restrict__ rot, const double2* __restrict__ offsets,
                                                int n_islands, double scale, double2* __restrict__ uv) {
  const long i = (long)blockIdx.x * kT + threadIdx.x;
  if (i >= n_slots) return;
  const long f = i / vmax;
  const int j = (int)(i - f * vmax);
  const int o0 = face_off[f], cnt = face_off[f + 1] - o0, isl = island[f];
  double2 r = make_double2(0.0, 0.0);
  if (j < cnt && isl >= 0 && isl < n_islands) {
    const double2 p = puv[o0 + j];
    const double umin = boxes[4l * isl], vmin = boxes[4l * isl + 1], umax = boxes[4l * isl + 2];
    const bool turned = rot[isl] != 0;
    const double lu = turned ? p.y - vmin : p.x - umin, lv = turned ? umax - p.x : p.y - vmin;
    const double2 off = offsets[isl];
    r = make_double2(lu * scale + off.x, lv * scale + off.y);
  }
  uv[i] = r;
}

// the tree's levels for n faces: n1 = ceil(n / 256) block sums, then ceil(n1 / 256) .. down to 1
long tree_doubles(long n_faces) {
  long total = 0;
  for (long n = nblocks(n_faces);; n = nblocks(n)) {
    total += 3 * n;
    if (n == 1) break;
  }
  return total;
}

}  // namespace

extern "C" long nlt_unwrap_workspace_bytes(long n_faces) {
  if (count_status(n_faces) != NLT_OK) return -1;
  return (tree_doubles(n_faces) + 2l * nblocks(n_faces)) * 8;
}

extern "C" int nlt_unwrap_frames(const double* verts, long n_verts, const int* loop_verts, long n_loops, const int* face_off,
                                 long n_faces, double* n, double* unit, double* area, unsigned char* ok, void* stream) {
  if (!verts || !loop_verts || !face_off || !n || !unit || !area || !ok) return NLT_ERR_BAD_ARG;
  int st = count_status(n_faces);
  if (st == NLT_OK) st = count_status(n_verts);
  if (st == NLT_OK) st = count_status(n_loops);
  if (st != NLT_OK) return st;
  hipLaunchKernelGGL(frames_kernel, dim3(nblocks(n_faces)), dim3(kT), 0, static_cast<hipStream_t>(stream), verts, (int)n_verts,
                     loop_verts, face_off, (int)n_faces, n, unit, area, ok);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_unwrap_seed(const double* area, const unsigned char* ok, long n_faces, unsigned char* remaining, void* ws,
                               long ws_bytes, long* pair, void* stream) {
  if (!area || !ok || !remaining || !ws || !pair) return NLT_ERR_BAD_ARG;
  const int st = count_status(n_faces);
  if (st != NLT_OK) return st;
  if (ws_bytes < nlt_unwrap_workspace_bytes(n_faces)) return NLT_ERR_BAD_ARG;
  const unsigned nb = nblocks(n_faces);
  double* pval = static_cast<double*>(ws) + tree_doubles(n_faces);
  long* pidx = reinterpret_cast<long*>(pval + nb);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(seed_kernel, dim3(nb), dim3(kT), 0, s, area, ok, (int)n_faces, remaining, pval, pidx);
  hipLaunchKernelGGL(argext_final_kernel<true>, dim3(1), dim3(kT), 0, s, pval, pidx, (int)nb, pair);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_unwrap_gather(const double* unit, const double* area, unsigned char* remaining, long n_faces, long seed,
                                 double cos_half, double aw, double omw, void* ws, long ws_bytes, double* vec, void* stream) {
  if (!unit || !area || !remaining || !ws || !vec) return NLT_ERR_BAD_ARG;
  const int st = count_status(n_faces);
  if (st != NLT_OK) return st;
  if (seed < 0 || seed >= n_faces || ws_bytes < nlt_unwrap_workspace_bytes(n_faces)) return NLT_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* level = static_cast<double*>(ws);
  long n = nblocks(n_faces);
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)n), dim3(kT), 0, s, unit, area, remaining, (int)n_faces, (int)seed, cos_half, aw, omw,
                     level);
  while (n > 1) {
    const long m = nblocks(n);
    hipLaunchKernelGGL(tree_kernel, dim3((unsigned)m), dim3(kT), 0, s, level, (int)n, level + 3 * n);
    level += 3 * n;
    n = m;
  }
  hipLaunchKernelGGL(normalize_kernel, dim3(1), dim3(64), 0, s, level, vec);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_unwrap_farthest(const double* unit, const unsigned char* ok, const unsigned char* remaining, double* best,
                                   long n_faces, const double* vec, int first, void* ws, long ws_bytes, long* pair, void* stream) {
  if (!unit || !ok || !remaining || !best || !vec || !ws || !pair) return NLT_ERR_BAD_ARG;
  const int st = count_status(n_faces);
  if (st != NLT_OK) return st;
  if (ws_bytes < nlt_unwrap_workspace_bytes(n_faces)) return NLT_ERR_BAD_ARG;
  const unsigned nb = nblocks(n_faces);
  double* pval = static_cast<double*>(ws) + tree_doubles(n_faces);
  long* pidx = reinterpret_cast<long*>(pval + nb);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(farthest_kernel, dim3(nb), dim3(kT), 0, s, unit, ok, remaining, best, (int)n_faces, vec, first, pval, pidx);
  hipLaunchKernelGGL(argext_final_kernel<false>, dim3(1), dim3(kT), 0, s, pval, pidx, (int)nb, pair);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_unwrap_assign(const double* unit, const unsigned char* ok, long n_faces, const double* vectors, int n_vectors,
                                 int* group, void* stream) {
  if (!unit || !ok || !vectors || !group || n_vectors <= 0) return NLT_ERR_BAD_ARG;
  const int st = count_status(n_faces);
  if (st != NLT_OK) return st;
  hipLaunchKernelGGL(assign_kernel, dim3(nblocks(n_faces)), dim3(kT), 0, static_cast<hipStream_t>(stream), unit, ok, (int)n_faces,
                     vectors, n_vectors, group);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_unwrap_edge_keys(const int* loop_verts, long n_loops, const int* face_off, long n_faces, long n_verts, long* keys,
                                    int* loop_face, void* stream) {
  if (!loop_verts || !face_off || !keys || !loop_face) return NLT_ERR_BAD_ARG;
  int st = count_status(n_faces);
  if (st == NLT_OK) st = count_status(n_verts);
  if (st == NLT_OK) st = count_status(n_loops);
  if (st != NLT_OK) return st;
  hipLaunchKernelGGL(edge_keys_kernel, dim3(nblocks(n_loops)), dim3(kT), 0, static_cast<hipStream_t>(stream), loop_verts, (int)n_loops,
                     face_off, (int)n_faces, n_verts, keys, loop_face);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_unwrap_islands_init(const int* group, long n_faces, int* label, void* stream) {
  if (!group || !label) return NLT_ERR_BAD_ARG;
  const int st = count_status(n_faces);
  if (st != NLT_OK) return st;
  hipLaunchKernelGGL(label_init_kernel, dim3(nblocks(n_faces)), dim3(kT), 0, static_cast<hipStream_t>(stream), group, (int)n_faces, label);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_unwrap_islands_round(const long* keys_sorted, const long* order, const int* loop_face, long n_loops, const int* group,
                                        long n_faces, int* label, int* changed, void* stream) {
  if (!keys_sorted || !order || !loop_face || !group || !label || !changed) return NLT_ERR_BAD_ARG;
  int st = count_status(n_faces);
  if (st == NLT_OK) st = count_status(n_loops);
  if (st != NLT_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(changed, 0, sizeof(int), s) != hipSuccess) return NLT_ERR_LAUNCH;
  hipLaunchKernelGGL(hook_kernel, dim3(nblocks(n_loops)), dim3(kT), 0, s, keys_sorted, order, loop_face, (int)n_loops, group, label, changed);
  hipLaunchKernelGGL(jump_kernel, dim3(nblocks(n_faces)), dim3(kT), 0, s, (int)n_faces, label);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_unwrap_boxes(const double* verts, const int* loop_verts, const int* loop_face, long n_loops, const int* group,
                                const int* island, long n_faces, const double* frames, int n_vectors, double* puv, double* boxes,
                                long n_islands, void* stream) {
  if (!verts || !loop_verts || !loop_face || !group || !island || !frames || !puv || !boxes || n_vectors <= 0) return NLT_ERR_BAD_ARG;
  int st = count_status(n_faces);
  if (st == NLT_OK) st = count_status(n_loops);
  if (st == NLT_OK) st = count_status(n_islands);
  if (st != NLT_OK) return st;
  if (n_islands > n_faces) return NLT_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(boxes);
  hipLaunchKernelGGL(box_init_kernel, dim3(nblocks(4 * n_islands)), dim3(kT), 0, s, keys, 4 * n_islands);
  hipLaunchKernelGGL(project_kernel, dim3(nblocks(n_loops)), dim3(kT), 0, s, verts, loop_verts, loop_face, (int)n_loops, group, island,
                     frames, n_vectors, (int)n_islands, reinterpret_cast<double2*>(puv), keys);
  hipLaunchKernelGGL(box_decode_kernel, dim3(nblocks(4 * n_islands)), dim3(kT), 0, s, keys, 4 * n_islands);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_unwrap_uv(const double* puv, long n_loops, const int* face_off, const int* island, long n_faces, const double* boxes,
                             const unsigned char* rot, const double* offsets, long n_islands, double scale, int vmax, double* uv,
                             void* stream) {
  if (!puv || !face_off || !island || !boxes || !rot || !offsets || !uv || vmax <= 0) return NLT_ERR_BAD_ARG;
  int st = count_status(n_faces);
  if (st == NLT_OK) st = count_status(n_loops);
  if (st == NLT_OK) st = count_status(n_islands);
  if (st != NLT_OK) return st;
  const long n_slots = n_faces * vmax;
  if ((n_slots + kT - 1) / kT >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(uv_kernel, dim3(nblocks(n_slots)), dim3(kT), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const double2*>(puv), face_off, island, n_slots, vmax, boxes, rot,
                     reinterpret_cast<const double2*>(offsets), (int)n_islands, scale, reinterpret_cast<double2*>(uv));
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}
