// Mesh ray casting: first-hit rays per camera pixel and shadow rays per hit pixel, the geometry step that feeds
// data_gen/render.py's dense `intersect` without Blender.
//   replaces: xm.blender.camera.backproject_to_3d (third_party/xiuminglib/xiuminglib/blender/camera.py:512-654) and the
//             shadow-ray loop of calc_light_cosines (data_gen/render.py:238-254), both Python loops over a mathutils BVH.
// Built with -ffp-contract=off (csrc/Makefile): results are compared bit for bit with NumPy (tests/raycast_ref.py).
//
// THE DEFINITION OF A HIT (one device function, `hit_triangle`; float64, two-sided Moeller-Trumbore, no fused operations):
//   e1 = v1 - v0, e2 = v2 - v0, p = d x e2, det = e1 . p;        miss unless det is finite and non-zero
//   inv = 1 / det, s = o - v0, u = (s . p) * inv;                miss if u < 0 or u > 1
//   q = s x e1, v = (d . q) * inv;                               miss if v < 0 or u + v > 1
//   t = (e2 . q) * inv;                                          hit iff t >= 0
// a . b = (ax*bx + ay*by) + az*bz; (a x b) = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx).  The closest hit is the smallest t,
// equal t goes to the lower ORIGINAL triangle index.  loc = o + t*d (a multiply, then an add); normal = (e1 x e2) / |e1 x e2|
// (component-wise division by sqrt((nx*nx + ny*ny) + nz*nz)): the geometric normal, not flipped towards the ray.
// A triangle whose e1 x e2 is the zero vector or not finite is DEGENERATE: it is never hit, it is left out of every box, and its
// NaNs reach nothing.  The test is not watertight: a ray aimed exactly at a shared edge can miss both triangles.
//
// THE HIERARCHY (two float64 buffers, sizes from nlt_bvh_tris_doubles / nlt_bvh_nodes_doubles; T triangles):
//   L  = ceil(T / 4) leaves of kLeaf = 4 slots, padded to Lp = the next power of two; depth D = log2(Lp).
//   tris  [Lp * 4][10]: v0 (3), e1 (3), e2 (3), original triangle index as a double (-1: empty slot -- padding or a degenerate
//         triangle; its nine other doubles are 0).  Slot s < T holds triangle order[s] (the caller's stable sort of the 30-bit
//         Morton codes of nlt_bvh_morton).
//   nodes [2 * Lp - 1][6]: box lo (3), hi (3) of a complete binary tree, children of node i at 2i + 1 and 2i + 2, leaf j at node
//         Lp - 1 + j.  A node without a hittable triangle has lo = (1,1,1), hi = (-1,-1,-1) (lo.x > hi.x marks "empty").
//   Boxes come level by level from the leaves up, one launch per level: no atomics, no spinning, equal inputs give equal bits.
//
// THE TRAVERSAL: one ray per lane, near child first, the far child on a per-lane stack in LDS ((D + 1) ints per lane, sized at
// launch from D; entry k of lane l at [k * 64 + l], so a wave's pushes and pops hit 64 different banks).  A node is pruned only
// when its entry distance is STRICTLY greater than the best t, so an equal-t, lower-index triangle is still reached.
// The box test is conservative.  Per axis the slab [lo - m, hi + m] is used with m = kBoxUlps ulps of max(|lo|, |hi|, |o|) plus
// the smallest normal double (so lo - m < o < hi + m strictly when o lies in a zero-thickness slab or on a box face, also at 0),
// t1 = (lo - m - o) * (1/d), t2 = (hi + m - o) * (1/d).  A direction component that is +0, -0 or so small that 1/d overflows gives
// t1, t2 = -inf / +inf in some order when o is strictly inside the widened slab (no constraint) and two infinities of one sign
// when it is outside (a miss: such a ray never enters the slab); 0 * inf cannot occur strictly inside.  NaNs are dropped by
// fmin / fmax, which is the accepting direction.  The interval ends are then moved outward by kSlabUlps ulps.
// Why these numbers suffice: t1 and t2 carry three roundings each (the subtraction, the reciprocal, the product), a relative
// error below 2 ulps, so 4 ulps outward make the interval contain every exact parameter of a point of the widened box.  The
// widening m covers what the triangle test itself may accept outside the exact triangle: u, v and t come from about a dozen
// rounded operations on coordinate differences, so for a triangle that is not a sliver seen edge-on (|e1||e2||d| / |det| up
// to ~4) an accepted point lies within a few tens of ulps of the largest coordinate involved (a vertex or the origin); 256 is
// that with margin.  For worse-conditioned slivers the bound grows with the condition number and is not claimed.
// Every store is a plain vector store.
//
// DIRECT LIGHTING (`render_kernel`, nlt_render_direct): one point light, Lambert + GGX, hard cast shadows, S x S box-filtered
// samples per pixel.  Not Cycles: no global illumination, no subsurface scattering, no light size (GLOBAL RENDERS below add one
// diffuse bounce and a sized light in a kernel of their own; this one stays as it is).  Float64 throughout, only
// + - * / sqrt, every operation in the order written here (tests/shade_ref.py restates it); one lane per pixel, the primary ray
// and the shadow ray share the lane's LDS stack in turn.  Per pixel (x, y), samples j = 0 .. S-1 (outer), i = 0 .. S-1 (inner):
//   px = x + ((2i + 1) / (2S) - 0.5), py = y + ((2j + 1) / (2S) - 0.5)        (S = 1: exactly (x, y), the ray of camera_kernel)
//   ray, closest hit, loc = cam + t*d and the geometric normal ng exactly as in camera_kernel, with (px, py) for (x, y)
//   a miss adds nothing.  (u, v) = the barycentrics of `hit_triangle` recomputed at the hit's slot with its operations:
//     p = d x e2, inv = 1 / (e1 . p), s = cam - v0, u = (s . p) * inv, q = s x e1, v = (d . q) * inv;  w = (1 - u) - v
//   blend(a0, a1, a2) = (w*a0 + u*a1) + v*a2 per component, corners of the caller's triangle index
//   n  = ng, or with tri_normals: m = blend(n0, n1, n2), lm = sqrt(m . m), n = m / lm when lm is finite and > 0, else ng
//   wo = (cam - loc) / |cam - loc|, co = n . wo;  co < 0: n = -n, co = -co                       (two-sided)
//   kd = the constant, or with tri_rgb: blend(c0, c1, c2)
//   wl = light - loc, r2 = wl . wl, wi = wl / sqrt(r2), ci = n . wi;  unless ci > 0 the sample adds nothing
//   shadow: the rule of shadow_kernel -- ds = (loc - light) / full, full = |loc - light|, closest hit from the light; a hit with
//     !(|t - full| <= 1e-8 + 1e-5 * |full|) is occluded and the sample adds nothing
//   spec = 0 unless co > 0; else with a2 = alpha * alpha:
//     hv = wi + wo, h = hv / sqrt(hv . hv), nh = n . h, vh = wo . h
//     dd = (nh*nh) * (a2 - 1) + 1, D = a2 / (pi * (dd*dd))
//     G1(c) = (2*c) / (c + sqrt(a2 + (1 - a2) * (c*c)))
//     m1 = 1 - vh, m2 = m1*m1, m5 = (m2*m2) * m1, F = ks + (1 - ks) * m5
//     spec = (((D * G1(ci)) * G1(co)) * F) / ((4*ci) * co)
//   radiance[c] = ((intensity / r2) * ci) * (kd[c] / pi + spec),   pi = 3.141592653589793
// rgb[c] = (float)(sum of radiance[c] in (j, i) order / (double)(S*S)); coverage = (float)((double)hits / (double)(S*S)).
//
// GLOBAL RENDERS (`render_global_kernel`, nlt_render_global): the above with a spherical light of radius light_radius sampled at
// n_l points (penumbrae) and one cosine-weighted diffuse bounce over n_b directions (colour bleeding, light in cast shadows).
// Still not Cycles: one bounce, no glossy indirect light, no subsurface scattering, one object.  Same form: float64, + - * / sqrt
// only, one lane per pixel, every traversal of a lane (primary, n_l shadow rays, n_b bounce rays and their shadow rays) uses the
// lane's LDS stack in turn.  The tables come from the host (data_gen/shade.py): light_pts [n_lsets][n_l][3] unit vectors,
// bounce_pts [n_bsets][n_b][2] points of the unit disc; no sine or cosine is evaluated here (tests/shade_global_ref.py restates
// every step in NumPy).  Per sample s = j*S + i, with light set s mod n_lsets and bounce set s mod n_bsets:
//   primary ray, hit (original index T0), loc, ng, (u, v, w), n, wo, co, the two-sided flip and kd exactly as above
//   DIRECT  a = 0; for k = 0 .. n_l-1:  Lk[c] = light[c] + light_radius * light_pts[set][k][c],  Ik = intensity / (double)n_l
//     the steps above from "wl = light - loc" on with Lk, Ik for light, intensity (ci > 0, shadow ray from Lk, spec);
//     a[c] += ((Ik / r2) * ci) * (kd[c] / pi + spec).   D[c] += a[c].   The light sphere is not geometry: it occludes nothing.
//   INDIRECT (n_b > 0, else 0)  ngf = ng, negated when ng . wo < 0
//     frame (Duff et al. 2017): sg = n.z >= 0 ? 1 : -1, fa = -1 / (sg + n.z), fb = (n.x*n.y) * fa
//       t1 = (1 + (sg * (n.x*n.x)) * fa, sg * fb, -sg * n.x),  t2 = (fb, sg + (n.y*n.y) * fa, -n.y)
//     b = 0; for k = 0 .. n_b-1:  (dx, dy) = bounce_pts[set][k], qz = (1 - dx*dx) - dy*dy, dz = sqrt(qz > 0 ? qz : 0)
//       wv[c] = (dx*t1[c] + dy*t2[c]) + dz*n[c], wb = wv / sqrt(wv . wv);  skipped unless ngf . wb > 0
//       closest hit of (loc, wb) over all triangles but original index T0 (`closest_hit<true>`); a miss adds nothing
//       loc2 = loc + t*wb; ng2, barycentrics (origin loc, direction wb), n2, kd2 by the primary's rules; n2 = -n2 when n2 . wb > 0
//       the light's CENTRE, full intensity, Lambert only: wl = light - loc2, r2, wi, ci = n2 . wi; ci > 0 or nothing; shadow ray
//       from the light towards loc2 (isclose rule);  b[c] += ((intensity / r2) * ci) * (kd2[c] / pi)
//     I[c] += (kd[c] * b[c]) / (double)n_b
// rgb[c] = (float)((D[c] + I[c]) / (double)(S*S)), rgb_indirect[c] = (float)(I[c] / (double)(S*S)), coverage as above.
// D and I are kept apart so that n_b = 0, n_l = 1, light_radius = 0 gives render_kernel's bits (x + 0 = x).
#include <math.h>
#include <stdint.h>

#include "nlt_common.h"

namespace {

constexpr int kThreads = 64;                    // one wave per workgroup: no barriers, the LDS stack is per lane
constexpr int kLeaf = 4;
constexpr int kTriDoubles = 10;
constexpr double kBoxUlps = 256.0 * 2.220446049250313e-16;
constexpr double kSlabUlps = 4.0 * 2.220446049250313e-16;
constexpr double kTiny = 2.2250738585072014e-308;

struct V3 { double x, y, z; };

__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 load3(const double* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ void store3(double* p, V3 a) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }
__device__ __forceinline__ bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

// the definition of a hit (file header)
__device__ __forceinline__ bool hit_triangle(V3 o, V3 d, V3 v0, V3 e1, V3 e2, double& t_out) {
  const V3 p = cross(d, e2);
  const double det = dot(e1, p);
  if (!isfinite(det) || det == 0.0) return false;
  const double inv = 1.0 / det;
  const V3 s = sub(o, v0);
  const double u = dot(s, p) * inv;
  if (!(u >= 0.0 && u <= 1.0)) return false;
  const V3 q = cross(s, e1);
  const double v = dot(d, q) * inv;
  if (!(v >= 0.0 && u + v <= 1.0)) return false;
  const double t = dot(e2, q) * inv;
  if (!(t >= 0.0)) return false;
  t_out = t;
  return true;
}

__device__ __forceinline__ bool degenerate(V3 e1, V3 e2) {
  const V3 n = cross(e1, e2);
  return !finite3(n) || (n.x == 0.0 && n.y == 0.0 && n.z == 0.0);
}

// dir = (to - from) / |to - from|, a division per component
__device__ __forceinline__ V3 unit_towards(V3 from, V3 to, double& len) {
  const V3 w = sub(to, from);
  len = sqrt(dot(w, w));
  return {w.x / len, w.y / len, w.z / len};
}

// ---------------------------------------------------------------- build
__device__ __forceinline__ unsigned spread10(unsigned v) {
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

__device__ __forceinline__ unsigned quant10(double c, double lo, double hi) {
  const double x = (c - lo) / (hi - lo) * 1024.0;
  if (!(x > 0.0)) return 0u;                        // (NaN, a zero extent, below the box)
  return x >= 1023.0 ? 1023u : (unsigned)x;
}

__global__ __launch_bounds__(256) void morton_kernel(const double* __restrict__ tv, int n, V3 lo, V3 hi, int* __restrict__ codes) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double* p = tv + (long)i * 9;
  const double cx = ((p[0] + p[3]) + p[6]) / 3.0, cy = ((p[1] + p[4]) + p[7]) / 3.0, cz = ((p[2] + p[5]) + p[8]) / 3.0;
  codes[i] = (int)((spread10(quant10(cx, lo.x, hi.x)) << 2) | (spread10(quant10(cy, lo.y, hi.y)) << 1) |
                   spread10(quant10(cz, lo.z, hi.z)));
}

// one thread per leaf: its four slots of `tris`, then its box
__global__ __launch_bounds__(256) void leaves_kernel(const double* __restrict__ tv, const int* __restrict__ order, int n, int lp,
                                                     double* __restrict__ tris, double* __restrict__ nodes) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= lp) return;
  V3 lo = {1.0, 1.0, 1.0}, hi = {-1.0, -1.0, -1.0};
  bool any = false;
  for (int k = 0; k < kLeaf; ++k) {
    const long s = (long)j * kLeaf + k;
    double* out = tris + s * kTriDoubles;
    bool keep = false;
    if (s < n) {
      const int i = order[s];
      const double* p = tv + (long)i * 9;
      const V3 v0 = load3(p), v1 = load3(p + 3), v2 = load3(p + 6);
      const V3 e1 = sub(v1, v0), e2 = sub(v2, v0);
      if (finite3(v0) && !degenerate(e1, e2)) {
        keep = true;
        store3(out, v0); store3(out + 3, e1); store3(out + 6, e2);
        out[9] = (double)i;
        const V3 tlo = {fmin(v0.x, fmin(v1.x, v2.x)), fmin(v0.y, fmin(v1.y, v2.y)), fmin(v0.z, fmin(v1.z, v2.z))};
        const V3 thi = {fmax(v0.x, fmax(v1.x, v2.x)), fmax(v0.y, fmax(v1.y, v2.y)), fmax(v0.z, fmax(v1.z, v2.z))};
        lo = any ? V3{fmin(lo.x, tlo.x), fmin(lo.y, tlo.y), fmin(lo.z, tlo.z)} : tlo;
        hi = any ? V3{fmax(hi.x, thi.x), fmax(hi.y, thi.y), fmax(hi.z, thi.z)} : thi;
        any = true;
      }
    }
    if (!keep) {
      for (int c = 0; c < 9; ++c) out[c] = 0.0;
      out[9] = -1.0;
    }
  }
  double* b = nodes + ((long)lp - 1 + j) * 6;
  store3(b, lo); store3(b + 3, hi);
}

// one thread per node of the level that starts at node `first` and has `count` nodes
__global__ __launch_bounds__(256) void level_kernel(double* __restrict__ nodes, int first, int count) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= count) return;
  const long i = (long)first + k;
  const double* a = nodes + (2 * i + 1) * 6;
  const double* b = a + 6;
  const V3 alo = load3(a), ahi = load3(a + 3), blo = load3(b), bhi = load3(b + 3);
  const bool ea = alo.x > ahi.x, eb = blo.x > bhi.x;
  V3 lo, hi;
  if (ea) { lo = blo; hi = bhi; }
  else if (eb) { lo = alo; hi = ahi; }
  else {
    lo = {fmin(alo.x, blo.x), fmin(alo.y, blo.y), fmin(alo.z, blo.z)};
    hi = {fmax(ahi.x, bhi.x), fmax(ahi.y, bhi.y), fmax(ahi.z, bhi.z)};
  }
  store3(nodes + i * 6, lo); store3(nodes + i * 6 + 3, hi);
}

// ---------------------------------------------------------------- traversal
struct Ray {
  V3 o, d, inv;
};

__device__ __forceinline__ void slab(double lo, double hi, double o, double inv, double& tn, double& tf) {
  const double m = fmax(fmax(fabs(lo), fabs(hi)), fabs(o)) * kBoxUlps + kTiny;
  const double t1 = ((lo - m) - o) * inv, t2 = ((hi + m) - o) * inv;
  tn = fmax(tn, fmin(t1, t2));
  tf = fmin(tf, fmax(t1, t2));
}

// Entry distance of the ray into the widened box, moved outward; false when the ray misses it.  (box: lo[3], hi[3])
__device__ __forceinline__ bool hit_box(const Ray& r, const double* __restrict__ box, double& enter) {
  const double lox = box[0], hix = box[3];
  if (lox > hix) return false;                      // an empty node
  double tn = -INFINITY, tf = INFINITY;
  slab(lox, hix, r.o.x, r.inv.x, tn, tf);
  slab(box[1], box[4], r.o.y, r.inv.y, tn, tf);
  slab(box[2], box[5], r.o.z, r.inv.z, tn, tf);
  tn -= fabs(tn) * kSlabUlps;
  tf += fabs(tf) * kSlabUlps;
  enter = tn;
  return !(tn > tf) && !(tf < 0.0);
}

struct Hit {
  double t;
  int tri;        // original index, -1: none
  long slot;      // where its (v0, e1, e2) lies in `tris`
};

// kSkip: the triangle whose ORIGINAL index is `skip` is passed over (the bounce rays of render_global_kernel leave from it);
// without it the code is what it was.
template <bool kSkip = false>
__device__ __forceinline__ Hit closest_hit(V3 o, V3 d, const double* __restrict__ tris, const double* __restrict__ nodes, int lp,
                                           int* __restrict__ stack /* this lane's entry 0; entries kThreads ints apart */,
                                           int skip = -1) {
  Ray r;
  r.o = o; r.d = d;
  r.inv = {1.0 / d.x, 1.0 / d.y, 1.0 / d.z};
  Hit best = {INFINITY, -1, 0};
  double enter;
  if (!hit_box(r, nodes, enter)) return best;
  int sp = 0;
  int node = 0;
  const int first_leaf = lp - 1;
  while (true) {
    if (node >= first_leaf) {
      const long s0 = (long)(node - first_leaf) * kLeaf;
      for (int k = 0; k < kLeaf; ++k) {
        const double* p = tris + (s0 + k) * kTriDoubles;
        const int idx = (int)p[9];
        if (idx < 0) continue;
        if (kSkip && idx == skip) continue;
        double t;
        if (hit_triangle(o, d, load3(p), load3(p + 3), load3(p + 6), t) && (t < best.t || (t == best.t && idx < best.tri))) {
          best.t = t; best.tri = idx; best.slot = s0 + k;
        }
      }
      node = -1;
    } else {
      const int c0 = 2 * node + 1;
      double ea, eb;
      const bool ha = hit_box(r, nodes + (long)c0 * 6, ea) && !(ea > best.t);
      const bool hb = hit_box(r, nodes + (long)c0 * 6 + 6, eb) && !(eb > best.t);
      if (ha && hb) {
        const bool a_first = !(eb < ea);
        stack[sp * kThreads] = a_first ? c0 + 1 : c0;
        ++sp;
        node = a_first ? c0 : c0 + 1;
      } else if (ha) node = c0;
      else if (hb) node = c0 + 1;
      else node = -1;
    }
    while (node < 0) {
      if (sp == 0) return best;
      --sp;
      const int cand = stack[sp * kThreads];
      // its entry distance again (cheaper than a second LDS word per entry): prune only when strictly beyond the best t
      double e;
      if (hit_box(r, nodes + (long)cand * 6, e) && !(e > best.t)) node = cand;
    }
  }
}

__global__ __launch_bounds__(kThreads) void raycast_kernel(const double* __restrict__ tris, const double* __restrict__ nodes, int lp,
                                                           const int* __restrict__ tri2face, const double* __restrict__ origins,
                                                           const double* __restrict__ dirs, int n, double* __restrict__ t_out,
                                                           int* __restrict__ tri_out, int* __restrict__ face_out) {
  extern __shared__ int s_stack[];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const Hit h = closest_hit(load3(origins + (long)i * 3), load3(dirs + (long)i * 3), tris, nodes, lp, s_stack + threadIdx.x);
  t_out[i] = h.t;
  tri_out[i] = h.tri;
  face_out[i] = h.tri < 0 ? -1 : (tri2face ? tri2face[h.tri] : h.tri);
}

struct Camera {
  double m[16];   // inverse of the 4 x 4 pixel <- world matrix, row-major
  V3 loc;
};

__global__ __launch_bounds__(kThreads) void camera_kernel(const double* __restrict__ tris, const double* __restrict__ nodes, int lp,
                                                          const int* __restrict__ tri2face, Camera cam, int imw, int n,
                                                          double* __restrict__ locs, double* __restrict__ normals,
                                                          unsigned char* __restrict__ valid, int* __restrict__ face_i) {
  extern __shared__ int s_stack[];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double x = (double)(i % imw), y = (double)(i / imw);
  const double* m = cam.m;
  // M^-1 . (x, y, 1, 1), each row summed left to right; then from_homo
  const double hx = ((m[0] * x + m[1] * y) + m[2]) + m[3], hy = ((m[4] * x + m[5] * y) + m[6]) + m[7];
  const double hz = ((m[8] * x + m[9] * y) + m[10]) + m[11], hw = ((m[12] * x + m[13] * y) + m[14]) + m[15];
  const V3 to = {hx / hw, hy / hw, hz / hw};
  double len;
  const V3 d = unit_towards(cam.loc, to, len);
  const Hit h = closest_hit(cam.loc, d, tris, nodes, lp, s_stack + threadIdx.x);
  V3 loc = {0.0, 0.0, 0.0}, nrm = {0.0, 0.0, 0.0};
  if (h.tri >= 0) {
    loc = {cam.loc.x + h.t * d.x, cam.loc.y + h.t * d.y, cam.loc.z + h.t * d.z};
    const double* p = tris + h.slot * kTriDoubles;
    const V3 c = cross(load3(p + 3), load3(p + 6));
    const double l = sqrt(dot(c, c));
    nrm = {c.x / l, c.y / l, c.z / l};
  }
  store3(locs + (long)i * 3, loc);
  store3(normals + (long)i * 3, nrm);
  valid[i] = h.tri >= 0 ? 1 : 0;
  face_i[i] = h.tri < 0 ? -1 : (tri2face ? tri2face[h.tri] : h.tri);
}

__global__ __launch_bounds__(kThreads) void shadow_kernel(const double* __restrict__ tris, const double* __restrict__ nodes, int lp,
                                                          const double* __restrict__ locs, const unsigned char* __restrict__ valid,
                                                          V3 light, int n, unsigned char* __restrict__ occluded) {
  extern __shared__ int s_stack[];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  unsigned char occ = 0;
  if (valid[i]) {
    double full;
    const V3 d = unit_towards(light, load3(locs + (long)i * 3), full);
    const Hit h = closest_hit(light, d, tris, nodes, lp, s_stack + threadIdx.x);
    // data_gen/render.py:248-253: no hit is "not blocked"; else np.isclose(t, full) with its defaults
    if (h.tri >= 0) occ = fabs(h.t - full) <= 1e-8 + 1e-5 * fabs(full) ? 0 : 1;
  }
  occluded[i] = occ;
}

// direct lighting (file header): every operation in the order stated there
struct Shade {
  V3 light, kd;
  double intensity, ks, alpha;
};

constexpr double kPi = 3.141592653589793;

__device__ __forceinline__ V3 blend3(const double* __restrict__ a, double w, double u, double v) {
  return {(w * a[0] + u * a[3]) + v * a[6], (w * a[1] + u * a[4]) + v * a[7], (w * a[2] + u * a[5]) + v * a[8]};
}

__device__ __forceinline__ double smith_g1(double c, double a2) { return (2.0 * c) / (c + sqrt(a2 + (1.0 - a2) * (c * c))); }

__global__ __launch_bounds__(kThreads) void render_kernel(const double* __restrict__ tris, const double* __restrict__ nodes, int lp,
                                                          const double* __restrict__ tri_normals, const double* __restrict__ tri_rgb,
                                                          Camera cam, Shade sh, int imw, int n, int spp_side,
                                                          float* __restrict__ rgb, float* __restrict__ coverage) {
  extern __shared__ int s_stack[];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  int* stack = s_stack + threadIdx.x;
  const double x = (double)(i % imw), y = (double)(i / imw);
  const double* m = cam.m;
  const double two_s = (double)(2 * spp_side), count = (double)(spp_side * spp_side);
  const double a2 = sh.alpha * sh.alpha;
  double sr = 0.0, sg = 0.0, sb = 0.0;
  int hits = 0;
  for (int sj = 0; sj < spp_side; ++sj) {
    const double py = y + ((double)(2 * sj + 1) / two_s - 0.5);
    for (int si = 0; si < spp_side; ++si) {
      const double px = x + ((double)(2 * si + 1) / two_s - 0.5);
      const double hx = ((m[0] * px + m[1] * py) + m[2]) + m[3], hy = ((m[4] * px + m[5] * py) + m[6]) + m[7];
      const double hz = ((m[8] * px + m[9] * py) + m[10]) + m[11], hw = ((m[12] * px + m[13] * py) + m[14]) + m[15];
      const V3 to = {hx / hw, hy / hw, hz / hw};
      double len;
      const V3 d = unit_towards(cam.loc, to, len);
      const Hit h = closest_hit(cam.loc, d, tris, nodes, lp, stack);
      if (h.tri < 0) continue;
      ++hits;
      const V3 loc = {cam.loc.x + h.t * d.x, cam.loc.y + h.t * d.y, cam.loc.z + h.t * d.z};
      const double* p = tris + h.slot * kTriDoubles;
      const V3 v0 = load3(p), e1 = load3(p + 3), e2 = load3(p + 6);
      const V3 c = cross(e1, e2);
      const double l = sqrt(dot(c, c));
      V3 nrm = {c.x / l, c.y / l, c.z / l};
      // the barycentrics of hit_triangle, its operations again
      const V3 pv = cross(d, e2);
      const double inv = 1.0 / dot(e1, pv);
      const V3 s = sub(cam.loc, v0);
      const double u = dot(s, pv) * inv;
      const V3 q = cross(s, e1);
      const double v = dot(d, q) * inv;
      const double w = (1.0 - u) - v;
      if (tri_normals) {
        const V3 mn = blend3(tri_normals + (long)h.tri * 9, w, u, v);
        const double lm = sqrt(dot(mn, mn));
        if (isfinite(lm) && lm > 0.0) nrm = {mn.x / lm, mn.y / lm, mn.z / lm};
      }
      double lo_;
      const V3 wo = unit_towards(loc, cam.loc, lo_);
      double co = dot(nrm, wo);
      if (co < 0.0) { nrm = {-nrm.x, -nrm.y, -nrm.z}; co = -co; }
      const V3 kd = tri_rgb ? blend3(tri_rgb + (long)h.tri * 9, w, u, v) : sh.kd;
      const V3 wl = sub(sh.light, loc);
      const double r2 = dot(wl, wl);
      const double lr = sqrt(r2);
      const V3 wi = {wl.x / lr, wl.y / lr, wl.z / lr};
      const double ci = dot(nrm, wi);
      if (!(ci > 0.0)) continue;
      double full;
      const V3 ds = unit_towards(sh.light, loc, full);
      const Hit hs = closest_hit(sh.light, ds, tris, nodes, lp, stack);
      if (hs.tri >= 0 && !(fabs(hs.t - full) <= 1e-8 + 1e-5 * fabs(full))) continue;
      double spec = 0.0;
      if (co > 0.0) {
        const V3 hv = {wi.x + wo.x, wi.y + wo.y, wi.z + wo.z};
        const double lh = sqrt(dot(hv, hv));
        const V3 hh = {hv.x / lh, hv.y / lh, hv.z / lh};
        const double nh = dot(nrm, hh), vh = dot(wo, hh);
        const double dd = (nh * nh) * (a2 - 1.0) + 1.0;
        const double D = a2 / (kPi * (dd * dd));
        const double m1 = 1.0 - vh, m2 = m1 * m1, m5 = (m2 * m2) * m1;
        const double F = sh.ks + (1.0 - sh.ks) * m5;
        spec = (((D * smith_g1(ci, a2)) * smith_g1(co, a2)) * F) / ((4.0 * ci) * co);
      }
      const double e = (sh.intensity / r2) * ci;
      sr += e * (kd.x / kPi + spec);
      sg += e * (kd.y / kPi + spec);
      sb += e * (kd.z / kPi + spec);
    }
  }
  rgb[(long)i * 3] = (float)(sr / count);
  rgb[(long)i * 3 + 1] = (float)(sg / count);
  rgb[(long)i * 3 + 2] = (float)(sb / count);
  coverage[i] = (float)((double)hits / count);
}

// global renders (file header): a kernel of its own beside render_kernel, which stays as it is
struct Tables {
  const double* light_pts;    // [n_lsets][n_l][3]
  const double* bounce_pts;   // [n_bsets][n_b][2]; not read when n_b == 0
  double light_radius;
  int n_l, n_lsets, n_b, n_bsets;
};

// ng, the shading normal n (blended corner normals where given and usable, else ng; not flipped) and kd of the hit at `slot`
// (original triangle `tri`) of the ray (o, d): the barycentrics are those of hit_triangle, its operations again.
__device__ __forceinline__ void surface_at(const double* __restrict__ tris, long slot, int tri, V3 o, V3 d,
                                           const double* __restrict__ tri_normals, const double* __restrict__ tri_rgb, V3 kd_const,
                                           V3& ng, V3& n, V3& kd) {
  const double* p = tris + slot * kTriDoubles;
  const V3 v0 = load3(p), e1 = load3(p + 3), e2 = load3(p + 6);
  const V3 c = cross(e1, e2);
  const double l = sqrt(dot(c, c));
  ng = {c.x / l, c.y / l, c.z / l};
  n = ng;
  const V3 pv = cross(d, e2);
  const double inv = 1.0 / dot(e1, pv);
  const V3 s = sub(o, v0);
  const double u = dot(s, pv) * inv;
  const V3 q = cross(s, e1);
  const double v = dot(d, q) * inv;
  const double w = (1.0 - u) - v;
  if (tri_normals) {
    const V3 mn = blend3(tri_normals + (long)tri * 9, w, u, v);
    const double lm = sqrt(dot(mn, mn));
    if (isfinite(lm) && lm > 0.0) n = {mn.x / lm, mn.y / lm, mn.z / lm};
  }
  kd = tri_rgb ? blend3(tri_rgb + (long)tri * 9, w, u, v) : kd_const;
}

// The light point L as seen from loc with normal n: r2, wi, ci; false unless ci > 0 and the shadow ray from L reaches loc.
__device__ __forceinline__ bool lit_from(V3 L, V3 loc, V3 n, const double* __restrict__ tris, const double* __restrict__ nodes, int lp,
                                         int* __restrict__ stack, double& r2, V3& wi, double& ci) {
  const V3 wl = sub(L, loc);
  r2 = dot(wl, wl);
  const double lr = sqrt(r2);
  wi = {wl.x / lr, wl.y / lr, wl.z / lr};
  ci = dot(n, wi);
  if (!(ci > 0.0)) return false;
  double full;
  const V3 ds = unit_towards(L, loc, full);
  const Hit hs = closest_hit(L, ds, tris, nodes, lp, stack);
  return !(hs.tri >= 0 && !(fabs(hs.t - full) <= 1e-8 + 1e-5 * fabs(full)));
}

__global__ __launch_bounds__(kThreads) void render_global_kernel(const double* __restrict__ tris, const double* __restrict__ nodes,
                                                                 int lp, const double* __restrict__ tri_normals,
                                                                 const double* __restrict__ tri_rgb, Camera cam, Shade sh, Tables tb,
                                                                 int imw, int n, int spp_side, float* __restrict__ rgb,
                                                                 float* __restrict__ coverage, float* __restrict__ rgb_indirect) {
  extern __shared__ int s_stack[];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  int* stack = s_stack + threadIdx.x;
  const double x = (double)(i % imw), y = (double)(i / imw);
  const double* m = cam.m;
  const double two_s = (double)(2 * spp_side), count = (double)(spp_side * spp_side);
  const double a2 = sh.alpha * sh.alpha;
  const double il = sh.intensity / (double)tb.n_l, nb = (double)tb.n_b;
  double dr = 0.0, dg = 0.0, db = 0.0, ir = 0.0, ig = 0.0, ib = 0.0;
  int hits = 0;
  for (int sj = 0; sj < spp_side; ++sj) {
    const double py = y + ((double)(2 * sj + 1) / two_s - 0.5);
    for (int si = 0; si < spp_side; ++si) {
      const double px = x + ((double)(2 * si + 1) / two_s - 0.5);
      const double hx = ((m[0] * px + m[1] * py) + m[2]) + m[3], hy = ((m[4] * px + m[5] * py) + m[6]) + m[7];
      const double hz = ((m[8] * px + m[9] * py) + m[10]) + m[11], hw = ((m[12] * px + m[13] * py) + m[14]) + m[15];
      const V3 to = {hx / hw, hy / hw, hz / hw};
      double len;
      const V3 d = unit_towards(cam.loc, to, len);
      const Hit h = closest_hit(cam.loc, d, tris, nodes, lp, stack);
      if (h.tri < 0) continue;
      ++hits;
      const V3 loc = {cam.loc.x + h.t * d.x, cam.loc.y + h.t * d.y, cam.loc.z + h.t * d.z};
      V3 ng, nrm, kd;
      surface_at(tris, h.slot, h.tri, cam.loc, d, tri_normals, tri_rgb, sh.kd, ng, nrm, kd);
      double lo_;
      const V3 wo = unit_towards(loc, cam.loc, lo_);
      double co = dot(nrm, wo);
      if (co < 0.0) { nrm = {-nrm.x, -nrm.y, -nrm.z}; co = -co; }
      const int s = sj * spp_side + si;
      // the direct term: the light points of this sample's set, in k order
      const double* lpts = tb.light_pts + (long)(s % tb.n_lsets) * tb.n_l * 3;
      double ar = 0.0, ag = 0.0, ab = 0.0;
      for (int k = 0; k < tb.n_l; ++k) {
        const V3 L = {sh.light.x + tb.light_radius * lpts[3 * k], sh.light.y + tb.light_radius * lpts[3 * k + 1],
                      sh.light.z + tb.light_radius * lpts[3 * k + 2]};
        double r2, ci;
        V3 wi;
        if (!lit_from(L, loc, nrm, tris, nodes, lp, stack, r2, wi, ci)) continue;
        double spec = 0.0;
        if (co > 0.0) {
          const V3 hv = {wi.x + wo.x, wi.y + wo.y, wi.z + wo.z};
          const double lh = sqrt(dot(hv, hv));
          const V3 hh = {hv.x / lh, hv.y / lh, hv.z / lh};
          const double nh = dot(nrm, hh), vh = dot(wo, hh);
          const double dd = (nh * nh) * (a2 - 1.0) + 1.0;
          const double D = a2 / (kPi * (dd * dd));
          const double m1 = 1.0 - vh, m2 = m1 * m1, m5 = (m2 * m2) * m1;
          const double F = sh.ks + (1.0 - sh.ks) * m5;
          spec = (((D * smith_g1(ci, a2)) * smith_g1(co, a2)) * F) / ((4.0 * ci) * co);
        }
        const double e = (il / r2) * ci;
        ar += e * (kd.x / kPi + spec);
        ag += e * (kd.y / kPi + spec);
        ab += e * (kd.z / kPi + spec);
      }
      dr += ar; dg += ag; db += ab;
      if (tb.n_b <= 0) continue;
      // the indirect term: one cosine-weighted bounce per point of this sample's set, in k order
      const double cg = dot(ng, wo);
      const V3 ngf = cg < 0.0 ? V3{-ng.x, -ng.y, -ng.z} : ng;
      const double sg = nrm.z >= 0.0 ? 1.0 : -1.0;
      const double fa = -1.0 / (sg + nrm.z);
      const double fb = (nrm.x * nrm.y) * fa;
      const V3 t1 = {1.0 + (sg * (nrm.x * nrm.x)) * fa, sg * fb, -sg * nrm.x};
      const V3 t2 = {fb, sg + (nrm.y * nrm.y) * fa, -nrm.y};
      const double* bpts = tb.bounce_pts + (long)(s % tb.n_bsets) * tb.n_b * 2;
      double br = 0.0, bg = 0.0, bb = 0.0;
      for (int k = 0; k < tb.n_b; ++k) {
        const double dx = bpts[2 * k], dy = bpts[2 * k + 1];
        const double qz = (1.0 - dx * dx) - dy * dy;
        const double dz = sqrt(qz > 0.0 ? qz : 0.0);
        const V3 wv = {(dx * t1.x + dy * t2.x) + dz * nrm.x, (dx * t1.y + dy * t2.y) + dz * nrm.y, (dx * t1.z + dy * t2.z) + dz * nrm.z};
        const double lw = sqrt(dot(wv, wv));
        const V3 wb = {wv.x / lw, wv.y / lw, wv.z / lw};
        if (!(dot(ngf, wb) > 0.0)) continue;
        const Hit h2 = closest_hit<true>(loc, wb, tris, nodes, lp, stack, h.tri);
        if (h2.tri < 0) continue;
        const V3 loc2 = {loc.x + h2.t * wb.x, loc.y + h2.t * wb.y, loc.z + h2.t * wb.z};
        V3 ng2, n2, kd2;
        surface_at(tris, h2.slot, h2.tri, loc, wb, tri_normals, tri_rgb, sh.kd, ng2, n2, kd2);
        if (dot(n2, wb) > 0.0) n2 = {-n2.x, -n2.y, -n2.z};
        double r2, ci;
        V3 wi;
        if (!lit_from(sh.light, loc2, n2, tris, nodes, lp, stack, r2, wi, ci)) continue;
        const double e = (sh.intensity / r2) * ci;
        br += e * (kd2.x / kPi);
        bg += e * (kd2.y / kPi);
        bb += e * (kd2.z / kPi);
      }
      ir += (kd.x * br) / nb;
      ig += (kd.y * bg) / nb;
      ib += (kd.z * bb) / nb;
    }
  }
  rgb[(long)i * 3] = (float)((dr + ir) / count);
  rgb[(long)i * 3 + 1] = (float)((dg + ig) / count);
  rgb[(long)i * 3 + 2] = (float)((db + ib) / count);
  coverage[i] = (float)((double)hits / count);
  if (rgb_indirect) {
    rgb_indirect[(long)i * 3] = (float)(ir / count);
    rgb_indirect[(long)i * 3 + 1] = (float)(ig / count);
    rgb_indirect[(long)i * 3 + 2] = (float)(ib / count);
  }
}

// ---------------------------------------------------------------- host
int leaves_padded(long n_tris) {
  const long l = (n_tris + kLeaf - 1) / kLeaf;
  long lp = 1;
  while (lp < l) lp <<= 1;
  return (int)lp;
}

int depth_of(int lp) {
  int d = 0;
  while ((1 << d) < lp) ++d;
  return d;
}

int tris_status(long n_tris) {
  if (n_tris <= 0) return NLT_ERR_BAD_ARG;
  if (n_tris >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  return NLT_OK;
}

int rays_status(long n) {
  if (n <= 0) return NLT_ERR_BAD_ARG;
  if (n >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  return NLT_OK;
}

size_t stack_bytes(int lp) { return (size_t)(depth_of(lp) + 1) * kThreads * sizeof(int); }

unsigned blocks(long n, int threads) { return (unsigned)((n + threads - 1) / threads); }

}  // namespace

extern "C" long nlt_bvh_tris_doubles(long n_tris) {
  if (tris_status(n_tris) != NLT_OK) return -1;
  return (long)leaves_padded(n_tris) * kLeaf * kTriDoubles;
}

extern "C" long nlt_bvh_nodes_doubles(long n_tris) {
  if (tris_status(n_tris) != NLT_OK) return -1;
  return (2l * leaves_padded(n_tris) - 1) * 6;
}

extern "C" int nlt_bvh_morton(const double* tri_verts, long n_tris, double lox, double loy, double loz, double hix, double hiy,
                              double hiz, int* codes, void* stream) {
  if (!tri_verts || !codes) return NLT_ERR_BAD_ARG;
  const int st = tris_status(n_tris);
  if (st != NLT_OK) return st;
  hipLaunchKernelGGL(morton_kernel, dim3(blocks(n_tris, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), tri_verts, (int)n_tris,
                     V3{lox, loy, loz}, V3{hix, hiy, hiz}, codes);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_bvh_build(const double* tri_verts, const int* order, long n_tris, double* tris, long tris_doubles, double* nodes,
                             long nodes_doubles, void* stream) {
  if (!tri_verts || !order || !tris || !nodes) return NLT_ERR_BAD_ARG;
  const int st = tris_status(n_tris);
  if (st != NLT_OK) return st;
  if (tris_doubles < nlt_bvh_tris_doubles(n_tris) || nodes_doubles < nlt_bvh_nodes_doubles(n_tris)) return NLT_ERR_BAD_ARG;
  const int lp = leaves_padded(n_tris);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(leaves_kernel, dim3(blocks(lp, 256)), dim3(256), 0, s, tri_verts, order, (int)n_tris, lp, tris, nodes);
  for (int count = lp >> 1; count >= 1; count >>= 1)              // the level of `count` nodes starts at node count - 1
    hipLaunchKernelGGL(level_kernel, dim3(blocks(count, 256)), dim3(256), 0, s, nodes, count - 1, count);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_raycast(const double* tris, const double* nodes, long n_tris, const int* tri2face, const double* origins,
                           const double* dirs, long n_rays, double* t, int* tri, int* face, void* stream) {
  if (!tris || !nodes || !origins || !dirs || !t || !tri || !face) return NLT_ERR_BAD_ARG;
  int st = tris_status(n_tris);
  if (st == NLT_OK) st = rays_status(n_rays);
  if (st == NLT_OK && n_rays * 3 >= (1l << 31)) st = NLT_ERR_UNSUPPORTED;
  if (st != NLT_OK) return st;
  const int lp = leaves_padded(n_tris);
  hipLaunchKernelGGL(raycast_kernel, dim3(blocks(n_rays, kThreads)), dim3(kThreads), stack_bytes(lp), static_cast<hipStream_t>(stream),
                     tris, nodes, lp, tri2face, origins, dirs, (int)n_rays, t, tri, face);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_raycast_camera(const double* tris, const double* nodes, long n_tris, const int* tri2face, const double* cam_host,
                                  int imh, int imw, double* locs, double* normals, unsigned char* valid, int* face_i, void* stream) {
  if (!tris || !nodes || !cam_host || !locs || !normals || !valid || !face_i) return NLT_ERR_BAD_ARG;
  if (imh <= 0 || imw <= 0) return NLT_ERR_BAD_ARG;
  const int st = tris_status(n_tris);
  if (st != NLT_OK) return st;
  const long n = (long)imh * imw;
  if (n * 3 >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  Camera cam;
  for (int k = 0; k < 16; ++k) cam.m[k] = cam_host[k];
  cam.loc = {cam_host[16], cam_host[17], cam_host[18]};
  const int lp = leaves_padded(n_tris);
  hipLaunchKernelGGL(camera_kernel, dim3(blocks(n, kThreads)), dim3(kThreads), stack_bytes(lp), static_cast<hipStream_t>(stream), tris,
                     nodes, lp, tri2face, cam, imw, (int)n, locs, normals, valid, face_i);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_raycast_shadow(const double* tris, const double* nodes, long n_tris, const double* locs, const unsigned char* valid,
                                  long n_pixels, double lx, double ly, double lz, unsigned char* occluded, void* stream) {
  if (!tris || !nodes || !locs || !valid || !occluded) return NLT_ERR_BAD_ARG;
  int st = tris_status(n_tris);
  if (st == NLT_OK) st = rays_status(n_pixels);
  if (st == NLT_OK && n_pixels * 3 >= (1l << 31)) st = NLT_ERR_UNSUPPORTED;
  if (st != NLT_OK) return st;
  const int lp = leaves_padded(n_tris);
  hipLaunchKernelGGL(shadow_kernel, dim3(blocks(n_pixels, kThreads)), dim3(kThreads), stack_bytes(lp), static_cast<hipStream_t>(stream),
                     tris, nodes, lp, locs, valid, V3{lx, ly, lz}, (int)n_pixels, occluded);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_render_direct(const double* tris, const double* nodes, long n_tris, const double* tri_normals, const double* tri_rgb,
                                 const double* cam_host, int imh, int imw, int spp_side, double lx, double ly, double lz,
                                 double intensity, double kd_r, double kd_g, double kd_b, double ks, double alpha, float* rgb_linear,
                                 float* coverage, void* stream) {
  if (!tris || !nodes || !cam_host || !rgb_linear || !coverage) return NLT_ERR_BAD_ARG;
  if (imh <= 0 || imw <= 0 || spp_side < 1 || spp_side > 8) return NLT_ERR_BAD_ARG;
  const int st = tris_status(n_tris);
  if (st != NLT_OK) return st;
  const long n = (long)imh * imw;
  if (n * 3 >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  Camera cam;
  for (int k = 0; k < 16; ++k) cam.m[k] = cam_host[k];
  cam.loc = {cam_host[16], cam_host[17], cam_host[18]};
  const Shade sh = {V3{lx, ly, lz}, V3{kd_r, kd_g, kd_b}, intensity, ks, alpha};
  const int lp = leaves_padded(n_tris);
  hipLaunchKernelGGL(render_kernel, dim3(blocks(n, kThreads)), dim3(kThreads), stack_bytes(lp), static_cast<hipStream_t>(stream), tris,
                     nodes, lp, tri_normals, tri_rgb, cam, sh, imw, (int)n, spp_side, rgb_linear, coverage);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}

extern "C" int nlt_render_global(const double* tris, const double* nodes, long n_tris, const double* tri_normals, const double* tri_rgb,
                                 const double* cam_host, int imh, int imw, int spp_side, double lx, double ly, double lz,
                                 double intensity, double kd_r, double kd_g, double kd_b, double ks, double alpha, double light_radius,
                                 const double* light_pts, int n_l, int n_lsets, const double* bounce_pts, int n_b, int n_bsets,
                                 float* rgb_linear, float* coverage, float* rgb_indirect, void* stream) {
  if (!tris || !nodes || !cam_host || !light_pts || !rgb_linear || !coverage) return NLT_ERR_BAD_ARG;
  if (imh <= 0 || imw <= 0 || spp_side < 1 || spp_side > 8) return NLT_ERR_BAD_ARG;
  if (n_l < 1 || n_l > 64 || n_b < 0 || n_b > 64 || n_lsets < 1 || n_bsets < 1) return NLT_ERR_BAD_ARG;
  if (n_b > 0 && !bounce_pts) return NLT_ERR_BAD_ARG;
  if (!(light_radius >= 0.0) || !isfinite(light_radius)) return NLT_ERR_BAD_ARG;
  const int st = tris_status(n_tris);
  if (st != NLT_OK) return st;
  const long n = (long)imh * imw;
  if (n * 3 >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  if ((long)n_lsets * n_l * 3 >= (1l << 31) || (long)n_bsets * (n_b > 0 ? n_b : 1) * 2 >= (1l << 31)) return NLT_ERR_UNSUPPORTED;
  Camera cam;
  for (int k = 0; k < 16; ++k) cam.m[k] = cam_host[k];
  cam.loc = {cam_host[16], cam_host[17], cam_host[18]};
  const Shade sh = {V3{lx, ly, lz}, V3{kd_r, kd_g, kd_b}, intensity, ks, alpha};
  const Tables tb = {light_pts, bounce_pts, light_radius, n_l, n_lsets, n_b, n_bsets};
  const int lp = leaves_padded(n_tris);
  hipLaunchKernelGGL(render_global_kernel, dim3(blocks(n, kThreads)), dim3(kThreads), stack_bytes(lp), static_cast<hipStream_t>(stream),
                     tris, nodes, lp, tri_normals, tri_rgb, cam, sh, tb, imw, (int)n, spp_side, rgb_linear, coverage, rgb_indirect);
  NLT_CHECK_LAUNCH();
  return NLT_OK;
}
