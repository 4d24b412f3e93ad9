// dist_core.h -- signed distance between two convex primitive geoms with witness points: mj_geomDistance for one pair,
// plain C++ that builds for the device (dist_kernels.hip) and for the host (dmc_geom_distance_host in dmc_api.hip,
// tests/emu/dist_emu.cpp).  It includes nothing of the step core.
//
//   dist = max over unit n of [ n.(cB - cA) - hA(n) - hB(-n) ]      (hX: support function about the centre cX)
//
// the Euclidean distance when the geoms are apart, minus the minimum-translation depth when they overlap.  A sphere is a
// point plus a radius and a capsule a segment plus a radius: the solver runs on the CORES (point, segment, ellipsoid,
// cylinder, box) and the radii are subtracted afterwards, so that every pair with a sphere or a capsule is exact while the
// cores stay apart and shallow contact never reaches EPA.  A plane is closed form: the other geom's support point along
// minus the plane's normal.
//
//   * dist_gjk: GJK on the Minkowski difference A - B with the simplex (difference points, the A-side points and the
//     barycentric weights) in named registers, reduced by conditional swaps with constant indices: nothing is indexed at
//     run time.  It stops on the duality gap upper - lower <= tolerance max(1, upper), upper = |v|, lower = max v.w / |v|.
//     Two polytopic cores (point, segment, box) have finitely many support points and terminate exactly; their gap test
//     runs at 64 machine epsilons where that is tighter than `tolerance`.
//   * dist_epa: the expanding polytope for overlapping cores.  Vertices (difference points only) and faces (three vertex
//     ids packed into one int, the plane's distance) live in caller memory addressed [element * stride]: LDS slices laid
//     out lane-fastest on the device, plain arrays (stride 1) on the host.  Visibility is a sign of a triple product, so no
//     normal is stored.  The depth reported is the smallest support value n.w seen (an attained value of the definition
//     above, with its n); the face distance is the lower bound of the gap test.  Caps: DistCaps<T>.
//   * witness points of an overlap: B is moved out along n by depth + a small gap and GJK runs once more -- the closest
//     points of the separated pair are the touching points, so EPA carries no A-side points.
//   * two convex geoms are solved in the frame of the first (dist_relative / dist_to_world): it needs no pose there.
//
// status: 0 converged; nonzero: a cap was reached or the arithmetic stopped making progress before the gap closed, and
// dist is the best bound found.  DistResult carries what stopped the solve (1 EPA iterations, 2 EPA vertices, 3 EPA face
// slots, 4 a horizon that rounding broke, 5 no face sees the support point, 7 GJK iterations); the C ABI reports 0 / 1.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dmc_model_layout.h"

#if defined(__HIPCC__)
#define DIST_DEV __host__ __device__ __forceinline__      // everything inlines: a call would put the simplex in scratch
#define DIST_UNROLL _Pragma("unroll")
#else
#define DIST_DEV inline
#define DIST_UNROLL
#endif

namespace dmc {

constexpr int kDistBlock = 64;      // lanes of one workgroup: one wave, which orders its own LDS passes without a barrier
constexpr int kDistGeomReals = 15;  // size, pos, mat of the second geom in the first one's frame, staged per lane
enum { DIST_CORE_POINT = 0, DIST_CORE_SEGMENT = 1, DIST_CORE_ELLIPSOID = 2, DIST_CORE_CYLINDER = 3, DIST_CORE_BOX = 4 };

// EPA caps.  V: the tetrahedron and one vertex per iteration at the default 50, two spare; a closed triangulated polytope
// of V vertices has 2 V - 4 faces, and two more slots cover the moment inside one expansion when new faces exist before
// the last visible one is released.  A lane's polytope takes 3 V sizeof(T) + F (sizeof(T) + 4) bytes: 2664 in fp64, 1552
// in fp32 -- more than 64 KB / 64 lanes, so a wave runs its EPA lanes K at a time (dist_kernels.hip).  With the 15 reals
// per lane of the staged second geom (kDistGeomReals): 21 x 2664 + 64 x 120 = 63624 B and 39 x 1552 + 64 x 60 = 64368 B
// of the 65536 B static limit.
template <typename T> struct DistCaps;
template <> struct DistCaps<float> { static constexpr int V = 56, F = 110, K = 39; };
template <> struct DistCaps<double> { static constexpr int V = 56, F = 110, K = 21; };

template <typename T> DIST_DEV T dist_sqrt(T x);
template <> DIST_DEV float dist_sqrt<float>(float x) { return sqrtf(x); }
template <> DIST_DEV double dist_sqrt<double>(double x) { return sqrt(x); }
template <typename T> DIST_DEV T dist_eps();      // 64 machine epsilons: what counts as zero next to the scene's scale
template <> DIST_DEV float dist_eps<float>() { return 64*1.1920929e-7f; }
template <> DIST_DEV double dist_eps<double>() { return 64*2.220446049250313e-16; }
template <typename T> DIST_DEV T dist_abs(T x) { return x < 0 ? -x : x; }
template <typename T> DIST_DEV T dist_max(T a, T b) { return a > b ? a : b; }
template <typename T> DIST_DEV T dist_min(T a, T b) { return a < b ? a : b; }

template <typename T> struct DVec { T x, y, z; };
template <typename T> DIST_DEV DVec<T> dv(T x, T y, T z) { DVec<T> r; r.x = x; r.y = y; r.z = z; return r; }
template <typename T> DIST_DEV DVec<T> operator+(DVec<T> a, DVec<T> b) { return dv(a.x + b.x, a.y + b.y, a.z + b.z); }
template <typename T> DIST_DEV DVec<T> operator-(DVec<T> a, DVec<T> b) { return dv(a.x - b.x, a.y - b.y, a.z - b.z); }
template <typename T> DIST_DEV DVec<T> operator*(T s, DVec<T> a) { return dv(s*a.x, s*a.y, s*a.z); }
template <typename T> DIST_DEV T dot(DVec<T> a, DVec<T> b) { return a.x*b.x + a.y*b.y + a.z*b.z; }
template <typename T> DIST_DEV DVec<T> cross(DVec<T> a, DVec<T> b) { return dv(a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x); }

// A geom is read through ty() / sz(k) / ps(k) / mt(k) so that the solver runs on any holder of one: DistGeom (registers,
// the host), DistGeomOrigin (a geom at the origin of its own frame: nothing but a type and a size) and the kernel's
// DistGeomLds (a lane's slice of LDS, read where it is used: a fp64 pair held in registers would spill).
template <typename T>
struct DistGeom {      // one geom in some frame; mat row-major: frame = pos + mat local
  typedef T real;
  static constexpr bool kOrigin = false;
  int type;
  T size[3], pos[3], mat[9];
  DIST_DEV int ty() const { return type; }
  DIST_DEV T sz(int k) const { return size[k]; }
  DIST_DEV T ps(int k) const { return pos[k]; }
  DIST_DEV T mt(int k) const { return mat[k]; }
};
template <typename T>
struct DistGeomOrigin {
  typedef T real;
  static constexpr bool kOrigin = true;
  int type;
  T size[3];
  DIST_DEV int ty() const { return type; }
  DIST_DEV T sz(int k) const { return size[k]; }
  DIST_DEV T ps(int) const { return (T)0; }
  DIST_DEV T mt(int k) const { return k % 4 == 0 ? (T)1 : (T)0; }
};

DIST_DEV bool dist_supported(int type) {
  return type == DMC_GEOM_PLANE || type == DMC_GEOM_SPHERE || type == DMC_GEOM_CAPSULE || type == DMC_GEOM_ELLIPSOID ||
         type == DMC_GEOM_CYLINDER || type == DMC_GEOM_BOX;
}
DIST_DEV int dist_core_kind(int type) {
  return type == DMC_GEOM_SPHERE ? DIST_CORE_POINT : type == DMC_GEOM_CAPSULE ? DIST_CORE_SEGMENT :
         type == DMC_GEOM_ELLIPSOID ? DIST_CORE_ELLIPSOID : type == DMC_GEOM_CYLINDER ? DIST_CORE_CYLINDER : DIST_CORE_BOX;
}
template <class G> DIST_DEV typename G::real dist_radius(const G& g) {      // what is subtracted after the solve
  typedef typename G::real T;
  return (g.ty() == DMC_GEOM_SPHERE || g.ty() == DMC_GEOM_CAPSULE) ? g.sz(0) : (T)0;
}
template <class G> DIST_DEV typename G::real dist_core_bound(const G& g) {      // radius of a sphere about pos that holds the core
  typedef typename G::real T;
  const T s0 = g.sz(0), s1 = g.sz(1), s2 = g.sz(2);
  switch (g.ty()) {
    case DMC_GEOM_CAPSULE: return s1;
    case DMC_GEOM_ELLIPSOID: return dist_max(s0, dist_max(s1, s2));
    case DMC_GEOM_CYLINDER: return dist_sqrt(s0*s0 + s1*s1);
    case DMC_GEOM_BOX: return dist_sqrt(s0*s0 + s1*s1 + s2*s2);
    default: return (T)0;
  }
}

// support point of the core of g along the direction d (any length > 0), both in the frame g is posed in; ties take the
// + side
template <typename T, class G>
DIST_DEV DVec<T> dist_support(const G& g, DVec<T> d) {
  const int type = g.ty();
  const T s0 = g.sz(0), s1 = g.sz(1), s2 = g.sz(2);
  T lx = d.x, ly = d.y, lz = d.z, m0 = 1, m1 = 0, m2 = 0, m3 = 0, m4 = 1, m5 = 0, m6 = 0, m7 = 0, m8 = 1;
  if constexpr (!G::kOrigin) {
    m0 = g.mt(0); m1 = g.mt(1); m2 = g.mt(2); m3 = g.mt(3); m4 = g.mt(4); m5 = g.mt(5); m6 = g.mt(6); m7 = g.mt(7); m8 = g.mt(8);
    lx = m0*d.x + m3*d.y + m6*d.z; ly = m1*d.x + m4*d.y + m7*d.z; lz = m2*d.x + m5*d.y + m8*d.z;
  }
  T px = 0, py = 0, pz = 0;
  switch (type) {
    case DMC_GEOM_CAPSULE: pz = lz >= 0 ? s1 : -s1; break;
    case DMC_GEOM_ELLIPSOID: {
      const T ax = s0*s0*lx, ay = s1*s1*ly, az = s2*s2*lz;
      const T q = ax*lx + ay*ly + az*lz;
      if (q > 0) { const T s = 1/dist_sqrt(q); px = ax*s; py = ay*s; pz = az*s; }
      break;
    }
    case DMC_GEOM_CYLINDER: {
      const T q = lx*lx + ly*ly;
      if (q > 0) { const T s = s0/dist_sqrt(q); px = lx*s; py = ly*s; }
      pz = lz >= 0 ? s1 : -s1;
      break;
    }
    case DMC_GEOM_BOX:
      px = lx >= 0 ? s0 : -s0; py = ly >= 0 ? s1 : -s1; pz = lz >= 0 ? s2 : -s2;
      break;
    default: break;      // sphere: the point
  }
  if constexpr (G::kOrigin) return dv(px, py, pz);
  else return dv(g.ps(0) + m0*px + m1*py + m2*pz, g.ps(1) + m3*px + m4*py + m5*pz, g.ps(2) + m6*px + m7*py + m8*pz);
}

// a point of the Minkowski difference A - (B + shift) along d, and the A-side point it came from
template <typename T, class GA, class GB>
DIST_DEV DVec<T> dist_support_diff(const GA& A, const GB& B, DVec<T> shift, DVec<T> d, DVec<T>* a) {
  *a = dist_support(A, d);
  return *a - (dist_support(B, dv(-d.x, -d.y, -d.z)) + shift);
}

template <typename T>
struct DistSimplex {      // up to four points of A - B, the A-side points, barycentric weights of the closest point
  DVec<T> w0, w1, w2, w3, a0, a1, a2, a3;
  T l0, l1, l2, l3;
  int n;
};

// Closest point of a segment / triangle to the origin: weights and squared distance, returned by value -- a pointer to a
// simplex member that merges over branches would keep the simplex in private memory.
template <typename T> struct DistBary { T l0, l1, l2, d2; };
template <typename T>
DIST_DEV DistBary<T> dist_seg(DVec<T> p, DVec<T> q) {
  const DVec<T> e = q - p;
  const T ee = dot(e, e);
  T t = ee > 0 ? -dot(p, e)/ee : (T)0;
  t = t < 0 ? (T)0 : t > 1 ? (T)1 : t;
  const DVec<T> c = p + t*e;
  DistBary<T> r;
  r.l0 = 1 - t; r.l1 = t; r.l2 = 0; r.d2 = dot(c, c);
  return r;
}
// triangle (p, q, r): the interior where the projection falls inside, else the best edge
template <typename T>
DIST_DEV DistBary<T> dist_tri(DVec<T> p, DVec<T> q, DVec<T> r) {
  const DVec<T> n = cross(q - p, r - p);
  const T nn = dot(n, n);
  const T u = dot(cross(q, r), n), v = dot(cross(r, p), n), w = dot(cross(p, q), n);
  DistBary<T> o;
  // (a sliver's plane is noise: its edges decide)
  if (nn > dist_eps<T>()*dist_eps<T>()*dot(q - p, q - p)*dot(r - p, r - p) && u > 0 && v > 0 && w > 0) {
    const T s = 1/(u + v + w), h = dot(p, n);
    o.l0 = u*s; o.l1 = v*s; o.l2 = w*s; o.d2 = h*h/nn;
    return o;
  }
  const DistBary<T> a = dist_seg(p, q), b = dist_seg(q, r), c = dist_seg(r, p);
  o.l0 = a.l0; o.l1 = a.l1; o.l2 = 0; o.d2 = a.d2;
  if (b.d2 < o.d2) { o.l0 = 0; o.l1 = b.l0; o.l2 = b.l1; o.d2 = b.d2; }
  if (c.d2 < o.d2) { o.l0 = c.l1; o.l1 = 0; o.l2 = c.l0; o.d2 = c.d2; }
  return o;
}

// Closest point of the simplex to the origin: sets the weights, drops the vertices with weight zero (conditional swaps with
// constant indices), returns false when a tetrahedron holds the origin (the weights are then untouched).
template <typename T>
DIST_DEV bool dist_simplex_solve(DistSimplex<T>& s) {
  if (s.n == 1) { s.l0 = 1; s.l1 = 0; s.l2 = 0; s.l3 = 0; return true; }
  if (s.n == 2) { const DistBary<T> b = dist_seg(s.w0, s.w1); s.l0 = b.l0; s.l1 = b.l1; s.l2 = 0; s.l3 = 0; }
  else if (s.n == 3) { const DistBary<T> b = dist_tri(s.w0, s.w1, s.w2); s.l0 = b.l0; s.l1 = b.l1; s.l2 = b.l2; s.l3 = 0; }
  else {
    // a face is tried when the origin is not strictly on the inner side of it (a flat tetrahedron tries every face)
    T best = -1, m0 = 0, m1 = 0, m2 = 0, m3 = 0;
#define DIST_FACE(P, Q, R, O, SET)                                                  \
    { const DVec<T> n = cross(Q - P, R - P);                                        \
      const T so = -dot(n, P), sd = dot(n, O - P);                                  \
      if (!(so*sd > 0)) { const DistBary<T> b = dist_tri(P, Q, R); if (best < 0 || b.d2 < best) { best = b.d2; SET; } } }
    DIST_FACE(s.w0, s.w1, s.w2, s.w3, (m0 = b.l0, m1 = b.l1, m2 = b.l2, m3 = 0))
    DIST_FACE(s.w0, s.w1, s.w3, s.w2, (m0 = b.l0, m1 = b.l1, m2 = 0, m3 = b.l2))
    DIST_FACE(s.w0, s.w2, s.w3, s.w1, (m0 = b.l0, m1 = 0, m2 = b.l1, m3 = b.l2))
    DIST_FACE(s.w1, s.w2, s.w3, s.w0, (m0 = 0, m1 = b.l0, m2 = b.l1, m3 = b.l2))
#undef DIST_FACE
    if (best < 0) return false;
    s.l0 = m0; s.l1 = m1; s.l2 = m2; s.l3 = m3;
  }
#define DIST_SWAP(I, J)                                                             \
  if (!(s.l##I > 0) && s.l##J > 0) { DVec<T> t = s.w##I; s.w##I = s.w##J; s.w##J = t; t = s.a##I; s.a##I = s.a##J; s.a##J = t; \
                                     const T l = s.l##I; s.l##I = s.l##J; s.l##J = l; }
  DIST_SWAP(0, 1) DIST_SWAP(1, 2) DIST_SWAP(2, 3) DIST_SWAP(0, 1) DIST_SWAP(1, 2) DIST_SWAP(0, 1)
#undef DIST_SWAP
  s.n = (s.l0 > 0) + (s.l1 > 0) + (s.l2 > 0) + (s.l3 > 0);
  if (s.n == 0) { s.n = 1; s.l0 = 1; }
  return true;
}
template <typename T> DIST_DEV DVec<T> dv_sel(bool c, DVec<T> a, DVec<T> b) { return dv(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }
template <typename T>
DIST_DEV void dist_simplex_push(DistSimplex<T>& s, DVec<T> w, DVec<T> a) {      // selects of values, not of addresses
  const int n = s.n;
  s.w0 = dv_sel(n == 0, w, s.w0); s.a0 = dv_sel(n == 0, a, s.a0);
  s.w1 = dv_sel(n == 1, w, s.w1); s.a1 = dv_sel(n == 1, a, s.a1);
  s.w2 = dv_sel(n == 2, w, s.w2); s.a2 = dv_sel(n == 2, a, s.a2);
  s.w3 = dv_sel(n >= 3, w, s.w3); s.a3 = dv_sel(n >= 3, a, s.a3);
  s.n = n + 1;
}
template <typename T> DIST_DEV DVec<T> dist_simplex_v(const DistSimplex<T>& s) {
  return s.l0*s.w0 + (s.l1*s.w1 + (s.l2*s.w2 + s.l3*s.w3));
}
template <typename T> DIST_DEV DVec<T> dist_simplex_a(const DistSimplex<T>& s) {
  return s.l0*s.a0 + (s.l1*s.a1 + (s.l2*s.a2 + s.l3*s.a3));
}

enum { DIST_GJK_APART = 0, DIST_GJK_OVERLAP = 1, DIST_GJK_CAP = 2 };

// GJK between the cores of A and B + shift.  APART / CAP: dist = |v| (an upper bound of the distance), a the closest
// point on A's core, nrm the unit vector from A towards B.  OVERLAP: the simplex holds the origin (on it or, with four
// vertices, inside it); a is the common point it implies.  (Results by value: see DistBary.)
template <typename T> struct DistGjkOut { int rc; T dist, gap; DVec<T> a, nrm; };      // gap: upper - lower as certified
template <typename T, class GA, class GB>
DIST_DEV DistGjkOut<T> dist_gjk(const GA& A, const GB& B, DVec<T> shift, T scale, T tol, T tol_user, int maxit,
                                         DistSimplex<T>& s) {
  const T tiny = dist_eps<T>()*scale;
  DVec<T> d = dv(B.ps(0) + shift.x - A.ps(0), B.ps(1) + shift.y - A.ps(1), B.ps(2) + shift.z - A.ps(2));
  if (!(dot(d, d) > tiny*tiny)) d = dv((T)1, (T)0, (T)0);
  s.n = 0; s.l0 = 1; s.l1 = 0; s.l2 = 0; s.l3 = 0;
  s.w1 = s.w2 = s.w3 = s.a1 = s.a2 = s.a3 = dv((T)0, (T)0, (T)0);
  DVec<T> aw;
  DVec<T> w = dist_support_diff(A, B, shift, d, &aw);
  dist_simplex_push(s, w, aw);
  DVec<T> v = w;
  T lower = 0, gap = (T)1e30;
  int rc = DIST_GJK_CAP;
  for (int it = 0; it < maxit; it++) {
    const T vv = dot(v, v);
    if (!(vv > tiny*tiny)) { rc = DIST_GJK_OVERLAP; break; }
    const T upper = dist_sqrt(vv);
    w = dist_support_diff(A, B, shift, dv(-v.x, -v.y, -v.z), &aw);
    const T lb = dot(v, w)/upper;
    if (lb > lower) lower = lb;
    gap = upper - lower;
    if (gap <= tol*dist_max((T)1, upper)) { rc = DIST_GJK_APART; break; }
    // the step is tried on a copy: a step that does not come closer is not taken, and the simplex and v of the last
    // good one stand
    DistSimplex<T> t = s;
    dist_simplex_push(t, w, aw);
    if (!dist_simplex_solve(t)) { s = t; rc = DIST_GJK_OVERLAP; break; }
    const DVec<T> vn = dist_simplex_v(t);
    if (!(dot(vn, vn) < vv)) {
      // No progress: |v| stands at the floor of the arithmetic (the classical end of GJK).  The certificate decides: where
      // the certified lower bound lags |v| beyond the tolerance the lane reports that (CAP) with the gap it reached.
      rc = upper - lower <= tol_user*dist_max((T)1, upper) ? DIST_GJK_APART : DIST_GJK_CAP;
      break;
    }
    s = t;
    v = vn;
  }
  DistGjkOut<T> o;
  o.a = dist_simplex_a(s);
  const T vv = dot(v, v);
  o.dist = dist_sqrt(vv);
  o.gap = gap;
  o.nrm = dv_sel(vv > 0, (-1/o.dist)*v, dv((T)0, (T)0, (T)1));
  o.rc = (rc == DIST_GJK_CAP && !(vv > tiny*tiny)) ? DIST_GJK_OVERLAP : rc;
  return o;
}

// ---- EPA -------------------------------------------------------------------------------------------------------------
template <typename T>
struct DistEpaMem {      // a lane's slices: element e at [e * stride]
  T* vtx;        // 3 V: difference points
  T* fdist;      // F: distance of a face's plane from the origin along its outward normal
  int* fidx;     // F: vertex ids a | b << 8 | c << 16, counter-clockwise seen from outside; -1: free slot
  int stride;
};
template <typename T> DIST_DEV DVec<T> epa_vtx(const DistEpaMem<T>& m, int i) {
  return dv(m.vtx[(3*i)*m.stride], m.vtx[(3*i + 1)*m.stride], m.vtx[(3*i + 2)*m.stride]);
}
template <typename T> DIST_DEV void epa_set_vtx(const DistEpaMem<T>& m, int i, DVec<T> p) {
  m.vtx[(3*i)*m.stride] = p.x; m.vtx[(3*i + 1)*m.stride] = p.y; m.vtx[(3*i + 2)*m.stride] = p.z;
}
constexpr int kEpaVisible = 1 << 24, kEpaNew = 1 << 25, kEpaSees = 1 << 26;
template <typename T>
DIST_DEV void epa_set_face(const DistEpaMem<T>& m, int f, int ia, int ib, int ic, int flags) {
  const DVec<T> p = epa_vtx(m, ia), n = cross(epa_vtx(m, ib) - p, epa_vtx(m, ic) - p);
  const T nn = dot(n, n);
  m.fidx[f*m.stride] = ia | ib << 8 | ic << 16 | flags;
  m.fdist[f*m.stride] = nn > 0 ? dot(n, p)/dist_sqrt(nn) : (T)1e30;      // a sliver is never the closest face
}

// Depth and outward unit normal of the origin inside A - B, from a GJK simplex that holds the origin, with the status
// (0, or what stopped it); flat is set when A - B has no interior there (depth 0).
template <typename T> struct DistEpaOut { int status; T depth, gap; DVec<T> nrm; bool flat; };      // gap: upper - lower as certified
template <typename T, class GA, class GB>
DIST_DEV DistEpaOut<T> dist_epa(const GA& A, const GB& B, T scale, T tol, T tol_user, int maxit,
                                         const DistSimplex<T>& s, const DistEpaMem<T>& m) {
  constexpr int V = DistCaps<T>::V, F = DistCaps<T>::F;
  const T tiny = dist_eps<T>()*scale, vis = tiny/8;      // a face sees w when w is above its plane by 8 machine epsilons of the scale
  const DVec<T> zero = dv((T)0, (T)0, (T)0);
  DVec<T> p0 = s.w0, p1 = s.w1, p2 = s.w2, p3 = s.w3, aw;
  int n = s.n;
  DistEpaOut<T> o;
  o.status = 0; o.flat = true; o.depth = 0; o.gap = 0; o.nrm = dv((T)0, (T)0, (T)1);
  // grow the simplex to a tetrahedron with the origin on or in it
  if (n == 1) {
    p1 = dist_support_diff(A, B, zero, dv((T)1, (T)0, (T)0), &aw);
    if (!(dot(p1 - p0, p1 - p0) > tiny*tiny)) p1 = dist_support_diff(A, B, zero, dv((T)-1, (T)0, (T)0), &aw);
    if (!(dot(p1 - p0, p1 - p0) > tiny*tiny)) {
      p1 = dist_support_diff(A, B, zero, dv((T)0, (T)1, (T)0), &aw);
      if (!(dot(p1 - p0, p1 - p0) > tiny*tiny)) p1 = dist_support_diff(A, B, zero, dv((T)0, (T)-1, (T)0), &aw);
      if (!(dot(p1 - p0, p1 - p0) > tiny*tiny)) p1 = dist_support_diff(A, B, zero, dv((T)0, (T)0, (T)1), &aw);
      if (!(dot(p1 - p0, p1 - p0) > tiny*tiny)) p1 = dist_support_diff(A, B, zero, dv((T)0, (T)0, (T)-1), &aw);
      if (!(dot(p1 - p0, p1 - p0) > tiny*tiny)) return o;      // A - B is a point
    }
    n = 2;
  }
  if (n == 2) {
    const DVec<T> e = p1 - p0;
    const T ax = dist_abs(e.x), ay = dist_abs(e.y), az = dist_abs(e.z);
    const DVec<T> axis = ax <= ay && ax <= az ? dv((T)1, (T)0, (T)0) : ay <= az ? dv((T)0, (T)1, (T)0) : dv((T)0, (T)0, (T)1);
    DVec<T> u = cross(e, axis);
    const T ee = dot(e, e);
    bool ok = false;
    for (int k = 0; k < 4 && !ok; k++) {      // +u, -u, then the other perpendicular
      if (k == 2) u = cross(e, u);
      p2 = dist_support_diff(A, B, zero, k & 1 ? dv(-u.x, -u.y, -u.z) : u, &aw);
      const DVec<T> c = cross(p2 - p0, e);
      ok = dot(c, c) > tiny*tiny*ee;
    }
    if (!ok) return o;      // A - B is a segment
    n = 3;
  }
  if (n == 3) {
    const DVec<T> nn = cross(p1 - p0, p2 - p0);
    const T len = dist_sqrt(dot(nn, nn));
    if (!(len > 0)) return o;
    p3 = dist_support_diff(A, B, zero, nn, &aw);
    if (!(dist_abs(dot(nn, p3 - p0)) > tiny*len)) p3 = dist_support_diff(A, B, zero, dv(-nn.x, -nn.y, -nn.z), &aw);
    if (!(dist_abs(dot(nn, p3 - p0)) > tiny*len)) { o.nrm = (1/len)*nn; return o; }      // A - B is flat
  }
  {
    const T vol = dot(cross(p1 - p0, p2 - p0), p3 - p0);
    if (vol == 0) return o;
    const DVec<T> q1 = dv_sel(vol > 0, p2, p1), q2 = dv_sel(vol > 0, p1, p2);      // (values, not addresses, change places)
    p1 = q1; p2 = q2;
  }
  o.flat = false;
  epa_set_vtx(m, 0, p0); epa_set_vtx(m, 1, p1); epa_set_vtx(m, 2, p2); epa_set_vtx(m, 3, p3);
  epa_set_face(m, 0, 0, 1, 2, 0); epa_set_face(m, 1, 0, 3, 1, 0); epa_set_face(m, 2, 0, 2, 3, 0); epa_set_face(m, 3, 1, 3, 2, 0);
  int nv = 4, nf = 4;      // nf: slots in use or freed below it
  T upper = (T)1e30, gap = (T)1e30;
  DVec<T> nbest = dv((T)0, (T)0, (T)1);
  int status = 1;
  for (int it = 0; it < maxit; it++) {
    int fmin = -1;
    T lower = (T)1e30;
    for (int f = 0; f < nf; f++) {
      const T d = m.fdist[f*m.stride];
      if (m.fidx[f*m.stride] >= 0 && d < lower) { lower = d; fmin = f; }
    }
    if (fmin < 0) { status = 8; break; }
    const int id = m.fidx[fmin*m.stride];
    const DVec<T> fa = epa_vtx(m, id & 255);
    DVec<T> nf_ = cross(epa_vtx(m, (id >> 8) & 255) - fa, epa_vtx(m, (id >> 16) & 255) - fa);
    nf_ = (1/dist_sqrt(dot(nf_, nf_)))*nf_;
    const DVec<T> w = dist_support_diff(A, B, zero, nf_, &aw);
    const T h = dot(nf_, w);
    if (h < upper) { upper = h; nbest = nf_; }
    if (lower < 0) lower = 0;
    gap = upper - lower;
    if (gap <= tol*dist_max((T)1, upper)) { status = 0; break; }
    if (nv == V) { status = 2; break; }
    // The faces that see w: the closest face, and what is reached from it across edges through faces that see w too -- a
    // connected patch whatever rounding decides about faces w is coplanar with elsewhere.  The closest face does not see
    // w (by more than rounding): the floor of the arithmetic.
    for (int f = 0; f < nf; f++) {
      const int fi = m.fidx[f*m.stride];
      if (fi < 0) continue;
      const DVec<T> a = epa_vtx(m, fi & 255), nn = cross(epa_vtx(m, (fi >> 8) & 255) - a, epa_vtx(m, (fi >> 16) & 255) - a);
      const T sgn = dot(nn, w - a);
      if (sgn > 0 && sgn*sgn > vis*vis*dot(nn, nn)) m.fidx[f*m.stride] = fi | kEpaSees;
    }
    if (!(m.fidx[fmin*m.stride] & kEpaSees)) {
      for (int f = 0; f < nf; f++) { const int fi = m.fidx[f*m.stride]; if (fi >= 0) m.fidx[f*m.stride] = fi & ~kEpaSees; }
      status = upper - lower <= tol_user*dist_max((T)1, upper) ? 0 : 5;
      break;
    }
    m.fidx[fmin*m.stride] |= kEpaVisible;
    int nvis = 1;
    for (bool grown = true; grown;) {
      grown = false;
      for (int f = 0; f < nf; f++) {
        const int fi = m.fidx[f*m.stride];
        if (fi < 0 || !(fi & kEpaSees) || (fi & kEpaVisible)) continue;
        const int va = fi & 255, vb = (fi >> 8) & 255, vc = (fi >> 16) & 255;
        bool touch = false;
        for (int g = 0; g < nf && !touch; g++) {
          const int gi = m.fidx[g*m.stride];
          if (gi < 0 || !(gi & kEpaVisible)) continue;
          const int ga = gi & 255, gb = (gi >> 8) & 255, gc = (gi >> 16) & 255;
          // a shared edge runs the other way round in the neighbour
          touch = (ga == vb && gb == va) || (gb == vb && gc == va) || (gc == vb && ga == va) ||
                  (ga == vc && gb == vb) || (gb == vc && gc == vb) || (gc == vc && ga == vb) ||
                  (ga == va && gb == vc) || (gb == va && gc == vc) || (gc == va && ga == vc);
        }
        if (touch) { m.fidx[f*m.stride] = fi | kEpaVisible; nvis++; grown = true; }
      }
    }
    for (int f = 0; f < nf; f++) { const int fi = m.fidx[f*m.stride]; if (fi >= 0) m.fidx[f*m.stride] = fi & ~kEpaSees; }
    epa_set_vtx(m, nv, w);
    // every edge of a visible face whose other side is an old face that does not see w gets a new face (edge, w)
    int nnew = 0, free_from = 0;
    bool full = false;
    for (int f = 0; f < nf && !full; f++) {
      const int fi = m.fidx[f*m.stride];
      if (fi < 0 || !(fi & kEpaVisible) || (fi & kEpaNew)) continue;
      const int va = fi & 255, vb = (fi >> 8) & 255, vc = (fi >> 16) & 255;
      bool own_used = false;
      for (int e = 0; e < 3 && !full; e++) {
        const int ea = e == 0 ? va : e == 1 ? vb : vc, eb = e == 0 ? vb : e == 1 ? vc : va;
        bool horizon = false;
        for (int g = 0; g < nf; g++) {
          const int gi = m.fidx[g*m.stride];
          if (gi < 0 || (gi & (kEpaVisible | kEpaNew))) continue;
          const int ga = gi & 255, gb = (gi >> 8) & 255, gc = (gi >> 16) & 255;
          if ((ga == eb && gb == ea) || (gb == eb && gc == ea) || (gc == eb && ga == ea)) { horizon = true; break; }
        }
        if (!horizon) continue;
        int slot = -1;
        if (e == 2 && !own_used) { slot = f; own_used = true; }      // the face's own slot once its last edge is read
        else {
          for (; free_from < F; free_from++)
            if (free_from >= nf || m.fidx[free_from*m.stride] < 0) break;
          if (free_from < F) { slot = free_from; if (slot >= nf) nf = slot + 1; free_from++; }
        }
        if (slot < 0) { full = true; break; }
        epa_set_face(m, slot, ea, eb, nv, kEpaNew);
        nnew++;
      }
      if (!own_used && !full) m.fidx[f*m.stride] = -1;
    }
    if (full || nnew != nvis + 2) { status = full ? 3 : 4; break; }      // out of face slots, or rounding broke the horizon: the best bound stands
    for (int f = 0; f < nf; f++) {
      const int fi = m.fidx[f*m.stride];
      if (fi >= 0) m.fidx[f*m.stride] = fi & ~kEpaNew;
    }
    nv++;
  }
  o.depth = upper; o.gap = gap; o.nrm = nbest; o.status = status;
  return o;
}

template <typename T>
struct DistResult {
  T dist;
  DVec<T> from, to, normal;      // (members, not arrays: nothing here is ever indexed)
  T gap;                // upper - lower of the core distance as the solver certified it: |dist - truth| <= gap
  int status, epa;      // epa: the pair's cores overlapped
};

template <typename T> DIST_DEV void dist_none(T distmax, DistResult<T>* r) {
  r->dist = distmax; r->gap = 0; r->status = 0; r->epa = 0;
  r->from = r->to = r->normal = dv((T)0, (T)0, (T)0);
}
template <typename T> DIST_DEV void dist_finish(DVec<T> from, DVec<T> n, T dist, T distmax, int status, int epa, DistResult<T>* r) {
  if (!(dist < distmax)) { dist_none(distmax, r); r->status = status; r->epa = epa; return; }
  r->dist = dist; r->gap = 0; r->status = status; r->epa = epa;
  r->from = from; r->to = from + dist*n; r->normal = n;
}

// a plane P against a convex geom G, world frame: G's support point along minus the plane's normal; `first`: the plane
// is geom1
template <typename T>
DIST_DEV void dist_plane(const DistGeom<T>& P, const DistGeom<T>& G, bool first, T distmax, DistResult<T>* r) {
  const DVec<T> n = dv(P.mat[2], P.mat[5], P.mat[8]);
  const DVec<T> p = dist_support(G, dv(-n.x, -n.y, -n.z)) - dist_radius(G)*n;
  const T d = dot(n, p - dv(P.pos[0], P.pos[1], P.pos[2]));
  if (first) dist_finish(p - d*n, n, d, distmax, 0, 0, r);
  else dist_finish(p, dv(-n.x, -n.y, -n.z), d, distmax, 0, 0, r);
}
// the pairs that need no solver; false: two convex geoms
template <typename T>
DIST_DEV bool dist_pair_plane(const DistGeom<T>& g1, const DistGeom<T>& g2, T distmax, DistResult<T>* r) {
  const bool pl1 = g1.type == DMC_GEOM_PLANE, pl2 = g2.type == DMC_GEOM_PLANE;
  if (pl1 && pl2) { dist_none(distmax, r); return true; }      // no collider in MuJoCo either
  if (pl1) { dist_plane(g1, g2, true, distmax, r); return true; }
  if (pl2) { dist_plane(g2, g1, false, distmax, r); return true; }
  return false;
}

// Two convex geoms are solved in the frame of geom1: it needs no pose there and geom2 a relative one.
template <typename T>
DIST_DEV void dist_relative(const DistGeom<T>& g1, const DistGeom<T>& g2, DistGeomOrigin<T>* a, DistGeom<T>* b) {
  a->type = g1.type; b->type = g2.type;
  DIST_UNROLL for (int k = 0; k < 3; k++) { a->size[k] = g1.size[k]; b->size[k] = g2.size[k]; }
  const T d0 = g2.pos[0] - g1.pos[0], d1 = g2.pos[1] - g1.pos[1], d2 = g2.pos[2] - g1.pos[2];
  DIST_UNROLL for (int i = 0; i < 3; i++) {
    b->pos[i] = g1.mat[i]*d0 + g1.mat[3 + i]*d1 + g1.mat[6 + i]*d2;
    DIST_UNROLL for (int j = 0; j < 3; j++) b->mat[3*i + j] = g1.mat[i]*g2.mat[j] + g1.mat[3 + i]*g2.mat[3 + j] + g1.mat[6 + i]*g2.mat[6 + j];
  }
}
// a result in the frame of a geom at (pos, mat) into the world frame; a clipped result (zeros) stays
template <typename T>
DIST_DEV void dist_to_world(const T* pos, const T* mat, T distmax, DistResult<T>* r) {
  if (!(r->dist < distmax)) return;
  const DVec<T> f = r->from, n = r->normal;
  const DVec<T> w = dv(mat[0]*n.x + mat[1]*n.y + mat[2]*n.z, mat[3]*n.x + mat[4]*n.y + mat[5]*n.z, mat[6]*n.x + mat[7]*n.y + mat[8]*n.z);
  const DVec<T> g = dv(pos[0] + (mat[0]*f.x + mat[1]*f.y + mat[2]*f.z), pos[1] + (mat[3]*f.x + mat[4]*f.y + mat[5]*f.z),
                       pos[2] + (mat[6]*f.x + mat[7]*f.y + mat[8]*f.z));
  r->normal = w; r->from = g; r->to = g + r->dist*w;
}

// What both phases of a pair derive from its geoms: the scale that zero is measured against and two tolerances of the gap
// test.  tol: what the iterations aim for -- `tolerance`, floored at 32 machine epsilons (3.8e-6 in fp32); two polytopic
// cores terminate exactly and aim for 64 machine epsilons where that is tighter.  tol_user: what status 0 CERTIFIES when
// the arithmetic stops making progress before tol is met -- `tolerance`, floored at 128 machine epsilons (1.5e-5 in fp32,
// where the certified lower bound v.w / |v| of a pair of the scene's size rounds at about 1e-5; 2.8e-14 in fp64: no
// floor in practice).  A gap above it is status nonzero, with the gap reached in DistResult.gap.
template <typename T>
struct DistSetup { T r1, r2, bound, scale, tol, tol_user; };
template <typename T, class GA, class GB>
DIST_DEV DistSetup<T> dist_setup(const GA& g1, const GB& g2, T tolerance) {
  DistSetup<T> u;
  u.r1 = dist_radius(g1); u.r2 = dist_radius(g2);
  const DVec<T> cc = dv(g2.ps(0) - g1.ps(0), g2.ps(1) - g1.ps(1), g2.ps(2) - g1.ps(2));
  u.bound = dist_core_bound(g1) + dist_core_bound(g2);
  u.scale = dist_max(u.bound + dist_sqrt(dot(cc, cc)), (T)1e-3);
  const int k1 = dist_core_kind(g1.ty()), k2 = dist_core_kind(g2.ty());
  const bool poly = k1 != DIST_CORE_ELLIPSOID && k1 != DIST_CORE_CYLINDER && k2 != DIST_CORE_ELLIPSOID && k2 != DIST_CORE_CYLINDER;
  const T run = dist_max(tolerance, dist_eps<T>()/2);
  u.tol = poly ? dist_min(run, dist_eps<T>()) : run;
  u.tol_user = dist_max(tolerance, 2*dist_eps<T>());
  return u;
}

// mj_geomDistance of two convex geoms in whatever frame they are posed in.  GJK on the cores; where they overlap,
// `run_epa(simplex, setup)` returns dist_epa's result and GJK runs once more for the touching points: B moved out along
// the normal by the depth and a gap.  The two GJK runs are one loop body, so the solver is inlined once; EPA is the
// caller's to run because a wave runs its EPA lanes in passes that share the LDS (dist_kernels.hip) -- on the host it is
// dist_epa on plain arrays (dist_pair_host).
template <typename T, class GA, class GB, class RunEpa>
DIST_DEV void dist_pair_convex(const GA& g1, const GB& g2, T distmax, T tolerance, int iterations, RunEpa&& run_epa, DistResult<T>* r) {
  const DistSetup<T> u = dist_setup(g1, g2, tolerance);
  DistSimplex<T> s;
  DVec<T> shift = dv((T)0, (T)0, (T)0), nrm = shift;
  T depth = 0, egap = 0;
  int status = 0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (int phase = 0; phase < 2; phase++) {
    // (the run for the touching points closes its gap to a quarter: the two runs' slack adds up in where the points lie)
    const DistGjkOut<T> g = dist_gjk(g1, g2, shift, u.scale, phase ? u.tol/4 : u.tol, u.tol_user, iterations, s);
    if (phase == 1) {
      // The touching points, both from this run (the point on B moved back); the normal is their direction, which is
      // nrm up to the accuracy nrm has, so that |to - from| is the depth to second order in it.  status certifies dist,
      // not this run.
      const DVec<T> fc = g.a, tc = g.a + g.dist*g.nrm - shift, e = fc - tc;
      const T len = dist_sqrt(dot(e, e));
      const DVec<T> n = dv_sel(len > 0 && depth > 0, (1/(len > 0 ? len : (T)1))*e, nrm);
      const T dist = -depth - u.r1 - u.r2;
      if (!(dist < distmax)) { dist_none(distmax, r); r->status = status; r->epa = 1; break; }
      r->dist = dist; r->gap = egap; r->status = status; r->epa = 1;
      r->from = fc + u.r1*n; r->to = tc - u.r2*n; r->normal = n;
      break;
    }
    if (g.rc != DIST_GJK_OVERLAP) {
      dist_finish(g.a + u.r1*g.nrm, g.nrm, g.dist - u.r1 - u.r2, distmax, g.rc == DIST_GJK_CAP ? 7 : 0, 0, r);
      r->gap = g.gap;
      break;
    }
    const DistEpaOut<T> e = run_epa(s, u);
    status = e.status; depth = e.depth; nrm = e.nrm; egap = e.gap;
    if (e.flat) { dist_finish(g.a + u.r1*nrm, nrm, -depth - u.r1 - u.r2, distmax, status, 1, r); break; }      // (flat: depth 0, gap 0)
    shift = (depth + (T)1e-3*dist_max(u.bound, (T)1e-3))*nrm;
  }
}

// one pair on the host, the kernel's sequence: planes, else geom2 relative to geom1, the solve there, back to the world
template <typename T>
DIST_DEV void dist_pair_host(const DistGeom<T>& g1, const DistGeom<T>& g2, T distmax, T tolerance, int iterations,
                             const DistEpaMem<T>& m, DistResult<T>* r) {
  if (dist_pair_plane(g1, g2, distmax, r)) return;
  DistGeomOrigin<T> a;
  DistGeom<T> b;
  dist_relative(g1, g2, &a, &b);
  dist_pair_convex(a, b, distmax, tolerance, iterations, [&](const DistSimplex<T>& s, const DistSetup<T>& u) {
    return dist_epa(a, b, u.scale, u.tol, u.tol_user, iterations, s, m);
  }, r);
  dist_to_world(g1.pos, g1.mat, distmax, r);
}

// the kernel's arguments (dist_kernels.hip); the members fill_pose_args sets carry the names CamArgs and RayArgs use
template <typename T>
struct DistArgs {
  const T *geom_xpos, *geom_xmat, *xpos, *xmat;      // (rows, B) fields of the batch
  const T* geom_size;      // the step kernel's live table, (ngeom, 3)
  const T* eg_data; const int* eg_slot;      // per-environment geoms ("env_geom" rows), or null
  const int* geom_type;      // (ngeom)
  // pair p: geoms member[adr[4 p] .. + adr[4 p + 1]) against member[adr[4 p + 2] .. + adr[4 p + 3])
  const int *adr, *member;
  const T* distmax;      // (npair)
  int B, npair, iterations;
  T tolerance;
  T *dist, *fromto, *normal;      // (B, P), (B, P, 6), (B, P, 3); each may be null
  int* status;      // (B, P): 0 / 1, bit 1 set when a geom pair of the lane entered EPA; may be null
};

int launch_dist_f32(const DistArgs<float>& a, void* stream);
int launch_dist_f64(const DistArgs<double>& a, void* stream);

}  // namespace dmc
