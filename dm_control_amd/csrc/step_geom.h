// step_geom.h -- geometry of the step core that reads no kernel state: the narrow-phase routines of one geom pair
// (same constructions and operation order as the oracle's) and the rays of touch and rangefinder sensors.
#pragma once
#include "step_defs.h"
#include "step_math.h"

namespace dmc {
// ---- narrow phase: one routine per pair of geom types (StepCore::narrow_phase dispatches) -------------
template <typename T> DMC_DEV void make_frame(T* f) {
  normalize3(f);
  if (t_sqrt(dot3(f + 3, f + 3)) < (T)0.5) {
    f[3] = f[4] = f[5] = 0;
    if (f[1] < (T)0.5 && f[1] > (T)-0.5) f[4] = 1; else f[5] = 1;
  }
  T t = dot3(f, f + 3);
  f[3] -= t*f[0]; f[4] -= t*f[1]; f[5] -= t*f[2];
  normalize3(f + 3);
  cross3(f + 6, f, f + 3);
}
template <typename T> struct Hit { T dist, pos[3], nrm[3]; };
template <typename T> DMC_DEV int plane_sphere(Hit<T>* h, T margin, const T* ppos, const T* nrm, const T* spos, T radius) {
  T dif[3] = {spos[0] - ppos[0], spos[1] - ppos[1], spos[2] - ppos[2]};
  T dist = dot3(dif, nrm) - radius;
  if (dist > margin) return 0;
  h->dist = dist;
  for (int k = 0; k < 3; k++) { h->pos[k] = spos[k] - nrm[k]*(radius + dist*(T)0.5); h->nrm[k] = nrm[k]; }
  return 1;
}
template <typename T> DMC_DEV int sphere_sphere(Hit<T>* h, T margin, const T* p1, T r1, const T* p2, T r2) {
  T dif[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  T cdist = t_sqrt(dot3(dif, dif));
  T dist = cdist - r1 - r2;
  if (dist > margin) return 0;
  T n[3];
  if (cdist < (T)DMC_MINVAL) { n[0] = 1; n[1] = n[2] = 0; } else { n[0] = dif[0]/cdist; n[1] = dif[1]/cdist; n[2] = dif[2]/cdist; }
  h->dist = dist;
  for (int k = 0; k < 3; k++) { h->pos[k] = p1[k] + n[k]*(r1 + dist*(T)0.5); h->nrm[k] = n[k]; }
  return 1;
}
// h[n] = x with every slot index a compile-time constant, so that the hit
// buffer stays in registers (a dynamically indexed local array lives in scratch)
template <typename T> struct Hits { Hit<T> s0, s1, s2, s3; };
template <typename T> DMC_DEV void sel_hit(Hit<T>& d, const Hit<T>& x, bool c) {
  d.dist = c ? x.dist : d.dist;
  for (int k = 0; k < 3; k++) { d.pos[k] = c ? x.pos[k] : d.pos[k]; d.nrm[k] = c ? x.nrm[k] : d.nrm[k]; }
}
template <typename T> DMC_DEV void put_hit(Hits<T>* h, int n, const Hit<T>& x) {
  sel_hit(h->s0, x, n == 0); sel_hit(h->s1, x, n == 1); sel_hit(h->s2, x, n == 2); sel_hit(h->s3, x, n == 3);
}
// ---- ellipsoid pairs: signed distance = max over unit n of the support-function gap F(n),
// Newton iteration on the unit sphere; a capsule is its swept sphere minimised over the axis
// parameter (regula falsi on n.axis).  Same iteration, same operation order as the oracle's
// "ellipsoid pairs" section; everything lives in registers (constant indexing only).
template <typename T> struct Quadric { T c[3], R[9], s[3]; };
template <typename T> DMC_DEV constexpr T ccd_tol() { return sizeof(T) == 8 ? (T)1e-10 : (T)1e-4; }
template <typename T> DMC_DEV constexpr int ccd_maxit() { return sizeof(T) == 8 ? 30 : 12; }
template <typename T> DMC_DEV T quadric_support(const Quadric<T>& q, const T* n, T* g, T* wh) {
  T w[3];
  for (int k = 0; k < 3; k++) w[k] = q.s[k]*(q.R[k]*n[0] + q.R[3 + k]*n[1] + q.R[6 + k]*n[2]);
  const T wn = t_sqrt(dot3(w, w));
  if (wn < (T)DMC_MINVAL) { g[0] = g[1] = g[2] = 0; wh[0] = wh[1] = wh[2] = 0; return 0; }
  T v[3];
  for (int k = 0; k < 3; k++) { wh[k] = w[k]/wn; v[k] = q.s[k]*wh[k]; }
  mul_mat_vec3(g, q.R, v);
  return wn;
}
template <typename T> DMC_DEV void quadric_curv(const Quadric<T>& q, const T* wh, T wn, const T* t1, const T* t2, T* K) {
  if (wn < (T)DMC_MINVAL) return;
  T y1[3], y2[3];
  for (int k = 0; k < 3; k++) {
    y1[k] = q.s[k]*(q.R[k]*t1[0] + q.R[3 + k]*t1[1] + q.R[6 + k]*t1[2]);
    y2[k] = q.s[k]*(q.R[k]*t2[0] + q.R[3 + k]*t2[1] + q.R[6 + k]*t2[2]);
  }
  const T a1 = dot3(y1, wh), a2 = dot3(y2, wh);
  K[0] += (dot3(y1, y1) - a1*a1)/wn; K[1] += (dot3(y1, y2) - a1*a2)/wn; K[2] += (dot3(y2, y2) - a2*a2)/wn;
}
template <typename T> DMC_DEV T quadric_gap_value(const Quadric<T>& A, const Quadric<T>& B, const T* n) {
  T g[3], wh[3], d[3] = {B.c[0] - A.c[0], B.c[1] - A.c[1], B.c[2] - A.c[2]};
  const T hA = quadric_support(A, n, g, wh), hB = quadric_support(B, n, g, wh);
  return dot3(n, d) - hA - hB;
}
template <typename T> DMC_DEV T quadric_gap(const Quadric<T>& A, const Quadric<T>& B, T* n, T* gA, T* gB) {
  const T d[3] = {B.c[0] - A.c[0], B.c[1] - A.c[1], B.c[2] - A.c[2]};
  T F = 0;
  for (int it = 0; ; it++) {
    T wA[3], wB[3];
    const T hA = quadric_support(A, n, gA, wA), hB = quadric_support(B, n, gB, wB);
    F = dot3(n, d) - hA - hB;
    if (it >= ccd_maxit<T>()) break;
    T f[9] = {n[0], n[1], n[2], 0, 0, 0, 0, 0, 0};
    make_frame(f);
    const T *t1 = f + 3, *t2 = f + 6;
    const T grad[3] = {d[0] - gA[0] - gB[0], d[1] - gA[1] - gB[1], d[2] - gA[2] - gB[2]};
    const T g1 = dot3(t1, grad), g2 = dot3(t2, grad);
    T K[3] = {F, 0, F};
    quadric_curv(A, wA, hA, t1, t2, K); quadric_curv(B, wB, hB, t1, t2, K);
    const T tr = K[0] + K[2];
    T det = K[0]*K[2] - K[1]*K[1];
    const T floor_ = (T)1e-3*(hA + hB) + (T)DMC_MINVAL;
    const T lmin = (T)0.5*(tr - t_sqrt(t_max((T)0, tr*tr - 4*det)));
    if (lmin < floor_) { const T sh = floor_ - lmin; K[0] += sh; K[2] += sh; det = K[0]*K[2] - K[1]*K[1]; }
    T d1 = (K[2]*g1 - K[1]*g2)/det, d2 = (K[0]*g2 - K[1]*g1)/det;
    if (d1*d1 + d2*d2 < ccd_tol<T>()*ccd_tol<T>()) break;
    T nn[3];
    for (int ls = 0; ; ls++) {
      for (int k = 0; k < 3; k++) nn[k] = n[k] + t1[k]*d1 + t2[k]*d2;
      normalize3(nn);
      if (ls >= 8 || quadric_gap_value(A, B, nn) >= F) break;
      d1 *= (T)0.5; d2 *= (T)0.5;
    }
    n[0] = nn[0]; n[1] = nn[1]; n[2] = nn[2];
  }
  return F;
}
template <typename T> DMC_DEV void quadric_init_dir(const Quadric<T>& A, const Quadric<T>& B, T* n) {
  for (int k = 0; k < 3; k++) n[k] = B.c[k] - A.c[k];
  if (dot3(n, n) < (T)DMC_MINVAL*(T)DMC_MINVAL) { n[0] = 1; n[1] = n[2] = 0; }
  normalize3(n);
}
template <typename T> DMC_DEV int quadric_contact(Hit<T>* h, T margin, const Quadric<T>& A, const Quadric<T>& B, T* n) {
  T gA[3], gB[3];
  const T dist = quadric_gap(A, B, n, gA, gB);
  if (dist > margin) return 0;
  h->dist = dist;
  for (int k = 0; k < 3; k++) { h->pos[k] = (T)0.5*((A.c[k] + gA[k]) + (B.c[k] - gB[k])); h->nrm[k] = n[k]; }
  return 1;
}
template <typename T> DMC_DEV Quadric<T> make_quadric(int type, const T* pos, const T* mat, const T* size) {
  Quadric<T> q;
  for (int k = 0; k < 3; k++) { q.c[k] = pos[k]; q.s[k] = type == DMC_GEOM_ELLIPSOID ? size[k] : size[0]; }
  for (int k = 0; k < 9; k++) q.R[k] = mat[k];
  return q;
}
// geom 2 is an ellipsoid; geom 1 a plane-less partner (sphere, capsule or ellipsoid)
template <typename T> DMC_DEV int ellipsoid_pair(Hit<T>* h, T margin, int t1, const T* p1, const T* m1, const T* s1,
                                  const T* p2, const T* m2, const T* s2) {
  Quadric<T> A = make_quadric(t1 == DMC_GEOM_CAPSULE ? DMC_GEOM_SPHERE : t1, p1, m1, s1);
  const Quadric<T> B = make_quadric(DMC_GEOM_ELLIPSOID, p2, m2, s2);
  T n[3];
  if (t1 != DMC_GEOM_CAPSULE) { quadric_init_dir(A, B, n); return quadric_contact(h, margin, A, B, n); }
  const T u[3] = {m1[2], m1[5], m1[8]};
  const T hl = s1[1];
  T gA[3], gB[3];
  T tlo = -hl, thi = hl, plo, phi = 0, t;
  for (int k = 0; k < 3; k++) A.c[k] = p1[k] + u[k]*tlo;
  quadric_init_dir(A, B, n);
  quadric_gap(A, B, n, gA, gB); plo = dot3(n, u);
  if (plo <= 0) t = tlo;
  else {
    for (int k = 0; k < 3; k++) A.c[k] = p1[k] + u[k]*thi;
    quadric_gap(A, B, n, gA, gB); phi = dot3(n, u);
    if (phi >= 0) t = thi;
    else {
      t = 0;
      int side = 0;
      for (int it = 0; it < 40; it++) {
        t = (tlo*phi - thi*plo)/(phi - plo);
        for (int k = 0; k < 3; k++) A.c[k] = p1[k] + u[k]*t;
        quadric_gap(A, B, n, gA, gB);
        const T pt = dot3(n, u);
        if (t_abs(pt) < ccd_tol<T>() || thi - tlo < ccd_tol<T>()*hl) break;
        if (pt > 0) { tlo = t; plo = pt; if (side == 1) phi *= (T)0.5; side = 1; }
        else { thi = t; phi = pt; if (side == -1) plo *= (T)0.5; side = -1; }
      }
    }
  }
  for (int k = 0; k < 3; k++) A.c[k] = p1[k] + u[k]*t;
  return quadric_contact(h, margin, A, B, n);
}
template <typename T> DMC_DEV int plane_ellipsoid(Hit<T>* h, T margin, const T* p1, const T* nrm, const T* p2, const T* m2, const T* s2) {
  const Quadric<T> q = make_quadric(DMC_GEOM_ELLIPSOID, p2, m2, s2);
  T g[3], wh[3];
  quadric_support(q, nrm, g, wh);
  const T pt[3] = {p2[0] - g[0], p2[1] - g[1], p2[2] - g[2]};
  const T dif[3] = {pt[0] - p1[0], pt[1] - p1[1], pt[2] - p1[2]};
  const T dist = dot3(dif, nrm);
  if (dist > margin) return 0;
  h->dist = dist;
  for (int k = 0; k < 3; k++) { h->pos[k] = pt[k] - nrm[k]*dist*(T)0.5; h->nrm[k] = nrm[k]; }
  return 1;
}
// ---- box pairs (sphere-box, capsule-box, box-box): same constructions, same operation order as the
// oracle's "box pairs" section.  The clipping polygon is a dynamically indexed local array (scratch
// memory); the code is compiled out of models without such pairs (d.nbox == 0).
template <typename T> DMC_DEV int sphere_box_core(Hit<T>* h, T margin, const T* ps, T r, const T* pb, const T* mb, const T* sb) {
  T dif[3] = {ps[0] - pb[0], ps[1] - pb[1], ps[2] - pb[2]}, cl[3], q[3], nb[3] = {0, 0, 0};
  mul_matT_vec3(cl, mb, dif);
  bool outside = false;
  for (int k = 0; k < 3; k++) { q[k] = t_max(-sb[k], t_min(sb[k], cl[k])); if (q[k] != cl[k]) outside = true; }
  T dist;
  if (outside) {
    const T d[3] = {cl[0] - q[0], cl[1] - q[1], cl[2] - q[2]};
    const T dn = t_sqrt(dot3(d, d));
    dist = dn - r;
    if (dist > margin) return 0;
    for (int k = 0; k < 3; k++) nb[k] = d[k]/dn;
  } else {
    const T d0 = sb[0] - t_abs(cl[0]), d1 = sb[1] - t_abs(cl[1]), d2 = sb[2] - t_abs(cl[2]);
    int best = 0; T depth = d0;
    if (d1 < depth) { depth = d1; best = 1; }
    if (d2 < depth) { depth = d2; best = 2; }
    for (int k = 0; k < 3; k++) if (k == best) { nb[k] = cl[k] >= 0 ? (T)1 : (T)-1; q[k] = nb[k]*sb[k]; }
    dist = -depth - r;
  }
  T nw[3], qw[3];
  mul_mat_vec3(nw, mb, nb); mul_mat_vec3(qw, mb, q);
  h->dist = dist;
  for (int k = 0; k < 3; k++) { h->pos[k] = pb[k] + qw[k] + nw[k]*dist*(T)0.5; h->nrm[k] = -nw[k]; }
  return 1;
}
template <typename T> DMC_DEV T seg_box_dd(const T* p0, const T* u, const T* sb, T t, T* deriv) {
  T f = 0, g = 0;
  for (int k = 0; k < 3; k++) {
    const T x = p0[k] + t*u[k], e = x - t_max(-sb[k], t_min(sb[k], x));
    f += e*e; g += 2*e*u[k];
  }
  *deriv = g;
  return f;
}
template <typename T> DMC_DEV int capsule_box(Hits<T>* hs, T margin, const T* p1, const T* m1, const T* s1, const T* p2, const T* m2, const T* s2) {
  const T axw[3] = {m1[2], m1[5], m1[8]}, dif[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
  T p0[3], u[3];
  mul_matT_vec3(p0, m2, dif); mul_matT_vec3(u, m2, axw);
  const T hl = s1[1];
  T lo = -hl, hi = hl, g, t;
  seg_box_dd(p0, u, s2, lo, &g);
  if (g >= 0) t = lo;
  else {
    seg_box_dd(p0, u, s2, hi, &g);
    if (g <= 0) t = hi;
    else {
      for (int it = 0; it < (sizeof(T) == 8 ? 60 : 30); it++) { t = (T)0.5*(lo + hi); seg_box_dd(p0, u, s2, t, &g); if (g > 0) hi = t; else lo = t; }
      t = (T)0.5*(lo + hi);
    }
  }
  int mask = 0;
  T ps[3];
  for (int k = 0; k < 3; k++) ps[k] = p1[k] + axw[k]*t;
  mask |= sphere_box_core(&hs->s0, margin, ps, s1[0], p2, m2, s2);
  const T t2 = t <= 0 ? hl : -hl;
  if (t_abs(t2 - t) > (T)1e-3*hl) {
    for (int k = 0; k < 3; k++) ps[k] = p1[k] + axw[k]*t2;
    Hit<T> x;
    if (sphere_box_core(&x, margin, ps, s1[0], p2, m2, s2)) { put_hit(hs, mask & 1, x); mask = (mask << 1) | 1; }
  }
  return mask;
}
template <typename T> DMC_DEV int box_box(Hits<T>* hs, T margin, const T* pA, const T* RA, const T* sA, const T* pB, const T* RB, const T* sB) {
  const T d[3] = {pB[0] - pA[0], pB[1] - pA[1], pB[2] - pA[2]};
  T colA[3][3], colB[3][3];
  for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) { colA[i][k] = RA[3*k + i]; colB[i][k] = RB[3*k + i]; }
  T best = (T)-1e30; int code = -1; T bestn[3] = {0, 0, 0};
  for (int i = 0; i < 6; i++) {
    T L[3];
    for (int k = 0; k < 3; k++) L[k] = i < 3 ? colA[i % 3][k] : colB[i % 3][k];
    T ra = 0, rb = 0;
    for (int k = 0; k < 3; k++) { ra += sA[k]*t_abs(dot3(L, colA[k])); rb += sB[k]*t_abs(dot3(L, colB[k])); }
    const T proj = dot3(L, d), sep = t_abs(proj) - ra - rb;
    if (sep > margin) return 0;
    if (sep > best) { best = sep; code = i; for (int k = 0; k < 3; k++) bestn[k] = proj >= 0 ? L[k] : -L[k]; }
  }
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
    T L[3];
    cross3(L, colA[i], colB[j]);
    const T ln = t_sqrt(dot3(L, L));
    if (ln < (T)1e-6) continue;
    for (int k = 0; k < 3; k++) L[k] /= ln;
    T ra = 0, rb = 0;
    for (int k = 0; k < 3; k++) { ra += sA[k]*t_abs(dot3(L, colA[k])); rb += sB[k]*t_abs(dot3(L, colB[k])); }
    const T proj = dot3(L, d), sep = t_abs(proj) - ra - rb;
    if (sep > margin) return 0;
    if (sep > 0 ? sep > best : sep*(T)1.05 > best) {
      if (!(sep > 0) && !(best < 0)) continue;
      best = sep; code = 6 + 3*i + j; for (int k = 0; k < 3; k++) bestn[k] = proj >= 0 ? L[k] : -L[k];
    }
  }
  if (code >= 6) {
    const int i = (code - 6)/3, j = (code - 6) % 3;
    T pa[3] = {pA[0], pA[1], pA[2]}, pb[3] = {pB[0], pB[1], pB[2]};
    for (int k = 0; k < 3; k++) if (k != i) { const T sg = dot3(bestn, colA[k]) > 0 ? (T)1 : (T)-1; for (int a = 0; a < 3; a++) pa[a] += sg*sA[k]*colA[k][a]; }
    for (int k = 0; k < 3; k++) if (k != j) { const T sg = dot3(bestn, colB[k]) > 0 ? (T)-1 : (T)1; for (int a = 0; a < 3; a++) pb[a] += sg*sB[k]*colB[k][a]; }
    T ua[3], ub[3];
    for (int k = 0; k < 3; k++) { ua[k] = colA[i][k]; ub[k] = colB[j][k]; }
    const T w[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
    const T uaub = dot3(ua, ub), q1 = dot3(ua, w), q2 = -dot3(ub, w), den = 1 - uaub*uaub;
    T alpha = 0, beta = 0;
    if (den > (T)1e-12) { alpha = (q1 + uaub*q2)/den; beta = (uaub*q1 + q2)/den; }
    alpha = t_max(-sA[i], t_min(sA[i], alpha)); beta = t_max(-sB[j], t_min(sB[j], beta));
    hs->s0.dist = best;
    for (int k = 0; k < 3; k++) { hs->s0.pos[k] = (T)0.5*((pa[k] + alpha*ua[k]) + (pb[k] + beta*ub[k])); hs->s0.nrm[k] = bestn[k]; }
    return 1;
  }
  const bool refA = code < 3;
  T pR[3], sR[3], pI[3], sI[3], cR[3][3], cI[3][3], nref[3];
  for (int k = 0; k < 3; k++) {
    pR[k] = refA ? pA[k] : pB[k]; sR[k] = refA ? sA[k] : sB[k]; pI[k] = refA ? pB[k] : pA[k]; sI[k] = refA ? sB[k] : sA[k];
    nref[k] = refA ? bestn[k] : -bestn[k];
    for (int a = 0; a < 3; a++) { cR[k][a] = refA ? colA[k][a] : colB[k][a]; cI[k][a] = refA ? colB[k][a] : colA[k][a]; }
  }
  const int ax = refA ? code : code - 3;
  int inc = 0; T incdot = (T)1e30;
  for (int k = 0; k < 3; k++) { const T dk = dot3(nref, cI[k]); if (-t_abs(dk) < incdot) { incdot = -t_abs(dk); inc = k; } }
  const T incsign = dot3(nref, cI[inc]) > 0 ? (T)-1 : (T)1;
  const int i1 = (inc + 1) % 3, i2 = (inc + 2) % 3, r1 = (ax + 1) % 3, r2 = (ax + 2) % 3;
  // (a quad clipped by four half-planes has at most eight vertices: each clip of a convex polygon adds at most one.  The
  // arrays are indexed at run time, i.e. they live in scratch memory: 2 x 8 x 3 reals, half of what 16 slots took; the
  // guards below only matter if rounding ever made a clipped polygon non-convex)
  T poly[8][3], tmp[8][3];
  int np_ = 4;
  for (int v = 0; v < 4; v++) {
    const T a = (v == 0 || v == 3) ? (T)1 : (T)-1, b = v < 2 ? (T)1 : (T)-1;
    T pt[3];
    for (int k = 0; k < 3; k++) pt[k] = pI[k] + incsign*sI[inc]*cI[inc][k] + a*sI[i1]*cI[i1][k] + b*sI[i2]*cI[i2][k] - pR[k];
    poly[v][0] = dot3(pt, cR[r1]); poly[v][1] = dot3(pt, cR[r2]); poly[v][2] = dot3(pt, nref) - sR[ax];
  }
  for (int side = 0; side < 4 && np_ > 0; side++) {
    const int coord = side >> 1; const T sg = (side & 1) ? (T)-1 : (T)1, lim = coord ? sR[r2] : sR[r1];
    int nn = 0;
    for (int v = 0; v < np_; v++) {
      const T* P = poly[v]; const T* Q = poly[(v + 1) % np_];
      const T dp = lim - sg*P[coord], dq = lim - sg*Q[coord];
      if (dp >= 0 && nn < 8) { tmp[nn][0] = P[0]; tmp[nn][1] = P[1]; tmp[nn][2] = P[2]; nn++; }
      if ((dp >= 0) != (dq >= 0) && nn < 8) { const T f = dp/(dp - dq); for (int k = 0; k < 3; k++) tmp[nn][k] = P[k] + f*(Q[k] - P[k]); nn++; }
    }
    np_ = nn;
    for (int v = 0; v < np_; v++) for (int k = 0; k < 3; k++) poly[v][k] = tmp[v][k];
  }
  int nk = 0;
  for (int v = 0; v < np_; v++) if (poly[v][2] <= margin) { for (int k = 0; k < 3; k++) poly[nk][k] = poly[v][k]; nk++; }
  if (!nk) return 0;
  int pick[4] = {0, 0, 0, 0}, npick = 0;
  if (nk <= 4) { for (int v = 0; v < nk; v++) pick[npick++] = v; }
  else {
    T cx = 0, cy = 0; int deep = 0;
    for (int v = 0; v < nk; v++) { cx += poly[v][0]; cy += poly[v][1]; if (poly[v][2] < poly[deep][2]) deep = v; }
    cx /= nk; cy /= nk;
    const T PI = (T)3.14159265358979323846;
    const T a0 = t_atan2(poly[deep][1] - cy, poly[deep][0] - cx);
    int used = 1 << deep;
    pick[npick++] = deep;
    for (int q = 1; q < 4; q++) {
      const T target = a0 + q*(PI/2);
      int bv = -1; T bd = (T)1e30;
      for (int v = 0; v < nk; v++) if (!((used >> v) & 1)) {
        const T da = t_abs(t_fmod(t_atan2(poly[v][1] - cy, poly[v][0] - cx) - target + 5*PI, 2*PI) - PI);
        if (da < bd) { bd = da; bv = v; }
      }
      pick[npick++] = bv; used |= 1 << bv;
    }
  }
  for (int q = 0; q < npick; q++) {
    const T* P = poly[pick[q]];
    Hit<T> x;
    x.dist = P[2];
    for (int k = 0; k < 3; k++) { x.pos[k] = pR[k] + P[0]*cR[r1][k] + P[1]*cR[r2][k] + (sR[ax] + (T)0.5*P[2])*nref[k]; x.nrm[k] = bestn[k]; }
    put_hit(hs, q, x);
  }
  return (1 << npick) - 1;
}
// ---- sphere / capsule against a cylinder (the oracle's point_cylinder / sphere_cylinder_core / collide_capsule_cylinder) ----
// closest point of the SOLID cylinder (centre p, unit axis a, radius R, half-height H) to q; returns the distance
template <typename T> DMC_DEV T point_cylinder(const T* q, const T* p, const T* a, T R, T H, T* closest) {
  const T v[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
  const T x = dot3(v, a), perp[3] = {v[0] - x*a[0], v[1] - x*a[1], v[2] - x*a[2]};
  const T d = t_sqrt(dot3(perp, perp)), xc = t_max(-H, t_min(H, x)), sc = d > R ? R/d : (T)1;
  for (int k = 0; k < 3; k++) closest[k] = p[k] + xc*a[k] + sc*perp[k];
  const T dif[3] = {q[0] - closest[0], q[1] - closest[1], q[2] - closest[2]};
  return t_sqrt(dot3(dif, dif));
}
template <typename T> DMC_DEV int sphere_cylinder_core(Hit<T>* hit, T margin, const T* ps, T rs, const T* p2, const T* m2, const T* s2) {
  const T a[3] = {m2[2], m2[5], m2[8]}, R = s2[0], H = s2[1];
  T closest[3], n[3], dist;
  const T g = point_cylinder(ps, p2, a, R, H, closest);
  const T v[3] = {ps[0] - p2[0], ps[1] - p2[1], ps[2] - p2[2]};
  const T x = dot3(v, a), perp[3] = {v[0] - x*a[0], v[1] - x*a[1], v[2] - x*a[2]}, d = t_sqrt(dot3(perp, perp));
  // the centre inside the solid is told from its coordinates: g is then the rounding noise of p + x a + perp - q, in
  // fp32 some 1e-8 and far above DMC_MINVAL (a normal made of noise, dist = -rs)
  const bool inside = t_abs(x) <= H && d <= R;
  if (!inside && g >= (T)DMC_MINVAL) {
    dist = g - rs;
    for (int k = 0; k < 3; k++) n[k] = (closest[k] - ps[k]) / g;
  } else {      // centre inside the solid: out through the nearest face
    if (H - t_abs(x) < R - d) { dist = -(H - t_abs(x)) - rs; for (int k = 0; k < 3; k++) n[k] = x >= 0 ? -a[k] : a[k]; }
    else {
      dist = -(R - d) - rs;
      if (d < (T)DMC_MINVAL) { n[0] = 1; n[1] = n[2] = 0; } else for (int k = 0; k < 3; k++) n[k] = -perp[k] / d;
    }
  }
  if (dist > margin) return 0;
  hit->dist = dist;
  for (int k = 0; k < 3; k++) { hit->pos[k] = ps[k] + n[k]*(rs + dist*(T)0.5); hit->nrm[k] = n[k]; }
  return 1;
}
// slope of the point-to-cylinder distance along the capsule axis at p1 + t u (nondecreasing in t)
template <typename T> DMC_DEV T segment_slope(T t, const T* p1, const T* u, const T* p2, const T* a, T R, T H) {
  const T q[3] = {p1[0] + t*u[0], p1[1] + t*u[1], p1[2] + t*u[2]};
  T closest[3];
  const T g = point_cylinder(q, p2, a, R, H, closest);
  if (g < (T)DMC_MINVAL) return 0;
  return ((q[0] - closest[0])*u[0] + (q[1] - closest[1])*u[1] + (q[2] - closest[2])*u[2]) / g;
}
template <typename T> DMC_DEV T slope_crossing(T thr, T h, const T* p1, const T* u, const T* p2, const T* a, T R, T H) {
  if (segment_slope(-h, p1, u, p2, a, R, H) > thr) return -h;
  if (!(segment_slope(h, p1, u, p2, a, R, H) > thr)) return h;
  T lo = -h, hi = h;
  for (int it = 0; it < (sizeof(T) == 4 ? 28 : 60); it++) {
    const T t = (T)0.5*(lo + hi);
    if (segment_slope(t, p1, u, p2, a, R, H) > thr) hi = t; else lo = t;
  }
  return (T)0.5*(lo + hi);
}
// returns 0 / 1 contacts, or -1 when the capsule's axis reaches the cylinder (no unique closest pair: the caller warns)
template <typename T> DMC_DEV int capsule_cylinder(Hit<T>* hit, T margin, const T* p1, const T* m1, const T* s1, const T* p2, const T* m2, const T* s2) {
  const T u[3] = {m1[2], m1[5], m1[8]}, a[3] = {m2[2], m2[5], m2[8]};
  const T tol = sizeof(T) == 4 ? (T)1e-4 : (T)1e-7;
  const T ta = slope_crossing(-tol, s1[1], p1, u, p2, a, s2[0], s2[1]);
  const T tb = slope_crossing(tol, s1[1], p1, u, p2, a, s2[0], s2[1]);
  const T t = (T)0.5*(ta + tb);
  const T q[3] = {p1[0] + t*u[0], p1[1] + t*u[1], p1[2] + t*u[2]};
  T closest[3];
  if (point_cylinder(q, p2, a, s2[0], s2[1], closest) < (sizeof(T) == 4 ? (T)1e-5 : (T)1e-9)*(s2[0] + s2[1])) return -1;
  return sphere_cylinder_core(hit, margin, q, s1[0], p2, m2, s2);
}
// ray (pnt, vec) against a site volume in its own frame; distance or -1
template <typename T> DMC_DEV T ray_geom(const T* pos, const T* mat, const T* size, const T* pnt, const T* vec, int type) {
  T dif[3] = {pnt[0] - pos[0], pnt[1] - pos[1], pnt[2] - pos[2]}, lp[3], lv[3];
  mul_matT_vec3(lp, mat, dif); mul_matT_vec3(lv, mat, vec);
  T best = -1;
  if (type == DMC_GEOM_SPHERE || type == DMC_GEOM_CAPSULE) {
    const T r = size[0];
    const int nparts = type == DMC_GEOM_CAPSULE ? 3 : 1;
    for (int part = 0; part < nparts; part++) {
      T a, b, c;
      if (type == DMC_GEOM_CAPSULE && part == 0) {
        a = lv[0]*lv[0] + lv[1]*lv[1]; b = lp[0]*lv[0] + lp[1]*lv[1]; c = lp[0]*lp[0] + lp[1]*lp[1] - r*r;
      } else {
        const T cz = type == DMC_GEOM_CAPSULE ? (part == 1 ? size[1] : -size[1]) : (T)0;
        T q[3] = {lp[0], lp[1], lp[2] - cz};
        a = dot3(lv, lv); b = dot3(q, lv); c = dot3(q, q) - r*r;
      }
      if (a < (T)DMC_MINVAL) continue;
      const T det = b*b - a*c;
      if (det < 0) continue;
      const T sq = t_sqrt(det);
      for (int k = 0; k < 2; k++) {
        const T x = k == 0 ? (-b - sq)/a : (-b + sq)/a;
        if (x < 0) continue;
        const T z = lp[2] + x*lv[2];
        if (type == DMC_GEOM_CAPSULE) {
          if (part == 0 && t_abs(z) > size[1]) continue;
          if (part == 1 && z < size[1]) continue;
          if (part == 2 && z > -size[1]) continue;
        }
        if (best < 0 || x < best) best = x;
      }
    }
    return best;
  }
  if (type == DMC_GEOM_ELLIPSOID) {
    T q[3] = {lp[0]/size[0], lp[1]/size[1], lp[2]/size[2]}, w[3] = {lv[0]/size[0], lv[1]/size[1], lv[2]/size[2]};
    const T a = dot3(w, w), b = dot3(q, w), c = dot3(q, q) - 1;
    if (a < (T)DMC_MINVAL) return -1;
    const T det = b*b - a*c;
    if (det < 0) return -1;
    const T sq = t_sqrt(det), x0 = (-b - sq)/a, x1 = (-b + sq)/a;
    return x0 >= 0 ? x0 : (x1 >= 0 ? x1 : (T)-1);
  }
  if (type == DMC_GEOM_BOX) {
    if (t_abs(lp[0]) <= size[0] && t_abs(lp[1]) <= size[1] && t_abs(lp[2]) <= size[2]) return 0;
    for (int ax = 0; ax < 3; ax++) {
      if (t_abs(lv[ax]) < (T)DMC_MINVAL) continue;
      for (int sg = -1; sg <= 1; sg += 2) {
        const T x = (sg*size[ax] - lp[ax]) / lv[ax];
        if (x < 0) continue;
        const int a1 = (ax + 1) % 3, a2 = (ax + 2) % 3;
        if (t_abs(lp[a1] + x*lv[a1]) <= size[a1] && t_abs(lp[a2] + x*lv[a2]) <= size[a2])
          if (best < 0 || x < best) best = x;
      }
    }
    return best;
  }
  return -1;
}
// rays of rangefinder sensors: every geom type (planes are front-side only and finite where their
// half-sizes are positive; a ray that starts inside a box leaves through a face)
template <typename T> DMC_DEV T ray_geom_any(const T* pos, const T* mat, const T* size, const T* pnt, const T* vec, int type) {
  if (type != DMC_GEOM_PLANE && type != DMC_GEOM_CYLINDER && type != DMC_GEOM_BOX) return ray_geom(pos, mat, size, pnt, vec, type);
  T dif[3] = {pnt[0] - pos[0], pnt[1] - pos[1], pnt[2] - pos[2]}, lp[3], lv[3];
  mul_matT_vec3(lp, mat, dif); mul_matT_vec3(lv, mat, vec);
  T best = -1;
  if (type == DMC_GEOM_PLANE) {
    if (lv[2] > -(T)DMC_MINVAL) return -1;
    const T x = -lp[2]/lv[2];
    if (x < 0) return -1;
    const T px = lp[0] + x*lv[0], py = lp[1] + x*lv[1];
    if ((size[0] <= 0 || t_abs(px) <= size[0]) && (size[1] <= 0 || t_abs(py) <= size[1])) return x;
    return -1;
  }
  if (type == DMC_GEOM_CYLINDER) {
    const T a = lv[0]*lv[0] + lv[1]*lv[1], b = lp[0]*lv[0] + lp[1]*lv[1], c = lp[0]*lp[0] + lp[1]*lp[1] - size[0]*size[0];
    if (a >= (T)DMC_MINVAL) {
      const T det = b*b - a*c;
      if (det >= 0) {
        const T sq = t_sqrt(det);
        for (int k = 0; k < 2; k++) {
          const T x = k == 0 ? (-b - sq)/a : (-b + sq)/a;
          if (x >= 0 && t_abs(lp[2] + x*lv[2]) <= size[1]) if (best < 0 || x < best) best = x;
        }
      }
    }
    if (t_abs(lv[2]) >= (T)DMC_MINVAL) for (int sg = -1; sg <= 1; sg += 2) {
      const T x = (sg*size[1] - lp[2]) / lv[2];
      if (x < 0) continue;
      const T px = lp[0] + x*lv[0], py = lp[1] + x*lv[1];
      if (px*px + py*py <= size[0]*size[0]) if (best < 0 || x < best) best = x;
    }
    return best;
  }
  for (int ax = 0; ax < 3; ax++) {
    if (t_abs(lv[ax]) < (T)DMC_MINVAL) continue;
    for (int sg = -1; sg <= 1; sg += 2) {
      const T x = (sg*size[ax] - lp[ax]) / lv[ax];
      if (x < 0) continue;
      const int a1 = (ax + 1) % 3, a2 = (ax + 2) % 3;
      if (t_abs(lp[a1] + x*lv[a1]) <= size[a1] && t_abs(lp[a2] + x*lv[a2]) <= size[a2])
        if (best < 0 || x < best) best = x;
    }
  }
  return best;
}
}  // namespace dmc
