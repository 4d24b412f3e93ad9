// dyn_core.h -- batched rigid-body dynamics of ONE environment: mj_crb + mj_fullM (the dense joint-space inertia M), mj_mulM
// (M v), mj_solveM (M^-1 f) and mj_rne (bias forces, inverse dynamics), as free function templates on the real type.  The
// same text builds for the device (dyn_kernels.hip) and for the host (tests/emu/dyn_emu.cpp, DMC_HOST_EMU).
//
// An environment is worked on by a group of W lanes.  Every function here is a sequence of PHASES; a phase is a set of
// independent items (a body, a dof, a matrix element ...), and an executor `par` hands them to the lanes:
//
//     par.run(n, [&](int item) { ... });      // every item once, by exactly one lane; a group-scope hand-off follows
//
// On the device the lanes of the group stride over the items and a wave-level fence ends the phase; the host build runs the
// lanes one after the other in the same item order.  An item reads only what EARLIER phases wrote and writes only its own
// elements, and every sum runs in a fixed order inside one item -- so the result does not depend on W, two launches give
// equal bits, and the fp64 kernels equal the host build bit for bit (no contraction; sine and cosine are jac_core.h's own).
//
// Only the kinematics need the tree level by level (a body's frame hangs off its parent's).  Everything else is a sum over
// a dof's ancestor path (dof_parent) or over a body's subtree (the host lists it), so it is one phase each:
//   kinematics   per level: body frames, every dof's world axis and anchor (mj_kinematics; jac_core.h's walk, body by body)
//   frames       per dof: cdof about the tree's reference point; per body: cinert about it (mj_comPos)
//   crb          per body: the composite inertia = the sum of cinert over its subtree; per dof i: M(i, j) for j on i's
//                ancestor path, plus armature (mj_crb, mj_fullM)
//   rne          per dof: cdof_dot; per body: cvel, cacc, the body force; per body: its subtree's sum; per dof: the
//                projection on cdof (mj_comVel, mj_rne)
//   factor       dense Cholesky M = L L', left-looking, a column per step; a pivot below DMC_MINVAL is replaced by it
//   solve        both substitutions column by column, every right-hand side of the chunk at once
//
// The reference point of a kinematic tree is the world position of its root body (PARITY_ASSUMPTIONS.md row 71): spatial
// quantities are exact about any point that is fixed at this instant, and the root is near everything that hangs off it.
#pragma once
#include "jac_core.h"
#include "step_defs.h"
#include "step_math.h"

namespace dmc {

constexpr int kDynMaxDof = 64;      // nv of a batch
constexpr int kDynBlock = 64;       // lanes per workgroup: one wave, 64 / W environments
constexpr int kDynChunk = 8;        // right-hand sides that pass through the workspace at once

// bodies (the world is body 0), joints, dofs, qpos entries, tree levels below the world, entries of the subtree lists
struct DynDims { int nb, nj, nv, nq, nlevel, nsub; };

// ints:  body_parent[nb] body_jntadr[nb] body_jntnum[nb] body_root[nb] body_lastdof[nb] sub_adr[nb + 1]
//        level_adr[nlevel + 1] level_body[nb - 1] jnt_type[nj] jnt_qadr[nj] jnt_dadr[nj]
//        dof_body[nv] dof_parent[nv] dof_pred[nv] dof_rot[nv] sub_body[nsub]
// reals: body_pos[3 nb] body_quat[4 nb] body_ipos[3 nb] body_iquat[4 nb] body_mass[nb] body_inertia[3 nb]
//        jnt_axis[3 nj] jnt_pos[3 nj] jnt_qpos0[nj] dof_armature[nv] gravity[3]
// (body_lastdof: the last dof on the body's path, -1: none; dof_pred: the last dof whose velocity the dof's axis is carried
// by -- its parent for a hinge or slide, the dof before the triple for a ball or a free joint's rotations; sub_body: every
// body's subtree, itself first, ascending; level_body: the bodies sorted by depth)
constexpr int dyn_nints(const DynDims& d) { return 6*d.nb + 1 + d.nlevel + 1 + d.nb - 1 + 3*d.nj + 4*d.nv + d.nsub; }
constexpr int dyn_nreals(const DynDims& d) { return 18*d.nb + 7*d.nj + d.nv + 3; }

template <typename T>
struct DynTab {
  DynDims d;
  const int *body_parent, *body_jntadr, *body_jntnum, *body_root, *body_lastdof, *sub_adr, *level_adr, *level_body, *jnt_type,
      *jnt_qadr, *jnt_dadr, *dof_body, *dof_parent, *dof_pred, *dof_rot, *sub_body;
  const T *body_pos, *body_quat, *body_ipos, *body_iquat, *body_mass, *body_inertia, *jnt_axis, *jnt_pos, *jnt_qpos0, *dof_armature,
      *gravity;
};
#ifdef DMC_HOST_EMU
#define DMC_DYN_HD inline
#else
#define DMC_DYN_HD __host__ __device__ __forceinline__      // (the entry points walk the same tables when they validate them)
#endif
template <typename T>
DMC_DYN_HD DynTab<T> dyn_tab(const DynDims& d, const int* i, const T* r) {
  DynTab<T> t;
  t.d = d;
  t.body_parent = i; i += d.nb; t.body_jntadr = i; i += d.nb; t.body_jntnum = i; i += d.nb; t.body_root = i; i += d.nb;
  t.body_lastdof = i; i += d.nb; t.sub_adr = i; i += d.nb + 1; t.level_adr = i; i += d.nlevel + 1; t.level_body = i; i += d.nb - 1;
  t.jnt_type = i; i += d.nj; t.jnt_qadr = i; i += d.nj; t.jnt_dadr = i; i += d.nj;
  t.dof_body = i; i += d.nv; t.dof_parent = i; i += d.nv; t.dof_pred = i; i += d.nv; t.dof_rot = i; i += d.nv; t.sub_body = i;
  t.body_pos = r; r += 3*d.nb; t.body_quat = r; r += 4*d.nb; t.body_ipos = r; r += 3*d.nb; t.body_iquat = r; r += 4*d.nb;
  t.body_mass = r; r += d.nb; t.body_inertia = r; r += 3*d.nb; t.jnt_axis = r; r += 3*d.nj; t.jnt_pos = r; r += 3*d.nj;
  t.jnt_qpos0 = r; r += d.nj; t.dof_armature = r; r += d.nv; t.gravity = r;
  return t;
}

// The workspace of one environment, offsets in reals.  kind 0 (mass_matrix, mul, solve): frames, crb, M, the chunk of
// right-hand sides and the chunk of results; kind 1 (bias, inverse): frames and the arrays of mj_rne.
struct DynLayout { int xpos, xquat, cinert, cdof, crb, M, dinv, rhs, res, qvel, qacc, cdd, cvel, cfrc, cfs, total; };
constexpr DynLayout dyn_layout(int nb, int nv, int kind) {
  DynLayout L = {};
  int o = 0;
  L.xpos = o; o += 3*nb; L.xquat = o; o += 4*nb; L.cinert = o; o += 10*nb; L.cdof = o; o += 6*nv;
  if (kind == 0) {
    L.crb = o; o += 10*nb; L.M = o; o += nv*nv; L.dinv = o; o += nv; L.rhs = o; o += kDynChunk*nv; L.res = o; o += kDynChunk*nv;
  } else {
    L.qvel = o; o += nv; L.qacc = o; o += nv; L.cdd = o; o += 6*nv; L.cvel = o; o += 6*nb; L.cfrc = o; o += 6*nb; L.cfs = o; o += 6*nb;
    L.res = o; o += nv;
  }
  L.total = (o + 1) & ~1;      // (an even number of reals: every environment's workspace starts on 16 bytes)
  return L;
}

// The kernels' static LDS arrays; which one the 64 / W workspaces of a workgroup fit (-1: none).
constexpr int kDynTiers = 3;
constexpr int kDynTierBytes[kDynTiers] = {16*1024, 32*1024, 64*1024};
constexpr int dyn_tier(int nb, int nv, int kind, int W, int real_bytes) {
  const long long need = (long long)dyn_layout(nb, nv, kind).total*(kDynBlock/W)*real_bytes;
  for (int k = 0; k < kDynTiers; k++) if (need <= kDynTierBytes[k]) return k;
  return -1;
}

template <typename T> DMC_DEV T dyn_dot6(const T* a, const T* b) {
  return a[0]*b[0] + a[1]*b[1] + a[2]*b[2] + a[3]*b[3] + a[4]*b[4] + a[5]*b[5];
}

// mj_kinematics of body b (its parent's frame is in the workspace): jac_walk's body step.  Leaves xpos / xquat and, in the
// cdof slots of the body's dofs, (world axis, anchor).
template <typename T, class Q>
DMC_DEV void dyn_body_kinematics(const DynTab<T>& t, T* ws, const DynLayout& L, Q q, int b) {
  const int p = t.body_parent[b], j0 = t.body_jntadr[b], jn = t.body_jntnum[b];
  T pos[3], quat[4], m[9], tv[3];
  for (int k = 0; k < 3; k++) pos[k] = ws[L.xpos + 3*p + k];
  for (int k = 0; k < 4; k++) quat[k] = ws[L.xquat + 4*p + k];
  auto emit = [&](int dof, const T* axis, const T* anchor) {
    T* c = ws + L.cdof + 6*dof;
    for (int k = 0; k < 3; k++) { c[k] = axis[k]; c[3 + k] = anchor[k]; }
  };
  T ballanchor[3] = {0, 0, 0};
  if (jn > 0 && t.jnt_type[j0] == DMC_JNT_FREE) {
    const int s = t.jnt_qadr[j0];
    for (int k = 0; k < 3; k++) pos[k] = q(s + k);
    for (int k = 0; k < 4; k++) quat[k] = q(s + 3 + k);
    normalize4(quat);
  } else {
    const T bp[3] = {t.body_pos[3*b], t.body_pos[3*b + 1], t.body_pos[3*b + 2]};
    const T bq[4] = {t.body_quat[4*b], t.body_quat[4*b + 1], t.body_quat[4*b + 2], t.body_quat[4*b + 3]};
    rot_vec_quat(tv, bp, quat);
    for (int k = 0; k < 3; k++) pos[k] += tv[k];
    mul_quat(quat, quat, bq);
    for (int j = j0; j < j0 + jn; j++) {
      const int type = t.jnt_type[j], s = t.jnt_qadr[j];
      const T a[3] = {t.jnt_axis[3*j], t.jnt_axis[3*j + 1], t.jnt_axis[3*j + 2]}, jp[3] = {t.jnt_pos[3*j], t.jnt_pos[3*j + 1], t.jnt_pos[3*j + 2]};
      T anchor[3], axis[3];
      quat2mat(m, quat);
      mul_mat_vec3(anchor, m, jp);
      for (int k = 0; k < 3; k++) anchor[k] += pos[k];
      mul_mat_vec3(axis, m, a);
      if (type == DMC_JNT_SLIDE) {
        const T x = q(s) - t.jnt_qpos0[j];
        for (int k = 0; k < 3; k++) pos[k] += axis[k]*x;
        emit(t.jnt_dadr[j], axis, anchor);
      } else {
        T ql[4];
        if (type == DMC_JNT_BALL) {
          for (int k = 0; k < 4; k++) ql[k] = q(s + k);
          normalize4(ql);
          for (int k = 0; k < 3; k++) ballanchor[k] = anchor[k];      // (its axes wait for the body's final orientation)
        } else {
          T sn, cs;
          jac_sincos((q(s) - t.jnt_qpos0[j])*(T)0.5, &sn, &cs);
          ql[0] = cs; ql[1] = a[0]*sn; ql[2] = a[1]*sn; ql[3] = a[2]*sn;
          emit(t.jnt_dadr[j], axis, anchor);
        }
        mul_quat(quat, quat, ql);
        rot_vec_quat(tv, jp, quat);
        for (int k = 0; k < 3; k++) pos[k] = anchor[k] - tv[k];
      }
    }
  }
  normalize4(quat);
  for (int j = j0; j < j0 + jn; j++) {      // the dofs whose axes are columns of the body's FINAL orientation
    const int type = t.jnt_type[j], c = t.jnt_dadr[j];
    if (type != DMC_JNT_BALL && type != DMC_JNT_FREE) continue;
    quat2mat(m, quat);
    for (int i = 0; i < 3; i++) {
      const T col[3] = {m[i], m[3 + i], m[6 + i]};
      if (type == DMC_JNT_BALL) { emit(c + i, col, ballanchor); continue; }
      const T e[3] = {i == 0 ? (T)1 : (T)0, i == 1 ? (T)1 : (T)0, i == 2 ? (T)1 : (T)0};
      emit(c + i, e, pos);
      emit(c + 3 + i, col, pos);
    }
  }
  for (int k = 0; k < 3; k++) ws[L.xpos + 3*b + k] = pos[k];
  for (int k = 0; k < 4; k++) ws[L.xquat + 4*b + k] = quat[k];
}

// Phase 1: the frames of the whole tree from qpos (q(a): the environment's qpos entry a), cdof and cinert.  `first(k)` runs
// with the first phase for dof k: the callers stage their per-dof inputs there.
template <typename T, class Q, class F, class P>
DMC_DEV void dyn_frames(const DynTab<T>& t, T* ws, const DynLayout& L, Q q, F first, P& par) {
  const DynDims d = t.d;
  par.run(d.nv + 1, [&](int i) {
    if (i < d.nv) { first(i); return; }
    ws[L.xpos] = ws[L.xpos + 1] = ws[L.xpos + 2] = 0;
    ws[L.xquat] = 1; ws[L.xquat + 1] = ws[L.xquat + 2] = ws[L.xquat + 3] = 0;
  });
  for (int l = 0; l < d.nlevel; l++) {
    const int a = t.level_adr[l], n = t.level_adr[l + 1] - a;
    par.run(n, [&](int i) { dyn_body_kinematics(t, ws, L, q, t.level_body[a + i]); });
  }
  par.run(d.nv + d.nb, [&](int i) {
    if (i < d.nv) {      // mj_comPos, the dof: (axis, anchor) -> cdof about the tree's reference point
      T* c = ws + L.cdof + 6*i;
      const T* ref = ws + L.xpos + 3*t.body_root[t.dof_body[i]];
      const T axis[3] = {c[0], c[1], c[2]};
      if (t.dof_rot[i]) {
        const T off[3] = {ref[0] - c[3], ref[1] - c[4], ref[2] - c[5]};
        cross3(c + 3, axis, off);
      } else {
        c[0] = c[1] = c[2] = 0;
        for (int k = 0; k < 3; k++) c[3 + k] = axis[k];
      }
      return;
    }
    const int b = i - d.nv;      // the body: its inertia about the reference point, world orientation
    const T* pos = ws + L.xpos + 3*b;
    const T* ref = ws + L.xpos + 3*t.body_root[b];
    const T quat[4] = {ws[L.xquat + 4*b], ws[L.xquat + 4*b + 1], ws[L.xquat + 4*b + 2], ws[L.xquat + 4*b + 3]};
    const T ip[3] = {t.body_ipos[3*b], t.body_ipos[3*b + 1], t.body_ipos[3*b + 2]};
    const T iq[4] = {t.body_iquat[4*b], t.body_iquat[4*b + 1], t.body_iquat[4*b + 2], t.body_iquat[4*b + 3]};
    const T inertia[3] = {t.body_inertia[3*b], t.body_inertia[3*b + 1], t.body_inertia[3*b + 2]};
    T tv[3], xiq[4], m[9], dif[3], ci[10];
    rot_vec_quat(tv, ip, quat);
    for (int k = 0; k < 3; k++) dif[k] = (pos[k] + tv[k]) - ref[k];
    mul_quat(xiq, quat, iq);
    quat2mat(m, xiq);
    inert_com(ci, inertia, m, dif, t.body_mass[b]);
    for (int k = 0; k < 10; k++) ws[L.cinert + 10*b + k] = ci[k];
  });
}

// Phase 2: composite inertias and the dense symmetric M (mj_crb, mj_fullM, armature on the diagonal).
template <typename T, class P>
DMC_DEV void dyn_crb(const DynTab<T>& t, T* ws, const DynLayout& L, P& par) {
  const DynDims d = t.d;
  const int nv = d.nv;
  par.run(d.nb + nv, [&](int i) {
    if (i >= d.nb) {      // (a row of zeros: what no ancestor pair writes below)
      T* row = ws + L.M + (i - d.nb)*nv;
      for (int j = 0; j < nv; j++) row[j] = 0;
      return;
    }
    T s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = t.sub_adr[i]; k < t.sub_adr[i + 1]; k++) {
      const T* c = ws + L.cinert + 10*t.sub_body[k];
      for (int a = 0; a < 10; a++) s[a] += c[a];
    }
    for (int a = 0; a < 10; a++) ws[L.crb + 10*i + a] = s[a];
  });
  par.run(nv, [&](int i) {
    T buf[6], crb[10], ci[6];
    for (int a = 0; a < 10; a++) crb[a] = ws[L.crb + 10*t.dof_body[i] + a];
    for (int a = 0; a < 6; a++) ci[a] = ws[L.cdof + 6*i + a];
    mul_inert_vec(buf, crb, ci);
    ws[L.M + i*nv + i] = dyn_dot6(ci, buf) + t.dof_armature[i];
    for (int j = t.dof_parent[i]; j >= 0; j = t.dof_parent[j]) {
      const T v = dyn_dot6(ws + L.cdof + 6*j, buf);
      ws[L.M + i*nv + j] = v;
      ws[L.M + j*nv + i] = v;
    }
  });
}

// Phase 4a: M = L L' in place in the lower triangle, column by column (left-looking); dinv[k] = 1 / L(k, k).  The diagonal
// keeps the pivot itself; a pivot below DMC_MINVAL counts as DMC_MINVAL.
template <typename T, class P>
DMC_DEV void dyn_factor(T* ws, const DynLayout& L, int nv, P& par) {
  T* M = ws + L.M;
  for (int k = 0; k < nv; k++) {
    par.run(nv - k, [&](int r) {
      const int i = k + r;
      T s = M[i*nv + k];
      for (int j = 0; j < k; j++) s -= M[i*nv + j]*M[k*nv + j];
      M[i*nv + k] = s;
    });
    par.run(nv - k, [&](int r) {
      const int i = k + r;
      T piv = M[k*nv + k];
      piv = piv < (T)DMC_MINVAL ? (T)DMC_MINVAL : piv;
      const T inv = 1/t_sqrt(piv);
      if (i == k) ws[L.dinv + k] = inv;
      else M[i*nv + k] *= inv;
    });
  }
}

// Phase 4b: x = M^-1 f for the kc right-hand sides in the workspace (rhs, kc rows of nv), in place.
template <typename T, class P>
DMC_DEV void dyn_solve_chunk(T* ws, const DynLayout& L, int nv, int kc, P& par) {
  const T* M = ws + L.M;
  const T* dinv = ws + L.dinv;
  T* b = ws + L.rhs;
  for (int j = 0; j + 1 < nv; j++) {      // L y = f: column j leaves the rows below it; y(j) = b(j) dinv(j)
    const int n = nv - 1 - j;
    par.run(kc*n, [&](int it) {
      const int k = it/n, i = j + 1 + it % n;
      b[k*nv + i] -= M[i*nv + j]*(b[k*nv + j]*dinv[j]);
    });
  }
  par.run(kc*nv, [&](int it) { b[it] *= dinv[it % nv]; });
  for (int i = nv - 1; i > 0; i--) {      // L' x = y: x(i) = c(i) dinv(i) leaves the rows above it
    par.run(kc*i, [&](int it) {
      const int k = it/i, j = it % i;
      b[k*nv + j] -= M[i*nv + j]*(b[k*nv + i]*dinv[i]);
    });
  }
  par.run(kc*nv, [&](int it) { b[it] *= dinv[it % nv]; });
}

// mj_mulM for the kc vectors in the workspace: res = M rhs, row sums in column order.
template <typename T, class P>
DMC_DEV void dyn_mul_chunk(T* ws, const DynLayout& L, int nv, int kc, P& par) {
  par.run(kc*nv, [&](int it) {
    const T* row = ws + L.M + (it % nv)*nv;
    const T* v = ws + L.rhs + (it/nv)*nv;
    T s = 0;
    for (int j = 0; j < nv; j++) s += row[j]*v[j];
    ws[L.res + it] = s;
  });
}

// Phase 3: mj_comVel + mj_rne after dyn_frames (which staged qvel and qacc): res = c(q, qvel) + M qacc (qacc staged as
// zeros: the bias forces alone).
template <typename T, class P>
DMC_DEV void dyn_rne(const DynTab<T>& t, T* ws, const DynLayout& L, P& par) {
  const DynDims d = t.d;
  const T* qvel = ws + L.qvel;
  const T* qacc = ws + L.qacc;
  par.run(d.nv, [&](int k) {      // cdof_dot = (the velocity that carries the dof's axis) x cdof
    T cv[6] = {0, 0, 0, 0, 0, 0}, cdd[6];
    for (int m = t.dof_pred[k]; m >= 0; m = t.dof_parent[m]) {
      const T* c = ws + L.cdof + 6*m;
      const T v = qvel[m];
      for (int a = 0; a < 6; a++) cv[a] += c[a]*v;
    }
    cross_motion(cdd, cv, ws + L.cdof + 6*k);
    for (int a = 0; a < 6; a++) ws[L.cdd + 6*k + a] = cdd[a];
  });
  par.run(d.nb, [&](int b) {      // the body's velocity, acceleration and force
    T cv[6] = {0, 0, 0, 0, 0, 0}, ca[6] = {0, 0, 0, -t.gravity[0], -t.gravity[1], -t.gravity[2]}, ci[10], f[6], h[6], x[6];
    for (int m = t.body_lastdof[b]; m >= 0; m = t.dof_parent[m]) {
      const T* c = ws + L.cdof + 6*m;
      const T* cd = ws + L.cdd + 6*m;
      const T v = qvel[m], acc = qacc[m];
      for (int a = 0; a < 6; a++) { cv[a] += c[a]*v; ca[a] += cd[a]*v + c[a]*acc; }
    }
    for (int a = 0; a < 10; a++) ci[a] = ws[L.cinert + 10*b + a];
    mul_inert_vec(f, ci, ca);
    mul_inert_vec(h, ci, cv);
    cross_force(x, cv, h);
    for (int a = 0; a < 6; a++) { ws[L.cvel + 6*b + a] = cv[a]; ws[L.cfrc + 6*b + a] = f[a] + x[a]; }
  });
  par.run(d.nb, [&](int b) {      // the force its joints carry: the subtree's sum
    T s[6] = {0, 0, 0, 0, 0, 0};
    for (int k = t.sub_adr[b]; k < t.sub_adr[b + 1]; k++) {
      const T* c = ws + L.cfrc + 6*t.sub_body[k];
      for (int a = 0; a < 6; a++) s[a] += c[a];
    }
    for (int a = 0; a < 6; a++) ws[L.cfs + 6*b + a] = s[a];
  });
  // (mj_rne itself leaves the armature out -- MuJoCo's callers add it; here the result is M qacc + bias with M as above)
  par.run(d.nv, [&](int k) { ws[L.res + k] = dyn_dot6(ws + L.cdof + 6*k, ws + L.cfs + 6*t.dof_body[k]) + t.dof_armature[k]*qacc[k]; });
}

#ifndef DMC_HOST_EMU
// ---- the launches (dyn_kernels.hip) -------------------------------------------------------------------------------------
enum { DYN_MASS = 0, DYN_MUL = 1, DYN_SOLVE = 2 };
template <typename T>
struct DynArgs {
  DynDims d;
  const int* ints;
  const T* reals;
  const T* qpos;        // (nq, B)
  const T* qvel;        // (nv, B)
  int B, W;             // W: lanes per environment
  int mode;             // DYN_MASS / DYN_MUL / DYN_SOLVE
  const T* in;          // mul, solve: (B, K, nv); inverse: qacc, element k of env e at in[e*in_se + k], or null
  long long in_se;
  int K;
  T* out;               // (B, nv, nv), (B, K, nv) or (B, nv)
};

int launch_dyn_crb_f32(const DynArgs<float>& a, void* stream);
int launch_dyn_crb_f64(const DynArgs<double>& a, void* stream);
int launch_dyn_rne_f32(const DynArgs<float>& a, void* stream);
int launch_dyn_rne_f64(const DynArgs<double>& a, void* stream);
#endif

}  // namespace dmc
