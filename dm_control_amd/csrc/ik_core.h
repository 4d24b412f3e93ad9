// ik_core.h -- batched inverse kinematics of one site: the damped least-squares iteration of the reference's
// dm_control/utils/inverse_kinematics.py:157-214 (qpos_from_site_pose) for ONE environment, as free function templates on
// the real type.  The same text builds for the device (ik_kernels.hip: one lane per environment) and for the host
// (tests/emu/ik_emu.cpp, DMC_HOST_EMU).
//
// Only the chain of bodies from the world to the site's body matters.  The host extracts it once (a snapshot of the
// compiled model) into two flat tables, IkChain::ints / ::reals; every lane walks it with uniform indices.  The
// environment's own numbers live in a strided workspace `w[slot*ws]` (device: a column of LDS, lane-major, so that a
// runtime slot index is an LDS address and never a runtime-indexed register array): the chain's qpos entries, one world
// axis and one anchor per chain dof, and the update.
//
// One iteration: walk the chain once (poses, axes, anchors), form the error, accumulate J J' over the movable dofs from
// the stored axes / anchors, factor the k x k matrix (k = 3 or 6) in registers, and take update = J' (J J' + lambda I)^-1 e
// -- the dual form of the reference's (J'J + lambda I)^-1 J' e: equal to it for lambda > 0 (push-through identity) and
// equal to its minimum-norm least-squares solution for lambda = 0 while J has full row rank.  A non-positive or
// non-finite pivot ends the environment with status IK_SINGULAR (the reference takes an rcond-truncated step there).
#pragma once
#include "step_defs.h"
#include "step_math.h"

namespace dmc {

enum { IK_POS = 1, IK_ROT = 2, IK_BOTH = 3 };                                        // which targets are given
enum { IK_CONVERGED = 0, IK_STEP_LIMIT = 1, IK_NO_PROGRESS = 2, IK_SINGULAR = 3 };   // per-environment status
constexpr int kIkMaxDof = 64;                                                        // chain dofs

struct IkDims { int nb, nj, nd, nqc; };      // chain bodies, joints, dofs, qpos entries

// ints:  body_jntadr[nb] body_jntnum[nb] jnt_type[nj] jnt_qslot[nj] jnt_dslot[nj] qmap[nqc] dof_movable[nd] dof_rot[nd]
// reals: body_pos[3 nb] body_quat[4 nb] jnt_axis[3 nj] jnt_pos[3 nj] jnt_qpos0[nj] site_pos[3] site_quat[4]
// (jnt_qslot / jnt_dslot: the joint's first qpos entry / dof counted along the chain; qmap: chain entry -> model qposadr)
template <typename T>
struct IkChain {
  IkDims d;
  const int* ints;
  const T* reals;
};
constexpr int ik_nints(const IkDims& d) { return 2*d.nb + 3*d.nj + d.nqc + 2*d.nd; }
constexpr int ik_nreals(const IkDims& d) { return 7*d.nb + 7*d.nj + 7; }
// workspace slots of one environment: qpos[nqc] axis[3 nd] anchor[3 nd] update[nd]
constexpr int ik_nslots(const IkDims& d) { return d.nqc + 7*d.nd; }

template <typename T>
struct IkOpts {
  T tol, rot_weight, reg_threshold, reg_strength, max_update_norm, progress_thresh;
  int max_steps;
};

// mj_kinematics along the chain, then the site: its world position and quaternion.  Leaves every chain dof's world
// axis and anchor in the workspace as mj_jac reads them (hinge: the joint's axis and anchor; slide: the axis; ball and
// the rotations of a free joint: the columns of the body's final orientation, about the joint's anchor / the body's
// origin; the translations of a free joint: the world axes).
template <typename T>
DMC_DEV void ik_kinematics(const IkChain<T>& ch, T* w, int ws, T* spos, T* squat) {
  const IkDims d = ch.d;
  const int* bj = ch.ints; const int* bn = bj + d.nb; const int* jt = bn + d.nb; const int* jq = jt + d.nj; const int* jd = jq + d.nj;
  const T* bpos = ch.reals; const T* bquat = bpos + 3*d.nb; const T* jaxis = bquat + 4*d.nb; const T* jpos = jaxis + 3*d.nj;
  const T* jq0 = jpos + 3*d.nj; const T* site = jq0 + d.nj;
  T* ax = w + (size_t)d.nqc*ws; T* an = ax + (size_t)3*d.nd*ws;
  T pos[3] = {0, 0, 0}, quat[4] = {1, 0, 0, 0}, m[9], t[3];
  for (int b = 0; b < d.nb; b++) {
    const int j0 = bj[b], jn = bn[b];
    if (jn > 0 && jt[j0] == DMC_JNT_FREE) {
      const int s = jq[j0];
      for (int k = 0; k < 3; k++) pos[k] = w[(size_t)(s + k)*ws];
      for (int k = 0; k < 4; k++) quat[k] = w[(size_t)(s + 3 + k)*ws];
      normalize4(quat);
    } else {
      const T p[3] = {bpos[3*b], bpos[3*b + 1], bpos[3*b + 2]}, q[4] = {bquat[4*b], bquat[4*b + 1], bquat[4*b + 2], bquat[4*b + 3]};
      rot_vec_quat(t, p, quat);
      for (int k = 0; k < 3; k++) pos[k] += t[k];
      mul_quat(quat, quat, q);
      for (int j = j0; j < j0 + jn; j++) {
        const int type = jt[j], s = jq[j], c = jd[j];
        const T a[3] = {jaxis[3*j], jaxis[3*j + 1], jaxis[3*j + 2]}, jp[3] = {jpos[3*j], jpos[3*j + 1], jpos[3*j + 2]};
        T anchor[3], axis[3];
        quat2mat(m, quat);
        mul_mat_vec3(anchor, m, jp);
        for (int k = 0; k < 3; k++) anchor[k] += pos[k];
        mul_mat_vec3(axis, m, a);
        if (type == DMC_JNT_SLIDE) {
          const T x = w[(size_t)s*ws] - jq0[j];
          for (int k = 0; k < 3; k++) pos[k] += axis[k]*x;
        } else {
          T ql[4];
          if (type == DMC_JNT_BALL) {
            for (int k = 0; k < 4; k++) ql[k] = w[(size_t)(s + k)*ws];
            normalize4(ql);
          } else {
            axisangle2quat(ql, a, w[(size_t)s*ws] - jq0[j]);
          }
          mul_quat(quat, quat, ql);
          rot_vec_quat(t, jp, quat);
          for (int k = 0; k < 3; k++) pos[k] = anchor[k] - t[k];
        }
        const int n = type == DMC_JNT_BALL ? 3 : 1;
        for (int i = 0; i < n; i++)
          for (int k = 0; k < 3; k++) { ax[(size_t)(3*(c + i) + k)*ws] = axis[k]; an[(size_t)(3*(c + i) + k)*ws] = anchor[k]; }
      }
    }
    normalize4(quat);
    // the dofs whose axes are columns of the body's FINAL orientation
    quat2mat(m, quat);
    for (int j = j0; j < j0 + jn; j++) {
      const int type = jt[j], c = jd[j];
      if (type == DMC_JNT_BALL) {
        for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) ax[(size_t)(3*(c + i) + k)*ws] = m[3*k + i];
      } else if (type == DMC_JNT_FREE) {
        for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) {
          ax[(size_t)(3*(c + i) + k)*ws] = i == k ? (T)1 : (T)0;
          an[(size_t)(3*(c + i) + k)*ws] = pos[k];
          ax[(size_t)(3*(c + 3 + i) + k)*ws] = m[3*k + i];
          an[(size_t)(3*(c + 3 + i) + k)*ws] = pos[k];
        }
      }
    }
  }
  const T sp[3] = {site[0], site[1], site[2]}, sq[4] = {site[3], site[4], site[5], site[6]};
  rot_vec_quat(t, sp, quat);
  for (int k = 0; k < 3; k++) spos[k] = pos[k] + t[k];
  mul_quat(squat, quat, sq);
}

// mju_quat2Vel(res, quat, 1): scale-invariant in quat
template <typename T>
DMC_DEV void ik_quat2vel(T* res, const T* quat) {
  T axis[3] = {quat[1], quat[2], quat[3]};
  const T s = normalize3(axis);
  T speed = 2*t_atan2(s, quat[0]);
  if (speed > (T)3.14159265358979323846) speed -= (T)(2*3.14159265358979323846);
  for (int k = 0; k < 3; k++) res[k] = axis[k]*speed;
}

// column c of the site Jacobian (mj_jacSite) restricted to the rows of kMode
template <typename T, int kMode>
DMC_DEV void ik_column(const T* ax, const T* an, int ws, int c, bool rot, const T* spos, T* col) {
  T a[3], r[3], jp[3];
  for (int k = 0; k < 3; k++) a[k] = ax[(size_t)(3*c + k)*ws];
  if (rot) {
    for (int k = 0; k < 3; k++) r[k] = spos[k] - an[(size_t)(3*c + k)*ws];
    cross3(jp, a, r);
  } else {
    for (int k = 0; k < 3; k++) jp[k] = a[k];
  }
  if (kMode == IK_POS) { for (int k = 0; k < 3; k++) col[k] = jp[k]; }
  else if (kMode == IK_ROT) { for (int k = 0; k < 3; k++) col[k] = rot ? a[k] : (T)0; }
  else { for (int k = 0; k < 3; k++) { col[k] = jp[k]; col[3 + k] = rot ? a[k] : (T)0; } }
}

// mj_integratePos(qpos, update, 1) on the chain's movable dofs
template <typename T>
DMC_DEV void ik_integrate(const IkChain<T>& ch, T* w, int ws, T scale) {
  const IkDims d = ch.d;
  const int* bn = ch.ints + d.nb; const int* jt = bn + d.nb; const int* jq = jt + d.nj; const int* jd = jq + d.nj;
  const int* mov = jd + d.nj + d.nqc;
  const T* u = w + (size_t)(d.nqc + 6*d.nd)*ws;
  for (int j = 0; j < d.nj; j++) {
    const int type = jt[j], s = jq[j], c = jd[j];
    if (!mov[c]) continue;      // (a joint is movable as a whole)
    if (type == DMC_JNT_SLIDE || type == DMC_JNT_HINGE) {
      w[(size_t)s*ws] += u[(size_t)c*ws]*scale;
      continue;
    }
    int sq = s, cr = c;
    if (type == DMC_JNT_FREE) {
      for (int k = 0; k < 3; k++) w[(size_t)(s + k)*ws] += u[(size_t)(c + k)*ws]*scale;
      sq = s + 3; cr = c + 3;
    }
    T q[4], v[3];
    for (int k = 0; k < 4; k++) q[k] = w[(size_t)(sq + k)*ws];
    for (int k = 0; k < 3; k++) v[k] = u[(size_t)(cr + k)*ws]*scale;
    quat_integrate(q, v, (T)1);
    for (int k = 0; k < 4; k++) w[(size_t)(sq + k)*ws] = q[k];
  }
}

// The whole solve of one environment.  tpos / tquat: the targets (read only where kMode asks for them; the quaternion
// is NOT normalised: quat2Vel is scale-invariant).  Returns the status; *err_norm and *steps as the reference reports
// them (steps: the loop index at exit; err_norm: the error the last iteration started from).
template <typename T, int kMode>
DMC_DEV int ik_solve_env(const IkChain<T>& ch, const IkOpts<T>& o, const T* tpos, const T* tquat, T* w, int ws, T* err_norm, int* steps) {
  constexpr int K = kMode == IK_BOTH ? 6 : 3;
  const IkDims d = ch.d;
  const int* mov = ch.ints + 2*d.nb + 3*d.nj + d.nqc; const int* isrot = mov + d.nd;
  const T* ax = w + (size_t)d.nqc*ws; const T* an = ax + (size_t)3*d.nd*ws;
  T* u = w + (size_t)(d.nqc + 6*d.nd)*ws;
  int status = IK_STEP_LIMIT, step = 0;
  T en = 0;
  for (step = 0; step < o.max_steps; step++) {
    T spos[3], squat[4], e[K];
    ik_kinematics(ch, w, ws, spos, squat);
    en = 0;
    if (kMode & IK_POS) {
      T ep[3];
      for (int k = 0; k < 3; k++) ep[k] = tpos[k] - spos[k];
      en += t_sqrt(dot3(ep, ep));
      for (int k = 0; k < 3; k++) e[k] = ep[k];
    }
    if (kMode & IK_ROT) {
      const T neg[4] = {squat[0], -squat[1], -squat[2], -squat[3]};
      T eq[4], er[3];
      mul_quat(eq, tquat, neg);
      ik_quat2vel(er, eq);
      en += t_sqrt(dot3(er, er))*o.rot_weight;
      for (int k = 0; k < 3; k++) e[K - 3 + k] = er[k];
    }
    if (en < o.tol) { status = IK_CONVERGED; break; }
    // A = J J' + lambda I (lower triangle), over the movable dofs
    T A[K][K];
    const T lambda = en > o.reg_threshold ? o.reg_strength : (T)0;
    for (int i = 0; i < K; i++) for (int j = 0; j < K; j++) A[i][j] = i == j ? lambda : (T)0;
    for (int c = 0; c < d.nd; c++) {
      if (!mov[c]) continue;
      T col[K];
      ik_column<T, kMode>(ax, an, ws, c, isrot[c] != 0, spos, col);
      for (int i = 0; i < K; i++) for (int j = 0; j <= i; j++) A[i][j] += col[i]*col[j];
    }
    // Cholesky A = L L', then y = A^-1 e; everything indexed at compile time
    bool bad = false;
    for (int j = 0; j < K; j++) {
      T p = A[j][j];
      for (int k = 0; k < j; k++) p -= A[j][k]*A[j][k];
      if (!(p > 0) || t_bad(p)) bad = true;
      const T l = t_sqrt(p), inv = 1/l;
      A[j][j] = l;
      for (int i = j + 1; i < K; i++) {
        T v = A[i][j];
        for (int k = 0; k < j; k++) v -= A[i][k]*A[j][k];
        A[i][j] = v*inv;
      }
    }
    if (bad) { status = IK_SINGULAR; break; }
    T y[K];
    for (int i = 0; i < K; i++) {
      T v = e[i];
      for (int k = 0; k < i; k++) v -= A[i][k]*y[k];
      y[i] = v/A[i][i];
    }
    for (int i = K - 1; i >= 0; i--) {
      T v = y[i];
      for (int k = i + 1; k < K; k++) v -= A[k][i]*y[k];
      y[i] = v/A[i][i];
    }
    // update = J' y
    T n2 = 0;
    for (int c = 0; c < d.nd; c++) {
      T v = 0;
      if (mov[c]) {
        T col[K];
        ik_column<T, kMode>(ax, an, ws, c, isrot[c] != 0, spos, col);
        for (int i = 0; i < K; i++) v += col[i]*y[i];
      }
      u[(size_t)c*ws] = v;
      n2 += v*v;
    }
    const T un = t_sqrt(n2);
    if (en/un > o.progress_thresh) { status = IK_NO_PROGRESS; break; }
    ik_integrate(ch, w, ws, un > o.max_update_norm ? o.max_update_norm/un : (T)1);
  }
  *err_norm = en;
  *steps = status == IK_STEP_LIMIT ? (o.max_steps > 0 ? o.max_steps - 1 : 0) : step;
  return status;
}

}  // namespace dmc
