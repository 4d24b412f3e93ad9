// jac_core.h -- batched Jacobians of points that move with a body: mj_jac / mj_jacBody / mj_jacBodyCom / mj_jacSite /
// mj_jacGeom, mj_objectVelocity as J qvel, and the joint-space image J' f of mj_applyFT, for ONE (environment, target), as
// free function templates on the real type.  The same text builds for the device (jac_kernels.hip) and for the host
// (tests/emu/jac_emu.cpp, DMC_HOST_EMU).
//
// A target is a frame (offset tpos, orientation tquat) fixed in a body.  Only the chain of bodies from the world to that
// body matters.  The host extracts it once per target (a snapshot of the compiled model) into two flat tables,
// JacChain::ints / ::reals; every lane walks it with uniform indices and reads its environment's qpos through a functor.
//
// The walk (jac_walk) is mj_kinematics along the chain.  It hands every chain dof's world axis and anchor to a visitor
// the moment they are known and keeps NOTHING indexed at run time: a column of the Jacobian needs the dof's axis and
// anchor AND the target's world point, which the walk knows only at its end, so a caller that needs the point walks twice
// -- once with an empty visitor for the target's pose, once to emit.  That trades a second pass of a few hundred
// dependent operations for a per-lane workspace of 6 reals per chain dof (24 KB per wave in fp64 for the CMU walker's
// hand, 196 KB for a 64-dof chain), which leaves the workgroup's LDS to the transposing tile of the outputs.
//
// Conventions (host_data.dof_axes): hinge: the joint's axis about its anchor; slide: the axis; ball: the columns of the
// body's FINAL orientation about the joint's anchor; free: the world axes for the translations, the columns of the
// body's orientation about the body's origin for the rotations.
//
// Sine and cosine are this file's own (jac_sincos): plain arithmetic that rounds the same on the host and on the device,
// so that the fp64 kernel equals the host build bit for bit -- the two math libraries differ in the last place.
#pragma once
#include "step_defs.h"
#include "step_math.h"

namespace dmc {

constexpr int kJacMaxDof = 64;      // chain dofs of one target
constexpr int kJacBlock = 64;       // lanes per workgroup: one wave, one environment per lane
constexpr int kJacHead = 8;         // ints per target in the head table: nb nj nd 0 int-offset real-offset 0 0

struct JacDims { int nb, nj, nd; };      // chain bodies, joints, dofs

// ints:  body_jntadr[nb] body_jntnum[nb] jnt_type[nj] jnt_qadr[nj] jnt_dslot[nj] dof_id[nd] dof_col[nd]
// reals: body_pos[3 nb] body_quat[4 nb] jnt_axis[3 nj] jnt_pos[3 nj] jnt_qpos0[nj] tpos[3] tquat[4]
// (jnt_qadr: the joint's qpos address in the MODEL; jnt_dslot: its first dof counted along the chain; dof_id: chain dof
// -> model dof; dof_col: chain dof -> output column, -1 where the caller's columns leave it out)
template <typename T>
struct JacChain {
  JacDims d;
  const int* ints;
  const T* reals;
};
constexpr int jac_nints(const JacDims& d) { return 2*d.nb + 3*d.nj + 2*d.nd; }
constexpr int jac_nreals(const JacDims& d) { return 7*d.nb + 7*d.nj + 7; }

template <typename T>
DMC_DEV JacChain<T> jac_chain(const int* head, const int* ints, const T* reals, int t) {
  const int* h = head + kJacHead*t;
  JacChain<T> ch;
  ch.d.nb = h[0]; ch.d.nj = h[1]; ch.d.nd = h[2];
  ch.ints = ints + h[4]; ch.reals = reals + h[5];
  return ch;
}

// sin and cos of x: x = k pi/2 + r with |r| <= pi/4 (two-part pi/2, exact for |k| < 2^20), Taylor polynomials in
// Horner form to r^17 / r^18 (remainder 8e-20 at pi/4), the quadrant from k.  No library call, no contraction.
template <typename T>
DMC_DEV void jac_sincos(T x, T* s, T* c) {
  T v = x*(T)0.63661977236758134308;
  v = v > (T)1e9 ? (T)1e9 : v < (T)-1e9 ? (T)-1e9 : v;
  const int k = (int)(v + (v >= 0 ? (T)0.5 : (T)-0.5));
  const T kf = (T)k;
  T r;
  if (sizeof(T) == 8) r = (x - kf*(T)1.57079632673412561417) - kf*(T)6.07710050650619224932e-11;
  else r = (x - kf*(T)1.5703125) - kf*(T)4.83826794896619231321e-4;
  const T r2 = r*r;
  T ps = (T)(1.0/355687428096000.0);
  ps = ps*r2 - (T)(1.0/1307674368000.0);
  ps = ps*r2 + (T)(1.0/6227020800.0);
  ps = ps*r2 - (T)(1.0/39916800.0);
  ps = ps*r2 + (T)(1.0/362880.0);
  ps = ps*r2 - (T)(1.0/5040.0);
  ps = ps*r2 + (T)(1.0/120.0);
  ps = ps*r2 - (T)(1.0/6.0);
  const T sr = r + r*(r2*ps);
  T pc = (T)(-1.0/6402373705728000.0);
  pc = pc*r2 + (T)(1.0/20922789888000.0);
  pc = pc*r2 - (T)(1.0/87178291200.0);
  pc = pc*r2 + (T)(1.0/479001600.0);
  pc = pc*r2 - (T)(1.0/3628800.0);
  pc = pc*r2 + (T)(1.0/40320.0);
  pc = pc*r2 - (T)(1.0/720.0);
  pc = pc*r2 + (T)(1.0/24.0);
  pc = pc*r2 - (T)0.5;
  const T cr = (T)1 + r2*pc;
  const int q = k & 3;
  *s = q == 0 ? sr : q == 1 ? cr : q == 2 ? -sr : -cr;
  *c = q == 0 ? cr : q == 1 ? -sr : q == 2 ? -cr : sr;
}

// mj_kinematics along the chain.  q(a): the environment's qpos entry at model address a.  emit(c, axis, anchor, rot):
// chain dof c turns about / slides along `axis` (world), through `anchor` where it rotates.  Leaves the body's world
// position and quaternion.
template <typename T, class Q, class E>
DMC_DEV void jac_walk(const JacChain<T>& ch, Q q, E emit, T* pos, T* quat) {
  const JacDims d = ch.d;
  const int* bj = ch.ints; const int* bn = bj + d.nb; const int* jt = bn + d.nb; const int* jq = jt + d.nj; const int* jd = jq + d.nj;
  const T* bpos = ch.reals; const T* bquat = bpos + 3*d.nb; const T* jaxis = bquat + 4*d.nb; const T* jpos = jaxis + 3*d.nj;
  const T* jq0 = jpos + 3*d.nj;
  T m[9], t[3];
  pos[0] = pos[1] = pos[2] = 0;
  quat[0] = 1; quat[1] = quat[2] = quat[3] = 0;
  for (int b = 0; b < d.nb; b++) {
    const int j0 = bj[b], jn = bn[b];
    T ballanchor[3] = {0, 0, 0};
    if (jn > 0 && jt[j0] == DMC_JNT_FREE) {
      const int s = jq[j0];
      for (int k = 0; k < 3; k++) pos[k] = q(s + k);
      for (int k = 0; k < 4; k++) quat[k] = q(s + 3 + k);
      normalize4(quat);
    } else {
      const T p[3] = {bpos[3*b], bpos[3*b + 1], bpos[3*b + 2]}, bq[4] = {bquat[4*b], bquat[4*b + 1], bquat[4*b + 2], bquat[4*b + 3]};
      rot_vec_quat(t, p, quat);
      for (int k = 0; k < 3; k++) pos[k] += t[k];
      mul_quat(quat, quat, bq);
      for (int j = j0; j < j0 + jn; j++) {
        const int type = jt[j], s = jq[j];
        const T a[3] = {jaxis[3*j], jaxis[3*j + 1], jaxis[3*j + 2]}, jp[3] = {jpos[3*j], jpos[3*j + 1], jpos[3*j + 2]};
        T anchor[3], axis[3];
        quat2mat(m, quat);
        mul_mat_vec3(anchor, m, jp);
        for (int k = 0; k < 3; k++) anchor[k] += pos[k];
        mul_mat_vec3(axis, m, a);
        if (type == DMC_JNT_SLIDE) {
          const T x = q(s) - jq0[j];
          for (int k = 0; k < 3; k++) pos[k] += axis[k]*x;
          emit(jd[j], axis, anchor, false);
        } else {
          T ql[4];
          if (type == DMC_JNT_BALL) {
            for (int k = 0; k < 4; k++) ql[k] = q(s + k);
            normalize4(ql);
            for (int k = 0; k < 3; k++) ballanchor[k] = anchor[k];      // (its axes wait for the body's final orientation)
          } else {
            T sn, cs;
            jac_sincos((q(s) - jq0[j])*(T)0.5, &sn, &cs);
            ql[0] = cs; ql[1] = a[0]*sn; ql[2] = a[1]*sn; ql[3] = a[2]*sn;
            emit(jd[j], axis, anchor, true);
          }
          mul_quat(quat, quat, ql);
          rot_vec_quat(t, jp, quat);
          for (int k = 0; k < 3; k++) pos[k] = anchor[k] - t[k];
        }
      }
    }
    normalize4(quat);
    // the dofs whose axes are columns of the body's FINAL orientation
    for (int j = j0; j < j0 + jn; j++) {
      const int type = jt[j], c = jd[j];
      if (type != DMC_JNT_BALL && type != DMC_JNT_FREE) continue;
      quat2mat(m, quat);
      for (int i = 0; i < 3; i++) {
        const T col[3] = {m[i], m[3 + i], m[6 + i]};
        if (type == DMC_JNT_BALL) { emit(c + i, col, ballanchor, true); continue; }
        const T e[3] = {i == 0 ? (T)1 : (T)0, i == 1 ? (T)1 : (T)0, i == 2 ? (T)1 : (T)0};
        emit(c + i, e, pos, false);
        emit(c + 3 + i, col, pos, true);
      }
    }
  }
}

struct JacNoEmit {
  template <typename T>
  DMC_DEV void operator()(int, const T*, const T*, bool) const {}
};

// the target's world point and quaternion from its body's pose
template <typename T>
DMC_DEV void jac_target_pose(const JacChain<T>& ch, const T* pos, const T* quat, T* tp, T* tq) {
  const T* tr = ch.reals + 7*ch.d.nb + 7*ch.d.nj;
  const T p[3] = {tr[0], tr[1], tr[2]}, tql[4] = {tr[3], tr[4], tr[5], tr[6]};
  T t[3];
  rot_vec_quat(t, p, quat);
  for (int k = 0; k < 3; k++) tp[k] = pos[k] + t[k];
  mul_quat(tq, quat, tql);
}

template <typename T, class Q>
DMC_DEV void jac_target(const JacChain<T>& ch, Q q, T* tp, T* tq) {
  T pos[3], quat[4];
  jac_walk(ch, q, JacNoEmit(), pos, quat);
  jac_target_pose(ch, pos, quat, tp, tq);
}

// one column of mj_jac at world point p
template <typename T>
DMC_DEV void jac_column(const T* axis, const T* anchor, bool rot, const T* p, T* jp, T* jr) {
  if (rot) {
    const T r[3] = {p[0] - anchor[0], p[1] - anchor[1], p[2] - anchor[2]};
    cross3(jp, axis, r);
    for (int k = 0; k < 3; k++) jr[k] = axis[k];
  } else {
    for (int k = 0; k < 3; k++) { jp[k] = axis[k]; jr[k] = 0; }
  }
}

// Every chain dof's column at the target's point (point == null) or at the caller's world point: sink(chain dof, output
// column or -1, jp, jr).
template <typename T, class Q, class S>
DMC_DEV void jac_columns(const JacChain<T>& ch, Q q, const T* point, S sink) {
  T p[3], tq[4], pos[3], quat[4];
  if (point) { for (int k = 0; k < 3; k++) p[k] = point[k]; }
  else jac_target(ch, q, p, tq);
  const int* dcol = ch.ints + 2*ch.d.nb + 3*ch.d.nj + ch.d.nd;
  jac_walk(ch, q, [&](int c, const T* axis, const T* anchor, bool rot) {
    T jp[3], jr[3];
    jac_column(axis, anchor, rot, p, jp, jr);
    sink(c, dcol[c], jp, jr);
  }, pos, quat);
}

// mj_objectVelocity as J qvel over ALL chain dofs: res = (angular, linear), world frame or the target's own.
// v(k): the environment's qvel entry of model dof k.
template <typename T, class Q, class V>
DMC_DEV void jac_velocity(const JacChain<T>& ch, Q q, V v, bool local, T* res) {
  T p[3], tq[4], pos[3], quat[4];
  jac_target(ch, q, p, tq);
  const int* dof = ch.ints + 2*ch.d.nb + 3*ch.d.nj;
  T ang[3] = {0, 0, 0}, lin[3] = {0, 0, 0};
  jac_walk(ch, q, [&](int c, const T* axis, const T* anchor, bool rot) {
    T jp[3], jr[3];
    jac_column(axis, anchor, rot, p, jp, jr);
    const T qd = v(dof[c]);
    for (int k = 0; k < 3; k++) { ang[k] += jr[k]*qd; lin[k] += jp[k]*qd; }
  }, pos, quat);
  if (local) {
    T m[9], a[3], l[3];
    normalize4(tq);
    quat2mat(m, tq);
    mul_matT_vec3(a, m, ang);
    mul_matT_vec3(l, m, lin);
    for (int k = 0; k < 3; k++) { ang[k] = a[k]; lin[k] = l[k]; }
  }
  for (int k = 0; k < 3; k++) { res[k] = ang[k]; res[3 + k] = lin[k]; }
}

// The target's share of mj_applyFT: add(output column, jp.f + jr.tau) for every chain dof the caller's columns hold.
template <typename T, class Q, class A>
DMC_DEV void jac_force(const JacChain<T>& ch, Q q, const T* f, const T* tau, A add) {
  jac_columns(ch, q, (const T*)nullptr, [&](int, int col, const T* jp, const T* jr) {
    if (col >= 0) add(col, dot3(jp, f) + dot3(jr, tau));
  });
}

#ifndef DMC_HOST_EMU
// ---- the launches (jac_kernels.hip) -------------------------------------------------------------------------------------
template <typename T>
struct JacArgs {
  const int* head;      // (T, kJacHead)
  const int* ints;
  const T* reals;
  const T* qpos;        // (nq, B)
  const T* qvel;        // (nv, B)
  int B, ntarget, ncol;
  const T* point;       // (B, T, 3) or null
  T* jacp;              // (B, T, 3, C) or null
  T* jacr;
  int vec;              // the outputs take 16-byte stores: aligned bases, C a multiple of 16 / sizeof(T)
  T* vel;               // (B, T, 6)
  int local;
  const T* force;       // element k of target t of env e at force[e*f_se + t*f_st + k]; null: zero
  long long f_se, f_st;
  const T* torque;
  long long t_se, t_st;
  T* qfrc;              // (B, C)
  int epb;              // force: environments per workgroup
};
template <typename T> struct JacTile { static constexpr int kChunk = 128/(int)sizeof(T); };      // columns per pass: 16 / 32
constexpr int kJacPad = kJacBlock + 1;      // the tile's lane stride: the transposed reads fall on different banks
constexpr int jac_tile_bytes(int rb) { return 6*(128/rb)*kJacPad*rb; }
constexpr int kJacForceLds = 60*1024;       // force: C x epb accumulators

int launch_jac_f32(const JacArgs<float>& a, void* stream);
int launch_jac_f64(const JacArgs<double>& a, void* stream);
int launch_jac_vel_f32(const JacArgs<float>& a, void* stream);
int launch_jac_vel_f64(const JacArgs<double>& a, void* stream);
int launch_jac_force_f32(const JacArgs<float>& a, void* stream);
int launch_jac_force_f64(const JacArgs<double>& a, void* stream);
#endif

}  // namespace dmc
