// lin_core.h -- the two ends of a finite-difference linearisation of the step (mujoco's mjd_transitionFD) for ONE column,
// as free function templates on the real type.  The same text builds for the device (lin_kernels.hip) and for the host
// (tests/emu/lin_emu.cpp, DMC_HOST_EMU).
//
// An environment is linearised by stepping P perturbed copies of its state -- its columns:
//   column 0                         the nominal state
//   column 1 + j                     input j nudged by +eps          (j < n = nx + nu)
//   column 1 + n + j     (centred)   input j nudged by -eps
//   column 1 + n + k     (forward)   control k nudged by -eps, used where the forward nudge leaves ctrlrange
// Inputs are mujoco's: dq (nv tangent directions of qpos), qvel (nv), act (na), then ctrl (nu); nx = 2 nv + na.
//
// lin_fan_column writes the state of one column: qpos through the joint table (slide and hinge add, ball and free
// rotations are renormalised and composed with a rotation by eps about local axis j on the right: mj_integratePos
// along a unit tangent), qvel, act and ctrl nudged, everything else the step reads copied as it is.  lin_diff_column turns
// the stepped columns of one input into column j of A / B (and C / D): velocity, activation and sensor rows are quotients,
// position rows come per joint from mju_subQuat (mj_differentiatePos).  A control whose nudge would leave ctrlrange
// follows mjd_transitionFD's clamped rule (LIN_FWD / LIN_BACK): central, one-sided against the nominal column, or zero.
//
// Memory is reached through an IO object only -- load / copy / store by (field, row) for the fan-out, x(field, row,
// column) / out / sens for the difference -- so the core knows no layout and no precision pair: arithmetic is in T (the
// scratch precision), the IO converts.  Each stored element is computed by one caller in a fixed order.
//
// cos(eps / 2) and sin(eps / 2) arrive as arguments (one pair per object, computed on the host), and the arc tangent of
// mju_subQuat is this file's own (lin_atan2: divisions, a square root and a polynomial, no library call, no contraction),
// so that the fp64 kernels equal the host build bit for bit -- the two math libraries differ in the last place.
#pragma once
#include "step_defs.h"
#include "step_math.h"

namespace dmc {

constexpr int kLinBlock = 256;      // lanes per workgroup, one column per lane

enum LinField { LIN_QPOS = 0, LIN_QVEL, LIN_ACT, LIN_CTRL, LIN_WARM, LIN_QFRC, LIN_XFRC, LIN_MPOS, LIN_MQUAT, LIN_SENSOR, LIN_NFIELD };
enum { LIN_FWD = 1, LIN_BACK = 2 };      // which nudges of an input are used

// xfrc: the source batch reads xfrc_applied (6 nbody rows are copied); centered: the minus columns of the state inputs exist
struct LinDims { int nj, nq, nv, na, nu, nbody, nmocap, nsensordata, xfrc, centered; };

constexpr int lin_nx(const LinDims& d) { return 2*d.nv + d.na; }
constexpr int lin_nin(const LinDims& d) { return 2*d.nv + d.na + d.nu; }
constexpr int lin_ncol(const LinDims& d) { return 1 + lin_nin(d) + (d.centered ? lin_nin(d) : d.nu); }
constexpr int lin_minus_col(const LinDims& d, int in) { return 1 + lin_nin(d) + (d.centered ? in : in - lin_nx(d)); }
constexpr int lin_nints(const LinDims& d) { return 3*d.nj + d.nu; }
constexpr int lin_nreals(const LinDims& d) { return 2*d.nu; }

// ints: jnt_type[nj] jnt_qadr[nj] jnt_dadr[nj] ctrllimited[nu]; reals: ctrlrange[2 nu], fp64 whatever the batches are
struct LinTab {
  const int *jnt_type, *jnt_qadr, *jnt_dadr, *ctrllimited;
  const double* ctrlrange;
};
constexpr LinTab lin_tab(const LinDims& d, const int* ints, const double* reals) {
  return {ints, ints + d.nj, ints + 2*d.nj, ints + 3*d.nj, reals};
}

// The input a column nudges (-1: the nominal column) and the sign of the nudge.
DMC_DEV void lin_column(const LinDims& d, int c, int* in, int* sign) {
  const int n = lin_nin(d);
  if (c == 0) { *in = -1; *sign = 0; }
  else if (c <= n) { *in = c - 1; *sign = 1; }
  else { *in = d.centered ? c - 1 - n : lin_nx(d) + c - 1 - n; *sign = -1; }
}

// mjd_transitionFD's rule for control u in [lo, hi]: the forward nudge is used if u and u + eps are in range, the backward
// one (asked for by a centred difference, or where the forward one is out) if u - eps and u are.  The values are the ones
// the columns hold (sums in T); they are compared, exactly, with the model's fp64 range in every precision pair -- an fp32
// control "at" a limit that fp32 cannot represent lies on one side of it, and the rule says which.
template <typename T>
DMC_DEV int lin_ctrl_flags(T u, T eps, int limited, double lo, double hi, int centered) {
  const double up = (double)(T)(u + eps), dn = (double)(T)(u - eps);
  const bool in = (double)u >= lo && (double)u <= hi;
  const bool fwd = !limited || (in && up >= lo && up <= hi);
  const bool back = (centered || !fwd) && (!limited || (in && dn >= lo && dn <= hi));
  return (fwd ? LIN_FWD : 0) | (back ? LIN_BACK : 0);
}

// One quaternion of qpos at address a: turned by eps about its local axis k (0 .. 2; sign of the turn `sign`), or copied.
template <typename T, class IO>
DMC_DEV void lin_fan_quat(const IO& io, int a, int k, int sign, T ch, T sh) {
  if (k < 0 || k > 2) {
    for (int i = 0; i < 4; i++) io.copy(LIN_QPOS, a + i);
    return;
  }
  T q[4];
  for (int i = 0; i < 4; i++) q[i] = io.load(LIN_QPOS, a + i);
  const T s = sign > 0 ? sh : -sh;
  const T r[4] = {ch, k == 0 ? s : (T)0, k == 1 ? s : (T)0, k == 2 ? s : (T)0};
  normalize4(q);      // (mju_quatIntegrate: the quaternion is renormalised, then turned)
  mul_quat(q, q, r);
  for (int i = 0; i < 4; i++) io.store(LIN_QPOS, a + i, q[i]);
}

// Column c of one environment: everything the step reads.  IO: T load(field, row) (the nominal value, converted to T),
// void store(field, row, T), void copy(field, row) (nominal -> column, exact), void flags(k, int) (control k's LIN_FWD |
// LIN_BACK, recorded by the nominal column), void rest() (time, the warning counters).
template <typename T, class IO>
DMC_DEV void lin_fan_column(const LinDims& d, const LinTab& t, int c, T eps, T ch, T sh, const IO& io) {
  int in, sign;
  lin_column(d, c, &in, &sign);
  const T step = sign > 0 ? eps : -eps;
  const int nv = d.nv, nx = lin_nx(d);
  const int pd = in >= 0 && in < nv ? in : -1;      // the tangent direction of qpos this column nudges
  for (int j = 0; j < d.nj; j++) {
    const int ty = t.jnt_type[j], a = t.jnt_qadr[j];
    const int k = pd >= 0 ? pd - t.jnt_dadr[j] : -1;      // ... counted within joint j
    if (ty == DMC_JNT_FREE) {
      for (int i = 0; i < 3; i++) {
        if (k == i) io.store(LIN_QPOS, a + i, io.load(LIN_QPOS, a + i) + step);
        else io.copy(LIN_QPOS, a + i);
      }
      lin_fan_quat<T>(io, a + 3, k - 3, sign, ch, sh);
    } else if (ty == DMC_JNT_BALL) {
      lin_fan_quat<T>(io, a, k, sign, ch, sh);
    } else {
      if (k == 0) io.store(LIN_QPOS, a, io.load(LIN_QPOS, a) + step);
      else io.copy(LIN_QPOS, a);
    }
  }
  for (int r = 0; r < nv; r++) {
    if (in == nv + r) io.store(LIN_QVEL, r, io.load(LIN_QVEL, r) + step);
    else io.copy(LIN_QVEL, r);
  }
  for (int r = 0; r < d.na; r++) {
    if (in == 2*nv + r) io.store(LIN_ACT, r, io.load(LIN_ACT, r) + step);
    else io.copy(LIN_ACT, r);
  }
  for (int k = 0; k < d.nu; k++) {
    if (c != 0 && in != nx + k) { io.copy(LIN_CTRL, k); continue; }
    const T u = io.load(LIN_CTRL, k);
    const int f = lin_ctrl_flags(u, eps, t.ctrllimited[k], t.ctrlrange[2*k], t.ctrlrange[2*k + 1], d.centered);
    if (c == 0) { io.flags(k, f); io.copy(LIN_CTRL, k); }
    else if (f & (sign > 0 ? LIN_FWD : LIN_BACK)) io.store(LIN_CTRL, k, u + step);
    else io.copy(LIN_CTRL, k);      // an unused nudge: the column is stepped at the nominal control and never read
  }
  for (int r = 0; r < nv; r++) { io.copy(LIN_WARM, r); io.copy(LIN_QFRC, r); }
  if (d.xfrc) for (int r = 0; r < 6*d.nbody; r++) io.copy(LIN_XFRC, r);
  for (int r = 0; r < 3*d.nmocap; r++) io.copy(LIN_MPOS, r);
  for (int r = 0; r < 4*d.nmocap; r++) io.copy(LIN_MQUAT, r);
  io.rest();
}

// atan(t) for |t| <= tan(pi / 8): the odd series in Horner form to t^43 (remainder below 2e-18 relative).
template <typename T>
DMC_DEV T lin_atan_small(T t) {
  const T z = t*t;
  T p = (T)(1.0/43.0);
#pragma unroll
  for (int k = 20; k >= 0; k--) p = (T)(1.0/(double)(2*k + 1)) - z*p;
  return t*p;
}
// atan2(s, w) for s >= 0, in [0, pi]: the quotient of the smaller by the larger, then atan(t) = pi / 4 + atan((t - 1) / (t + 1))
// above tan(pi / 8).
template <typename T>
DMC_DEV T lin_atan2(T s, T w) {
  const T pi = (T)3.14159265358979323846;
  const T aw = w < 0 ? -w : w;
  const bool swap = s > aw;
  const T big = swap ? s : aw, small = swap ? aw : s;
  T a = 0;
  if (big > 0) {
    const T t = small/big;
    a = t > (T)0.41421356237309503 ? (T)0.25*pi + lin_atan_small((t - 1)/(t + 1)) : lin_atan_small(t);
  }
  if (swap) a = (T)0.5*pi - a;
  return w < 0 ? pi - a : a;
}
// mju_subQuat: the rotation vector, in qb's frame, that takes qb to qa.
template <typename T>
DMC_DEV void lin_sub_quat(T* res, const T* qa, const T* qb) {
  const T pi = (T)3.14159265358979323846;
  const T cb[4] = {qb[0], -qb[1], -qb[2], -qb[3]};
  T q[4];
  mul_quat(q, cb, qa);
  T ax[3] = {q[1], q[2], q[3]};
  const T s = normalize3(ax);
  T ang = 2*lin_atan2(s, q[0]);
  if (ang > pi) ang -= 2*pi;
  res[0] = ax[0]*ang; res[1] = ax[1]*ang; res[2] = ax[2]*ang;
}

// Column `in` of A / B (and C / D where sensors are asked for) of one environment from its stepped columns.  flags:
// LIN_FWD | LIN_BACK of the input (a state input: LIN_FWD, and LIN_BACK when centred).  IO: T x(field, row, column) (the
// stepped scratch state as T), void out(row, T) (row of A or B, column `in`), void sens(row, T) (row of C or D).
template <typename T, class IO>
DMC_DEV void lin_diff_column(const LinDims& d, const LinTab& t, int in, int flags, T eps, bool sensors, const IO& io) {
  const int nv = d.nv;
  const bool fwd = flags & LIN_FWD, back = flags & LIN_BACK, none = !fwd && !back;
  const int ca = fwd ? 1 + in : 0, cb = back ? lin_minus_col(d, in) : 0;      // (x[ca] - x[cb]) / h
  const T h = fwd && back ? 2*eps : eps;
  for (int j = 0; j < d.nj; j++) {
    const int ty = t.jnt_type[j], a = t.jnt_qadr[j], r = t.jnt_dadr[j];
    int nlin = 1, aq = -1;
    if (ty == DMC_JNT_FREE) { nlin = 3; aq = a + 3; }
    else if (ty == DMC_JNT_BALL) { nlin = 0; aq = a; }
    for (int i = 0; i < nlin; i++) io.out(r + i, none ? (T)0 : (io.x(LIN_QPOS, a + i, ca) - io.x(LIN_QPOS, a + i, cb))/h);
    if (aq >= 0) {
      T qa[4], qb[4], w[3] = {0, 0, 0};
      if (!none) {
        for (int i = 0; i < 4; i++) { qa[i] = io.x(LIN_QPOS, aq + i, ca); qb[i] = io.x(LIN_QPOS, aq + i, cb); }
        lin_sub_quat(w, qa, qb);
      }
      for (int i = 0; i < 3; i++) io.out(r + nlin + i, none ? (T)0 : w[i]/h);
    }
  }
  for (int r = 0; r < nv; r++) io.out(nv + r, none ? (T)0 : (io.x(LIN_QVEL, r, ca) - io.x(LIN_QVEL, r, cb))/h);
  for (int r = 0; r < d.na; r++) io.out(2*nv + r, none ? (T)0 : (io.x(LIN_ACT, r, ca) - io.x(LIN_ACT, r, cb))/h);
  if (sensors)
    for (int r = 0; r < d.nsensordata; r++) io.sens(r, none ? (T)0 : (io.x(LIN_SENSOR, r, ca) - io.x(LIN_SENSOR, r, cb))/h);
}

#ifndef DMC_HOST_EMU
// ---- the launches (lin_kernels.hip) -------------------------------------------------------------------------------------
// Ts: the real type of the source batch and of the outputs; Tc: of the scratch batch.
template <typename Ts, typename Tc>
struct LinArgs {
  LinDims d;
  const int* ints;
  const double* reals;
  const Ts* src[LIN_NFIELD];      // the source batch's fields, (rows, B); read only
  const double* src_time;         // (B)
  Tc* scr[LIN_NFIELD];            // the scratch batch's fields, (rows, Bs)
  double* scr_time;               // (Bs)
  int* scr_warning;               // (DMC_NWARNING, Bs): zeroed by the fan-out, counted by the step, read by the difference
  int* flags;                     // (B, nu): LIN_FWD | LIN_BACK per (environment, control)
  int* warn;                      // (B): bit w set where some column of the environment raised warning w
  int B, Bs, first_env, nenv, P;  // this chunk: source environments [first_env, first_env + nenv), nenv P scratch environments
  Tc eps, ch, sh;                 // the nudge, cos(eps / 2), sin(eps / 2)
  Ts *A, *Bm, *C, *D;             // (B, nx, nx), (B, nx, nu), (B, nsensordata, nx), (B, nsensordata, nu); C, D null: no sensors
};

// which: 0 the fan-out, 1 the difference
int launch_lin_f64_f64(const LinArgs<double, double>& a, int which, void* stream);
int launch_lin_f32_f64(const LinArgs<float, double>& a, int which, void* stream);
int launch_lin_f32_f32(const LinArgs<float, float>& a, int which, void* stream);
#endif

}  // namespace dmc
