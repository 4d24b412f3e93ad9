// step_math.h -- scalar functions (t_*) and the vec3 / quaternion / inertia / spatial-vector helpers of the step core.
#pragma once
#include "step_defs.h"

namespace dmc {
// ---------------------------------------------------------------------------
// scalar math (expression order mirrors the oracle)
// ---------------------------------------------------------------------------
template <typename T> DMC_DEV T t_sqrt(T x) { return (T)sqrt((double)x); }
template <> DMC_DEV float t_sqrt<float>(float x) { return sqrtf(x); }
// 1 / sqrt(x) for the Cholesky pivots.  fp32: the hardware reciprocal square root (v_rsq_f32, 1 ulp) instead of a
// correctly rounded sqrt followed by a correctly rounded division -- ~25 instructions less on the dependent chain of
// every column (a fifth of the 62 x 62 factorisation); fp64 keeps the exact sequence the oracle uses.
template <typename T> DMC_DEV T t_rsqrt(T x) { return 1 / t_sqrt(x); }
#ifndef DMC_HOST_EMU
template <> DMC_DEV float t_rsqrt<float>(float x) { return __builtin_amdgcn_rsqf(x); }
#endif
template <typename T> DMC_DEV T t_sin(T x) { return (T)sin((double)x); }
template <> DMC_DEV float t_sin<float>(float x) { return sinf(x); }
template <typename T> DMC_DEV T t_cos(T x) { return (T)cos((double)x); }
template <> DMC_DEV float t_cos<float>(float x) { return cosf(x); }
template <typename T> DMC_DEV T t_pow(T x, T y) { return (T)pow((double)x, (double)y); }
template <> DMC_DEV float t_pow<float>(float x, float y) { return powf(x, y); }
template <typename T> DMC_DEV T t_exp(T x) { return (T)exp((double)x); }
template <typename T> DMC_DEV T t_atan2(T y, T x) { return (T)atan2((double)y, (double)x); }
template <> DMC_DEV float t_atan2<float>(float y, float x) { return atan2f(y, x); }
template <typename T> DMC_DEV T t_fmod(T x, T y) { return (T)fmod((double)x, (double)y); }
template <> DMC_DEV float t_fmod<float>(float x, float y) { return fmodf(x, y); }
template <> DMC_DEV float t_exp<float>(float x) { return expf(x); }
// Correctly rounded fp32 division / square root whatever the build's fp32 division mode (step_kernels_f32 is compiled
// with the 2.5-ulp hardware forms): for the few places whose branch decisions sit on an absolute 1e-10 (the PGS block
// updates) and are not on the hot path of any BASELINE configuration.
template <typename T> DMC_DEV T t_div_exact(T a, T b) { return a / b; }
template <> DMC_DEV float t_div_exact<float>(float a, float b) { return (float)((double)a / (double)b); }
template <typename T> DMC_DEV T t_sqrt_exact(T x) { return (T)sqrt((double)x); }
template <typename T> DMC_DEV T t_abs(T x) { return x < 0 ? -x : x; }
template <typename T> DMC_DEV T t_max(T a, T b) { return a > b ? a : b; }
template <typename T> DMC_DEV T t_min(T a, T b) { return a < b ? a : b; }
template <typename T> DMC_DEV bool t_bad(T x) { return !(x == x) || x > (T)DMC_MAXVAL || x < -(T)DMC_MAXVAL; }

template <typename T> DMC_DEV T dot3(const T* a, const T* b) { return a[0]*b[0] + a[1]*b[1] + a[2]*b[2]; }
template <typename T> DMC_DEV void cross3(T* r, const T* a, const T* b) {
  T t0 = a[1]*b[2] - a[2]*b[1], t1 = a[2]*b[0] - a[0]*b[2], t2 = a[0]*b[1] - a[1]*b[0];
  r[0] = t0; r[1] = t1; r[2] = t2;
}
template <typename T> DMC_DEV T normalize3(T* v) {
  T n = t_sqrt(dot3(v, v));
  if (n < (T)DMC_MINVAL) { v[0] = 1; v[1] = 0; v[2] = 0; }
  else { T s = 1 / n; v[0] *= s; v[1] *= s; v[2] *= s; }
  return n;
}
template <typename T> DMC_DEV void normalize4(T* q) {
  T n = t_sqrt(q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3]);
  if (n < (T)DMC_MINVAL) { q[0] = 1; q[1] = q[2] = q[3] = 0; }
  else if (t_abs(n - 1) > (T)DMC_MINVAL) { T s = 1 / n; q[0] *= s; q[1] *= s; q[2] *= s; q[3] *= s; }
}
template <typename T> DMC_DEV void mul_quat(T* r, const T* a, const T* b) {
  T t0 = a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3];
  T t1 = a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2];
  T t2 = a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1];
  T t3 = a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0];
  r[0] = t0; r[1] = t1; r[2] = t2; r[3] = t3;
}
template <typename T> DMC_DEV void quat2mat(T* m, const T* q) {
  T q00 = q[0]*q[0], q01 = q[0]*q[1], q02 = q[0]*q[2], q03 = q[0]*q[3];
  T q11 = q[1]*q[1], q12 = q[1]*q[2], q13 = q[1]*q[3];
  T q22 = q[2]*q[2], q23 = q[2]*q[3], q33 = q[3]*q[3];
  m[0] = q00 + q11 - q22 - q33; m[4] = q00 - q11 + q22 - q33; m[8] = q00 - q11 - q22 + q33;
  m[1] = 2*(q12 - q03); m[2] = 2*(q13 + q02);
  m[3] = 2*(q12 + q03); m[5] = 2*(q23 - q01);
  m[6] = 2*(q13 - q02); m[7] = 2*(q23 + q01);
}
template <typename T> DMC_DEV void mul_mat_vec3(T* r, const T* m, const T* v) {
  T t0 = m[0]*v[0] + m[1]*v[1] + m[2]*v[2];
  T t1 = m[3]*v[0] + m[4]*v[1] + m[5]*v[2];
  T t2 = m[6]*v[0] + m[7]*v[1] + m[8]*v[2];
  r[0] = t0; r[1] = t1; r[2] = t2;
}
template <typename T> DMC_DEV void mul_matT_vec3(T* r, const T* m, const T* v) {
  T t0 = m[0]*v[0] + m[3]*v[1] + m[6]*v[2];
  T t1 = m[1]*v[0] + m[4]*v[1] + m[7]*v[2];
  T t2 = m[2]*v[0] + m[5]*v[1] + m[8]*v[2];
  r[0] = t0; r[1] = t1; r[2] = t2;
}
template <typename T> DMC_DEV void rot_vec_quat(T* r, const T* v, const T* q) {
  T m[9]; quat2mat(m, q); mul_mat_vec3(r, m, v);
}
template <typename T> DMC_DEV void axisangle2quat(T* q, const T* axis, T angle) {
  // Straight-line on purpose: angle == 0 gives s = 0, c = 1, i.e. the identity MuJoCo
  // returns early with; an early-out branch (or sincos()'s pointer outputs) makes the
  // compiler route q through scratch memory.
  const T s = t_sin(angle * (T)0.5), c = t_cos(angle * (T)0.5);
  q[0] = c; q[1] = axis[0]*s; q[2] = axis[1]*s; q[3] = axis[2]*s;
}
template <typename T> DMC_DEV void quat_integrate(T* quat, const T* vel, T scale) {
  T tmp[3] = {vel[0], vel[1], vel[2]}, qrot[4];
  T angle = scale * normalize3(tmp);
  axisangle2quat(qrot, tmp, angle);
  normalize4(quat);
  mul_quat(quat, quat, qrot);
}
template <typename T> DMC_DEV void inert_com(T* res, const T* inert, const T* mat, const T* dif, T mass) {
  T tmp[9];
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) tmp[3*r + c] = mat[3*r + c] * inert[c];
  res[0] = tmp[0]*mat[0] + tmp[1]*mat[1] + tmp[2]*mat[2];
  res[1] = tmp[3]*mat[3] + tmp[4]*mat[4] + tmp[5]*mat[5];
  res[2] = tmp[6]*mat[6] + tmp[7]*mat[7] + tmp[8]*mat[8];
  res[3] = tmp[0]*mat[3] + tmp[1]*mat[4] + tmp[2]*mat[5];
  res[4] = tmp[0]*mat[6] + tmp[1]*mat[7] + tmp[2]*mat[8];
  res[5] = tmp[3]*mat[6] + tmp[4]*mat[7] + tmp[5]*mat[8];
  res[0] += mass * (dif[1]*dif[1] + dif[2]*dif[2]);
  res[1] += mass * (dif[0]*dif[0] + dif[2]*dif[2]);
  res[2] += mass * (dif[0]*dif[0] + dif[1]*dif[1]);
  res[3] -= mass * dif[0]*dif[1];
  res[4] -= mass * dif[0]*dif[2];
  res[5] -= mass * dif[1]*dif[2];
  res[6] = mass*dif[0]; res[7] = mass*dif[1]; res[8] = mass*dif[2];
  res[9] = mass;
}
template <typename T> DMC_DEV void mul_inert_vec(T* res, const T* i, const T* v) {
  res[0] = i[0]*v[0] + i[3]*v[1] + i[4]*v[2] - i[8]*v[4] + i[7]*v[5];
  res[1] = i[3]*v[0] + i[1]*v[1] + i[5]*v[2] + i[8]*v[3] - i[6]*v[5];
  res[2] = i[4]*v[0] + i[5]*v[1] + i[2]*v[2] - i[7]*v[3] + i[6]*v[4];
  res[3] = i[8]*v[1] - i[7]*v[2] + i[9]*v[3];
  res[4] = i[6]*v[2] - i[8]*v[0] + i[9]*v[4];
  res[5] = i[7]*v[0] - i[6]*v[1] + i[9]*v[5];
}
template <typename T> DMC_DEV void cross_motion(T* res, const T* vel, const T* v) {
  res[0] = -vel[2]*v[1] + vel[1]*v[2];
  res[1] =  vel[2]*v[0] - vel[0]*v[2];
  res[2] = -vel[1]*v[0] + vel[0]*v[1];
  res[3] = -vel[2]*v[4] + vel[1]*v[5];
  res[4] =  vel[2]*v[3] - vel[0]*v[5];
  res[5] = -vel[1]*v[3] + vel[0]*v[4];
  res[3] += -vel[5]*v[1] + vel[4]*v[2];
  res[4] +=  vel[5]*v[0] - vel[3]*v[2];
  res[5] += -vel[4]*v[0] + vel[3]*v[1];
}
template <typename T> DMC_DEV void cross_force(T* res, const T* vel, const T* f) {
  res[0] = -vel[2]*f[1] + vel[1]*f[2];
  res[1] =  vel[2]*f[0] - vel[0]*f[2];
  res[2] = -vel[1]*f[0] + vel[0]*f[1];
  res[3] = -vel[2]*f[4] + vel[1]*f[5];
  res[4] =  vel[2]*f[3] - vel[0]*f[5];
  res[5] = -vel[1]*f[3] + vel[0]*f[4];
  res[0] += -vel[5]*f[4] + vel[4]*f[5];
  res[1] +=  vel[5]*f[3] - vel[3]*f[5];
  res[2] += -vel[4]*f[3] + vel[3]*f[4];
}
template <typename T> DMC_DEV T dot_n(const T* a, const T* b, int n) {
  T s = 0; for (int i = 0; i < n; i++) s += a[i]*b[i]; return s;
}
}  // namespace dmc
