// con_core.h -- batched contact wrenches: the world wrench of one contact and the net contact wrench on a set of geoms,
// for ONE environment (and one contact slot or one target), as free function templates on the real type.  The same text
// builds for the device (con_kernels.hip) and for the host (tests/emu/con_emu.cpp, DMC_HOST_EMU).  Stateless: everything is
// read from the contact arrays the last step / forward launch wrote (step_core.h store_outputs under OUT_CONTACT).
//
// Contact c < ncon between geoms g1, g2 with the contact-frame force lf[6] (mj_contactForce) and the frame F (rows normal,
// tangent, tangent): the force ON geom2's body is f_c = F' lf[0:3], the torque about the contact point t_c = F' lf[3:6];
// geom1's body receives -f_c, -t_c (mj_rnePostConstraint).
//
// A target is two bit masks over the geoms, S (the set) and O (the filter).  A contact counts with s = +1 when g2 is in S,
// g1 in O and g1 not in S; with s = -1 when g1 is in S, g2 in O and g2 not in S; a contact with both geoms in S is
// internal and skipped.  force = sum s f_c, torque = sum s (t_c + (p_c - r) x f_c), normal = sum lf[0], count, dist = the
// smallest contact distance.  The contacts are visited in index order in plain arithmetic: no atomic, no cross-lane sum.
#pragma once
#include <limits>

#include "step_defs.h"

namespace dmc {

constexpr int kConBlock = 64;          // lanes per workgroup: one wave, one environment per lane
constexpr int kConMaxTargets = 64;
constexpr int kConMaxWords = 256;      // words of one mask: at most 8192 geoms
constexpr int kConHead = 4;            // ints per target: the named body, 0, 0, 0
enum { CON_ABOUT_COM = 0, CON_ABOUT_ORIGIN = 1, CON_ABOUT_WORLD = 2 };

constexpr int con_words(int ngeom) { return (ngeom + 31)/32; }

// The arrays of a batch as the step kernels leave them: structure of arrays, element `row` of environment `env` at
// [row*B + env].  xpos / xipos / xmat may be null where `about` / `local` do not read them.
template <typename T>
struct ConIn {
  const int *ncon, *geom1, *geom2;
  const T *dist, *pos, *frame, *force;
  const T *xpos, *xipos, *xmat;
  size_t B;
  int nconmax, ngeom;
};

template <typename T>
struct ConNet {
  T force[3], torque[3], normal, dist;
  int count;
};

DMC_DEV bool con_member(const uint32_t* mask, int g) { return (mask[g >> 5] >> (g & 31)) & 1u; }

// +1 / -1: the contact counts for the target with that sign; 0: it does not.  A geom id outside [0, ngeom) never counts.
DMC_DEV int con_sign(const uint32_t* S, const uint32_t* O, int ngeom, int g1, int g2) {
  if ((unsigned)g1 >= (unsigned)ngeom || (unsigned)g2 >= (unsigned)ngeom) return 0;
  const bool s1 = con_member(S, g1), s2 = con_member(S, g2);
  if (s1 == s2) return 0;      // internal to the set, or none of its business
  if (s2) return con_member(O, g1) ? 1 : 0;
  return con_member(O, g2) ? -1 : 0;
}

// The lane's own contact count, held inside the arrays whatever the memory says.
template <typename T>
DMC_DEV int con_count(const ConIn<T>& in, size_t env) {
  const int n = in.ncon[env];
  return n < 0 ? 0 : n > in.nconmax ? in.nconmax : n;
}

// f = F' lf[0:3], t = F' lf[3:6] of contact c: the wrench on geom2's body, the torque about the contact point.
template <typename T>
DMC_DEV void con_world(const ConIn<T>& in, size_t env, int c, T* f, T* t, T* lf0) {
  const size_t B = in.B;
  T F[9], lf[6];
  for (int k = 0; k < 9; k++) F[k] = in.frame[(size_t)(9*c + k)*B + env];
  for (int k = 0; k < 6; k++) lf[k] = in.force[(size_t)(6*c + k)*B + env];
  for (int k = 0; k < 3; k++) {
    f[k] = F[k]*lf[0] + F[3 + k]*lf[1] + F[6 + k]*lf[2];
    t[k] = F[k]*lf[3] + F[3 + k]*lf[4] + F[6 + k]*lf[5];
  }
  *lf0 = lf[0];
}

// One slot of the per-contact output: [f_c, t_c], zeros past the environment's ncon.
template <typename T>
DMC_DEV void con_wrench(const ConIn<T>& in, size_t env, int c, T* w6) {
  for (int k = 0; k < 6; k++) w6[k] = 0;
  if (c >= con_count(in, env)) return;
  T n;
  con_world(in, env, c, w6, w6 + 3, &n);
}

// The net wrench of one target on one environment.  body: the named body (r and the local frame are its own).
template <typename T>
DMC_DEV void con_net(const ConIn<T>& in, size_t env, const uint32_t* S, const uint32_t* O, int body, int about, bool local,
                     ConNet<T>* o) {
  const size_t B = in.B;
  T r[3] = {0, 0, 0};
  if (about == CON_ABOUT_COM) { for (int k = 0; k < 3; k++) r[k] = in.xipos[(size_t)(3*body + k)*B + env]; }
  else if (about == CON_ABOUT_ORIGIN) { for (int k = 0; k < 3; k++) r[k] = in.xpos[(size_t)(3*body + k)*B + env]; }
  T af[3] = {0, 0, 0}, at[3] = {0, 0, 0}, an = 0, dmin = std::numeric_limits<T>::infinity();
  int cnt = 0;
  const int nc = con_count(in, env);
  for (int c = 0; c < nc; c++) {
    const int g1 = in.geom1[(size_t)c*B + env], g2 = in.geom2[(size_t)c*B + env];
    const int sg = con_sign(S, O, in.ngeom, g1, g2);
    if (!sg) continue;
    T f[3], t[3], d[3], n;
    con_world(in, env, c, f, t, &n);
    for (int k = 0; k < 3; k++) d[k] = in.pos[(size_t)(3*c + k)*B + env] - r[k];
    const T x[3] = {d[1]*f[2] - d[2]*f[1], d[2]*f[0] - d[0]*f[2], d[0]*f[1] - d[1]*f[0]};
    const T s = (T)sg;
    for (int k = 0; k < 3; k++) { af[k] += s*f[k]; at[k] += s*(t[k] + x[k]); }
    an += n;
    cnt++;
    const T di = in.dist[(size_t)c*B + env];
    if (di < dmin) dmin = di;
  }
  if (local) {      // into the named body's frame: xmat' v
    T R[9], lf[3], lt[3];
    for (int k = 0; k < 9; k++) R[k] = in.xmat[(size_t)(9*body + k)*B + env];
    for (int k = 0; k < 3; k++) {
      lf[k] = R[k]*af[0] + R[3 + k]*af[1] + R[6 + k]*af[2];
      lt[k] = R[k]*at[0] + R[3 + k]*at[1] + R[6 + k]*at[2];
    }
    for (int k = 0; k < 3; k++) { af[k] = lf[k]; at[k] = lt[k]; }
  }
  for (int k = 0; k < 3; k++) { o->force[k] = af[k]; o->torque[k] = at[k]; }
  o->normal = an; o->dist = dmin; o->count = cnt;
}

// What a launch passes: the arrays, the tables uploaded at create time and the outputs (any may be null).
template <typename T>
struct ConArgs {
  ConIn<T> in;
  const int* head;            // (ntarget, kConHead)
  const uint32_t* masks;      // (ntarget, 2, words): S then O
  int ntarget, words, about, local;
  T *wrench;                  // (B, nconmax, 6)
  T *force, *torque;          // (B, ntarget, 3)
  T *normal, *mindist;        // (B, ntarget)
  int* count;                 // (B, ntarget)
};

#ifndef DMC_HOST_EMU
int launch_con_wrench_f32(const ConArgs<float>& a, void* stream);
int launch_con_wrench_f64(const ConArgs<double>& a, void* stream);
int launch_con_net_f32(const ConArgs<float>& a, void* stream);
int launch_con_net_f64(const ConArgs<double>& a, void* stream);
#endif

}  // namespace dmc
