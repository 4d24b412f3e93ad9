// TEST INFRASTRUCTURE: host build of the Jacobian unit's core (dm_control_amd/csrc/jac_core.h) -- the same text the device
// kernels compile, in the host-emulation form of step_defs.h, one environment per call, in fp32 and fp64.
#define DMC_HOST_EMU 1
#include <vector>

#include "../../dm_control_amd/csrc/jac_core.h"

using namespace dmc;

namespace {
template <typename T>
void run_t(int ntarget, int ncol, const int* dims, const int* ints, const double* reals, int nreals, int nq, int nv, const double* qpos,
           const double* qvel, const double* point, const double* force, const double* torque, int local, double* jacp, double* jacr,
           double* vel, double* qfrc) {
  std::vector<T> r(reals, reals + nreals), q(qpos, qpos + nq), v(qvel, qvel + nv), acc(ncol, (T)0);
  std::vector<int> head((size_t)ntarget*kJacHead, 0);
  int io = 0, ro = 0;
  for (int t = 0; t < ntarget; t++) {
    const JacDims d = {dims[3*t], dims[3*t + 1], dims[3*t + 2]};
    int* h = &head[(size_t)t*kJacHead];
    h[0] = d.nb; h[1] = d.nj; h[2] = d.nd; h[4] = io; h[5] = ro;
    io += jac_nints(d); ro += jac_nreals(d);
  }
  auto qr = [&](int a) { return q[a]; };
  auto vr = [&](int k) { return v[k]; };
  for (int t = 0; t < ntarget; t++) {
    const JacChain<T> ch = jac_chain<T>(head.data(), ints, r.data(), t);
    // the Jacobian launch: the target's point (or the caller's), then one column per chain dof; the rest stays zero
    T p[3], tq[4];
    if (point) { for (int k = 0; k < 3; k++) p[k] = (T)point[3*t + k]; }
    else jac_target(ch, qr, p, tq);
    for (int k = 0; k < 3*ncol; k++) jacp[(size_t)t*3*ncol + k] = jacr[(size_t)t*3*ncol + k] = 0;
    jac_columns(ch, qr, (const T*)p, [&](int, int col, const T* jp, const T* jr) {
      if (col < 0) return;
      for (int k = 0; k < 3; k++) {
        jacp[((size_t)t*3 + k)*ncol + col] = (double)jp[k];
        jacr[((size_t)t*3 + k)*ncol + col] = (double)jr[k];
      }
    });
    T res[6];
    jac_velocity(ch, qr, vr, local != 0, res);
    for (int k = 0; k < 6; k++) vel[6*t + k] = (double)res[k];
    // the force launch: the targets in order into one accumulator per column
    T f[3] = {0, 0, 0}, tau[3] = {0, 0, 0};
    if (force) for (int k = 0; k < 3; k++) f[k] = (T)force[3*t + k];
    if (torque) for (int k = 0; k < 3; k++) tau[k] = (T)torque[3*t + k];
    jac_force(ch, qr, (const T*)f, (const T*)tau, [&](int col, T x) { acc[col] += x; });
  }
  for (int c = 0; c < ncol; c++) qfrc[c] = (double)acc[c];
}
}  // namespace

// One environment: dims (T, 3), the concatenated tables of dmc_jac_tables, qpos (nq), qvel (nv); point / force / torque
// (T, 3) or null; out: jacp, jacr (T, 3, C), vel (T, 6), qfrc (C)
extern "C" void jac_emu_run(int prec, int ntarget, int ncol, const int* dims, const int* ints, const double* reals, int nreals, int nq,
                            int nv, const double* qpos, const double* qvel, const double* point, const double* force,
                            const double* torque, int local, double* jacp, double* jacr, double* vel, double* qfrc) {
  if (prec == 64) run_t<double>(ntarget, ncol, dims, ints, reals, nreals, nq, nv, qpos, qvel, point, force, torque, local, jacp, jacr, vel, qfrc);
  else run_t<float>(ntarget, ncol, dims, ints, reals, nreals, nq, nv, qpos, qvel, point, force, torque, local, jacp, jacr, vel, qfrc);
}

// sin and cos as the unit computes them
extern "C" void jac_emu_sincos(int prec, int n, const double* x, double* s, double* c) {
  for (int i = 0; i < n; i++) {
    if (prec == 64) jac_sincos<double>(x[i], &s[i], &c[i]);
    else { float sf, cf; jac_sincos<float>((float)x[i], &sf, &cf); s[i] = sf; c[i] = cf; }
  }
}

extern "C" void jac_emu_caps(int* out) { out[0] = kJacMaxDof; out[1] = kJacBlock; out[2] = kJacHead; }
