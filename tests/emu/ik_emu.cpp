// TEST INFRASTRUCTURE: host build of the inverse-kinematics core (dm_control_amd/csrc/ik_core.h) -- the same text the
// device kernel compiles, in the host-emulation form of step_defs.h, one "lane" (a workspace of stride 1) per
// environment.
#define DMC_HOST_EMU 1
#include <vector>

#include "../../dm_control_amd/csrc/ik_core.h"

using namespace dmc;

namespace {
template <typename T>
int solve_t(int mode, const IkDims& d, const int* ints, const double* reals, const double* opts, int max_steps, const double* tpos,
            const double* tquat, double* qchain, double* err, int* steps) {
  std::vector<T> r(ik_nreals(d)), w(ik_nslots(d), (T)0);
  for (size_t k = 0; k < r.size(); k++) r[k] = (T)reals[k];
  for (int k = 0; k < d.nqc; k++) w[k] = (T)qchain[k];
  IkChain<T> ch;
  ch.d = d; ch.ints = ints; ch.reals = r.data();
  IkOpts<T> o;
  o.tol = (T)opts[0]; o.rot_weight = (T)opts[1]; o.reg_threshold = (T)opts[2]; o.reg_strength = (T)opts[3];
  o.max_update_norm = (T)opts[4]; o.progress_thresh = (T)opts[5]; o.max_steps = max_steps;
  T tp[3] = {0, 0, 0}, tq[4] = {1, 0, 0, 0}, en = 0;
  if (mode & IK_POS) for (int k = 0; k < 3; k++) tp[k] = (T)tpos[k];
  if (mode & IK_ROT) for (int k = 0; k < 4; k++) tq[k] = (T)tquat[k];
  int status;
  if (mode == IK_BOTH) status = ik_solve_env<T, IK_BOTH>(ch, o, tp, tq, w.data(), 1, &en, steps);
  else if (mode == IK_POS) status = ik_solve_env<T, IK_POS>(ch, o, tp, tq, w.data(), 1, &en, steps);
  else status = ik_solve_env<T, IK_ROT>(ch, o, tp, tq, w.data(), 1, &en, steps);
  for (int k = 0; k < d.nqc; k++) qchain[k] = (double)w[k];
  *err = (double)en;
  return status;
}
}  // namespace

// dims = {nb, nj, nd, nqc}; opts = {tol, rot_weight, reg_threshold, reg_strength, max_update_norm, progress_thresh};
// qchain: the chain's qpos entries, in and out
extern "C" int ik_emu_solve(int prec, int mode, const int* dims, const int* ints, const double* reals, const double* opts,
                            int max_steps, const double* tpos, const double* tquat, double* qchain, double* err, int* steps) {
  const IkDims d = {dims[0], dims[1], dims[2], dims[3]};
  if (prec == 64) return solve_t<double>(mode, d, ints, reals, opts, max_steps, tpos, tquat, qchain, err, steps);
  return solve_t<float>(mode, d, ints, reals, opts, max_steps, tpos, tquat, qchain, err, steps);
}

// site pose and the per-dof axes / anchors of one walk (fp64)
extern "C" void ik_emu_pose(const int* dims, const int* ints, const double* reals, const double* qchain, double* spos,
                            double* squat, double* axes, double* anchors) {
  const IkDims d = {dims[0], dims[1], dims[2], dims[3]};
  std::vector<double> w(ik_nslots(d), 0.0);
  for (int k = 0; k < d.nqc; k++) w[k] = qchain[k];
  IkChain<double> ch;
  ch.d = d; ch.ints = ints; ch.reals = reals;
  ik_kinematics(ch, w.data(), 1, spos, squat);
  for (int k = 0; k < 3*d.nd; k++) { axes[k] = w[d.nqc + k]; anchors[k] = w[d.nqc + 3*d.nd + k]; }
}
