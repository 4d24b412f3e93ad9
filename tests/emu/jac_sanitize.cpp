// TEST INFRASTRUCTURE: a stand-alone program around dm_control_amd/csrc/jac_core.h for the sanitizers (built with
// -fsanitize=address,undefined by tests/test_jacobian_cpu.py).  stdin: "ntarget ncol nints nreals nq nv ncase", the dims
// (3 per target), the int and the real tables, then per case qpos (nq), qvel (nv), force and torque (3 per target each).
// stdout: per case and precision (fp64 first) one line: the sum of |jacp|, the sum of |jacr|, vel (6 per target), qfrc (ncol).
// Every array is a heap allocation of exactly its size, so that an index past a table is an error the sanitizer reports.
#include <cmath>
#include <cstdio>
#include <vector>

#include "jac_emu.cpp"

static bool read_ints(std::vector<int>* v) {
  for (int& x : *v) if (scanf("%d", &x) != 1) return false;
  return true;
}
static bool read_reals(std::vector<double>* v) {
  for (double& x : *v) if (scanf("%lf", &x) != 1) return false;
  return true;
}

int main() {
  int T, C, ni, nr, nq, nv, ncase;
  if (scanf("%d %d %d %d %d %d %d", &T, &C, &ni, &nr, &nq, &nv, &ncase) != 7 || T < 1 || C < 1 || ni < 0 || nr < 0 || nq < 1 || nv < 1) return 2;
  std::vector<int> dims(3*(size_t)T), ints(ni);
  std::vector<double> reals(nr);
  if (!read_ints(&dims) || !read_ints(&ints) || !read_reals(&reals)) return 2;
  for (int i = 0; i < ncase; i++) {
    std::vector<double> qpos(nq), qvel(nv), force(3*(size_t)T), torque(3*(size_t)T);
    if (!read_reals(&qpos) || !read_reals(&qvel) || !read_reals(&force) || !read_reals(&torque)) return 2;
    for (int prec = 64; prec >= 32; prec -= 32) {
      std::vector<double> jacp(3*(size_t)T*C), jacr(3*(size_t)T*C), vel(6*(size_t)T), qfrc(C);
      jac_emu_run(prec, T, C, dims.data(), ints.data(), reals.data(), nr, nq, nv, qpos.data(), qvel.data(), nullptr, force.data(),
                  torque.data(), i & 1, jacp.data(), jacr.data(), vel.data(), qfrc.data());
      double sp = 0, sr = 0;
      for (double x : jacp) sp += std::fabs(x);
      for (double x : jacr) sr += std::fabs(x);
      printf("%.17g %.17g", sp, sr);
      for (double x : vel) printf(" %.17g", x);
      for (double x : qfrc) printf(" %.17g", x);
      printf("\n");
    }
  }
  return 0;
}
