// TEST INFRASTRUCTURE: a stand-alone program around dm_control_amd/csrc/dyn_core.h for the sanitizers (built with
// -fsanitize=address,undefined by tests/test_dynamics_cpu.py).  stdin: "nb nj nv nq nlevel nsub K ncase", the int and the
// real tables, then per case qpos (nq), qvel (nv), qacc (nv), vec (K nv).  stdout: per case, precision (fp64 first) and
// lanes per environment (16, 64) one line: the sum of |M|, then bias, inverse (nv each), mul, solve (K nv each).
// Every array is a heap allocation of exactly its size, so that an index past a table is an error the sanitizer reports.
#include <cmath>
#include <cstdio>
#include <vector>

#include "dyn_emu.cpp"

static bool read_ints(std::vector<int>* v) {
  for (int& x : *v) if (scanf("%d", &x) != 1) return false;
  return true;
}
static bool read_reals(std::vector<double>* v) {
  for (double& x : *v) if (scanf("%lf", &x) != 1) return false;
  return true;
}

int main() {
  int dims[6], K, ncase;
  if (scanf("%d %d %d %d %d %d %d %d", &dims[0], &dims[1], &dims[2], &dims[3], &dims[4], &dims[5], &K, &ncase) != 8) return 2;
  const DynDims d = {dims[0], dims[1], dims[2], dims[3], dims[4], dims[5]};
  if (d.nb < 2 || d.nj < 1 || d.nv < 1 || d.nq < 1 || d.nlevel < 1 || d.nsub < 1 || K < 1) return 2;
  std::vector<int> ints(dyn_nints(d));
  std::vector<double> reals(dyn_nreals(d));
  if (!read_ints(&ints) || !read_reals(&reals)) return 2;
  const size_t nv = d.nv;
  for (int i = 0; i < ncase; i++) {
    std::vector<double> qpos(d.nq), qvel(nv), qacc(nv), vec(K*nv);
    if (!read_reals(&qpos) || !read_reals(&qvel) || !read_reals(&qacc) || !read_reals(&vec)) return 2;
    for (int prec = 64; prec >= 32; prec -= 32) {
      for (int W = 16; W <= 64; W += 48) {
        std::vector<double> M(nv*nv), bias(nv), inv(nv), mul(K*nv), sol(K*nv);
        dyn_emu_run(prec, dims, ints.data(), reals.data(), W, 31, qpos.data(), qvel.data(), qacc.data(), K, vec.data(), M.data(),
                    bias.data(), inv.data(), mul.data(), sol.data());
        double sm = 0;
        for (double x : M) sm += std::fabs(x);
        printf("%.17g", sm);
        for (const std::vector<double>* v : {&bias, &inv, &mul, &sol}) for (double x : *v) printf(" %.17g", x);
        printf("\n");
      }
    }
  }
  return 0;
}
