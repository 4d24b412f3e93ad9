// TEST INFRASTRUCTURE: host build of the dynamics unit's core (dm_control_amd/csrc/dyn_core.h) -- the same text the device
// kernels compile, in the host-emulation form of step_defs.h, one environment per call, in fp32 and fp64.  The executor
// runs the W lanes of a group one after the other, each over the items the device lane would take.
#define DMC_HOST_EMU 1
#include <vector>

#include "../../dm_control_amd/csrc/dyn_core.h"

using namespace dmc;

namespace {
struct HostPar {
  int W;
  template <class F>
  void run(int n, F f) {
    for (int lane = 0; lane < W; lane++)
      for (int i = lane; i < n; i += W) f(i);
  }
};

// what: bit 0 M, bit 1 bias, bit 2 inverse(qacc), bit 3 mul(vec), bit 4 solve(vec)
template <typename T>
void run_t(const int* dims, const int* ints, const double* reals, int W, int what, const double* qpos, const double* qvel,
           const double* qacc, int K, const double* vec, double* M, double* bias, double* inv, double* mul, double* sol) {
  const DynDims d = {dims[0], dims[1], dims[2], dims[3], dims[4], dims[5]};
  const int nv = d.nv;
  std::vector<T> r(reals, reals + dyn_nreals(d)), q(qpos, qpos + d.nq);
  const DynTab<T> t = dyn_tab<T>(d, ints, r.data());
  HostPar par = {W};
  auto qr = [&](int a) { return q[a]; };
  if (what & (1 | 8 | 16)) {
    const DynLayout L = dyn_layout(d.nb, nv, 0);
    std::vector<T> ws(L.total, (T)0);
    dyn_frames(t, ws.data(), L, qr, [](int) {}, par);
    dyn_crb(t, ws.data(), L, par);
    if (what & 1) for (int k = 0; k < nv*nv; k++) M[k] = (double)ws[L.M + k];
    for (int pass = 0; pass < 2; pass++) {      // mul on M, then the factorisation and solve
      if (!(what & (pass ? 16 : 8))) continue;
      if (pass) dyn_factor(ws.data(), L, nv, par);
      for (int c0 = 0; c0 < K; c0 += kDynChunk) {
        const int kc = K - c0 < kDynChunk ? K - c0 : kDynChunk;
        for (int k = 0; k < kc*nv; k++) ws[L.rhs + k] = (T)vec[c0*nv + k];
        if (pass) dyn_solve_chunk(ws.data(), L, nv, kc, par);
        else dyn_mul_chunk(ws.data(), L, nv, kc, par);
        for (int k = 0; k < kc*nv; k++) (pass ? sol : mul)[c0*nv + k] = (double)ws[(pass ? L.rhs : L.res) + k];
      }
    }
  }
  for (int pass = 0; pass < 2; pass++) {
    if (!(what & (pass ? 4 : 2))) continue;
    const DynLayout L = dyn_layout(d.nb, nv, 1);
    std::vector<T> ws(L.total, (T)0);
    dyn_frames(t, ws.data(), L, qr, [&](int k) { ws[L.qvel + k] = (T)qvel[k]; ws[L.qacc + k] = pass ? (T)qacc[k] : (T)0; }, par);
    dyn_rne(t, ws.data(), L, par);
    for (int k = 0; k < nv; k++) (pass ? inv : bias)[k] = (double)ws[L.res + k];
  }
}
}  // namespace

// One environment: dims {nb, nj, nv, nq, nlevel, nsub}, the tables of dmc_dyn_tables, qpos (nq), qvel (nv), qacc (nv),
// vec (K, nv); out: M (nv, nv), bias, inv (nv), mul, sol (K, nv) -- those `what` selects.
extern "C" void dyn_emu_run(int prec, const int* dims, const int* ints, const double* reals, int W, int what, const double* qpos,
                            const double* qvel, const double* qacc, int K, const double* vec, double* M, double* bias, double* inv,
                            double* mul, double* sol) {
  if (prec == 64) run_t<double>(dims, ints, reals, W, what, qpos, qvel, qacc, K, vec, M, bias, inv, mul, sol);
  else run_t<float>(dims, ints, reals, W, what, qpos, qvel, qacc, K, vec, M, bias, inv, mul, sol);
}

// {max dofs, lanes per workgroup, chunk, workspace reals of kind 0 and 1 for (nb, nv), their LDS tier at W lanes in fp64 and fp32}
extern "C" void dyn_emu_caps(int nb, int nv, int W, int* out) {
  out[0] = kDynMaxDof; out[1] = kDynBlock; out[2] = kDynChunk;
  out[3] = dyn_layout(nb, nv, 0).total; out[4] = dyn_layout(nb, nv, 1).total;
  out[5] = dyn_tier(nb, nv, 0, W, 8); out[6] = dyn_tier(nb, nv, 0, W, 4);
  out[7] = dyn_nints({nb, 0, nv, 0, 0, 0}); out[8] = dyn_nreals({nb, 0, nv, 0, 0, 0});
}
