// TEST INFRASTRUCTURE: host build of the contact-wrench unit's core (dm_control_amd/csrc/con_core.h) -- the same text the
// device kernels compile, in the host-emulation form of step_defs.h, in fp32 and fp64.  The inputs arrive environment-major
// in fp64, are rounded to the real type and laid out as the step kernels leave them (structure of arrays, (rows, B)); every
// (environment, slot) and (environment, target) is then one call of the function a device lane calls.
#define DMC_HOST_EMU 1
#include <vector>

#include "../../dm_control_amd/csrc/con_core.h"

using namespace dmc;

namespace {
template <typename T>
std::vector<T> soa(const double* a, size_t B, size_t rows) {      // (B, rows) -> (rows, B); exactly rows*B elements
  std::vector<T> out(rows*B);
  for (size_t e = 0; e < B; e++) for (size_t k = 0; k < rows; k++) out[k*B + e] = (T)a[e*rows + k];
  return out;
}
std::vector<int> soa_i(const int* a, size_t B, size_t rows) {
  std::vector<int> out(rows*B);
  for (size_t e = 0; e < B; e++) for (size_t k = 0; k < rows; k++) out[k*B + e] = a[e*rows + k];
  return out;
}

template <typename T>
void run_t(int B, int K, int ngeom, int nbody, const int* ncon, const int* g1, const int* g2, const double* dist, const double* pos,
           const double* frame, const double* force, const double* xpos, const double* xipos, const double* xmat, int nt, int words,
           const int* body, const uint32_t* masks, int about, int local, double* wrench, double* f_out, double* t_out, double* n_out,
           int* c_out, double* d_out) {
  const size_t nB = (size_t)B;
  const std::vector<int> vn(ncon, ncon + nB), v1 = soa_i(g1, nB, K), v2 = soa_i(g2, nB, K);
  const std::vector<T> vd = soa<T>(dist, nB, K), vp = soa<T>(pos, nB, 3*(size_t)K), vf = soa<T>(frame, nB, 9*(size_t)K),
                       vl = soa<T>(force, nB, 6*(size_t)K), vx = soa<T>(xpos, nB, 3*(size_t)nbody), vi = soa<T>(xipos, nB, 3*(size_t)nbody),
                       vm = soa<T>(xmat, nB, 9*(size_t)nbody);
  // (heap copies of exactly the tables' sizes: an index past a table is an error a sanitizer reports)
  const std::vector<uint32_t> vmask(masks, masks + (size_t)nt*2*words);
  const std::vector<int> vbody(body, body + nt);
  ConIn<T> in = {vn.data(), v1.data(), v2.data(), vd.data(), vp.data(), vf.data(), vl.data(), vx.data(), vi.data(), vm.data(), nB, K, ngeom};
  for (size_t e = 0; e < nB; e++) {
    if (wrench) for (int c = 0; c < K; c++) {
      T w[6];
      con_wrench(in, e, c, w);
      for (int k = 0; k < 6; k++) wrench[(e*K + c)*6 + k] = (double)w[k];
    }
    for (int t = 0; t < nt; t++) {
      ConNet<T> o;
      const uint32_t* S = vmask.data() + (size_t)t*2*words;
      con_net(in, e, S, S + words, vbody[t], about, local != 0, &o);
      const size_t row = e*nt + t;
      for (int k = 0; k < 3; k++) { if (f_out) f_out[row*3 + k] = (double)o.force[k]; if (t_out) t_out[row*3 + k] = (double)o.torque[k]; }
      if (n_out) n_out[row] = (double)o.normal;
      if (c_out) c_out[row] = o.count;
      if (d_out) d_out[row] = (double)o.dist;
    }
  }
}
}  // namespace

// B environments, environment-major inputs ((B, K), (B, K, 3), ...); out: wrench (B, K, 6), force, torque (B, T, 3), normal,
// dist (B, T) as doubles, count (B, T); any may be null.
extern "C" void con_emu_run(int prec, int B, int K, int ngeom, int nbody, const int* ncon, const int* g1, const int* g2, const double* dist,
                            const double* pos, const double* frame, const double* force, const double* xpos, const double* xipos,
                            const double* xmat, int nt, int words, const int* body, const uint32_t* masks, int about, int local,
                            double* wrench, double* f_out, double* t_out, double* n_out, int* c_out, double* d_out) {
  if (prec == 64) run_t<double>(B, K, ngeom, nbody, ncon, g1, g2, dist, pos, frame, force, xpos, xipos, xmat, nt, words, body, masks, about,
                                local, wrench, f_out, t_out, n_out, c_out, d_out);
  else run_t<float>(B, K, ngeom, nbody, ncon, g1, g2, dist, pos, frame, force, xpos, xipos, xmat, nt, words, body, masks, about, local,
                    wrench, f_out, t_out, n_out, c_out, d_out);
}

// {lanes per workgroup, most targets, most mask words, head ints per target, words of a mask over ngeom geoms}
extern "C" void con_emu_caps(int ngeom, int* out) {
  out[0] = kConBlock; out[1] = kConMaxTargets; out[2] = kConMaxWords; out[3] = kConHead; out[4] = con_words(ngeom);
}
