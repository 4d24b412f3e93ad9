// TEST INFRASTRUCTURE: a stand-alone program around dm_control_amd/csrc/con_core.h for the sanitizers (built with
// -fsanitize=address,undefined by tests/test_contact_wrench_cpu.py).  stdin: "B K ngeom nbody T words about local", then
// ncon (B), geom1, geom2 (B K), dist (B K), pos (3 B K), frame (9 B K), force (6 B K), xpos, xipos (3 B nbody), xmat
// (9 B nbody), body (T), masks (2 T words).  stdout: per precision (fp64 first) one line: wrench (6 B K), force, torque
// (3 B T), normal, dist (B T), count (B T).
// Every array is a heap allocation of exactly its size, so that an index past a table is an error the sanitizer reports.
#include <cstdio>
#include <vector>

#include "con_emu.cpp"

static bool read_ints(std::vector<int>* v) {
  for (int& x : *v) if (scanf("%d", &x) != 1) return false;
  return true;
}
static bool read_words(std::vector<uint32_t>* v) {
  for (uint32_t& x : *v) if (scanf("%u", &x) != 1) return false;
  return true;
}
static bool read_reals(std::vector<double>* v) {
  for (double& x : *v) if (scanf("%lf", &x) != 1) return false;
  return true;
}

int main() {
  int B, K, ngeom, nbody, T, words, about, local;
  if (scanf("%d %d %d %d %d %d %d %d", &B, &K, &ngeom, &nbody, &T, &words, &about, &local) != 8) return 2;
  if (B < 1 || K < 1 || ngeom < 1 || nbody < 1 || T < 1 || words != con_words(ngeom)) return 2;
  const size_t n = (size_t)B*K, nb = (size_t)B*nbody, nt = (size_t)B*T;
  std::vector<int> ncon(B), g1(n), g2(n), body(T);
  std::vector<double> dist(n), pos(3*n), frame(9*n), force(6*n), xpos(3*nb), xipos(3*nb), xmat(9*nb);
  std::vector<uint32_t> masks((size_t)2*T*words);
  if (!read_ints(&ncon) || !read_ints(&g1) || !read_ints(&g2) || !read_reals(&dist) || !read_reals(&pos) || !read_reals(&frame) ||
      !read_reals(&force) || !read_reals(&xpos) || !read_reals(&xipos) || !read_reals(&xmat) || !read_ints(&body) || !read_words(&masks))
    return 2;
  for (int prec = 64; prec >= 32; prec -= 32) {
    std::vector<double> w(6*n), f(3*nt), t(3*nt), nn(nt), d(nt);
    std::vector<int> c(nt);
    con_emu_run(prec, B, K, ngeom, nbody, ncon.data(), g1.data(), g2.data(), dist.data(), pos.data(), frame.data(), force.data(),
                xpos.data(), xipos.data(), xmat.data(), T, words, body.data(), masks.data(), about, local, w.data(), f.data(), t.data(),
                nn.data(), c.data(), d.data());
    for (const std::vector<double>* v : {&w, &f, &t, &nn, &d}) for (double x : *v) printf("%.17g ", x);
    for (int x : c) printf("%d ", x);
    printf("\n");
  }
  return 0;
}
