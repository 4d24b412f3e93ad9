// TEST INFRASTRUCTURE: a stand-alone program around dm_control_amd/csrc/dist_core.h for the sanitizers (built with
// -fsanitize=address,undefined by tests/test_distance_cpu.py).  stdin: one pair per line, for each geom its type, size (3),
// pos (3), mat (9); stdout: per pair the fp64 distance and status, the fp32 distance and status.  The EPA arrays are
// heap allocations of exactly the caps, so that an index past a cap is an error the sanitizer reports.
#include <cstdio>
#include <vector>

#include "../../dm_control_amd/csrc/dist_core.h"

using namespace dmc;

template <typename T>
static void solve(const int* type, const double* v, double* dist, int* status) {
  DistGeom<T> g[2];
  for (int i = 0; i < 2; i++) {
    g[i].type = type[i];
    for (int k = 0; k < 3; k++) { g[i].size[k] = (T)v[15*i + k]; g[i].pos[k] = (T)v[15*i + 3 + k]; }
    for (int k = 0; k < 9; k++) g[i].mat[k] = (T)v[15*i + 6 + k];
  }
  std::vector<T> vtx(3*DistCaps<T>::V), fdist(DistCaps<T>::F);
  std::vector<int> fidx(DistCaps<T>::F);
  DistEpaMem<T> m;
  m.vtx = vtx.data(); m.fdist = fdist.data(); m.fidx = fidx.data(); m.stride = 1;
  DistResult<T> r;
  dist_pair_host(g[0], g[1], (T)10, (T)1e-6, 50, m, &r);
  *dist = (double)r.dist; *status = r.status;
}

int main() {
  int type[2];
  double v[30];
  for (;;) {
    bool ok = true;
    for (int i = 0; i < 2 && ok; i++) {
      ok = scanf("%d", &type[i]) == 1;
      for (int k = 0; k < 15 && ok; k++) ok = scanf("%lf", &v[15*i + k]) == 1;
    }
    if (!ok) break;
    double d64, d32;
    int s64, s32;
    solve<double>(type, v, &d64, &s64);
    solve<float>(type, v, &d32, &s32);
    printf("%.17g %d %.9g %d\n", d64, s64, d32, s32);
  }
  return 0;
}
