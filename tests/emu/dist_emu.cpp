// TEST INFRASTRUCTURE: host build of the distance unit's per-pair solver (dm_control_amd/csrc/dist_core.h) in fp32 and fp64
// with the EPA polytope in plain arrays of the device's caps (stride 1 instead of the LDS slices).
#include "../../dm_control_amd/csrc/dist_core.h"

using namespace dmc;

template <typename T>
static void pair_t(int type1, const double* size1, const double* pos1, const double* mat1, int type2, const double* size2,
                   const double* pos2, const double* mat2, double distmax, double tolerance, int iterations, double* out) {
  DistGeom<T> g1, g2;
  g1.type = type1; g2.type = type2;
  for (int k = 0; k < 3; k++) { g1.size[k] = (T)size1[k]; g1.pos[k] = (T)pos1[k]; g2.size[k] = (T)size2[k]; g2.pos[k] = (T)pos2[k]; }
  for (int k = 0; k < 9; k++) { g1.mat[k] = (T)mat1[k]; g2.mat[k] = (T)mat2[k]; }
  T vtx[3*DistCaps<T>::V], fdist[DistCaps<T>::F];
  int fidx[DistCaps<T>::F];
  DistEpaMem<T> m;
  m.vtx = vtx; m.fdist = fdist; m.fidx = fidx; m.stride = 1;
  DistResult<T> r;
  dist_pair_host(g1, g2, (T)distmax, (T)tolerance, iterations, m, &r);
  out[0] = (double)r.dist;
  out[1] = (double)r.from.x; out[2] = (double)r.from.y; out[3] = (double)r.from.z;
  out[4] = (double)r.to.x; out[5] = (double)r.to.y; out[6] = (double)r.to.z;
  out[7] = (double)r.normal.x; out[8] = (double)r.normal.y; out[9] = (double)r.normal.z;
  out[10] = r.status; out[11] = r.epa; out[12] = (double)r.gap;
}

// n pairs: types (n, 2), sizes (n, 2, 3), poses (n, 2, 3) and (n, 2, 9); out (n, 13) = dist, from, to, normal, status, epa, gap
extern "C" void dist_emu_pairs(int prec, int n, const int* type, const double* size, const double* pos, const double* mat,
                               const double* distmax, double tolerance, int iterations, double* out) {
  for (int i = 0; i < n; i++) {
    if (prec == 64) pair_t<double>(type[2*i], size + 6*i, pos + 6*i, mat + 18*i, type[2*i + 1], size + 6*i + 3, pos + 6*i + 3, mat + 18*i + 9,
                                   distmax[i], tolerance, iterations, out + 13*i);
    else pair_t<float>(type[2*i], size + 6*i, pos + 6*i, mat + 18*i, type[2*i + 1], size + 6*i + 3, pos + 6*i + 3, mat + 18*i + 9,
                       distmax[i], tolerance, iterations, out + 13*i);
  }
}

extern "C" void dist_emu_caps(int* out) {
  out[0] = DistCaps<float>::V; out[1] = DistCaps<float>::F; out[2] = DistCaps<double>::V; out[3] = DistCaps<double>::F; out[4] = kDistBlock; out[5] = DistCaps<float>::K; out[6] = DistCaps<double>::K;
}
