// TEST INFRASTRUCTURE: host build of the ray unit's per-ray functions (dm_control_amd/csrc/ray_core.h, which restates
// nothing: the closed forms are camera_core.h's) in fp32 and fp64, walking the geoms the way the two kernels do, and of
// the step kernel's ray_geom_any (step_geom.h) on the same rays.
#define DMC_HOST_EMU 1
#include <vector>

#include "../../dm_control_amd/csrc/step_geom.h"
#include "../../dm_control_amd/csrc/ray_core.h"

using namespace dmc;

// the cast kernel's walk: world-frame rays, the transform per (ray, geom)
template <typename T>
static void cast_t(int n, const double* pnt, const double* vec, const int* bex, int ngeom, const int* type, const int* body,
                   const int* skip, const double* size, const double* gpos, const double* gmat, double cutoff, double* dist,
                   int* gid, double* normal) {
  std::vector<T> s(size, size + 3*ngeom), p(gpos, gpos + 3*ngeom), m(gmat, gmat + 9*ngeom);
  for (int i = 0; i < n; i++) {
    const T o[3] = {(T)pnt[3*i], (T)pnt[3*i + 1], (T)pnt[3*i + 2]}, v[3] = {(T)vec[3*i], (T)vec[3*i + 1], (T)vec[3*i + 2]};
    const T len = cam_sqrt(v[0]*v[0] + v[1]*v[1] + v[2]*v[2]);
    RayHit<T> h;
    h.id = -1; h.x = 0;
    for (int g = 0; g < ngeom; g++) {
      if (skip[g] || body[g] == bex[i]) continue;
      ray_take(ray_geom_world(type[g], &s[3*g], &p[3*g], &m[9*g], o, v), g, len, (T)cutoff, &h);
    }
    dist[i] = h.id >= 0 ? (double)h.x : -1.0;
    gid[i] = h.id;
    T nn[3] = {0, 0, 0};
    if (h.id >= 0) ray_normal_world(type[h.id], &s[3*h.id], &p[3*h.id], &m[9*h.id], o, v, nn);
    for (int k = 0; k < 3; k++) normal[3*i + k] = (double)nn[k];
  }
}

// the scan kernel's walk: the frame's pose, geoms staged in ray-ready form (dropped beyond the cutoff), nine
// multiply-adds per (ray, geom).  fpos (3) / fmat (9): the frame's world pose (ignored for the world frame).
template <typename T>
static void scan_t(int frame_type, const double* fpos, const double* fmat, const double* offset, int bex, int n,
                   const double* dirs, int ngeom, const int* type, const int* body, const int* skip, const double* size,
                   const double* gpos, const double* gmat, double cutoff, double* dist, int* gid) {
  std::vector<T> s(size, size + 3*ngeom), p(gpos, gpos + 3*ngeom), m(gmat, gmat + 9*ngeom);
  RayScan<T> sc;
  sc.frame_type = frame_type; sc.frame_id = 0; sc.bodyexclude = bex;
  for (int k = 0; k < 3; k++) sc.offset[k] = (T)offset[k];
  T fp[3], fm[9], origin[3], R[9];
  for (int k = 0; k < 3; k++) fp[k] = (T)fpos[k];
  for (int k = 0; k < 9; k++) fm[k] = (T)fmat[k];
  ray_frame_pose(sc, fp, fm, 1, origin, R);
  std::vector<CamGeom<T>> staged;
  for (int g = 0; g < ngeom; g++) {
    if (skip[g] || body[g] == bex) continue;
    if (ray_beyond_cutoff(&p[3*g], cam_rbound(type[g], &s[3*g]), origin, (T)cutoff)) continue;
    CamGeom<T> e;
    cam_stage_geom(&e, &p[3*g], &m[9*g], &s[3*g], type[g], g, origin, R);
    staged.push_back(e);
  }
  for (int i = 0; i < n; i++) {
    const T d[3] = {(T)dirs[3*i], (T)dirs[3*i + 1], (T)dirs[3*i + 2]};
    const T len = cam_sqrt(d[0]*d[0] + d[1]*d[1] + d[2]*d[2]);
    RayHit<T> h;
    h.id = -1; h.x = 0;
    for (const CamGeom<T>& e : staged) {
      T lv[3];
      for (int r = 0; r < 3; r++) lv[r] = e.M[3*r]*d[0] + e.M[3*r + 1]*d[1] + e.M[3*r + 2]*d[2];
      int part;
      ray_take(cam_ray_local(e.type, e.size, e.lp, lv, &part), e.id, len, (T)cutoff, &h);
    }
    dist[i] = h.id >= 0 ? (double)h.x : -1.0;
    gid[i] = h.id;
  }
}

extern "C" void ray_emu_cast(int prec, int n, const double* pnt, const double* vec, const int* bex, int ngeom, const int* type,
                             const int* body, const int* skip, const double* size, const double* gpos, const double* gmat,
                             double cutoff, double* dist, int* gid, double* normal) {
  if (prec == 64) cast_t<double>(n, pnt, vec, bex, ngeom, type, body, skip, size, gpos, gmat, cutoff, dist, gid, normal);
  else cast_t<float>(n, pnt, vec, bex, ngeom, type, body, skip, size, gpos, gmat, cutoff, dist, gid, normal);
}

extern "C" void ray_emu_scan(int prec, int frame_type, const double* fpos, const double* fmat, const double* offset, int bex,
                             int n, const double* dirs, int ngeom, const int* type, const int* body, const int* skip,
                             const double* size, const double* gpos, const double* gmat, double cutoff, double* dist, int* gid) {
  if (prec == 64) scan_t<double>(frame_type, fpos, fmat, offset, bex, n, dirs, ngeom, type, body, skip, size, gpos, gmat, cutoff, dist, gid);
  else scan_t<float>(frame_type, fpos, fmat, offset, bex, n, dirs, ngeom, type, body, skip, size, gpos, gmat, cutoff, dist, gid);
}

// the step kernel's rangefinder code on the same rays: nearest ray_geom_any over the same geoms, fp64
extern "C" void ray_emu_step(int n, const double* pnt, const double* vec, const int* bex, int ngeom, const int* type,
                             const int* body, const int* skip, const double* size, const double* gpos, const double* gmat,
                             double* dist, int* gid) {
  for (int i = 0; i < n; i++) {
    double best = -1;
    int id = -1;
    for (int g = 0; g < ngeom; g++) {
      if (skip[g] || body[g] == bex[i]) continue;
      const double x = ray_geom_any(gpos + 3*g, gmat + 9*g, size + 3*g, pnt + 3*i, vec + 3*i, type[g]);
      if (x >= 0 && (id < 0 || x < best)) { best = x; id = g; }
    }
    dist[i] = best;
    gid[i] = id;
  }
}
