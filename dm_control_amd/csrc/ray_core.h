// ray_core.h -- caller-chosen rays against the primitive geoms: mj_ray for one ray, plain C++ that builds for the device
// (ray_kernels.hip) and for the host (tests/emu/ray_emu.cpp).
//
// The closed forms are the camera's (camera_core.h cam_ray_local / cam_normal_local, roots through the point of closest
// approach: nothing cancels in fp32 for a thin primitive far away); this header adds what a ray that is not a pixel needs:
// the transform of a world-frame ray into a geom's frame, the running nearest hit with the cutoff in metres, the
// world-frame normal, and the frames a scan moves with.  x is in units of |vec|, as in mj_ray and ray_geom_any.
#pragma once
#include "camera_core.h"

namespace dmc {

enum { RAY_FRAME_WORLD = 0, RAY_FRAME_BODY = 1, RAY_FRAME_SITE = 2, RAY_FRAME_GEOM = 3 };
constexpr int kRayBlock = 256;     // lanes of one cast workgroup = static geom records staged per pass
constexpr int kRayTile = 256;      // rays (= lanes) of one scan workgroup
constexpr int kRayPass = 64;       // geoms one staging pass of the scan kernel looks at: one wave, one ballot

template <typename T>
struct RayHit {      // the running nearest hit of one ray
  T x;
  int id;
};

// the ray (pnt, vec) of the world frame in the frame of the geom at (gpos, gmat)
template <typename T>
CAM_DEV void ray_to_local(const T* gpos, const T* gmat, const T* pnt, const T* vec, T* lp, T* lv) {
  const T d[3] = {pnt[0] - gpos[0], pnt[1] - gpos[1], pnt[2] - gpos[2]};
  for (int i = 0; i < 3; i++) {
    lp[i] = gmat[i]*d[0] + gmat[3 + i]*d[1] + gmat[6 + i]*d[2];
    lv[i] = gmat[i]*vec[0] + gmat[3 + i]*vec[1] + gmat[6 + i]*vec[2];
  }
}

// keeps x when it is a hit (x >= 0), not beyond the cutoff in metres (len = |vec|; cutoff = +inf: none) and nearer than
// what is held; equal distances keep the lower geom id, as a walk in geom order with a strict comparison does
template <typename T>
CAM_DEV void ray_take(T x, int id, T len, T cutoff, RayHit<T>* h) {
  if (x < 0 || x*len > cutoff || (h->id >= 0 && !(x < h->x))) return;
  h->x = x; h->id = id;
}

// one geom given by its world pose against one world-frame ray: mj_rayGeom's value, -1 on a miss
template <typename T>
CAM_DEV T ray_geom_world(int type, const T* size, const T* gpos, const T* gmat, const T* pnt, const T* vec) {
  T lp[3], lv[3];
  int part;
  ray_to_local(gpos, gmat, pnt, vec, lp, lv);
  return cam_ray_local(type, size, lp, lv, &part);
}

// world-frame outward unit normal where the ray meets the geom (evaluated again on the final hit only, so that the walk
// over the geoms carries a distance and an id and nothing else); false when the ray misses
template <typename T>
CAM_DEV bool ray_normal_world(int type, const T* size, const T* gpos, const T* gmat, const T* pnt, const T* vec, T* n) {
  T lp[3], lv[3], ln[3];
  int part;
  ray_to_local(gpos, gmat, pnt, vec, lp, lv);
  const T x = cam_ray_local(type, size, lp, lv, &part);
  if (x < 0) return false;
  cam_normal_local(type, size, lp, lv, x, part, ln);
  for (int i = 0; i < 3; i++) n[i] = gmat[3*i]*ln[0] + gmat[3*i + 1]*ln[1] + gmat[3*i + 2]*ln[2];
  return true;
}

template <typename T>
struct RayScan {      // one scan: a frame by id, an offset in it, the body its rays skip
  int frame_type, frame_id, bodyexclude, pad;
  T offset[3], pad2;
};

// World pose of a scan's frame for one environment: origin = frame position + R offset.  pos / mat: the environment's
// rows of the field the frame type names (xpos / xmat, site_xpos / site_xmat, geom_xpos / geom_xmat), element k at
// [k * stride]; unused (may be null) for the world frame.
template <typename T>
CAM_DEV void ray_frame_pose(const RayScan<T>& s, const T* pos, const T* mat, size_t stride, T* origin, T* R) {
  if (s.frame_type == RAY_FRAME_WORLD) {
    for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? (T)1 : (T)0;
    for (int k = 0; k < 3; k++) origin[k] = s.offset[k];
    return;
  }
  const int f = s.frame_id;
  for (int k = 0; k < 9; k++) R[k] = mat[(size_t)(9*f + k)*stride];
  for (int i = 0; i < 3; i++)
    origin[i] = pos[(size_t)(3*f + i)*stride] + (R[3*i]*s.offset[0] + R[3*i + 1]*s.offset[1] + R[3*i + 2]*s.offset[2]);
}

// whether the geom's bounding sphere (radius rb > 0 around gpos) lies wholly beyond `cutoff` metres from `origin`: no ray
// from there can hit it within the cutoff.  The comparison carries a relative margin far above the rounding of the
// distance, so that a geom is only ever dropped when ray_take would refuse its hit anyway.
template <typename T>
CAM_DEV bool ray_beyond_cutoff(const T* gpos, T rb, const T* origin, T cutoff) {
  if (!(rb > 0) || !(cutoff < (T)1e30)) return false;
  const T d[3] = {gpos[0] - origin[0], gpos[1] - origin[1], gpos[2] - origin[2]};
  const T reach = (cutoff + rb)*((T)1 + (T)1e-4);
  return d[0]*d[0] + d[1]*d[1] + d[2]*d[2] > reach*reach;
}

template <typename T>
struct RayArgs {
  const T *geom_xpos, *geom_xmat, *xpos, *xmat, *site_xpos, *site_xmat;      // (rows, B) fields of the batch
  const T* geom_size;      // the step kernel's table, (ngeom, 3)
  const T* eg_data; const int* eg_slot;      // per-environment geoms ("env_geom" rows), or null
  const int *geom_type, *geom_body;      // (ngeom)
  const int* list;      // the geoms that pass the filters fixed at create time, ascending
  int B, ngeom, nlist;
  T cutoff;      // metres; +inf: none
  // cast: (B, nray, 3) origins and directions; the excluded body as one id, (B) or (B, nray) ids
  int nray, bodyexclude, bodyexclude_per_ray;
  const T *pnt, *vec;
  const int* bodyexclude_dev;
  // scan: nscan frames, one table of ndir frame-local directions each
  int nscan, ndir;
  const RayScan<T>* scans;
  const T* dirs;      // (nscan, ndir, 3)
  // outputs, each may be null: (B, nray) or (B, nscan, ndir); normal (..., 3)
  T* dist; int* geomid; T* normal;
};

int launch_ray_cast_f32(const RayArgs<float>& a, void* stream);
int launch_ray_cast_f64(const RayArgs<double>& a, void* stream);
int launch_ray_scan_f32(const RayArgs<float>& a, void* stream);
int launch_ray_scan_f64(const RayArgs<double>& a, void* stream);

}  // namespace dmc
