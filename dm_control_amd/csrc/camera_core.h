// camera_core.h -- the geometric camera: ray / primitive closed forms in a geom's own frame, surface normals, camera
// poses and the headlight shading.  Everything here is plain C++ on one pixel or one camera, so that the same text
// builds for the device (camera_kernels.hip) and for the host (tests/emu/camera_emu.cpp).
//
// The rays are the ones rangefinder sensors cast (step_core.h ray_geom / ray_geom_any: planes front-side only and finite
// where their half-sizes are positive, a ray that starts inside a box leaves through a face).  Those functions take a
// world-frame pose and transform the ray themselves; a camera shares one origin between all its pixels, so the render
// kernel transforms once per (camera, geom) -- lp = Rg' (cam_pos - geom_pos), M = Rg' Rcam -- and the closed forms are
// restated here on (lp, lv) with the part of the surface that was hit, which the normals need.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dmc_model_layout.h"

#if defined(__HIPCC__)
#define CAM_DEV __host__ __device__ __forceinline__
#else
#define CAM_DEV inline
#endif

namespace dmc {

enum { CAM_FIXED = 0, CAM_TRACK = 1, CAM_TRACKCOM = 2, CAM_TARGETBODY = 3, CAM_TARGETBODYCOM = 4 };
enum { CAM_RGB = 1, CAM_DEPTH = 2, CAM_SEG = 4 };
constexpr int kCamTile = 256;      // pixels (= lanes) of one workgroup: consecutive in the row-major image
constexpr int kCamObjGeom = 5;     // mjOBJ_GEOM

template <typename T>
struct CamDev {      // one camera, device form of dmc_camera_spec
  int mode, body, target, pad;
  T pos[3], mat[9], pos0[3], poscom0[3], mat0[9], inv_f;      // inv_f = 1 / (0.5 H / tan(fovy / 2))
};

template <typename T>
struct CamGeom {      // a geom staged for one camera: ray-ready
  T lp[3], M[9], size[3];
  int type, id;
};

template <typename T> CAM_DEV T cam_sqrt(T x);
template <> CAM_DEV float cam_sqrt<float>(float x) { return sqrtf(x); }
template <> CAM_DEV double cam_sqrt<double>(double x) { return sqrt(x); }
template <typename T> CAM_DEV T cam_abs(T x) { return x < 0 ? -x : x; }

// roots x0 <= x1 of |q + x v|^2 = r2 over the first n components, through the point of closest approach: x = t0 -+ h with
// t0 = -(q.v) / (v.v), h^2 = (r2 - |q + t0 v|^2) / (v.v).  The textbook discriminant b^2 - a c cancels catastrophically
// for a thin primitive far away (fp32: |x|^2 / r^2 ulps); this form loses nothing to the distance.
template <typename T>
CAM_DEV bool cam_quadratic(const T* q, const T* v, int n, T r2, T* x0, T* x1) {
  T a = 0, b = 0;
  for (int k = 0; k < n; k++) { a += v[k]*v[k]; b += q[k]*v[k]; }
  if (a < (T)DMC_MINVAL) return false;
  const T t0 = -b/a;
  T cc = -r2;
  for (int k = 0; k < n; k++) { const T p = q[k] + t0*v[k]; cc += p*p; }
  if (cc > 0) return false;
  const T h = cam_sqrt(-cc/a);
  *x0 = t0 - h; *x1 = t0 + h;
  return true;
}

// nearest non-negative ray parameter of (lp + x lv) on the primitive, or -1; *part says which piece of the surface:
// capsule 0 side / 1 upper cap / 2 lower cap, cylinder 0 side / 1 top / 2 bottom, box 2 axis + (positive face)
template <typename T>
CAM_DEV T cam_ray_local(int type, const T* size, const T* lp, const T* lv, int* part) {
  T best = -1;
  *part = 0;
  if (type == DMC_GEOM_PLANE) {
    if (lv[2] > -(T)DMC_MINVAL) return -1;
    const T x = -lp[2]/lv[2];
    if (x < 0) return -1;
    const T px = lp[0] + x*lv[0], py = lp[1] + x*lv[1];
    if ((size[0] <= 0 || cam_abs(px) <= size[0]) && (size[1] <= 0 || cam_abs(py) <= size[1])) return x;
    return -1;
  }
  if (type == DMC_GEOM_SPHERE || type == DMC_GEOM_CAPSULE) {
    const T r = size[0];
    const int nparts = type == DMC_GEOM_CAPSULE ? 3 : 1;
    for (int p = 0; p < nparts; p++) {
      const T cz = type == DMC_GEOM_CAPSULE ? (p == 1 ? size[1] : p == 2 ? -size[1] : (T)0) : (T)0;
      const T q[3] = {lp[0], lp[1], lp[2] - cz};
      T xs[2];
      if (!cam_quadratic(q, lv, type == DMC_GEOM_CAPSULE && p == 0 ? 2 : 3, r*r, &xs[0], &xs[1])) continue;
      for (int k = 0; k < 2; k++) {
        const T x = xs[k];
        if (x < 0) continue;
        const T z = lp[2] + x*lv[2];
        if (type == DMC_GEOM_CAPSULE) {
          if (p == 0 && cam_abs(z) > size[1]) continue;
          if (p == 1 && z < size[1]) continue;
          if (p == 2 && z > -size[1]) continue;
        }
        if (best < 0 || x < best) { best = x; *part = p; }
      }
    }
    return best;
  }
  if (type == DMC_GEOM_ELLIPSOID) {
    const T q[3] = {lp[0]/size[0], lp[1]/size[1], lp[2]/size[2]}, w[3] = {lv[0]/size[0], lv[1]/size[1], lv[2]/size[2]};
    T x0, x1;
    if (!cam_quadratic(q, w, 3, (T)1, &x0, &x1)) return -1;
    return x0 >= 0 ? x0 : (x1 >= 0 ? x1 : (T)-1);
  }
  if (type == DMC_GEOM_CYLINDER) {
    T xs[2];
    if (cam_quadratic(lp, lv, 2, size[0]*size[0], &xs[0], &xs[1])) for (int k = 0; k < 2; k++) {
      const T x = xs[k];
      if (x >= 0 && cam_abs(lp[2] + x*lv[2]) <= size[1]) if (best < 0 || x < best) { best = x; *part = 0; }
    }
    if (cam_abs(lv[2]) >= (T)DMC_MINVAL) for (int sg = -1; sg <= 1; sg += 2) {
      const T x = (sg*size[1] - lp[2]) / lv[2];
      if (x < 0) continue;
      const T px = lp[0] + x*lv[0], py = lp[1] + x*lv[1];
      if (px*px + py*py <= size[0]*size[0]) if (best < 0 || x < best) { best = x; *part = sg > 0 ? 1 : 2; }
    }
    return best;
  }
  if (type == DMC_GEOM_BOX) {
    for (int ax = 0; ax < 3; ax++) {
      if (cam_abs(lv[ax]) < (T)DMC_MINVAL) continue;
      const int a1 = (ax + 1) % 3, a2 = (ax + 2) % 3;
      for (int sg = -1; sg <= 1; sg += 2) {
        const T x = (sg*size[ax] - lp[ax]) / lv[ax];
        if (x < 0) continue;
        if (cam_abs(lp[a1] + x*lv[a1]) <= size[a1] && cam_abs(lp[a2] + x*lv[a2]) <= size[a2])
          if (best < 0 || x < best) { best = x; *part = 2*ax + (sg > 0); }
      }
    }
    return best;
  }
  return -1;      // meshes and height fields are scenery the camera does not draw
}

// outward unit normal, in the geom's frame, of the point lp + x lv found by cam_ray_local
template <typename T>
CAM_DEV void cam_normal_local(int type, const T* size, const T* lp, const T* lv, T x, int part, T* n) {
  T p[3] = {lp[0] + x*lv[0], lp[1] + x*lv[1], lp[2] + x*lv[2]};
  n[0] = 0; n[1] = 0; n[2] = 1;
  if (type == DMC_GEOM_PLANE) return;
  if (type == DMC_GEOM_BOX) { n[2] = 0; n[part >> 1] = (part & 1) ? (T)1 : (T)-1; return; }
  if (type == DMC_GEOM_CYLINDER && part != 0) { n[2] = part == 1 ? (T)1 : (T)-1; return; }
  if (type == DMC_GEOM_CYLINDER || (type == DMC_GEOM_CAPSULE && part == 0)) p[2] = 0;
  else if (type == DMC_GEOM_CAPSULE) p[2] -= part == 1 ? size[1] : -size[1];
  else if (type == DMC_GEOM_ELLIPSOID) for (int k = 0; k < 3; k++) p[k] /= size[k]*size[k];
  const T len = cam_sqrt(p[0]*p[0] + p[1]*p[1] + p[2]*p[2]);
  if (len < (T)DMC_MINVAL) return;
  for (int k = 0; k < 3; k++) n[k] = p[k]/len;
}

// bounding radius from the size in force (mjcf_compiler._geom_rbound; 0 = unbounded: planes are never culled)
template <typename T>
CAM_DEV T cam_rbound(int type, const T* s) {
  switch (type) {
    case DMC_GEOM_SPHERE: return s[0];
    case DMC_GEOM_CAPSULE: return s[0] + s[1];
    case DMC_GEOM_CYLINDER: return cam_sqrt(s[0]*s[0] + s[1]*s[1]);
    case DMC_GEOM_ELLIPSOID: return s[0] > s[1] ? (s[0] > s[2] ? s[0] : s[2]) : (s[1] > s[2] ? s[1] : s[2]);
    case DMC_GEOM_BOX: return cam_sqrt(s[0]*s[0] + s[1]*s[1] + s[2]*s[2]);
    default: return 0;
  }
}

// Camera frame of one environment.  xpos / xmat / subtree_com: the environment's rows, element k at [k * stride].
// targetbody modes: -z looks at the target, x = normalise(z_world x z_cam), y = z_cam x x (x = world x when the line of
// sight is vertical).
template <typename T>
CAM_DEV void cam_pose(const CamDev<T>& c, const T* xpos, const T* xmat, const T* subtree_com, size_t stride, T* pos, T* R) {
  const int b = c.body;
  if (c.mode == CAM_TRACK || c.mode == CAM_TRACKCOM) {
    const T* base = c.mode == CAM_TRACK ? xpos : subtree_com;
    const T* off = c.mode == CAM_TRACK ? c.pos0 : c.poscom0;
    for (int k = 0; k < 3; k++) pos[k] = base[(size_t)(3*b + k)*stride] + off[k];
    for (int k = 0; k < 9; k++) R[k] = c.mat0[k];
    return;
  }
  T bm[9];
  for (int k = 0; k < 9; k++) bm[k] = xmat[(size_t)(9*b + k)*stride];
  for (int i = 0; i < 3; i++)
    pos[i] = xpos[(size_t)(3*b + i)*stride] + (bm[3*i]*c.pos[0] + bm[3*i + 1]*c.pos[1] + bm[3*i + 2]*c.pos[2]);
  if (c.mode == CAM_FIXED) {
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++)
      R[3*i + j] = bm[3*i]*c.mat[j] + bm[3*i + 1]*c.mat[3 + j] + bm[3*i + 2]*c.mat[6 + j];
    return;
  }
  const T* tp = c.mode == CAM_TARGETBODY ? xpos : subtree_com;
  T z[3], x[3], y[3];
  for (int k = 0; k < 3; k++) z[k] = pos[k] - tp[(size_t)(3*c.target + k)*stride];
  T len = cam_sqrt(z[0]*z[0] + z[1]*z[1] + z[2]*z[2]);
  if (len < (T)DMC_MINVAL) { z[0] = 0; z[1] = 0; z[2] = 1; len = 1; }
  for (int k = 0; k < 3; k++) z[k] /= len;
  x[0] = -z[1]; x[1] = z[0]; x[2] = 0;      // (0, 0, 1) x z
  len = cam_sqrt(x[0]*x[0] + x[1]*x[1]);
  if (len < (T)DMC_MINVAL) { x[0] = 1; x[1] = 0; len = 1; }
  x[0] /= len; x[1] /= len;
  y[0] = z[1]*x[2] - z[2]*x[1]; y[1] = z[2]*x[0] - z[0]*x[2]; y[2] = z[0]*x[1] - z[1]*x[0];
  for (int i = 0; i < 3; i++) { R[3*i] = x[i]; R[3*i + 1] = y[i]; R[3*i + 2] = z[i]; }
}

// a geom in ray-ready form for a camera at (cpos, R): gpos / gmat are the geom's world frame
template <typename T>
CAM_DEV void cam_stage_geom(CamGeom<T>* e, const T* gpos, const T* gmat, const T* size, int type, int id, const T* cpos, const T* R) {
  const T d[3] = {cpos[0] - gpos[0], cpos[1] - gpos[1], cpos[2] - gpos[2]};
  for (int i = 0; i < 3; i++) {
    e->lp[i] = gmat[i]*d[0] + gmat[3 + i]*d[1] + gmat[6 + i]*d[2];
    for (int j = 0; j < 3; j++) e->M[3*i + j] = gmat[i]*R[j] + gmat[3 + i]*R[3 + j] + gmat[6 + i]*R[6 + j];
  }
  for (int k = 0; k < 3; k++) e->size[k] = size[k];
  e->type = type; e->id = id;
}

// the running nearest hit of one pixel
template <typename T>
struct CamHit {
  T t, lp[3], lv[3], size[3];
  int id, type, part;
};

// one staged geom against the pixel whose camera-frame direction is (dx, dy, -1)
template <typename T>
CAM_DEV void cam_pixel_geom(const CamGeom<T>& e, T dx, T dy, T near_, T far_, CamHit<T>* h) {
  T lv[3];
  for (int i = 0; i < 3; i++) lv[i] = e.M[3*i]*dx + e.M[3*i + 1]*dy - e.M[3*i + 2];
  int part;
  const T t = cam_ray_local(e.type, e.size, e.lp, lv, &part);
  if (t < 0 || t < near_ || t > far_ || (h->id >= 0 && !(t < h->t))) return;
  h->t = t; h->id = e.id; h->type = e.type; h->part = part;
  for (int k = 0; k < 3; k++) { h->lp[k] = e.lp[k]; h->lv[k] = lv[k]; h->size[k] = e.size[k]; }
}

// The same for a record that holds the geom's WORLD frame (lp = geom_xpos, M = geom_xmat) -- the tuning study's path
// without the per-(camera, geom) pre-transform: origin and direction go into the geom's frame per pixel, 18 multiply-adds.
// wdir = Rcam (dx, dy, -1).
template <typename T>
CAM_DEV void cam_pixel_geom_world(const CamGeom<T>& e, const T* cpos, const T* wdir, T near_, T far_, CamHit<T>* h) {
  const T d[3] = {cpos[0] - e.lp[0], cpos[1] - e.lp[1], cpos[2] - e.lp[2]};
  T lp[3], lv[3];
  for (int i = 0; i < 3; i++) {
    lp[i] = e.M[i]*d[0] + e.M[3 + i]*d[1] + e.M[6 + i]*d[2];
    lv[i] = e.M[i]*wdir[0] + e.M[3 + i]*wdir[1] + e.M[6 + i]*wdir[2];
  }
  int part;
  const T t = cam_ray_local(e.type, e.size, lp, lv, &part);
  if (t < 0 || t < near_ || t > far_ || (h->id >= 0 && !(t < h->t))) return;
  h->t = t; h->id = e.id; h->type = e.type; h->part = part;
  for (int k = 0; k < 3; k++) { h->lp[k] = lp[k]; h->lv[k] = lv[k]; h->size[k] = e.size[k]; }
}

// headlight at the camera: colour (ambient + diffuse max(0, n . -d)); floor(255 clip(x, 0, 1) + 0.5)
template <typename T>
CAM_DEV void cam_shade(const CamHit<T>& h, T dx, T dy, const float* rgb, T ambient, T diffuse, uint8_t* out) {
  T n[3];
  cam_normal_local(h.type, h.size, h.lp, h.lv, h.t, h.part, n);
  const T dn = cam_sqrt(dx*dx + dy*dy + 1);
  T c = -(n[0]*h.lv[0] + n[1]*h.lv[1] + n[2]*h.lv[2])/dn;
  c = ambient + diffuse*(c > 0 ? c : (T)0);
  for (int k = 0; k < 3; k++) {
    T v = (T)rgb[k]*c;
    v = v < 0 ? (T)0 : (v > 1 ? (T)1 : v);
    out[k] = (uint8_t)(int)floor((double)(255*v + (T)0.5));
  }
}

template <typename T>
struct CamArgs {
  const T *geom_xpos, *geom_xmat, *xpos, *xmat, *subtree_com;      // (rows, B) fields of the batch
  const T* geom_size;      // the step kernel's table, (ngeom, 3)
  const T* eg_data; const int* eg_slot;      // per-environment geoms ("env_geom" rows), or null
  const int* geom_type; const int* geom_skip; const float* geom_color;      // (ngeom), (ngeom), (ngeom, 3)
  const CamDev<T>* cams;
  int B, ngeom, ncam, H, W, cull, pretransform;
  T near_, far_, ambient, diffuse;
  uint8_t bg[4];
  uint8_t* rgb; T* depth; int* seg;      // outputs, or null
};

int launch_camera_f32(const CamArgs<float>& a, void* stream);
int launch_camera_f64(const CamArgs<double>& a, void* stream);

}  // namespace dmc
