// camera_core.h -- the geometric camera: ray / primitive closed forms in a geom's own frame, surface normals, camera
// poses, the headlight shading and the analytic textures.  Everything here is plain C++ on one pixel or one camera, so that the same text
// builds for the device (camera_kernels.hip) and for the host (tests/emu/camera_emu.cpp).
//
// The rays are the ones rangefinder sensors cast (step_geom.h ray_geom / ray_geom_any: planes front-side only and finite
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
// the primitives cam_ray_local has a closed form for: what the cameras draw and the rays hit
CAM_DEV bool cam_primitive(int type) {
  return type == DMC_GEOM_PLANE || type == DMC_GEOM_SPHERE || type == DMC_GEOM_CAPSULE || type == DMC_GEOM_ELLIPSOID ||
         type == DMC_GEOM_CYLINDER || type == DMC_GEOM_BOX;
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

// ---- analytic textures ------------------------------------------------------------------------------------------------
// The builtin patterns are closed-form functions of (u, v); nothing is stored as texels.  A texture has W x H texels and
// nearest sampling is the ground truth: i = floor(frac(u) W), j = floor(frac(v) H).  Along each axis a texel belongs to
// one of three classes -- 0 mark, 1 first half (2 i < W), 2 second half -- and the colour depends on the class pair only
// (the gradient: on the texel), which is what makes the box filter below exact.
enum { CAM_MAP_NONE = 0, CAM_MAP_PLANE = 1, CAM_MAP_CUBE = 2 };      // how (u, v) comes from the hit point
enum { CAM_TEX_FLAT = 0, CAM_TEX_CHECKER = 1, CAM_TEX_GRADIENT = 2 };
enum { CAM_MARK_NONE = 0, CAM_MARK_EDGE = 1, CAM_MARK_CROSS = 2 };
enum { CAM_FILTER_NEAREST = 0, CAM_FILTER_BOX = 1 };

template <typename T>
struct CamMat {      // the material of one geom, device form of dmc_camera_material
  int mapping, builtin, mark, W, H, uniform;
  T rep[2];
  float rgb1[3], rgb2[3], markrgb[3];
};

template <typename T> CAM_DEV T cam_floor(T x);
template <> CAM_DEV float cam_floor<float>(float x) { return floorf(x); }
template <> CAM_DEV double cam_floor<double>(double x) { return floor(x); }

template <typename T>
CAM_DEV int cam_texel_index(T u, int W) {
  const int i = (int)cam_floor((u - cam_floor(u))*(T)W);
  return i < 0 ? 0 : (i > W - 1 ? W - 1 : i);      // (frac(u) W can round up to W)
}

CAM_DEV int cam_texel_class(int i, int W, int mark) {
  if (mark == CAM_MARK_EDGE && (i == 0 || i == W - 1)) return 0;
  if (mark == CAM_MARK_CROSS && i == W/2) return 0;
  return 2*i < W ? 1 : 2;
}

// smooth step of the distance of texel (i, j)'s centre from the middle of the texture, in [-1, 1]^2
template <typename T>
CAM_DEV T cam_gradient_step(int i, int j, int W, int H) {
  const T x = (T)(2*i + 1)/(T)W - 1, y = (T)(2*j + 1)/(T)H - 1;
  T p = cam_sqrt(x*x + y*y);
  p = p > 1 ? (T)1 : p;
  return p*p*(3 - 2*p);
}

// colour of the class pair (cu, cv); gs: the gradient's step at the texel
template <typename T>
CAM_DEV void cam_pair_color(const CamMat<T>& m, int cu, int cv, T gs, T* out) {
  for (int k = 0; k < 3; k++) {
    if (cu == 0 || cv == 0) out[k] = (T)m.markrgb[k];
    else if (m.builtin == CAM_TEX_GRADIENT) out[k] = (T)m.rgb1[k] + ((T)m.rgb2[k] - (T)m.rgb1[k])*gs;
    else out[k] = (T)(m.builtin == CAM_TEX_CHECKER && cu != cv ? m.rgb2[k] : m.rgb1[k]);
  }
}

template <typename T>
CAM_DEV void cam_texel(const CamMat<T>& m, T u, T v, float* out) {
  const int i = cam_texel_index(u, m.W), j = cam_texel_index(v, m.H);
  T c[3];
  cam_pair_color(m, cam_texel_class(i, m.W, m.mark), cam_texel_class(j, m.H, m.mark),
                 m.builtin == CAM_TEX_GRADIENT ? cam_gradient_step<T>(i, j, m.W, m.H) : (T)0, c);
  for (int k = 0; k < 3; k++) out[k] = (float)c[k];
}

// integral over [0, x] of the 1-periodic indicator of [a, b), 0 <= a <= b <= 1: whole periods plus the clamped remainder
template <typename T>
CAM_DEV T cam_periodic_integral(T x, T a, T b) {
  const T n = cam_floor(x), f = x - n;
  return n*(b - a) + (f < a ? (T)0 : (f > b ? b : f) - a);
}
template <typename T>
CAM_DEV T cam_interval_share(T x0, T x1, T a, T b) {
  return (cam_periodic_integral(x1, a, b) - cam_periodic_integral(x0, a, b))/(x1 - x0);
}

// the exact shares w[0..2] of [u - h, u + h] that fall into the three classes of a W-texel axis; h <= 0: the texel at u
template <typename T>
CAM_DEV void cam_class_shares(T u, T h, int W, int mark, T* w) {
  if (!(h > 0)) {
    const int c = cam_texel_class(cam_texel_index(u, W), W, mark);
    w[0] = c == 0; w[1] = c == 1; w[2] = c == 2;
    return;
  }
  T a0 = 0, b0 = 0, a1 = 0, b1 = 0;      // the mark's texels: at most two intervals of [0, 1)
  if (mark == CAM_MARK_EDGE) { b0 = (T)1/(T)W; if (W > 1) { a1 = (T)(W - 1)/(T)W; b1 = 1; } }
  else if (mark == CAM_MARK_CROSS) { a0 = (T)(W/2)/(T)W; b0 = (T)(W/2 + 1)/(T)W; }
  const T hb = (T)((W + 1)/2)/(T)W;      // the first half ends where 2 i < W does
  const T x0 = u - h, x1 = u + h;
  w[0] = cam_interval_share(x0, x1, a0, b0) + cam_interval_share(x0, x1, a1, b1);
  w[1] = cam_interval_share(x0, x1, (T)0, hb) - cam_interval_share(x0, x1, a0 < hb ? a0 : hb, b0 < hb ? b0 : hb)
       - cam_interval_share(x0, x1, a1 < hb ? a1 : hb, b1 < hb ? b1 : hb);
  w[2] = 1 - w[0] - w[1];
}

// box filter: the mean of the nearest-sampled pattern over the uv box (u -+ hu, v -+ hv), as the sum over the 3 x 3 class
// pairs of share_u share_v colour(pair).  The gradient is evaluated at the centre.
template <typename T>
CAM_DEV void cam_texel_box(const CamMat<T>& m, T u, T v, T hu, T hv, float* out) {
  T wu[3], wv[3], acc[3] = {0, 0, 0};
  cam_class_shares(u, hu, m.W, m.mark, wu);
  cam_class_shares(v, hv, m.H, m.mark, wv);
  const T gs = m.builtin == CAM_TEX_GRADIENT ? cam_gradient_step<T>(cam_texel_index(u, m.W), cam_texel_index(v, m.H), m.W, m.H) : (T)0;
  for (int cu = 0; cu < 3; cu++) for (int cv = 0; cv < 3; cv++) {
    T c[3];
    cam_pair_color(m, cu, cv, gs, c);
    for (int k = 0; k < 3; k++) acc[k] += wu[cu]*wv[cv]*c[k];
  }
  for (int k = 0; k < 3; k++) out[k] = (float)acc[k];
}

// 2d texture on a plane: (u, v) of the hit point (px, py) in the plane's frame and the scales du/dpx, dv/dpy
template <typename T>
CAM_DEV void cam_plane_uv(const CamMat<T>& m, const T* size, T px, T py, T* uv, T* scale) {
  if (m.uniform) { scale[0] = m.rep[0]; scale[1] = m.rep[1]; uv[0] = px*m.rep[0]; uv[1] = py*m.rep[1]; return; }
  const T sx = size[0] > 0 ? size[0] : (T)1, sy = size[1] > 0 ? size[1] : (T)1;
  scale[0] = m.rep[0]/(2*sx); scale[1] = m.rep[1]/(2*sy);
  uv[0] = m.rep[0]*(px/(2*sx) + (T)0.5); uv[1] = m.rep[1]*(py/(2*sy) + (T)0.5);
}

// Half-widths (in the plane's x and y) of a pixel's footprint, 0.5 (|dp/dcol| + |dp/drow|), from the closed-form
// derivative of the ray / plane intersection p = lp - (lp_z / lv_z) lv with respect to the pixel direction:
// lv = M (dx, dy, -1), d(dx)/d(col) = inv_f, d(dy)/d(row) = -inv_f.
template <typename T>
CAM_DEV void cam_plane_footprint(const T* lp, const T* lv, const T* M, T inv_f, T* half) {
  const T s = -lp[2]/(lv[2]*lv[2])*inv_f;
  for (int k = 0; k < 2; k++) {
    const T dc = s*(M[3*k]*lv[2] - lv[k]*M[6]), dr = s*(M[3*k + 1]*lv[2] - lv[k]*M[7]);
    half[k] = (T)0.5*(cam_abs(dc) + cam_abs(dr));
  }
}

// cube texture on a solid: the face is the largest |component| of the local hit point q (divided by the half-extents
// unless texuniform), lowest axis on ties; the other two components in cyclic order, over |q_face|, go to [0, 1] x repeat
template <typename T>
CAM_DEV int cam_cube_uv(const CamMat<T>& m, int type, const T* size, const T* p, T* uv) {
  T q[3] = {p[0], p[1], p[2]};
  if (!m.uniform) {
    const bool round = type == DMC_GEOM_SPHERE || type == DMC_GEOM_CAPSULE || type == DMC_GEOM_CYLINDER;
    const T ex = size[0], ey = round ? size[0] : size[1];
    const T ez = type == DMC_GEOM_SPHERE ? size[0] : type == DMC_GEOM_CAPSULE ? size[0] + size[1] : type == DMC_GEOM_CYLINDER ? size[1] : size[2];
    q[0] /= ex; q[1] /= ey; q[2] /= ez;
  }
  const T a0 = cam_abs(q[0]), a1 = cam_abs(q[1]), a2 = cam_abs(q[2]);
  int face = a1 > a0 ? 1 : 0;
  if (a2 > (face ? a1 : a0)) face = 2;
  const T den = face == 0 ? a0 : face == 1 ? a1 : a2;
  const T s = face == 0 ? q[1] : face == 1 ? q[2] : q[0], t = face == 0 ? q[2] : face == 1 ? q[0] : q[1];
  const bool ok = den >= (T)DMC_MINVAL;
  uv[0] = m.rep[0]*(T)0.5*((ok ? s/den : (T)0) + 1);
  uv[1] = m.rep[1]*(T)0.5*((ok ? t/den : (T)0) + 1);
  return face;
}

// texel colour at the final hit of a pixel (white where the material maps nothing onto this geom type).  M = Rg' Rcam of
// the hit geom and inv_f are read only under the box filter on a plane.
template <typename T>
CAM_DEV void cam_texture(const CamMat<T>& m, const CamHit<T>& h, const T* M, T inv_f, int filter, float* out) {
  out[0] = 1; out[1] = 1; out[2] = 1;
  const T p[3] = {h.lp[0] + h.t*h.lv[0], h.lp[1] + h.t*h.lv[1], h.lp[2] + h.t*h.lv[2]};
  T uv[2];
  if (m.mapping == CAM_MAP_PLANE && h.type == DMC_GEOM_PLANE) {
    T scale[2];
    cam_plane_uv(m, h.size, p[0], p[1], uv, scale);
    if (filter == CAM_FILTER_BOX) {
      T half[2];
      cam_plane_footprint(h.lp, h.lv, M, inv_f, half);
      cam_texel_box(m, uv[0], uv[1], cam_abs(scale[0])*half[0], cam_abs(scale[1])*half[1], out);
    } else cam_texel(m, uv[0], uv[1], out);
  } else if (m.mapping == CAM_MAP_CUBE && h.type != DMC_GEOM_PLANE) {
    cam_cube_uv(m, h.type, h.size, p, uv);
    cam_texel(m, uv[0], uv[1], out);
  }
}

template <typename T>
CAM_DEV uint8_t cam_round8(T v) {
  v = v < 0 ? (T)0 : (v > 1 ? (T)1 : v);
  return (uint8_t)(int)floor((double)(255*v + (T)0.5));
}

// skybox: the smooth step of p = (1 - w_z) / 2 between rgb1 (zenith) and rgb2 (nadir), w the unit world direction of
// the ray; unshaded
template <typename T>
CAM_DEV void cam_sky(const float* rgb1, const float* rgb2, int builtin, const T* R, T dx, T dy, uint8_t* out) {
  const T wz = (R[6]*dx + R[7]*dy - R[8])/cam_sqrt(dx*dx + dy*dy + 1);
  const T p = (T)0.5*(1 - wz), s = builtin == CAM_TEX_GRADIENT ? p*p*(3 - 2*p) : (T)0;
  for (int k = 0; k < 3; k++) out[k] = cam_round8((T)rgb1[k] + ((T)rgb2[k] - (T)rgb1[k])*s);
}

template <typename T>
struct CamTexArgs {      // what a render with textures reads beside CamArgs
  const CamMat<T>* mat;      // (ngeom)
  int filter, sky;           // CAM_FILTER_*; sky: 0 constant background, else 1 + CAM_TEX_FLAT / CAM_TEX_GRADIENT
  float sky1[3], sky2[3];
};

int launch_camera_tex_f32(const CamArgs<float>& a, const CamTexArgs<float>& t, void* stream);
int launch_camera_tex_f64(const CamArgs<double>& a, const CamTexArgs<double>& t, void* stream);

}  // namespace dmc
