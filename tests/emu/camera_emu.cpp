// TEST INFRASTRUCTURE: host build of the camera's per-pixel device functions (dm_control_amd/csrc/camera_core.h) -- the
// same text the render kernel compiles, run by a plain loop over cameras, geoms and pixels.
#include <vector>

#include "../../dm_control_amd/csrc/camera_core.h"

using namespace dmc;

namespace {
template <typename T>
void render_t(const double* cam_pos, const double* cam_mat, double fovy_deg, int H, int W, int ngeom, const int* type,
              const int* skip, const double* size, const double* gpos, const double* gmat, const float* color, double near_,
              double far_, double ambient, double diffuse, double* depth, int* gid, uint8_t* rgb) {
  T cpos[3], R[9];
  for (int k = 0; k < 3; k++) cpos[k] = (T)cam_pos[k];
  for (int k = 0; k < 9; k++) R[k] = (T)cam_mat[k];
  const T inv_f = (T)(tan(0.5*fovy_deg*3.14159265358979323846/180.0)/(0.5*H));
  std::vector<CamGeom<T>> list;
  for (int g = 0; g < ngeom; g++) {
    if (skip[g]) continue;
    T gp[3], gm[9], sz[3];
    for (int k = 0; k < 3; k++) { gp[k] = (T)gpos[3*g + k]; sz[k] = (T)size[3*g + k]; }
    for (int k = 0; k < 9; k++) gm[k] = (T)gmat[9*g + k];
    CamGeom<T> e;
    cam_stage_geom(&e, gp, gm, sz, type[g], g, cpos, R);
    list.push_back(e);
  }
  const T hx = (T)0.5*(W - 1), hy = (T)0.5*(H - 1);
  for (int r = 0; r < H; r++) for (int c = 0; c < W; c++) {
    const T dx = (c - hx)*inv_f, dy = -(r - hy)*inv_f;
    CamHit<T> h;
    h.id = -1; h.t = 0; h.type = 0; h.part = 0;
    for (const CamGeom<T>& e : list) cam_pixel_geom(e, dx, dy, (T)near_, (T)far_, &h);
    const int o = r*W + c;
    depth[o] = h.id >= 0 ? (double)h.t : far_;
    gid[o] = h.id;
    uint8_t px[3] = {0, 0, 0};
    if (h.id >= 0) cam_shade(h, dx, dy, color + 3*h.id, (T)ambient, (T)diffuse, px);
    for (int k = 0; k < 3; k++) rgb[3*o + k] = px[k];
  }
}
}  // namespace

extern "C" void cam_emu_render(int prec, const double* cam_pos, const double* cam_mat, double fovy_deg, int H, int W, int ngeom,
                               const int* type, const int* skip, const double* size, const double* gpos, const double* gmat,
                               const float* color, double near_, double far_, double ambient, double diffuse, double* depth,
                               int* gid, uint8_t* rgb) {
  if (prec == 64) render_t<double>(cam_pos, cam_mat, fovy_deg, H, W, ngeom, type, skip, size, gpos, gmat, color, near_, far_, ambient, diffuse, depth, gid, rgb);
  else render_t<float>(cam_pos, cam_mat, fovy_deg, H, W, ngeom, type, skip, size, gpos, gmat, color, near_, far_, ambient, diffuse, depth, gid, rgb);
}

// camera frames: xpos (nbody, 3), xmat (nbody, 9), com (nbody, 3) of one environment
extern "C" void cam_emu_pose(int mode, int body, int target, const double* pos, const double* mat, const double* pos0,
                             const double* poscom0, const double* mat0, const double* xpos, const double* xmat,
                             const double* com, double* out_pos, double* out_mat) {
  CamDev<double> c;
  c.mode = mode; c.body = body; c.target = target; c.pad = 0; c.inv_f = 1;
  for (int k = 0; k < 3; k++) { c.pos[k] = pos[k]; c.pos0[k] = pos0[k]; c.poscom0[k] = poscom0[k]; }
  for (int k = 0; k < 9; k++) { c.mat[k] = mat[k]; c.mat0[k] = mat0[k]; }
  cam_pose(c, xpos, xmat, com, (size_t)1, out_pos, out_mat);
}
