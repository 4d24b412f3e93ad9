// TEST INFRASTRUCTURE: host build of the camera's texture functions (dm_control_amd/csrc/camera_core.h) -- the same text
// the render kernel's textured instantiation compiles, run by a plain loop over geoms and pixels the way the kernel's
// shading stage calls them.  Materials arrive as flat arrays: mi (ngeom, 6) = mapping, builtin, mark, W, H, texuniform;
// md (ngeom, 11) = texrepeat (2), rgb1 (3), rgb2 (3), markrgb (3).
#include <vector>

#include "../../dm_control_amd/csrc/camera_core.h"

using namespace dmc;

namespace {
template <typename T>
CamMat<T> material(const int* mi, const double* md) {
  CamMat<T> m;
  m.mapping = mi[0]; m.builtin = mi[1]; m.mark = mi[2]; m.W = mi[3]; m.H = mi[4]; m.uniform = mi[5];
  for (int k = 0; k < 2; k++) m.rep[k] = (T)md[k];
  for (int k = 0; k < 3; k++) { m.rgb1[k] = (float)md[2 + k]; m.rgb2[k] = (float)md[5 + k]; m.markrgb[k] = (float)md[8 + k]; }
  return m;
}

template <typename T>
void render_t(const double* cam_pos, const double* cam_mat, double fovy_deg, int H, int W, int ngeom, const int* type,
              const int* skip, const double* size, const double* gpos, const double* gmat, const float* color, const int* mi,
              const double* md, int filter, int sky, const float* sky1, const float* sky2, double near_, double far_,
              double ambient, double diffuse, double* depth, int* gid, uint8_t* rgb) {
  T cpos[3], R[9];
  for (int k = 0; k < 3; k++) cpos[k] = (T)cam_pos[k];
  for (int k = 0; k < 9; k++) R[k] = (T)cam_mat[k];
  const T inv_f = (T)(tan(0.5*fovy_deg*3.14159265358979323846/180.0)/(0.5*H));
  std::vector<CamGeom<T>> list, all((size_t)ngeom);
  for (int g = 0; g < ngeom; g++) {
    T gp[3], gm[9], sz[3];
    for (int k = 0; k < 3; k++) { gp[k] = (T)gpos[3*g + k]; sz[k] = (T)size[3*g + k]; }
    for (int k = 0; k < 9; k++) gm[k] = (T)gmat[9*g + k];
    cam_stage_geom(&all[g], gp, gm, sz, type[g], g, cpos, R);
    if (!skip[g]) list.push_back(all[g]);
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
    if (h.id >= 0) {
      const CamMat<T> m = material<T>(mi + 6*h.id, md + 11*h.id);
      float col[3] = {color[3*h.id], color[3*h.id + 1], color[3*h.id + 2]};
      if (m.mapping != CAM_MAP_NONE) {
        float tex[3];
        cam_texture(m, h, all[h.id].M, inv_f, filter, tex);
        for (int k = 0; k < 3; k++) col[k] *= tex[k];
      }
      cam_shade(h, dx, dy, col, (T)ambient, (T)diffuse, px);
    } else if (sky) cam_sky(sky1, sky2, sky - 1, R, dx, dy, px);
    for (int k = 0; k < 3; k++) rgb[3*o + k] = px[k];
  }
}
}  // namespace

extern "C" void cam_tex_emu_render(int prec, const double* cam_pos, const double* cam_mat, double fovy_deg, int H, int W, int ngeom,
                                   const int* type, const int* skip, const double* size, const double* gpos, const double* gmat,
                                   const float* color, const int* mi, const double* md, int filter, int sky, const float* sky1,
                                   const float* sky2, double near_, double far_, double ambient, double diffuse, double* depth,
                                   int* gid, uint8_t* rgb) {
  if (prec == 64) render_t<double>(cam_pos, cam_mat, fovy_deg, H, W, ngeom, type, skip, size, gpos, gmat, color, mi, md, filter, sky, sky1, sky2, near_, far_, ambient, diffuse, depth, gid, rgb);
  else render_t<float>(cam_pos, cam_mat, fovy_deg, H, W, ngeom, type, skip, size, gpos, gmat, color, mi, md, filter, sky, sky1, sky2, near_, far_, ambient, diffuse, depth, gid, rgb);
}

// unit access, fp64: texel colour at (u, v); the box-filtered colour over (u -+ hu, v -+ hv)
extern "C" void cam_tex_emu_texel(const int* mi, const double* md, double u, double v, float* out) {
  cam_texel(material<double>(mi, md), u, v, out);
}
extern "C" void cam_tex_emu_box(int prec, const int* mi, const double* md, double u, double v, double hu, double hv, float* out) {
  if (prec == 64) cam_texel_box(material<double>(mi, md), u, v, hu, hv, out);
  else cam_texel_box(material<float>(mi, md), (float)u, (float)v, (float)hu, (float)hv, out);
}
// cube mapping of the local point p on a geom of `type` and `size`: returns the face, writes (u, v)
extern "C" int cam_tex_emu_cube(const int* mi, const double* md, int type, const double* size, const double* p, double* uv) {
  return cam_cube_uv(material<double>(mi, md), type, size, p, uv);
}
extern "C" void cam_tex_emu_sky(const float* rgb1, const float* rgb2, int builtin, const double* R, double dx, double dy, uint8_t* out) {
  cam_sky(rgb1, rgb2, builtin, R, dx, dy, out);
}
