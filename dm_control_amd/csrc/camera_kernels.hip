// camera_kernels.hip -- batched ray-cast cameras (dmc_camera_render): depth, segmentation and shaded RGB of every
// (environment, camera) from the geom poses a step / forward launch left in HBM.  A geometric camera, not OpenGL:
// see camera_core.h for the model.
//
// One workgroup per (environment, camera, tile of kCamTile consecutive pixels), one lane per pixel.  The camera frame is
// derived once per workgroup; the environment's visible geoms are staged into LDS in ray-ready form (origin in the
// geom's frame and M = Rg' Rcam, so a pixel's local direction is nine multiply-adds), culled against the tile's
// bounding pyramid and compacted in geom order with a ballot.  Every lane then walks the same LDS list: same-address
// reads broadcast.  Outputs are env-major and a tile's pixels are consecutive, so the stores coalesce.
#include <hip/hip_runtime.h>

#include "camera_core.h"

namespace dmc {

// kPre = false: the tuning study's kernel without the pre-transform (an instantiation of its own, so that the production
// kernel's registers do not pay for it)
// kTex = true: textures and skybox in the shading stage, again an instantiation of its own: the kTex = false kernel never
// reads `t` and is the flat-colour kernel instruction for instruction
template <typename T, bool kPre, bool kTex>
__global__ void __launch_bounds__(kCamTile) camera_kernel(const CamArgs<T> a, const CamTexArgs<T> t) {
  __shared__ CamGeom<T> s_geom[kCamTile];
  __shared__ T s_cam[12];
  __shared__ int s_cnt[kCamTile/64 + 1];
  const int tid = threadIdx.x, npix = a.H*a.W, ntile = (npix + kCamTile - 1)/kCamTile;
  const int tile = blockIdx.x % ntile, cam = (blockIdx.x / ntile) % a.ncam, env = blockIdx.x / (ntile*a.ncam);
  if (env >= a.B) return;
  const CamDev<T>& c = a.cams[cam];
  const size_t B = a.B;
  if (tid == 0) cam_pose(c, a.xpos + env, a.xmat + env, a.subtree_com + env, B, s_cam, s_cam + 3);
  __syncthreads();
  T cpos[3], R[9];
  for (int k = 0; k < 3; k++) cpos[k] = s_cam[k];
  for (int k = 0; k < 9; k++) R[k] = s_cam[3 + k];
  // the tile's pixel rectangle -> the four side planes of its bounding pyramid (camera frame, through the origin)
  const int p0 = tile*kCamTile, p1 = min(npix, p0 + kCamTile) - 1;
  const int r0 = p0/a.W, r1 = p1/a.W, c0 = r0 == r1 ? p0 % a.W : 0, c1 = r0 == r1 ? p1 % a.W : a.W - 1;
  const T hx = (T)0.5*(a.W - 1), hy = (T)0.5*(a.H - 1);
  const T xl = (c0 - (T)0.5 - hx)*c.inv_f, xr = (c1 + (T)0.5 - hx)*c.inv_f;
  const T yt = -(r0 - (T)0.5 - hy)*c.inv_f, yb = -(r1 + (T)0.5 - hy)*c.inv_f;
  const T nl = 1/cam_sqrt(1 + xl*xl), nr = 1/cam_sqrt(1 + xr*xr), nt = 1/cam_sqrt(1 + yt*yt), nb = 1/cam_sqrt(1 + yb*yb);

  const int pix = p0 + tid;
  const bool live = pix < npix;
  const int row = live ? pix/a.W : 0, col = live ? pix % a.W : 0;
  const T dx = (col - hx)*c.inv_f, dy = -(row - hy)*c.inv_f;
  CamHit<T> h;
  h.id = -1; h.t = 0; h.type = 0; h.part = 0;
  for (int k = 0; k < 3; k++) { h.lp[k] = 0; h.lv[k] = 0; h.size[k] = 0; }

  for (int g0 = 0; g0 < a.ngeom; g0 += kCamTile) {
    const int g = g0 + tid;
    bool keep = g < a.ngeom && !a.geom_skip[g];
    T gp[3], gm[9], sz[3];
    int type = 0;
    if (keep) {
      type = a.geom_type[g];
      for (int k = 0; k < 3; k++) gp[k] = a.geom_xpos[(size_t)(3*g + k)*B + env];
      const int slot = a.eg_slot ? a.eg_slot[g] : -1;
      for (int k = 0; k < 3; k++) sz[k] = slot >= 0 ? a.eg_data[(size_t)(16*slot + 12 + k)*B + env] : a.geom_size[3*g + k];
      const T rb = cam_rbound(type, sz);
      if (a.cull && rb > 0) {
        // centre in the camera frame; outside one side plane by more than the bounding radius, or wholly behind
        const T d[3] = {gp[0] - cpos[0], gp[1] - cpos[1], gp[2] - cpos[2]};
        const T x = R[0]*d[0] + R[3]*d[1] + R[6]*d[2], y = R[1]*d[0] + R[4]*d[1] + R[7]*d[2], z = R[2]*d[0] + R[5]*d[1] + R[8]*d[2];
        if (z > rb || (x + xl*z)*nl < -rb || (-x - xr*z)*nr < -rb || (-y - yt*z)*nt < -rb || (y + yb*z)*nb < -rb) keep = false;
      }
    }
    if (keep) for (int k = 0; k < 9; k++) gm[k] = a.geom_xmat[(size_t)(9*g + k)*B + env];
    // compaction in geom order: ballot inside the wave, prefix over the waves through LDS
    const unsigned long long m = __ballot(keep);
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();      // (also: every lane is done with the previous pass's list)
    int off = 0, total = 0;
    for (int w = 0; w < kCamTile/64; w++) { if (w < wave) off += s_cnt[w]; total += s_cnt[w]; }
    if (keep) {
      CamGeom<T>* e = &s_geom[off + __popcll(m & ((1ull << lane) - 1))];
      if (kPre) cam_stage_geom(e, gp, gm, sz, type, g, cpos, R);
      else {      // tuning study: the world frame as it is, transformed per pixel
        for (int k = 0; k < 3; k++) { e->lp[k] = gp[k]; e->size[k] = sz[k]; }
        for (int k = 0; k < 9; k++) e->M[k] = gm[k];
        e->type = type; e->id = g;
      }
    }
    __syncthreads();
    if (live) {
      if (kPre) for (int k = 0; k < total; k++) cam_pixel_geom(s_geom[k], dx, dy, a.near_, a.far_, &h);
      else {
        const T wdir[3] = {R[0]*dx + R[1]*dy - R[2], R[3]*dx + R[4]*dy - R[5], R[6]*dx + R[7]*dy - R[8]};
        for (int k = 0; k < total; k++) cam_pixel_geom_world(s_geom[k], cpos, wdir, a.near_, a.far_, &h);
      }
    }
    __syncthreads();
  }
  if (!live) return;
  const size_t o = ((size_t)env*a.ncam + cam)*npix + pix;
  if (a.depth) a.depth[o] = h.id >= 0 ? h.t : a.far_;
  if (a.seg) { a.seg[2*o] = h.id; a.seg[2*o + 1] = h.id >= 0 ? kCamObjGeom : -1; }
  if (a.rgb) {
    uint8_t px[3] = {a.bg[0], a.bg[1], a.bg[2]};
    if (!kTex) {
      if (h.id >= 0) cam_shade(h, dx, dy, a.geom_color + 3*h.id, a.ambient, a.diffuse, px);
    } else if (h.id >= 0) {
      // once per pixel, on the final hit: texel x the geom's colour goes through the same shade and rounding
      const CamMat<T> m = t.mat[h.id];
      float col[3] = {a.geom_color[3*h.id], a.geom_color[3*h.id + 1], a.geom_color[3*h.id + 2]};
      if (m.mapping != CAM_MAP_NONE) {
        T M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (t.filter == CAM_FILTER_BOX && m.mapping == CAM_MAP_PLANE) {      // M = Rg' Rcam of the hit geom, for the footprint
          T gm[9];
          for (int k = 0; k < 9; k++) gm[k] = a.geom_xmat[(size_t)(9*h.id + k)*B + env];
          for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) M[3*i + j] = gm[i]*R[j] + gm[3 + i]*R[3 + j] + gm[6 + i]*R[6 + j];
        }
        float tex[3];
        cam_texture(m, h, M, c.inv_f, t.filter, tex);
        for (int k = 0; k < 3; k++) col[k] *= tex[k];
      }
      cam_shade(h, dx, dy, col, a.ambient, a.diffuse, px);
    } else if (t.sky) cam_sky(t.sky1, t.sky2, t.sky - 1, R, dx, dy, px);
    for (int k = 0; k < 3; k++) a.rgb[3*o + k] = px[k];
  }
}

template <typename T, bool kTex>
static int launch_camera(const CamArgs<T>& a, const CamTexArgs<T>& t, void* stream) {
  const int ntile = (a.H*a.W + kCamTile - 1)/kCamTile;
  const long long grid = (long long)a.B*a.ncam*ntile;
  if (grid <= 0 || grid > 0x7fffffffLL) return -1;
  if (a.pretransform) hipLaunchKernelGGL((camera_kernel<T, true, kTex>), dim3((unsigned)grid), dim3(kCamTile), 0, (hipStream_t)stream, a, t);
  else hipLaunchKernelGGL((camera_kernel<T, false, kTex>), dim3((unsigned)grid), dim3(kCamTile), 0, (hipStream_t)stream, a, t);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
int launch_camera_f32(const CamArgs<float>& a, void* stream) { return launch_camera<float, false>(a, CamTexArgs<float>{}, stream); }
int launch_camera_f64(const CamArgs<double>& a, void* stream) { return launch_camera<double, false>(a, CamTexArgs<double>{}, stream); }
int launch_camera_tex_f32(const CamArgs<float>& a, const CamTexArgs<float>& t, void* stream) {
  if (!t.mat) return -3;
  return launch_camera<float, true>(a, t, stream);
}
int launch_camera_tex_f64(const CamArgs<double>& a, const CamTexArgs<double>& t, void* stream) {
  if (!t.mat) return -3;
  return launch_camera<double, true>(a, t, stream);
}

}  // namespace dmc
