// ray_kernels.hip -- batched ray casts (dmc_rays_cast, dmc_rays_scan): mj_ray for every environment of a batch from the
// geom poses a step / forward launch left in HBM.  See ray_core.h for the model.
//
// ray_cast_kernel: arbitrary rays, one lane per (environment, ray) with the environment fastest, so that the SoA pose
// loads geom_xpos[(3 g + k) B + env] coalesce (and for one ray per environment the inputs and outputs too).  What does
// not depend on the environment -- id, type, body, env-geom slot and model size of the geoms that pass the filters -- is
// staged once per workgroup in LDS; every lane walks that list in the same order: same-address reads broadcast.
//
// ray_scan_kernel: a table of directions fixed in a moving frame, one workgroup per (environment, scan, tile of kRayTile
// rays), one lane per ray: the camera kernel's shape.  The frame's pose is derived once per workgroup; the geoms are
// staged in ray-ready form (origin in the geom's frame, M = Rg' Rframe: a lane's local direction is nine multiply-adds)
// in passes of kRayPass, compacted in geom order with one wave's ballot; geoms of the excluded body and geoms wholly
// beyond the cutoff are dropped there.
#include <hip/hip_runtime.h>

#include "ray_core.h"

namespace dmc {

template <typename T>
struct RayStatic {      // what the cast kernel stages of one geom
  T size[3];
  int id, type, body, slot;
};

// size in force: the environment's own where the geom was declared per environment, else the live model table
template <typename T>
__device__ __forceinline__ void ray_size(const RayArgs<T>& a, int g, int slot, size_t env, T* sz) {
  for (int k = 0; k < 3; k++) sz[k] = slot >= 0 ? a.eg_data[(size_t)(16*slot + 12 + k)*a.B + env] : a.geom_size[3*g + k];
}

template <typename T>
__device__ __forceinline__ void ray_store(const RayArgs<T>& a, size_t o, size_t env, const RayHit<T>& h, const T* pnt, const T* vec) {
  if (a.dist) a.dist[o] = h.id >= 0 ? h.x : (T)-1;
  if (a.geomid) a.geomid[o] = h.id;
  if (!a.normal) return;
  T n[3] = {0, 0, 0};
  if (h.id >= 0) {
    const size_t B = a.B;
    const int g = h.id;
    T gp[3], gm[9], sz[3];
    for (int k = 0; k < 3; k++) gp[k] = a.geom_xpos[(size_t)(3*g + k)*B + env];
    for (int k = 0; k < 9; k++) gm[k] = a.geom_xmat[(size_t)(9*g + k)*B + env];
    ray_size(a, g, a.eg_slot ? a.eg_slot[g] : -1, env, sz);
    if (!ray_normal_world(a.geom_type[g], sz, gp, gm, pnt, vec, n)) { n[0] = 0; n[1] = 0; n[2] = 0; }
  }
  for (int k = 0; k < 3; k++) a.normal[3*o + k] = n[k];
}

template <typename T>
__global__ void __launch_bounds__(kRayBlock) ray_cast_kernel(const RayArgs<T> a) {
  __shared__ RayStatic<T> s_geom[kRayBlock];
  const int tid = threadIdx.x;
  const size_t B = a.B;
  const long long i = (long long)blockIdx.x*kRayBlock + tid, total = (long long)a.B*a.nray;
  const bool live = i < total;      // the last wave is ragged; its idle lanes still stage and meet the barriers
  const size_t env = live ? (size_t)(i % a.B) : 0, ray = live ? (size_t)(i / a.B) : 0;
  const size_t o = env*a.nray + ray;
  T pnt[3] = {0, 0, 0}, vec[3] = {0, 0, 1};
  int bex = a.bodyexclude;
  if (live) {
    for (int k = 0; k < 3; k++) { pnt[k] = a.pnt[3*o + k]; vec[k] = a.vec[3*o + k]; }
    if (a.bodyexclude_dev) bex = a.bodyexclude_dev[a.bodyexclude_per_ray ? o : env];
  }
  const T len = cam_sqrt(vec[0]*vec[0] + vec[1]*vec[1] + vec[2]*vec[2]);
  RayHit<T> h;
  h.id = -1; h.x = 0;
  for (int g0 = 0; g0 < a.nlist; g0 += kRayBlock) {
    if (g0 + tid < a.nlist) {
      RayStatic<T>& e = s_geom[tid];
      const int g = a.list[g0 + tid];
      e.id = g; e.type = a.geom_type[g]; e.body = a.geom_body[g]; e.slot = a.eg_slot ? a.eg_slot[g] : -1;
      for (int k = 0; k < 3; k++) e.size[k] = a.geom_size[3*g + k];
    }
    __syncthreads();
    const int n = min(kRayBlock, a.nlist - g0);
    if (live) for (int j = 0; j < n; j++) {
      const RayStatic<T>& e = s_geom[j];
      if (e.body == bex) continue;
      const int g = e.id;
      T gp[3], gm[9], sz[3];
      for (int k = 0; k < 3; k++) gp[k] = a.geom_xpos[(size_t)(3*g + k)*B + env];
      for (int k = 0; k < 9; k++) gm[k] = a.geom_xmat[(size_t)(9*g + k)*B + env];
      for (int k = 0; k < 3; k++) sz[k] = e.slot >= 0 ? a.eg_data[(size_t)(16*e.slot + 12 + k)*B + env] : e.size[k];
      ray_take(ray_geom_world(e.type, sz, gp, gm, pnt, vec), g, len, a.cutoff, &h);
    }
    __syncthreads();
  }
  if (live) ray_store(a, o, env, h, pnt, vec);
}

template <typename T>
__global__ void __launch_bounds__(kRayTile) ray_scan_kernel(const RayArgs<T> a) {
  static_assert(kRayPass == 64, "one staging pass is one wave's ballot");
  __shared__ CamGeom<T> s_geom[kRayPass];
  __shared__ T s_frame[12];
  __shared__ int s_cnt;
  const int tid = threadIdx.x, ntile = (a.ndir + kRayTile - 1)/kRayTile;
  const int tile = blockIdx.x % ntile, scan = (blockIdx.x / ntile) % a.nscan;
  const size_t env = blockIdx.x / (ntile*a.nscan), B = a.B;
  if (env >= B) return;
  const RayScan<T> s = a.scans[scan];
  if (tid == 0) {
    const T* pos = s.frame_type == RAY_FRAME_BODY ? a.xpos : s.frame_type == RAY_FRAME_SITE ? a.site_xpos : a.geom_xpos;
    const T* mat = s.frame_type == RAY_FRAME_BODY ? a.xmat : s.frame_type == RAY_FRAME_SITE ? a.site_xmat : a.geom_xmat;
    ray_frame_pose(s, pos + env, mat + env, B, s_frame, s_frame + 3);
  }
  __syncthreads();
  T origin[3], R[9];
  for (int k = 0; k < 3; k++) origin[k] = s_frame[k];
  for (int k = 0; k < 9; k++) R[k] = s_frame[3 + k];
  const int r = tile*kRayTile + tid;
  const bool live = r < a.ndir;      // the last tile is ragged
  T d[3] = {0, 0, 1};
  if (live) for (int k = 0; k < 3; k++) d[k] = a.dirs[((size_t)scan*a.ndir + r)*3 + k];
  const T len = cam_sqrt(d[0]*d[0] + d[1]*d[1] + d[2]*d[2]);
  RayHit<T> h;
  h.id = -1; h.x = 0;
  for (int g0 = 0; g0 < a.nlist; g0 += kRayPass) {
    if (tid < kRayPass) {      // the first wave stages; compaction in geom order with its ballot
      bool keep = g0 + tid < a.nlist;
      int g = 0, type = 0;
      T gp[3], gm[9], sz[3];
      if (keep) {
        g = a.list[g0 + tid];
        keep = a.geom_body[g] != s.bodyexclude;
      }
      if (keep) {
        type = a.geom_type[g];
        for (int k = 0; k < 3; k++) gp[k] = a.geom_xpos[(size_t)(3*g + k)*B + env];
        ray_size(a, g, a.eg_slot ? a.eg_slot[g] : -1, env, sz);
        keep = !ray_beyond_cutoff(gp, cam_rbound(type, sz), origin, a.cutoff);
      }
      if (keep) for (int k = 0; k < 9; k++) gm[k] = a.geom_xmat[(size_t)(9*g + k)*B + env];
      const unsigned long long m = __ballot(keep);
      if (tid == 0) s_cnt = __popcll(m);
      if (keep) cam_stage_geom(&s_geom[__popcll(m & ((1ull << tid) - 1))], gp, gm, sz, type, g, origin, R);
    }
    __syncthreads();
    const int n = s_cnt;
    if (live) for (int j = 0; j < n; j++) {
      const CamGeom<T>& e = s_geom[j];
      T lv[3];
      for (int i = 0; i < 3; i++) lv[i] = e.M[3*i]*d[0] + e.M[3*i + 1]*d[1] + e.M[3*i + 2]*d[2];
      int part;
      ray_take(cam_ray_local(e.type, e.size, e.lp, lv, &part), e.id, len, a.cutoff, &h);
    }
    __syncthreads();      // every lane is done with this pass's list
  }
  if (!live) return;
  const T vec[3] = {R[0]*d[0] + R[1]*d[1] + R[2]*d[2], R[3]*d[0] + R[4]*d[1] + R[5]*d[2], R[6]*d[0] + R[7]*d[1] + R[8]*d[2]};
  ray_store(a, (env*a.nscan + scan)*a.ndir + r, env, h, origin, vec);
}

template <typename T>
static int launch_ray_cast(const RayArgs<T>& a, void* stream) {
  const long long grid = ((long long)a.B*a.nray + kRayBlock - 1)/kRayBlock;
  if (a.B < 1 || a.nray < 1 || grid <= 0 || grid > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL((ray_cast_kernel<T>), dim3((unsigned)grid), dim3(kRayBlock), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template <typename T>
static int launch_ray_scan(const RayArgs<T>& a, void* stream) {
  if (a.B < 1 || a.nscan < 1 || a.ndir < 1) return -1;
  const long long ntile = (a.ndir + kRayTile - 1)/kRayTile, grid = (long long)a.B*a.nscan*ntile;
  if (grid <= 0 || grid > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL((ray_scan_kernel<T>), dim3((unsigned)grid), dim3(kRayTile), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
int launch_ray_cast_f32(const RayArgs<float>& a, void* stream) { return launch_ray_cast<float>(a, stream); }
int launch_ray_cast_f64(const RayArgs<double>& a, void* stream) { return launch_ray_cast<double>(a, stream); }
int launch_ray_scan_f32(const RayArgs<float>& a, void* stream) { return launch_ray_scan<float>(a, stream); }
int launch_ray_scan_f64(const RayArgs<double>& a, void* stream) { return launch_ray_scan<double>(a, stream); }

}  // namespace dmc
