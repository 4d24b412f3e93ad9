/* dmc_ray.h -- C-ABI of the batched ray casts (libdmc_hip.so, csrc/ray_kernels.hip; entry points in csrc/dmc_api.hip).
 *
 * Replaces, for every environment of a dmc_batch at once and without leaving the device, the reference's calls of
 * mujoco.mj_ray (locomotion/tasks/random_goal_maze.py:157-200: a fan of rays from a spawn point) and the per-site
 * <rangefinder> sensors a range scan would otherwise need in the model.
 *
 * One ray pnt + x vec (vec need not be unit length): the smallest x >= 0 over the geoms that pass the filter and that
 * geom's id; -1 / -1 when nothing is hit.  x is in units of |vec|.  A geom is skipped when it lies on the excluded body,
 * is invisible (alpha 0 on the geom or its material), its group's flag is zero (groups clamped to 0..5), flg_static is 0
 * and its body is welded to the world, or it is a mesh / height field (scenery the rays pass through).  Planes are hit
 * from the front only and are finite where their half-sizes are positive; a ray that starts inside a closed primitive
 * leaves through its surface.  Geom sizes are the ones the step kernel uses (dmc_batch_set_model_real, per-environment
 * geoms).
 *
 * Every function returns 0 on success or a negative error code and never throws; dmc_last_error() (dmc_batch.h) returns a
 * thread-local message.
 */
#ifndef DMC_RAY_H_
#define DMC_RAY_H_

#include <stdint.h>

#include "dmc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmc_rays dmc_rays;

/* The filter arguments of mj_ray that stay fixed for the object's life.
 *   has_geomgroup 0: every group (mj_ray's geomgroup = NULL); else geomgroup[6] holds the flags.
 *   flg_static: 0 skips the geoms of bodies welded to the world.
 *   cutoff: metres, like the rangefinder's attribute -- farther hits become misses; <= 0 or infinite: none.
 *   geom_group[ngeom_group]: mjModel.geom_group (the C model does not hold it); ngeom_group must be the model's ngeom. */
typedef struct dmc_rays_options {
  int32_t has_geomgroup, flg_static;
  int32_t geomgroup[6];
  double cutoff;
  const int32_t* geom_group;
  int32_t ngeom_group, reserved;
} dmc_rays_options;

/* Replaces the set-up of a mj_ray call (random_goal_maze.py:176-178: geomgroup, flg_static). */
int dmc_rays_create(dmc_batch* b, const dmc_rays_options* options, dmc_rays** out);

/* Replaces mj_ray(model, data, pnt, vec, geomgroup, flg_static, bodyexclude, geomid) (random_goal_maze.py:179-187) for
 * nray rays of every environment in ONE launch on `hip_stream`; asynchronous, no host read, capturable in a HIP graph.
 *   pnt_dev / vec_dev: device (B, nray, 3) in the batch precision.
 *   bodyexclude: one body id (-1: none) when bodyexclude_dev is NULL; else bodyexclude_dev holds int32 ids, (B) or, with
 *   bodyexclude_per_ray != 0, (B, nray).
 *   dist_out (B, nray) in the batch precision (-1 on a miss), geomid_out (B, nray) int32, normal_out (B, nray, 3) the
 *   world-frame unit normal at the hit (0 on a miss); each may be NULL, not all.
 * Returns -3 when the batch's output mask excludes the geom poses, did when the last step / forward launch ran, or no
 * such launch has run yet. */
int dmc_rays_cast(dmc_rays* r, int nray, const void* pnt_dev, const void* vec_dev, int bodyexclude,
                  const int32_t* bodyexclude_dev, int bodyexclude_per_ray, void* dist_out, int32_t* geomid_out,
                  void* normal_out, void* hip_stream);

/* Replaces one <site> + <rangefinder> per ray in the model (a "lidar"): adds a scan -- a frame (frame_type 0 world,
 * 1 body, 2 site, 3 geom; frame_id its id), an offset in that frame, the body its rays skip (-1: none) and ndir
 * directions in that frame, host (ndir, 3).  All scans of one object have the same ndir.  Synchronous (uploads the
 * tables); not inside a graph capture. */
int dmc_rays_add_scan(dmc_rays* r, int frame_type, int frame_id, const double* offset, int bodyexclude, int ndir,
                      const double* dirs_host);

/* Replaces reading those rangefinders' sensordata: all scans in ONE launch; outputs (B, nscan, ndir[, 3]) as for
 * dmc_rays_cast; asynchronous, capturable.  -3 as for dmc_rays_cast, over the arrays the scans' frames read too. */
int dmc_rays_scan(dmc_rays* r, void* dist_out, int32_t* geomid_out, void* normal_out, void* hip_stream);

/* info[0..7] = {B, precision, geoms that pass the fixed filters, nscan, ndir, cast block, scan tile, scan staging pass}
 * (no counterpart in the reference: the launch shapes that stand in for its Python loop over rays). */
int dmc_rays_info(const dmc_rays* r, int* info);

/* Replaces nothing in the reference (mj_ray holds no state); releases the device tables. */
void dmc_rays_destroy(dmc_rays* r);

#ifdef __cplusplus
}
#endif
#endif  /* DMC_RAY_H_ */
