/* dmc_dist.h -- C-ABI of the batched geom distances (libdmc_hip.so, csrc/dist_kernels.hip; entry points in
 * csrc/dmc_api.hip).
 *
 * Replaces, for every environment of a dmc_batch at once and without leaving the device, mujoco's mj_geomDistance and the
 * <distance>, <normal> and <fromto> sensors built on it (dm_control/mjcf/schema.xml:3047-3095).
 *
 * One pair of convex geoms A, B: dist = max over unit n of [n.(cB - cA) - hA(n) - hB(-n)] -- the Euclidean distance when
 * they are apart, minus the minimum-translation depth when they overlap; fromto the point on A's surface and the point on
 * B's that realise it; normal = (to - from) / dist, from A towards B when apart.  The result is bounded by the pair's
 * distmax: a pair with no distance below it returns distmax, a zero fromto and a zero normal.  Planes are infinite;
 * plane-plane has no distance (distmax).  A member that lists several geoms (a body) stands for the minimum over the geom
 * pairs.  Meshes and height fields are refused.  Geom sizes are the ones the step kernel uses
 * (dmc_batch_set_model_real, per-environment geoms).  Witness points are not unique for parallel faces or edges.
 *
 * Every function returns 0 on success or a negative error code and never throws; dmc_last_error() (dmc_batch.h) returns a
 * thread-local message.
 */
#ifndef DMC_DIST_H_
#define DMC_DIST_H_

#include <stdint.h>

#include "dmc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmc_dist dmc_dist;

/* mjOption.ccd_tolerance (default 1e-6) and ccd_iterations (default 50): the solver stops when its bounds on the distance
 * of the pair's cores are closer than tolerance * max(1, upper), or after `iterations` iterations of GJK or of EPA.  The
 * iterations aim for the tolerance floored at 32 machine epsilons of the batch precision (3.8e-6 in fp32); where the
 * arithmetic stops making progress first, status 0 certifies a gap of max(tolerance, 128 machine epsilons) * max(1, upper)
 * (1.5e-5 in fp32) and a larger gap is status 1. */
typedef struct dmc_dist_options {
  double tolerance;
  int32_t iterations, reserved;
} dmc_dist_options;

/* Replaces the <distance geom1= geom2= cutoff=> (or body1 / body2) elements of a model: npair pairs.
 *   pair_adr (npair, 4): {first, count} into `member` for geom1's side, then for geom2's side; a geom is one entry, a
 *   body the geoms directly attached to it.  member[nmember]: geom ids.  distmax[npair]: the cutoffs (mj_geomDistance's
 *   distmax; infinity allowed, and then what an unreached pair or plane-plane reads).
 * Fails on a member that is a mesh or a height field, or out of range.  Synchronous (uploads the tables). */
int dmc_dist_create(dmc_batch* b, int npair, const int32_t* pair_adr, const int32_t* member, int nmember,
                    const double* distmax, const dmc_dist_options* options, dmc_dist** out);

/* Replaces mj_geomDistance(m, d, geom1, geom2, distmax, fromto) for every pair of every environment in ONE launch on
 * `hip_stream`; asynchronous, no allocation and no host read: capturable in a HIP graph.
 *   dist_out (B, npair), fromto_out (B, npair, 6), normal_out (B, npair, 3) in the batch precision; status_out
 *   (B, npair) int32: bit 0 set when a cap was reached (iterations, polytope vertices or faces) and dist is the best bound
 *   found, bit 1 set when the cores of a geom pair overlapped (EPA ran).  Each may be NULL, not all.
 * Returns -3 when the batch's output mask excludes the geom poses, did when the last step / forward launch ran, or no
 * such launch has run yet. */
int dmc_dist_query(dmc_dist* d, void* dist_out, void* fromto_out, void* normal_out, int32_t* status_out, void* hip_stream);

/* info[0..9] = {B, precision, npair, nmember, iterations, lanes per workgroup, EPA vertex cap, EPA face cap, EPA lanes
 * per LDS pass, static LDS bytes per workgroup} (no counterpart in the reference: the launch shape). */
int dmc_dist_info(const dmc_dist* d, int* info);

/* Replaces nothing in the reference (mj_geomDistance holds no state); releases the device tables. */
void dmc_dist_destroy(dmc_dist* d);

/* Replaces mj_geomDistance for ONE pair on the host, in fp64, from poses the caller holds (no batch, no device): the
 * same solver text as the kernel.  type: mjtGeom; size (3); pos (3); mat (9) row-major.  Returns the distance and
 * writes fromto (6, may be NULL) and *status (0 / 1 as bit 0 above, -1 on an argument error; may be NULL). */
double dmc_geom_distance_host(int type1, const double* size1, const double* pos1, const double* mat1, int type2,
                              const double* size2, const double* pos2, const double* mat2, double distmax,
                              double tolerance, int iterations, double* fromto, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif  /* DMC_DIST_H_ */
