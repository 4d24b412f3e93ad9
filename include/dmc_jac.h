/* dmc_jac.h -- C-ABI of the batched Jacobians (libdmc_hip.so, csrc/jac_kernels.hip; entry points in csrc/dmc_api.hip).
 *
 * Replaces, for every environment of a dmc_batch at once and without leaving the device, mujoco's mj_jac family
 * (mj_jac, mj_jacBody, mj_jacBodyCom, mj_jacSite, mj_jacGeom), mj_objectVelocity (as J qvel) and the joint-space image of
 * mj_applyFT (J' f).
 *
 * A target is a frame fixed in a body: an offset and an orientation in the body's frame (a site, a geom, the body's
 * origin or inertial frame, any point).  For every target the caller extracts the chain of bodies and joints from the
 * world to the target's body; the kernels compute the kinematics along that chain from the qpos in device memory, so the
 * result is mj_jac AFTER mj_kinematics at the current qpos -- no pose array is read and none can be stale (MuJoCo's own
 * call reads whatever mj_kinematics last left).
 *
 * Column conventions: hinge: axis x (p - anchor) / axis; slide: axis / 0; ball: the columns of the body's orientation
 * about the joint's anchor; free: the world axes for the translations, the columns of the body's orientation about the
 * body's origin for the rotations.
 *
 * Every function returns 0 on success or a negative error code and never throws; dmc_last_error() (dmc_batch.h) returns a
 * thread-local message.
 */
#ifndef DMC_JAC_H_
#define DMC_JAC_H_

#include <stdint.h>

#include "dmc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmc_jac dmc_jac;

#define DMC_JAC_MAX_CHAIN_DOFS 64

/* The chains of `ntarget` targets, concatenated target after target.
 *   dims (ntarget, 3): {nb, nj, nd} = the chain's bodies (root first, the world left out), joints and dofs.
 *   ints, per target:  body_jntadr[nb] body_jntnum[nb] (into the chain's joints) jnt_type[nj] jnt_qadr[nj] (the joint's
 *                      qpos address in the model) jnt_dslot[nj] (its first dof counted along the chain) dof_id[nd] (chain
 *                      dof -> model dof) dof_col[nd] (chain dof -> output column, -1: not among the columns).
 *   reals, per target: body_pos[3 nb] body_quat[4 nb] jnt_axis[3 nj] jnt_pos[3 nj] jnt_qpos0[nj] target_pos[3]
 *                      target_quat[4] (the target's frame in its body's).
 *   ncol: the number of output columns C. */
typedef struct dmc_jac_tables {
  int32_t ntarget, ncol, nints, nreals;
  const int32_t* dims;
  const int32_t* ints;
  const double* reals;
} dmc_jac_tables;

/* Validates every index the kernels follow (again: the Python side built them) and uploads the tables once.  Fails on a
 * chain of more than DMC_JAC_MAX_CHAIN_DOFS dofs, on addresses outside the model and on inconsistent sizes.  Synchronous. */
int dmc_jac_create(dmc_batch* b, const dmc_jac_tables* tables, dmc_jac** out);

/* Replaces mj_jac for every (environment, target) in ONE launch on `hip_stream`; asynchronous, no allocation, no host
 * read: capturable in a HIP graph.
 *   jacp_out, jacr_out: (B, ntarget, 3, C) in the batch precision, either may be NULL (not both); EVERY element is
 *   written, columns of dofs off a target's chain as zeros.
 *   point: NULL (each target's own point) or (B, ntarget, 3) world points that replace them -- mj_jac's general form,
 *   where target t only names the body. */
int dmc_jac_jacobian(dmc_jac* j, const void* point, void* jacp_out, void* jacr_out, void* hip_stream);

/* Replaces mj_objectVelocity: vel_out (B, ntarget, 6) = J qvel over ALL dofs of the chain (not only the C columns),
 * (angular, linear), in the world frame or (local != 0) rotated into the target's own.  ONE launch, as above. */
int dmc_jac_velocity(dmc_jac* j, int local, void* vel_out, void* hip_stream);

/* The joint-space image of mj_applyFT: qfrc_out (B, C) = sum over targets of Jp' force + Jr' torque, the targets summed
 * in order in plain arithmetic (no atomics: the same bits on every launch).  force / torque: NULL (zero) or reals in
 * the batch precision, element k of target t of environment e at [e*env_stride + t*target_stride + k] (a stride of 0
 * broadcasts).  The batch's qfrc_applied is NOT written.  ONE launch, as above. */
int dmc_jac_force(dmc_jac* j, const void* force, int64_t force_env_stride, int64_t force_target_stride, const void* torque,
                  int64_t torque_env_stride, int64_t torque_target_stride, void* qfrc_out, void* hip_stream);

/* info[0..9] = {B, precision, ntarget, C, lanes per workgroup, column chunk of the jacobian launch, its static LDS bytes,
 * environments per workgroup of the force launch, its static LDS bytes, the longest chain's dofs} (no counterpart in the
 * reference: the launch shape). */
int dmc_jac_info(const dmc_jac* j, int* info);

/* Replaces nothing in the reference (mj_jac holds no state); releases the device tables. */
void dmc_jac_destroy(dmc_jac* j);

#ifdef __cplusplus
}
#endif
#endif  /* DMC_JAC_H_ */
