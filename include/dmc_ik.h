/* dmc_ik.h -- C-ABI of the batched inverse kinematics (libdmc_hip.so, csrc/ik_kernels.hip).
 *
 * Replaces, for every environment of a dmc_batch at once and without leaving the device, the reference's
 * dm_control/utils/inverse_kinematics.py: qpos_from_site_pose (:37-230) with its solve nullspace_method (:233-260).
 * The object reaches the batch only through the public entry points of dmc_batch.h (dmc_batch_device_ptr,
 * dmc_batch_info, dmc_batch_field_rows, dmc_batch_invalidate_async).  Every function returns 0 on success or a negative
 * error code and never throws; dmc_ik_last_error() returns a thread-local message.
 */
#ifndef DMC_IK_H_
#define DMC_IK_H_

#include <stdint.h>

#include "dmc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmc_ik dmc_ik;

const char* dmc_ik_last_error(void);

/* The kinematic chain from the world to the site's body, root first, in mjModel's terms -- what mj_fwdPosition and
 * mj_jacSite (inverse_kinematics.py:127,179-180,211) read of the model.  A SNAPSHOT: edits made later through
 * dmc_batch_set_model_real (body_pos, body_quat, site_pos, ...) need a new object.
 *   per chain body:  body_jntadr / body_jntnum index the chain's joint list below; body_pos / body_quat.
 *   per chain joint: jnt_type (0 free, 1 ball, 2 slide, 3 hinge), jnt_qslot / jnt_dslot = the joint's first entry among
 *                    the chain's qpos entries / dofs, jnt_axis, jnt_pos, jnt_qpos0 (qpos0 at the joint's address).
 *   qmap[nqchain]:   chain qpos entry -> mjModel qpos address.
 *   dof_movable[ndof]: 1 where the dof belongs to a joint the solve may move (joint_names, :139-152), joint-wise.
 *   site_pos / site_quat: the site in its body's frame.
 * At most 64 chain dofs; at least one must be movable. */
typedef struct dmc_ik_chain {
  int32_t nbody, njnt, ndof, nqchain;
  const int32_t* body_jntadr;
  const int32_t* body_jntnum;
  const int32_t* jnt_type;
  const int32_t* jnt_qslot;
  const int32_t* jnt_dslot;
  const int32_t* qmap;
  const int32_t* dof_movable;
  const double* body_pos;
  const double* body_quat;
  const double* jnt_axis;
  const double* jnt_pos;
  const double* jnt_qpos0;
  double site_pos[3], site_quat[4];
} dmc_ik_chain;

/* The keyword arguments of qpos_from_site_pose (:42-48). */
typedef struct dmc_ik_options {
  double tol, rot_weight, regularization_threshold, regularization_strength, max_update_norm, progress_thresh;
  int32_t max_steps, reserved;
} dmc_ik_options;

/* Replaces the set-up of qpos_from_site_pose (:97-152: buffers, site id, dof indices of the named joints). */
int dmc_ik_create(dmc_batch* b, const dmc_ik_chain* chain, const dmc_ik_options* options, dmc_ik** out);

/* Replaces the iteration of qpos_from_site_pose (:157-214: error, mj_jacSite, nullspace_method, progress test, clamp,
 * mj_integratePos, mj_fwdPosition, up to max_steps times) and its result (:220-230), for every environment in ONE
 * launch on `hip_stream`; asynchronous, no host read, capturable in a HIP graph.
 *   target_pos / target_quat: device (B, 3) / (B, 4) in the batch precision, either may be NULL, not both.
 *   qpos_in: device (B, nq) start positions, or NULL = the batch's own qpos (fetched anew at every call: a field can be
 *     rebound).  inplace != 0: the result is also written to the batch's qpos and its stashes are invalidated on the
 *     stream; otherwise the batch is left untouched.
 *   qpos_out (B, nq), err_norm_out (B) in the batch precision; steps_out, status_out (B) int32.  status: 0 converged
 *   (success), 1 step limit, 2 progress stop, 3 singular pivot in the dual solve. */
int dmc_ik_solve(dmc_ik* ik, const void* target_pos, const void* target_quat, const void* qpos_in, int inplace,
                 void* qpos_out, void* err_norm_out, int32_t* steps_out, int32_t* status_out, void* hip_stream);

/* info[0..6] = {B, precision, envs_per_block, lds_bytes_per_block, grid, ndof, nqchain} of the launch dmc_ik_solve
 * makes (no counterpart in inverse_kinematics.py: the launch shape that stands in for its Python loop, :157). */
int dmc_ik_info(const dmc_ik* ik, int* info);

/* Replaces the release of the reference's temporary Physics copy (:123-124, :220-225). */
void dmc_ik_destroy(dmc_ik* ik);

#ifdef __cplusplus
}
#endif
#endif  /* DMC_IK_H_ */
