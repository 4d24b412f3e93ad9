/* dmc_dyn.h -- C-ABI of the batched dynamics (libdmc_hip.so, csrc/dyn_kernels.hip; entry points in csrc/dmc_api.hip).
 *
 * Replaces, for every environment of a dmc_batch at once and without leaving the device, mujoco's mj_crb + mj_fullM (the
 * dense joint-space inertia M), mj_mulM (M v), mj_solveM (M^-1 f) and mj_rne (bias forces; inverse dynamics M qacc + bias).
 *
 * Everything is computed from the qpos / qvel in device memory in the launch itself -- the kinematics of the whole tree,
 * the composite inertias, the recursive Newton-Euler passes, a dense Cholesky factorisation -- so no pose array is read
 * and none can be stale.  Rigid-body terms only: passive, actuator and constraint forces are not part of any result
 * (dmc_dyn_inverse is mj_rne plus the armature term, not mj_inverse).
 *
 * A group of 16 / 32 / 64 lanes of a wavefront works on one environment; 64 / lanes environments share a workgroup and
 * their working sets live in its LDS (at most 64 KB, static).  Every stored element is computed by one lane with sums in
 * a fixed order: two launches give equal bits, and fp64 results do not depend on the lanes per environment.
 *
 * Every function returns 0 on success or a negative error code and never throws; dmc_last_error() (dmc_batch.h) returns a
 * thread-local message.
 */
#ifndef DMC_DYN_H_
#define DMC_DYN_H_

#include <stdint.h>

#include "dmc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmc_dyn dmc_dyn;

#define DMC_DYN_MAX_DOFS 64

/* The model's tables, a snapshot taken by the caller (model constants are read once: later model edits need a new object).
 * Bodies are the caller's own numbering: body 0 is the world, a parent precedes its children; bodies that carry no dof and
 * have no joint below them (mocap bodies, scenery) may be left out.  Joints and dofs are the model's.
 *   nb, nj, nv, nq: bodies, joints, dofs, qpos entries; nlevel: the depth of the tree; nsub: entries of sub_body.
 *   ints:  body_parent[nb] body_jntadr[nb] body_jntnum[nb] body_root[nb] (the body below the world its tree hangs off)
 *          body_lastdof[nb] (the last dof on the path from the world to the body, -1: none) sub_adr[nb + 1]
 *          level_adr[nlevel + 1] level_body[nb - 1] (the bodies sorted by depth; level l is
 *          level_body[level_adr[l] .. level_adr[l + 1])) jnt_type[nj] jnt_qadr[nj] jnt_dadr[nj] dof_body[nv]
 *          dof_parent[nv] dof_pred[nv] (the last dof whose motion carries the dof's axis: dof_parent for a hinge or a
 *          slide, the dof before the triple for a ball joint, the third translation for a free joint's rotations, -1)
 *          dof_rot[nv] (1: the dof rotates) sub_body[nsub] (body b's subtree, b included, is
 *          sub_body[sub_adr[b] .. sub_adr[b + 1]), ascending).
 *   reals: body_pos[3 nb] body_quat[4 nb] body_ipos[3 nb] body_iquat[4 nb] body_mass[nb] body_inertia[3 nb]
 *          jnt_axis[3 nj] jnt_pos[3 nj] jnt_qpos0[nj] dof_armature[nv] gravity[3] (zeros where gravity is disabled). */
typedef struct dmc_dyn_tables {
  int32_t nb, nj, nv, nq, nlevel, nsub, nints, nreals;
  const int32_t* ints;
  const double* reals;
} dmc_dyn_tables;

/* Validates every index the kernels follow and uploads the tables once.  lanes_per_env: 16, 32 or 64; fails where the
 * 64 / lanes_per_env working sets do not fit 64 KB of LDS.  Synchronous. */
int dmc_dyn_create(dmc_batch* b, const dmc_dyn_tables* tables, int lanes_per_env, dmc_dyn** out);

/* Each of the following is ONE launch on `hip_stream`; asynchronous, no allocation, no host read: capturable in a HIP
 * graph.  Outputs are in the batch precision, contiguous per environment, and EVERY element is written. */

/* mj_crb + mj_fullM: M_out (B, nv, nv), dense, exactly symmetric, dof_armature on the diagonal, exact zeros where neither
 * dof is an ancestor of the other. */
int dmc_dyn_mass_matrix(dmc_dyn* d, void* M_out, void* hip_stream);

/* mj_rne(flg_acc = 0): bias_out (B, nv) = mjData.qfrc_bias at the qpos / qvel in device memory. */
int dmc_dyn_bias(dmc_dyn* d, void* bias_out, void* hip_stream);

/* mj_rne(flg_acc = 1) plus the armature term: tau_out (B, nv) = M qacc + bias.  Element k of environment e of qacc is
 * qacc[e*qacc_env_stride + k] (a stride of 0 broadcasts one vector). */
int dmc_dyn_inverse(dmc_dyn* d, const void* qacc, int64_t qacc_env_stride, void* tau_out, void* hip_stream);

/* mj_mulM: out (B, K, nv) = M vec for the K >= 1 vectors of every environment, vec (B, K, nv). */
int dmc_dyn_mul(dmc_dyn* d, const void* vec, int K, void* out, void* hip_stream);

/* mj_solveM: out (B, K, nv) = M^-1 vec; one Cholesky factorisation per environment serves its K right-hand sides, which
 * pass through LDS in chunks of 8.  A pivot below mjMINVAL is replaced by it. */
int dmc_dyn_solve(dmc_dyn* d, const void* vec, int K, void* out, void* hip_stream);

/* info[0..9] = {B, precision, nv, bodies in the tables, lanes per environment, environments per workgroup, static LDS
 * bytes of the mass_matrix / mul / solve launch, of the bias / inverse launch, right-hand sides per chunk, tree levels}
 * (no counterpart in the reference: the launch shape). */
int dmc_dyn_info(const dmc_dyn* d, int* info);

/* Replaces nothing in the reference; releases the device tables. */
void dmc_dyn_destroy(dmc_dyn* d);

#ifdef __cplusplus
}
#endif
#endif  /* DMC_DYN_H_ */
