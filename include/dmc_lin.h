/* dmc_lin.h -- C-ABI of the batched linearisation (libdmc_hip.so, csrc/lin_kernels.hip; entry points in csrc/dmc_api.hip).
 *
 * Replaces, for every environment of a dmc_batch at once and without leaving the device, mujoco's mjd_transitionFD: the
 * finite-difference matrices of the discrete step,
 *     x' ~ A dx + B du,   y ~ C dx + D du,     x = [dq (nv), qvel (nv), act (na)], nx = 2 nv + na,
 * A (nx, nx), B (nx, nu), C (nsensordata, nx), D (nsensordata, nu), row-major, A[i, j] = d x'_i / d x_j.
 *
 * The object ties a SOURCE batch, which is only ever read, to a SCRATCH batch of the same compiled model that the caller
 * creates and owns: P scratch environments per linearised environment, P = 1 + 2 (nx + nu) centred, 1 + nx + 2 nu forward
 * (csrc/lin_core.h: the columns).  One dmc_lin_transition is three launches on one stream: the fan-out of a chunk of
 * source environments into their perturbed columns, dmc_batch_step of the scratch batch exactly as it is, and the
 * differencing of the stepped columns.  Position columns are perturbed as mj_integratePos does and position rows are
 * differenced as mj_differentiatePos does; controls follow mjd_transitionFD's clamped rule against ctrlrange.  Every
 * column takes a full step: there are no skip stages.
 *
 * The scratch batch may be fp64 under an fp32 source batch (the state is converted up in the fan-out, A .. D are
 * converted down on the store); an fp32 scratch batch under an fp64 source is refused.  Every stored element is computed
 * by one lane in a fixed order: two calls give equal bits.
 *
 * Every function returns 0 on success or a negative error code and never throws; dmc_last_error() (dmc_batch.h) returns a
 * thread-local message.
 */
#ifndef DMC_LIN_H_
#define DMC_LIN_H_

#include <stdint.h>

#include "dmc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmc_lin dmc_lin;

/* The joint and actuator tables, a snapshot taken by the caller (later model edits need a new object).
 *   ints:  jnt_type[nj] jnt_qadr[nj] jnt_dadr[nj] ctrllimited[nu]
 *   reals: ctrlrange[2 nu] */
typedef struct dmc_lin_tables {
  int32_t nj, nq, nv, na, nu, nints, nreals;
  const int32_t* ints;
  const double* reals;
} dmc_lin_tables;

/* Validates the tables against both batches' model (sizes, every address the kernels follow, one joint per dof) and
 * uploads them.  eps > 0: the nudge; centered: central differences; nstep >= 1: mj_steps per transition.  The scratch
 * batch must live on the source's device, hold at least P environments and be no less precise than the source; a source
 * batch with per-environment geoms is refused (they are not mirrored).  Synchronous. */
int dmc_lin_create(dmc_batch* src, dmc_batch* scratch, const dmc_lin_tables* tables, double eps, int centered, int nstep,
                   dmc_lin** out);

/* One chunk: source environments [first_env, first_env + nenv), nenv P <= the scratch batch's size.  A (B, nx, nx) and
 * Bm (B, nx, nu) are the WHOLE outputs in the source batch's precision (the chunk's environments are written, every
 * element of them); C (B, nsensordata, nx) and D (B, nsensordata, nu) likewise, or both null: no sensor derivatives
 * (with them the scratch batch's output mask must include the sensors).  Fan-out, dmc_batch_invalidate_async and
 * dmc_batch_step(nstep, plain mj_step) of the scratch batch, difference: all on `hip_stream`, asynchronous, no allocation,
 * no host read.  The source batch is not written. */
int dmc_lin_transition(dmc_lin* l, int first_env, int nenv, void* A, void* Bm, void* C, void* D, void* hip_stream);

/* The first launch of dmc_lin_transition alone: the chunk's perturbed columns are written to the scratch batch (and its
 * stashes invalidated), nothing is stepped.  For inspection, and for callers that step the columns themselves. */
int dmc_lin_fan_out(dmc_lin* l, int first_env, int nenv, void* hip_stream);

/* warn_out (B) int32 on the device: bit w set where some column of the environment raised warning w (DMC_WARN_*) in the
 * last transition that covered it.  A copy on `hip_stream`. */
int dmc_lin_warnings(dmc_lin* l, int32_t* warn_out, void* hip_stream);

/* info[0..11] = {B, columns per environment P, nx, nu, nsensordata, scratch batch size, environments per chunk, source
 * precision, scratch precision, nstep, centered, lanes per workgroup}. */
int dmc_lin_info(const dmc_lin* l, int* info);

/* Releases the device tables; the batches stay the caller's. */
void dmc_lin_destroy(dmc_lin* l);

#ifdef __cplusplus
}
#endif
#endif  /* DMC_LIN_H_ */
