/* dmc_con.h -- C-ABI of the batched contact wrenches (libdmc_hip.so, csrc/con_kernels.hip; entry points in
 * csrc/dmc_api.hip).
 *
 * Replaces, for every environment of a dmc_batch at once and without leaving the device, the loop over mjData.contact a
 * task layer runs on the host -- mj_contactForce per contact, the rotation into the world mj_rnePostConstraint applies,
 * the sum over the contacts of a body or a set of geoms -- and the <touch> sensor a model would otherwise need.
 *
 * Contact c < ncon between geom1 and geom2 has the contact-frame force lf[6] ("contact_force") and the frame F
 * ("contact_frame", rows normal, tangent, tangent).  The force ON geom2's body is f_c = F' lf[0:3], the torque about the
 * contact point t_c = F' lf[3:6]; geom1's body receives -f_c, -t_c.
 *
 * A target is a set of geoms S, a filter set O and a named body.  A contact counts with s = +1 when geom2 is in S, geom1
 * in O and geom1 not in S; with s = -1 when geom1 is in S, geom2 in O and geom2 not in S.  Contacts with both geoms in S
 * are internal and skipped.  Per (environment, target): force = sum s f_c, torque = sum s (t_c + (p_c - r) x f_c) with r
 * the named body's xipos / xpos / 0, normal = sum lf[0], count, dist = the smallest contact_dist (+inf: none).  The
 * contacts are summed in index order in plain arithmetic (no atomics: the same bits on every launch).
 *
 * The kernels read what the LAST step / forward launch wrote: ncon, contact_geom1/2, contact_dist, contact_pos,
 * contact_frame, contact_force (OUT_CONTACT) and, for r and the local frame, xipos / xpos / xmat.  After a plain legacy
 * step the contact list is newer than the forces (the trailing partial mj_step1 re-runs the collision without the
 * constraints): run a forward first -- dmc_con_warmstart brackets one so that the solver's warm start is not moved.
 * The field pointers are read from the batch at every call, so a field rebound with dmc_batch_bind is followed.
 *
 * Every function returns 0 on success or a negative error code and never throws; dmc_last_error() (dmc_batch.h) returns a
 * thread-local message.
 */
#ifndef DMC_CON_H_
#define DMC_CON_H_

#include <stdint.h>

#include "dmc_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmc_con dmc_con;

#define DMC_CON_MAX_TARGETS 64
#define DMC_CON_ABOUT_COM 0
#define DMC_CON_ABOUT_ORIGIN 1
#define DMC_CON_ABOUT_WORLD 2

/* ntarget targets over a model of ngeom geoms.
 *   words: ceil(ngeom / 32), the words of one mask; bit g of a mask is bit (g % 32) of word g / 32.
 *   body (ntarget): the named body of every target (r and the local frame are its own).
 *   masks (ntarget, 2, words): S, then O.
 *   about: DMC_CON_ABOUT_*. */
typedef struct dmc_con_tables {
  int32_t ntarget, ngeom, words, about;
  const int32_t* body;
  const uint32_t* masks;
} dmc_con_tables;

/* Validates the tables again (the Python side built them) and uploads them once.  Fails, by message, on a batch with
 * nconmax == 0, on more than DMC_CON_MAX_TARGETS targets, on an empty S, on a mask bit or a body id outside the model
 * and on a mask size that is not the model's.  Synchronous. */
int dmc_con_create(dmc_batch* b, const dmc_con_tables* tables, dmc_con** out);

/* wrench_out (B, nconmax, 6) in the batch precision = [f_c, t_c] of every contact slot, zeros past the environment's
 * ncon; EVERY element is written.  ONE launch on `hip_stream`; asynchronous, no allocation, no host read: capturable
 * in a HIP graph.  Fails (-3) when the batch's output mask lacks OUT_CONTACT, or lacked it at the last launch. */
int dmc_con_wrench(dmc_con* c, void* wrench_out, void* hip_stream);

/* The net contact wrench of every (environment, target) in ONE launch, as above.  force_out, torque_out (B, ntarget, 3)
 * and normal_out, dist_out (B, ntarget) in the batch precision, count_out (B, ntarget) int32; any may be NULL (not all).
 * local != 0: force and torque rotated into the named body's frame (xmat').  Fails (-3) when the batch's output mask
 * lacks OUT_CONTACT or the pose array `about` / `local` reads. */
int dmc_con_net(dmc_con* c, int local, void* force_out, void* torque_out, void* normal_out, void* count_out, void* dist_out,
                void* hip_stream);

/* restore == 0: copies the batch's qacc_warmstart into a buffer the object owns; restore != 0: copies it back.  Device
 * to device on `hip_stream`, asynchronous, capturable.  Brackets the forward launch of a refresh: a query must not move
 * the solver's warm start. */
int dmc_con_warmstart(dmc_con* c, int restore, void* hip_stream);

/* info[0..7] = {B, precision, ntarget, nconmax, lanes per workgroup, words per mask, static LDS bytes of the net launch,
 * the output-mask bits (OUT_*) the net launch needs with local == 0} (no counterpart in the reference: the launch shape). */
int dmc_con_info(const dmc_con* c, int* info);

/* Replaces nothing in the reference; releases the device tables. */
void dmc_con_destroy(dmc_con* c);

#ifdef __cplusplus
}
#endif
#endif  /* DMC_CON_H_ */
