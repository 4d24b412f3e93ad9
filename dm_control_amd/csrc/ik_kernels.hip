// ik_kernels.hip -- batched inverse kinematics (include/dmc_ik.h): qpos_from_site_pose for every environment of a batch
// in one launch.  The iteration itself is ik_core.h.
//
// One lane per environment, one wave per workgroup.  An environment's solve is a chain walk, a k x k factorisation
// (k = 3 or 6) and two passes over the chain's dofs: nothing in it is shared between environments and nothing needs a
// second lane, so there is no cross-lane traffic, no barrier and no masking of finished groups -- a lane that is done
// simply leaves the loop.  The chain constants are staged once per workgroup at the head of its LDS.  What an environment indexes
// at run time (its qpos entries, one axis and anchor per dof, the update) sits in its own column of LDS, lane-major:
// slot s of lane t at (s * envs_per_block + t), conflict-free across the wave and never a register array.  A long chain
// simply seats fewer environments in a wave (64 KiB of LDS per workgroup, tables included).
//
// The host entry points live here too and reach the batch through its public C ABI only.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/dmc_ik.h"
#include "ik_core.h"

namespace dmc {

constexpr int kIkBlock = 64;
constexpr int kIkLdsBudget = 64*1024;
// bytes of the chain tables at the head of a workgroup's LDS (the workspace that follows stays 16-byte aligned)
constexpr int ik_table_bytes(const IkDims& d, int rb) { return (ik_nreals(d)*rb + ik_nints(d)*4 + 15) & ~15; }

template <typename T>
struct IkArgs {
  IkChain<T> ch;
  IkOpts<T> o;
  int B, nq, epb;
  const T* tpos;       // (B, 3) or null
  const T* tquat;      // (B, 4) or null
  const T* qin;        // element k of env e at qin[k*qin_sk + e*qin_se]
  long long qin_sk, qin_se;
  T* qbatch;           // the batch's qpos, (nq, B), or null
  T* qout;             // (B, nq)
  T* err;
  int* steps;
  int* status;
};

template <typename T, int kMode>
__global__ void __launch_bounds__(kIkBlock) ik_kernel(const IkArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ik_smem[];
  const int tid = threadIdx.x;
  const IkDims d = a.ch.d;
  // the chain tables once per workgroup: LDS reads at a uniform address broadcast, and the constants stay out of the
  // scalar registers (read straight from memory they and their addresses overflowed the SGPR file)
  T* sreal = reinterpret_cast<T*>(ik_smem);
  int* sint = reinterpret_cast<int*>(sreal + ik_nreals(d));
  for (int i = tid; i < ik_nreals(d); i += kIkBlock) sreal[i] = a.ch.reals[i];
  for (int i = tid; i < ik_nints(d); i += kIkBlock) sint[i] = a.ch.ints[i];
  __syncthreads();
  const long long env = (long long)blockIdx.x*a.epb + tid;
  if (tid >= a.epb || env >= a.B) return;
  IkChain<T> ch;
  ch.d = d; ch.ints = sint; ch.reals = sreal;
  const int ws = a.epb;
  T* w = reinterpret_cast<T*>(ik_smem + ik_table_bytes(d, (int)sizeof(T))) + tid;
  const int* qmap = sint + 2*d.nb + 3*d.nj;
  for (int s = 0; s < d.nqc; s++) w[(size_t)s*ws] = a.qin[qmap[s]*a.qin_sk + env*a.qin_se];
  T tp[3] = {0, 0, 0}, tq[4] = {1, 0, 0, 0};
  if (kMode & IK_POS) for (int k = 0; k < 3; k++) tp[k] = a.tpos[3*env + k];
  if (kMode & IK_ROT) for (int k = 0; k < 4; k++) tq[k] = a.tquat[4*env + k];
  T en;
  int steps;
  const int status = ik_solve_env<T, kMode>(ch, a.o, tp, tq, w, ws, &en, &steps);
  T* out = a.qout + env*a.nq;
  for (int k = 0; k < a.nq; k++) out[k] = a.qin[k*a.qin_sk + env*a.qin_se];
  for (int s = 0; s < d.nqc; s++) out[qmap[s]] = w[(size_t)s*ws];
  if (a.qbatch) {
    // (the start state may have been the caller's: every entry goes back, the chain's last)
    for (int k = 0; k < a.nq; k++) a.qbatch[(long long)k*a.B + env] = a.qin[k*a.qin_sk + env*a.qin_se];
    for (int s = 0; s < d.nqc; s++) a.qbatch[(long long)qmap[s]*a.B + env] = w[(size_t)s*ws];
  }
  a.err[env] = en;
  a.steps[env] = steps;
  a.status[env] = status;
}

}  // namespace dmc

using namespace dmc;

struct dmc_ik {
  dmc_batch* b = nullptr;
  int B = 0, precision = 0, nq = 0, device = 0, epb = 0, lds = 0;
  IkDims d{};
  dmc_ik_options opt{};
  int* d_ints = nullptr;
  void* d_reals = nullptr;
};

// On purpose not on dmc_api.hip's scaffold of the camera and ray units (dev_alloc, poses_fresh, by_precision): these entry
// points see the batch through its public ABI alone, with their own error channel, DeviceScope and pointer checks.
static thread_local std::string g_ik_err;
static int ik_fail(const std::string& msg, int code = -1) { g_ik_err = msg; return code; }
extern "C" const char* dmc_ik_last_error(void) { return g_ik_err.c_str(); }

namespace {
struct DeviceScope {      // the batch's device for the duration of a call
  int prev = -1;
  bool ok = true;
  explicit DeviceScope(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) { ok = false; prev = -1; return; }
    if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    if (prev == dev) prev = -1;
  }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

template <typename T>
int launch_ik(const dmc_ik* ik, const void* tpos, const void* tquat, const void* qin, T* qbatch, bool inplace, void* qout,
              void* err, int32_t* steps, int32_t* status, hipStream_t stream) {
  IkArgs<T> a;
  a.ch.d = ik->d;
  a.ch.ints = ik->d_ints;
  a.ch.reals = static_cast<const T*>(ik->d_reals);
  const dmc_ik_options& o = ik->opt;
  a.o.tol = (T)o.tol; a.o.rot_weight = (T)o.rot_weight; a.o.reg_threshold = (T)o.regularization_threshold;
  a.o.reg_strength = (T)o.regularization_strength; a.o.max_update_norm = (T)o.max_update_norm;
  a.o.progress_thresh = (T)o.progress_thresh; a.o.max_steps = o.max_steps;
  a.B = ik->B; a.nq = ik->nq; a.epb = ik->epb;
  a.tpos = static_cast<const T*>(tpos); a.tquat = static_cast<const T*>(tquat);
  if (qin) { a.qin = static_cast<const T*>(qin); a.qin_sk = 1; a.qin_se = ik->nq; }
  else { a.qin = qbatch; a.qin_sk = ik->B; a.qin_se = 1; }
  a.qbatch = inplace ? qbatch : nullptr;
  a.qout = static_cast<T*>(qout); a.err = static_cast<T*>(err); a.steps = steps; a.status = status;
  const dim3 grid((unsigned)((ik->B + ik->epb - 1)/ik->epb)), block(kIkBlock);
  const size_t lds = (size_t)ik->lds;
  if (tpos && tquat) hipLaunchKernelGGL((ik_kernel<T, IK_BOTH>), grid, block, lds, stream, a);
  else if (tpos) hipLaunchKernelGGL((ik_kernel<T, IK_POS>), grid, block, lds, stream, a);
  else hipLaunchKernelGGL((ik_kernel<T, IK_ROT>), grid, block, lds, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
}  // namespace

extern "C" int dmc_ik_create(dmc_batch* b, const dmc_ik_chain* c, const dmc_ik_options* opt, dmc_ik** out) {
  if (!b || !c || !opt || !out) return ik_fail("dmc_ik_create: null argument");
  *out = nullptr;
  int info[22] = {0};
  if (dmc_batch_info(b, info) != 0) return ik_fail(std::string("dmc_ik_create: ") + dmc_last_error());
  int nq = 0, is_int = 0;
  if (dmc_batch_field_rows(b, "qpos", &nq, &is_int) != 0 || is_int) return ik_fail("dmc_ik_create: the batch has no qpos");
  IkDims d = {c->nbody, c->njnt, c->ndof, c->nqchain};
  if (d.nb < 1 || d.nj < 1 || d.nd < 1 || d.nqc < 1) return ik_fail("dmc_ik_create: the site's chain has no joint");
  if (d.nd > kIkMaxDof) return ik_fail("dmc_ik_create: " + std::to_string(d.nd) + " chain dofs, at most " + std::to_string(kIkMaxDof));
  if (d.nqc > 2*kIkMaxDof || d.nj > d.nd || d.nb > 4096) return ik_fail("dmc_ik_create: inconsistent chain sizes");
  if (opt->max_steps < 1) return ik_fail("dmc_ik_create: max_steps must be at least 1");
  // every index the kernel follows is checked here, once
  static const int qw[4] = {7, 4, 1, 1}, dw[4] = {6, 3, 1, 1};
  std::vector<int> rot(d.nd, 0), seen(d.nj, 0);
  int nmov = 0;
  for (int k = 0; k < d.nb; k++) {
    const int j0 = c->body_jntadr[k], jn = c->body_jntnum[k];
    if (jn < 0 || (jn > 0 && (j0 < 0 || j0 + jn > d.nj))) return ik_fail("dmc_ik_create: body joint range outside the chain");
    for (int j = j0; j < j0 + jn; j++) {
      seen[j]++;
      if (c->jnt_type[j] == DMC_JNT_FREE && jn != 1) return ik_fail("dmc_ik_create: a free joint must be its body's only joint");
    }
  }
  for (int j = 0; j < d.nj; j++) {
    const int t = c->jnt_type[j];
    if (seen[j] != 1) return ik_fail("dmc_ik_create: every chain joint must belong to exactly one chain body");
    if (t < 0 || t > 3) return ik_fail("dmc_ik_create: unknown joint type");
    if (c->jnt_qslot[j] < 0 || c->jnt_qslot[j] + qw[t] > d.nqc || c->jnt_dslot[j] < 0 || c->jnt_dslot[j] + dw[t] > d.nd)
      return ik_fail("dmc_ik_create: joint address outside the chain");
    for (int i = 0; i < dw[t]; i++) {
      rot[c->jnt_dslot[j] + i] = t == DMC_JNT_BALL || t == DMC_JNT_HINGE || (t == DMC_JNT_FREE && i >= 3);
      if ((c->dof_movable[c->jnt_dslot[j] + i] != 0) != (c->dof_movable[c->jnt_dslot[j]] != 0))
        return ik_fail("dmc_ik_create: dof_movable must be uniform over a joint");
    }
  }
  for (int s = 0; s < d.nqc; s++) if (c->qmap[s] < 0 || c->qmap[s] >= nq) return ik_fail("dmc_ik_create: qpos address outside the model");
  for (int k = 0; k < d.nd; k++) nmov += c->dof_movable[k] != 0;
  if (!nmov) return ik_fail("dmc_ik_create: no movable dof on the site's chain");

  dmc_ik* ik = new dmc_ik;
  ik->b = b; ik->B = info[0]; ik->precision = info[1]; ik->nq = nq; ik->d = d; ik->opt = *opt;
  const int rb = ik->precision == 64 ? 8 : 4;
  ik->epb = (kIkLdsBudget - ik_table_bytes(d, rb))/(ik_nslots(d)*rb);
  if (ik->epb > kIkBlock) ik->epb = kIkBlock;
  if (ik->epb < 1) { delete ik; return ik_fail("dmc_ik_create: the chain does not fit one workgroup's LDS"); }
  ik->lds = ik_table_bytes(d, rb) + ik->epb*ik_nslots(d)*rb;
  void* qp = dmc_batch_device_ptr(b, "qpos");
  hipPointerAttribute_t attr;
  if (!qp || hipPointerGetAttributes(&attr, qp) != hipSuccess) { delete ik; return ik_fail("dmc_ik_create: the batch's qpos is not device memory"); }
  ik->device = attr.device;
  DeviceScope dev(ik->device);
  if (!dev.ok) { delete ik; return ik_fail("dmc_ik_create: cannot select the batch's device"); }

  std::vector<int> ints;
  auto put = [&](const int32_t* p, int n) { ints.insert(ints.end(), p, p + n); };
  put(c->body_jntadr, d.nb); put(c->body_jntnum, d.nb); put(c->jnt_type, d.nj); put(c->jnt_qslot, d.nj); put(c->jnt_dslot, d.nj);
  put(c->qmap, d.nqc);
  for (int k = 0; k < d.nd; k++) ints.push_back(c->dof_movable[k] != 0);
  ints.insert(ints.end(), rot.begin(), rot.end());
  std::vector<double> reals;
  auto putr = [&](const double* p, int n) { reals.insert(reals.end(), p, p + n); };
  putr(c->body_pos, 3*d.nb); putr(c->body_quat, 4*d.nb); putr(c->jnt_axis, 3*d.nj); putr(c->jnt_pos, 3*d.nj); putr(c->jnt_qpos0, d.nj);
  putr(c->site_pos, 3); putr(c->site_quat, 4);
  if ((int)ints.size() != ik_nints(d) || (int)reals.size() != ik_nreals(d)) { delete ik; return ik_fail("dmc_ik_create: table size mismatch"); }
  std::vector<float> reals32(reals.begin(), reals.end());
  const void* src = rb == 8 ? (const void*)reals.data() : (const void*)reals32.data();
  bool ok = hipMalloc((void**)&ik->d_ints, ints.size()*sizeof(int)) == hipSuccess;
  ok = ok && hipMalloc(&ik->d_reals, reals.size()*rb) == hipSuccess;
  ok = ok && hipMemcpy(ik->d_ints, ints.data(), ints.size()*sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipMemcpy(ik->d_reals, src, reals.size()*rb, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) { dmc_ik_destroy(ik); return ik_fail("dmc_ik_create: device allocation failed"); }
  *out = ik;
  return 0;
}

extern "C" int dmc_ik_solve(dmc_ik* ik, const void* target_pos, const void* target_quat, const void* qpos_in, int inplace,
                            void* qpos_out, void* err_norm_out, int32_t* steps_out, int32_t* status_out, void* hip_stream) {
  if (!ik) return ik_fail("dmc_ik_solve: null handle (a dmc_ik needs a batch on a GPU; there is no CPU fallback)");
  if (!target_pos && !target_quat) return ik_fail("dmc_ik_solve: at least one of target_pos or target_quat must be given");
  if (!qpos_out || !err_norm_out || !steps_out || !status_out) return ik_fail("dmc_ik_solve: null output");
  void* qb = dmc_batch_device_ptr(ik->b, "qpos");      // (every call: the field can be rebound)
  if (!qb) return ik_fail("dmc_ik_solve: the batch has no qpos");
  DeviceScope dev(ik->device);
  if (!dev.ok) return ik_fail("dmc_ik_solve: cannot select the batch's device");
  const hipStream_t s = (hipStream_t)hip_stream;
  const int rc = ik->precision == 64
      ? launch_ik<double>(ik, target_pos, target_quat, qpos_in, static_cast<double*>(qb), inplace != 0, qpos_out, err_norm_out, steps_out, status_out, s)
      : launch_ik<float>(ik, target_pos, target_quat, qpos_in, static_cast<float*>(qb), inplace != 0, qpos_out, err_norm_out, steps_out, status_out, s);
  if (rc) return ik_fail("dmc_ik_solve: kernel launch failed", rc);
  if (inplace && dmc_batch_invalidate_async(ik->b, hip_stream) != 0) return ik_fail(std::string("dmc_ik_solve: ") + dmc_last_error());
  return 0;
}

extern "C" int dmc_ik_info(const dmc_ik* ik, int* info) {
  if (!ik || !info) return ik_fail("dmc_ik_info: null argument");
  const int v[7] = {ik->B, ik->precision, ik->epb, ik->lds, (ik->B + ik->epb - 1)/ik->epb, ik->d.nd, ik->d.nqc};
  for (int k = 0; k < 7; k++) info[k] = v[k];
  return 0;
}

extern "C" void dmc_ik_destroy(dmc_ik* ik) {
  if (!ik) return;
  if (ik->d_ints) (void)hipFree(ik->d_ints);
  if (ik->d_reals) (void)hipFree(ik->d_reals);
  delete ik;
}
