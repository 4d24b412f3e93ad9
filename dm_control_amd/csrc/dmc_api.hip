// dmc_api.hip -- host side of libdmc_hip.so: the C-ABI of include/dmc_batch.h.
// Owns device memory (SoA mjData arrays), builds the kernel tables / LDS layout
// and launches the fused step kernel.  No CPU fallback exists: every entry point
// that computes runs the HIP kernel or returns an error.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/dmc_batch.h"
#include "step_kernel.hip.h"
#include "step_tables.h"

namespace dmc {
hipError_t launch_step_f32(const LaunchGeom& g, hipStream_t stream, const StepLayout* d_layout, const StepOpts<float>& o,
                           const int* g_mi, const float* g_mr, const int* g_mc, const StepIO<float>& io, int nstep, int legacy, int mode, int outmask, int nsub);
hipError_t launch_step_f64(const LaunchGeom& g, hipStream_t stream, const StepLayout* d_layout, const StepOpts<double>& o,
                           const int* g_mi, const double* g_mr, const int* g_mc, const StepIO<double>& io, int nstep, int legacy, int mode, int outmask, int nsub);
int step_coop_open_f32(const LaunchGeom& g);
}  // namespace dmc

using namespace dmc;

static thread_local std::string g_err;
static int fail(const std::string& msg, int code = -1) { g_err = msg; return code; }
#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_), -2); \
  } while (0)

struct dmc_model {
  HostModel hm;
};

// The batch's data fields: one id per entry of DMC_DATA_REAL_FIELDS / DMC_DATA_INT_FIELDS (dmc_model_layout.h), in that
// order, and one reserved slot for the per-environment geoms, which exist once dmc_batch_set_env_geoms declared them.
enum FieldId {
#define X(name, count, flags) F_##name,
  DMC_DATA_REAL_FIELDS(X) DMC_DATA_INT_FIELDS(X)
#undef X
  F_env_geom, F_COUNT
};
struct Field {
  const char* name = nullptr;      // null: not declared (F_env_geom)
  int rows = 0;
  bool is_int = false;
  int flags = 0;             // DMC_FIELD_*
  void* dev = nullptr;       // current binding
  void* owned = nullptr;     // allocated by us (may differ from dev after dmc_batch_bind)
};

struct TimerPair { hipEvent_t e0, e1; int which, count; };
struct Profiler {
  bool on = false;
  double duration[2] = {0, 0};      // seconds: [mjTIMER_STEP, mjTIMER_FORWARD]
  long long number[2] = {0, 0};
  std::vector<TimerPair> pending, spare;
};
struct Xfer {
  static constexpr int kSlots = 4;
  void* h_in[kSlots] = {}; void* d_in[kSlots] = {}; size_t cap_in[kSlots] = {}; hipEvent_t ev_in[kSlots] = {}; int next = 0;
  void* h_out = nullptr; void* d_out = nullptr; size_t cap_out = 0; hipEvent_t ev_out = nullptr;
  std::vector<std::pair<Field*, size_t>> pending;      // fields of the enqueued get and their offsets (elements) in the staging
  bool out_in_flight = false;
};

struct dmc_batch {
  const dmc_model* model = nullptr;
  int B = 0, device = 0, precision = 0;
  StepTables tb;
  LaunchGeom geom;
  std::vector<void*> dev_bufs;      // every device allocation of the batch (dev_alloc), freed by dmc_batch_destroy
  int* d_mi = nullptr;
  int* d_mc = nullptr;      // cold int tables (stay in global memory)
  void* d_mr = nullptr;
  StepLayout* d_layout = nullptr;
  Field fields[F_COUNT];      // fixed: a Field* stays valid for the life of the batch
  int outmask = OUT_ALL;
  int launched_mask = 0;      // the output mask the last step / forward launch ran with (what the derived arrays in HBM hold)
  int ndebug = 0;
  void* d_debug = nullptr;
  int* d_debug_i = nullptr;
  long long* d_prof = nullptr;
  size_t elem = 0;  // sizeof(T)
  // per-env stash of the position / velocity stage between legacy steps (StepIO::stash_*); epoch: bumped by every
  // host-side edit that can change what the stage depends on, which invalidates all stashes at once
  void* d_stash_r = nullptr; int* d_stash_i = nullptr; int* d_epoch = nullptr; int stash_on = 0; int stash_auto = 0;
  int xfrc_on = 0;               // xfrc_applied was written / bound / exposed: the kernel reads it from now on
  void* d_ns_A = nullptr;        // noslip: (B, nslip, nslip) reals in global memory (StepOpts::ns_A)
  int* d_work = nullptr;         // work queue of launches with a resident-only grid: {next item, finished waves} (StepIO::work)
  int ncu = 0;                   // compute units of the device
  void* d_kstash = nullptr; int* d_kstash_i = nullptr;      // kinematic stash (StepIO::kstash), on unless DMC_NO_KSTASH
  int *d_cost = nullptr, *d_order = nullptr; int lpt = 0, nitems = 0;      // longest-first scheduling of queued launches (StepIO::cost / order)
  int* d_prog = nullptr; int max_slices = 0;   // sliced items of queued multi-step launches (StepIO::prog / slices)
  unsigned long long* d_hand = nullptr; int hand_n = 0; int nxcd = 1;      // hand-off records of the pieces; queues per launch (one per XCD)
  void* d_gscr = nullptr;        // large models: (B, n_gs) reals of per-env global scratch (StepOpts::gscr)
  int* d_trace = nullptr;        // wave trace (dmc_batch_wave_trace): ring of 8 launches x (8, nitems) ints, or null
  Profiler* prof = nullptr;      // launch timers (dmc_batch_enable_profiling), or null
  Xfer* xfer = nullptr;      // pinned / device staging of the asynchronous host transfers (dmc_batch_set_async / get_async), or null
  void* d_probe = nullptr; int probe_geom = 0, probe_cap = 0;      // substep probe (dmc_batch_set_step_probe): caller-owned (cap, 3, B) reals
  int trace_launch = 0;    // launches since the trace was switched on (ring slot = trace_launch % 8)
  int* d_rj_i = nullptr; double* d_rj_r = nullptr;      // joint randomisation: (4, njnt) ints {type, qposadr, limited, 0} and (2, njnt) ranges
  int* d_eg_slot = nullptr;      // per-env world geoms: (ngeom) slot table on the device (field F_env_geom holds the values)
  // a model-specialised kernel built on demand for this model (dmc_batch_attach_specialised): the loaded object, its launch
  // entry, whether it holds the optional launch features (step_core.h kFeat)
  void* spec_so = nullptr; void* spec_launch = nullptr; int spec_features = 0; int spec_coop = 0;
  int spec_task_bytes = 0;      // > 0: the attached kernel carries a task epilogue with an argument block of this size
  void* d_task_args = nullptr; int task_on = 0;      // its arguments on the device; whether the next step launches run it
};

// Device memory of an owner (the batch, a camera set, a rays object: whatever holds a `dev_bufs` list): allocate, optionally
// zero or fill from `init`, record; a failure leaves *ptr null and the error "hipMalloc <what>: <hip error>".  The owner's
// destroy frees what is recorded (dev_free_all); dev_free releases one buffer early.
template <class Owner, typename P>
static int dev_alloc(Owner* b, P** ptr, size_t bytes, bool zero, const char* what, const void* init = nullptr) {
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e == hipSuccess && zero) e = hipMemset(p, 0, bytes);
  if (e == hipSuccess && init) e = hipMemcpy(p, init, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) { if (p) (void)hipFree(p); return fail(std::string("hipMalloc") + (*what ? " " : "") + what + ": " + hipGetErrorString(e), -2); }
  b->dev_bufs.push_back(p);
  *ptr = (P*)p;
  return 0;
}
template <class Owner, typename P>
static void dev_free(Owner* b, P** ptr) {
  if (!*ptr) return;
  b->dev_bufs.erase(std::find(b->dev_bufs.begin(), b->dev_bufs.end(), (void*)*ptr));
  (void)hipFree(*ptr);
  *ptr = nullptr;
}
template <class Owner>
static void dev_free_all(Owner* b) {
  for (void* p : b->dev_bufs) (void)hipFree(p);
  b->dev_bufs.clear();
}

extern "C" const char* dmc_last_error(void) { return g_err.c_str(); }

extern "C" int dmc_model_create(const int32_t* ints, int n_ints, const double* reals, int n_reals, dmc_model** out) {
  if (!ints || !reals || !out) return fail("null argument");
  dmc_model* m = new dmc_model;
  std::string err;
  if (!host_model_parse(&m->hm, ints, n_ints, reals, n_reals, &err)) { delete m; return fail(err); }
  *out = m;
  return 0;
}
extern "C" void dmc_model_destroy(dmc_model* m) { delete m; }

// (only where a caller passes a name: everything inside the library addresses fields by id)
static Field* find_field(dmc_batch* b, const char* name) {
  if (name) for (Field& f : b->fields) if (f.name && !strcmp(f.name, name)) return &f;
  return nullptr;
}

// ---- profiling contract (mujoco/engine.py:135-137 enable_profiling -> wrapper.enable_timer; mjData.timer[]) ------
// MuJoCo brackets mj_step / mj_forward with the mjcb_time callback and accumulates duration and call count per timer.
// Here a launch IS the step: with profiling enabled every launch is bracketed by two hipEvents on its stream; the pairs
// are resolved lazily (completed ones whenever a new launch is issued, all of them when the timer is read), so an
// asynchronous caller is not serialised.  Launches recorded into a HIP graph are not timed (events cannot be queried
// across replays).
static void prof_drain(Profiler* p, bool all) {
  size_t k = 0;
  for (; k < p->pending.size(); k++) {
    TimerPair& t = p->pending[k];
    if (all || p->pending.size() - k > 256) { if (hipEventSynchronize(t.e1) != hipSuccess) break; }
    else if (hipEventQuery(t.e1) != hipSuccess) break;
    float ms = 0;
    if (hipEventElapsedTime(&ms, t.e0, t.e1) == hipSuccess) { p->duration[t.which] += 1e-3 * ms; p->number[t.which] += t.count; }
    p->spare.push_back(t);
  }
  (void)hipGetLastError();      // (hipErrorNotReady from the query is not an error of the caller)
  p->pending.erase(p->pending.begin(), p->pending.begin() + k);
}
static void prof_free(Profiler* p) {
  (void)hipDeviceSynchronize();
  for (auto* v : {&p->pending, &p->spare}) for (TimerPair& t : *v) { (void)hipEventDestroy(t.e0); (void)hipEventDestroy(t.e1); }
  delete p;
}
static bool prof_begin(dmc_batch* b, hipStream_t stream, TimerPair* t) {
  Profiler* p = b->prof;
  if (!p || !p->on) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (stream && hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return false;
  prof_drain(p, false);
  if (!p->spare.empty()) { *t = p->spare.back(); p->spare.pop_back(); }
  else if (hipEventCreate(&t->e0) != hipSuccess || hipEventCreate(&t->e1) != hipSuccess) return false;
  return hipEventRecord(t->e0, stream) == hipSuccess;
}
static void prof_end(dmc_batch* b, hipStream_t stream, TimerPair t, int which, int count) {
  t.which = which; t.count = count;
  if (hipEventRecord(t.e1, stream) == hipSuccess) b->prof->pending.push_back(t); else b->prof->spare.push_back(t);
}
static void xfer_free(Xfer* x) {
  (void)hipDeviceSynchronize();
  for (int k = 0; k < Xfer::kSlots; k++) { if (x->h_in[k]) (void)hipHostFree(x->h_in[k]); if (x->d_in[k]) (void)hipFree(x->d_in[k]); if (x->ev_in[k]) (void)hipEventDestroy(x->ev_in[k]); }
  if (x->h_out) (void)hipHostFree(x->h_out);
  if (x->d_out) (void)hipFree(x->d_out);
  if (x->ev_out) (void)hipEventDestroy(x->ev_out);
  delete x;
}

static int choose_geometry(dmc_batch* b, int lanes_per_env) {
  const StepLayout& L = b->tb.L;
  const size_t tables = (size_t)(b->precision == 64 ? opts_lds_bytes<double>() : opts_lds_bytes<float>()) +
                        (size_t)L.n_mi * sizeof(int) + (size_t)L.n_mr_lds * b->elem + (L.d.coldlds ? (size_t)L.n_mc * sizeof(int) : 0);
  const size_t env_bytes = (size_t)L.n_sr * b->elem + (size_t)L.n_si * sizeof(int);
  const size_t lds_cu = 160 * 1024;
  // automatic: small models (cheetah, nv = 9) leave most of a 64-lane group idle, so
  // two environments share a wavefront; measured on MI355X (scripts/perf_probe.py)
  int lpe = lanes_per_env ? lanes_per_env : (b->tb.L.d.nv <= 12 ? 32 : 64);
  if (lpe != 64 && lpe != 32 && lpe != 16) return fail("lanes_per_env must be 64, 32 or 16");
  const int epw = 64 / lpe;
  int best_w = 0; long best_score = -1, best_blocks = 1;
  // The kernels are built for 2 waves per SIMD (256 VGPRs): at most 8 resident waves per CU whatever the LDS would
  // allow.  Workgroups of more than 4 waves were tried (512 threads: humanoid 7 environments in one workgroup instead
  // of 2 x 3) and measured slower (1.20 M vs 1.29 M env-steps/s), so 4 waves stays the largest shape.
  const int force_w = getenv("DMC_WAVES") ? atoi(getenv("DMC_WAVES")) : 0;      // tuning studies only
  // ... with one exception: FIVE waves when that is what holds one more environment than any smaller shape (the 62-dof
  // models at offload level 3: 5 x 29.8 KB + one 10.8 KB table copy = 159.6 KB; +25 % residency, round 4)
  for (int w = force_w > 5 ? force_w : 5; w >= 1; w--) {      // (more than five waves only when forced: needs kernels built with -DDMC_MAX_THREADS=<64 w>)
    if (force_w && w != force_w) continue;
    const size_t bytes = tables + (size_t)w * epw * env_bytes;
    if (bytes > lds_cu) continue;
    long blocks = (long)(lds_cu / bytes);
    if (blocks * w > 8) blocks = 8 / w;             // VGPR-limited: 2 waves per SIMD
    if (blocks < 1) continue;
    const long score = blocks * w * epw;            // resident envs per CU
    // fewer waves per workgroup only for a clear gain in residency: 4-wave groups give grids that divide the
    // batch evenly (cartpole, B = 4096: 3-wave groups = 683 workgroups ran 1.8x slower than 4-wave = 512)
    if (best_score < 0 || score * 100 > best_score * 115) { best_score = score; best_w = w; best_blocks = blocks; }
  }
  // a batch too small to fill the chip (soccer: 256 environments per GPU): spread it over as many CUs as possible --
  // the smallest workgroup that still holds the batch in one round (one wave alone on a CU shares nothing)
  if (best_w) {
    const long cus = b->ncu > 0 ? b->ncu : 256, need = ((long)b->B + cus * epw - 1) / (cus * epw);      // waves per CU to hold B at once
    if (need < best_w && !force_w) { best_w = (int)std::max(1L, need); best_blocks = std::min(8L / best_w, (long)(lds_cu / (tables + (size_t)best_w * epw * env_bytes))); }
  }
  if (!best_w) return fail("environment scratch does not fit in 160 KiB of LDS; lower nconmax/njmax");
  LaunchGeom& g = b->geom;
  g.lpe = lpe; g.waves = best_w; g.envs_per_block = best_w * epw;
  g.lds_bytes = (int)(tables + (size_t)g.envs_per_block * env_bytes);
  g.grid = (b->B + g.envs_per_block - 1) / g.envs_per_block;
  g.blocks_per_cu = (int)std::max(1L, best_blocks);
  // a batch of more workgroups than the chip holds at once: launch the resident ones, their waves claim the rest
  // from the work queue as they finish (step_kernel_body)
  g.queue = 0;
  if (g.grid > b->ncu * g.blocks_per_cu && !getenv("DMC_NO_QUEUE")) { g.grid = b->ncu * g.blocks_per_cu; g.queue = 1; }
  g.static_id = -1;
#if DMC_NSTATIC > 0
  {
    static const StepLayout baked[DMC_NSTATIC] = DMC_STATIC_LAYOUT_LIST;
    for (int k = 0; k < DMC_NSTATIC; k++) if (!memcmp(&baked[k], &L, sizeof(StepLayout))) g.static_id = k;
    if (getenv("DMC_NO_STATIC")) g.static_id = -1;
  }
#endif
  return 0;
}

static int upload_tables(dmc_batch* b) {
  const StepLayout& L = b->tb.L;
  HIP_TRY(hipMemcpy(b->d_mi, b->tb.mi.data(), (size_t)L.n_mi * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->d_mc, b->tb.mc.data(), b->tb.mc.size() * sizeof(int), hipMemcpyHostToDevice));
  if (b->precision == 64) {
    HIP_TRY(hipMemcpy(b->d_mr, b->tb.mr.data(), (size_t)L.n_mr * sizeof(double), hipMemcpyHostToDevice));
  } else {
    std::vector<float> f(b->tb.mr.begin(), b->tb.mr.end());
    HIP_TRY(hipMemcpy(b->d_mr, f.data(), (size_t)L.n_mr * sizeof(float), hipMemcpyHostToDevice));
  }
  return 0;
}

extern "C" int dmc_batch_create(const dmc_model* m, int batch_size, int device_id, int precision,
                                int nconmax, int njmax, int lanes_per_env, dmc_batch** out) {
  const int caps[3] = {nconmax, njmax, lanes_per_env};
  return dmc_batch_create_caps(m, batch_size, device_id, precision, caps, 3, out);
}
// the data fields of DMC_DATA_*_FIELDS, zeroed
static int create_fields(dmc_batch* b) {
  const StepDims& d = b->tb.L.d;
  const int nq = d.nq, nv = d.nv, nu = d.nu, na = d.na, nbody = d.nbody, ngeom = d.ngeom, nsite = d.nsite,
            nsensordata = d.nsensordata, nmocap = d.nmocap, nconmax = d.nconmax;
  auto add = [&](FieldId id, const char* name, int rows, bool is_int, int flags) {
    Field& f = b->fields[id];
    f.name = name; f.rows = rows; f.is_int = is_int; f.flags = flags;
    const size_t es = is_int ? sizeof(int) : ((flags & DMC_FIELD_F64) ? sizeof(double) : b->elem);
    if (dev_alloc(b, &f.owned, (size_t)std::max(1, rows) * b->B * es, true, "field")) return -2;
    f.dev = f.owned;
    return 0;
  };
#define X(name, count, flags) if (add(F_##name, #name, count, false, flags)) return -2;
  DMC_DATA_REAL_FIELDS(X)
#undef X
#define X(name, count, flags) if (add(F_##name, #name, count, true, flags)) return -2;
  DMC_DATA_INT_FIELDS(X)
#undef X
  return 0;
}
// (what dmc_batch_create_caps does to the new batch: any failure returns, and the caller destroys the batch)
static int batch_init(dmc_batch* b, int nconmax, int njmax, int lanes_per_env, int njcon, int jlevel) {
  const dmc_model* m = b->model;
  const int batch_size = b->B;
  std::string err;
  { int ncu = 0; if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, b->device) != hipSuccess || ncu < 1) ncu = 256; b->ncu = ncu; }
  // The contact rows and the kept factor of M leave LDS for the per-env global scratch on the 17 .. 32-dof models so that
  // more environments are resident per CU (level 1: config 3 +24 %).  A batch of at most one environment per CU has
  // nothing to gain from residency and pays a global round trip wherever a row is read: it keeps them in LDS
  // (soccer 2v2, B = 256: +3 %; at B = 4096 the same choice costs 8 %).  DMC_JLEVEL=<n>: tuning override.
  if (jlevel < 0 && getenv("DMC_JLEVEL")) jlevel = atoi(getenv("DMC_JLEVEL"));
  const bool small_auto = jlevel < 0 && batch_size <= b->ncu && DMC_JGLOBAL_LEVEL(m->hm.nv) == 1;
  if (!step_tables_build(&b->tb, m->hm, nconmax, njmax, &err, njcon, small_auto ? 0 : jlevel)) return fail(err);
  if (small_auto) {
    // ... unless only the default layout has a baked model-specialised kernel (the generic one is 2 - 3 x slower: that
    // would be a bad trade for a global round trip per row)
    // ... and unless the level-0 layout does not fit 160 KiB of LDS at all (a large caller-chosen nconmax / njmax): the
    // default level, which keeps those rows out of LDS, is what such a batch was built with before this choice existed
    const bool fits = choose_geometry(b, lanes_per_env) == 0;
    if (!fits || b->geom.static_id < 0) {
      StepTables def;
      if (step_tables_build(&def, m->hm, nconmax, njmax, &err, njcon, -1)) {
        StepTables keep = b->tb; LaunchGeom kg = b->geom;
        b->tb = def;
        const bool def_fits = choose_geometry(b, lanes_per_env) == 0;
        if (fits && (!def_fits || b->geom.static_id < 0)) { b->tb = keep; b->geom = kg; }
      } else if (!fits) return fail(err);
    }
  }
  if (choose_geometry(b, lanes_per_env)) return -1;
  const StepLayout& L = b->tb.L;
  const StepDims& d = L.d;
  if (dev_alloc(b, &b->d_mi, (size_t)L.n_mi * sizeof(int), false, "") || dev_alloc(b, &b->d_mc, b->tb.mc.size() * sizeof(int), false, "") ||
      dev_alloc(b, &b->d_mr, (size_t)L.n_mr * b->elem, false, "") || dev_alloc(b, &b->d_layout, sizeof(StepLayout), false, "", &L)) return -2;
  if (upload_tables(b)) return -2;
  b->tb.opts.g_mr = b->d_mr;
  if (d.nslip) {
    if (dev_alloc(b, &b->d_ns_A, (size_t)b->B * d.nslip * d.nslip * b->elem, false, "noslip matrix")) return -2;
    b->tb.opts.ns_A = b->d_ns_A;
  }
  const int one = 1;
  if (dev_alloc(b, &b->d_epoch, sizeof(int), false, "stash epoch", &one)) return -2;
  // work[1]: finished waves; work[32 (1 + x)]: head of XCD x's queue (a 128-byte line each)
  if (dev_alloc(b, &b->d_work, 32 * 9 * sizeof(int), true, "work queue")) return -2;
  // (a mocap pose is an input of mj_kinematics that the stash's (qpos, qvel) comparison does not see: no stash for those models)
  if (!getenv("DMC_NO_KSTASH") && !d.nmocap) {
    const size_t nk = (size_t)kstash_record(d.nq, d.nv, L.s_qM - L.s_xpos, L.s_xpos, (int)b->elem).stride;      // (step_layout.h)
    if (dev_alloc(b, &b->d_kstash, (size_t)b->B * nk * b->elem, false, "kinematic stash") ||
        dev_alloc(b, &b->d_kstash_i, (size_t)b->B * sizeof(int), true, "kinematic stash")) return -2;      // epoch 0: never valid
  }
  if (b->geom.queue) {
    // queued step launches of several physics steps hand an item out in pieces (StepIO::slices; DMC_SLICES=<n>: at most n
    // pieces, 1 = whole items)
    const int nit = (b->B * b->geom.lpe + 63) / 64;
    // One queue per XCD, served by the waves that run on it (step_kernel_body): what an environment leaves in global
    // memory between its pieces then stays behind ONE L2.  An MI355X in SPX mode is 8 XCDs x 32 CUs; a device of at most
    // one XCD's worth of CUs (CPX partitions) has one L2 and one queue; anything else keeps whole items in one queue
    // per launch (DMC_XCDS overrides the count).
    b->nxcd = getenv("DMC_XCDS") ? std::max(1, std::min(8, atoi(getenv("DMC_XCDS")))) : (b->ncu == 256 ? 8 : 1);
    if (b->geom.grid < 8 * b->nxcd) b->nxcd = 1;      // (every queue needs waves of its own XCD: the dispatcher deals workgroups round)
    const bool one_l2_per_queue = b->nxcd > 1 || b->ncu <= 40 || getenv("DMC_XCDS");
    b->max_slices = getenv("DMC_SLICES") ? atoi(getenv("DMC_SLICES")) : (one_l2_per_queue ? 8 : 1);
    auto hw = [&](int n) { return b->precision == 64 ? n : (n + 1) / 2; };
    b->hand_n = hw(d.nq) + 2 * hw(d.nv) + hw(d.na) + 1;
    if (dev_alloc(b, &b->d_prog, (size_t)nit * sizeof(int), true, "piece counters") ||
        dev_alloc(b, &b->d_hand, (size_t)b->B * b->hand_n * sizeof(unsigned long long), false, "piece counters")) return -2;
  }
  if (b->geom.queue && !getenv("DMC_NO_LPT")) {
    b->nitems = (b->B * b->geom.lpe + 63) / 64;
    if (dev_alloc(b, &b->d_cost, (size_t)b->nitems * sizeof(int), true, "schedule") ||
        dev_alloc(b, &b->d_order, (size_t)b->nitems * sizeof(int), false, "schedule")) return -2;
    b->lpt = 1;
  }
  if (L.n_gs) {
    if (dev_alloc(b, &b->d_gscr, (size_t)b->B * L.n_gs * b->elem, true, "global scratch")) return -2;
    b->tb.opts.gscr = b->d_gscr;
  }
  if (create_fields(b)) return -2;
  // The stash of the position / velocity stage between legacy steps is opt-in (option "stash", or DMC_STASH=1):
  // measured on MI355X (cheetah, B = 4096) the 2 x 7.3 KB per env of stash traffic cost more than the partial
  // trailing pass it replaces (0.139 vs 0.134 ms per launch).
  if (getenv("DMC_STASH") && atoi(getenv("DMC_STASH")) && dmc_batch_set_opt_int(b, "stash", 1)) return -2;
  return dmc_batch_reset(b, nullptr, -1);
}
extern "C" int dmc_batch_create_caps(const dmc_model* m, int batch_size, int device_id, int precision,
                                     const int* caps, int ncaps, dmc_batch** out) {
  if (ncaps < 0 || (ncaps > 0 && !caps)) return fail("null argument");
  const int nconmax = ncaps > 0 ? caps[0] : 0, njmax = ncaps > 1 ? caps[1] : 0, lanes_per_env = ncaps > 2 ? caps[2] : 0;
  const int njcon = ncaps > 3 ? caps[3] : 0;
  const int jlevel = ncaps > 4 ? caps[4] - 1 : -1;      // caps[4]: StepDims::jglobal + 1, 0 = automatic
  if (!m || !out) return fail("null argument");
  *out = nullptr;
  if (batch_size < 1) return fail("batch_size must be >= 1");
  if (precision != 32 && precision != 64) return fail("precision must be 32 or 64");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail("no HIP device available: the batched step has no CPU fallback", -3);
  if (device_id < 0 || device_id >= ndev) return fail("invalid device id");
  HIP_TRY(hipSetDevice(device_id));
  dmc_batch* b = new dmc_batch();
  b->model = m; b->B = batch_size; b->device = device_id; b->precision = precision;
  b->elem = precision == 64 ? sizeof(double) : sizeof(float);
  const int rc = batch_init(b, nconmax, njmax, lanes_per_env, njcon, jlevel);
  if (rc) { dmc_batch_destroy(b); return rc; }      // (g_err is the failure's: destroying sets none)
  *out = b;
  return 0;
}

extern "C" void dmc_batch_destroy(dmc_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  if (b->prof) prof_free(b->prof);
  if (b->xfer) xfer_free(b->xfer);
  dev_free_all(b);
  delete b;
}

template <typename T>
static void fill_io(dmc_batch* b, StepIO<T>* io) {
  io->B = b->B;
#define X(name, count, flags) if constexpr (!((flags) & DMC_FIELD_OPTS)) io->name = (decltype(io->name))b->fields[F_##name].dev;
  DMC_DATA_REAL_FIELDS(X) DMC_DATA_INT_FIELDS(X)
#undef X
  io->prof = b->d_prof;
  io->work = b->geom.queue ? b->d_work : nullptr;
  io->cost = b->lpt ? b->d_cost : nullptr; io->order = b->lpt ? b->d_order : nullptr;
  io->prog = nullptr; io->slices = 0; io->hand = b->d_hand; io->hand_n = b->hand_n;      // (slices: launch_untimed, step launches of a queued batch only)
  io->nxcd = b->geom.queue ? b->nxcd : 1;
  io->task_args = (b->task_on && b->spec_launch) ? b->d_task_args : nullptr;
  io->trace = b->d_trace; io->trace_slot = b->d_trace ? b->trace_launch++ : 0;
  io->debug = (T*)b->d_debug; io->debug_i = b->d_debug_i; io->ndebug = b->ndebug;
  io->kstash = (T*)b->d_kstash; io->kstash_i = b->d_kstash_i;
  io->probe = (T*)b->d_probe; io->probe_geom = b->probe_geom; io->probe_cap = b->probe_cap;
  io->stash_r = b->stash_on ? (T*)b->d_stash_r : nullptr; io->stash_i = b->stash_on ? b->d_stash_i : nullptr; io->epoch = b->d_epoch;
}

// order[k] = the item handed out k-th: items by DESCENDING cost of the previous launch (1024 linear buckets of the
// largest cost; the order inside a bucket does not matter).  One workgroup; a few microseconds for 4096 items.
__global__ void __launch_bounds__(1024) order_kernel(const int* __restrict__ cost, int* __restrict__ order, int n) {
  __shared__ int hist[1024];
  __shared__ int mx;
  const int tid = threadIdx.x;
  hist[tid] = 0;
  if (tid == 0) mx = 0;
  __syncthreads();
  int m = 0;
  for (int i = tid; i < n; i += 1024) m = max(m, cost[i]);
  atomicMax(&mx, m);
  __syncthreads();
  const int top = mx;
  if (top <= 0) { for (int i = tid; i < n; i += 1024) order[i] = i; return; }      // first launch: nothing measured yet
  const float sc = 1023.0f / (float)top;
  for (int i = tid; i < n; i += 1024) atomicAdd(&hist[1023 - min(1023, (int)((float)cost[i] * sc))], 1);   // bucket 0 = costliest
  __syncthreads();
  if (tid == 0) { int acc = 0; for (int k = 0; k < 1024; k++) { const int c = hist[k]; hist[k] = acc; acc += c; } }
  __syncthreads();
  for (int i = tid; i < n; i += 1024) order[atomicAdd(&hist[1023 - min(1023, (int)((float)cost[i] * sc))], 1)] = i;
}

struct SeqArgs { const void* ctrl; void* qpos; void* qvel; void* sensor; int nsub; };
template <typename T>
static int launch_t(dmc_batch* b, int nstep, int legacy, LaunchMode mode, void* stream, const SeqArgs* sq) {
  StepOpts<double>& opts = b->tb.opts;
  if (opts.eg_n) opts.eg_data = b->fields[F_env_geom].dev;      // follows dmc_batch_bind
  opts.xfrc = b->xfrc_on ? b->fields[F_xfrc_applied].dev : nullptr; opts.xfrc_B = b->B;
  if (b->tb.L.d.nmocap) { opts.mocap_pos = b->fields[F_mocap_pos].dev; opts.mocap_quat = b->fields[F_mocap_quat].dev; opts.mocap_B = b->B; }      // follow dmc_batch_bind
  const int nsub = sq ? sq->nsub : 1;
  // pieces of a queued Physics.step(nstep) launch (never with the full stash, whose trailing stage belongs to the last step)
  // (models of more than 16 dofs: the kernels of the small ones are built without the hand-off code, step_core.h kSlices)
  const int slices = (b->geom.queue && b->d_prog && mode == MODE_STEP && !b->stash_on && b->tb.L.d.nv > 16) ? std::min(nstep, b->max_slices) : 1;
  // a specialisation plugin takes the launch unless it was built lean and the launch needs an optional feature
  const bool need_feat = legacy == 2 || b->d_probe != nullptr || b->tb.opts.integrator == DMC_INT_IMPLICITFAST;
  const bool spec = b->spec_launch && (b->spec_features || !need_feat);
  // ... but a kernel with a task epilogue (suite/fused_env.py) is the only one that runs the task layer: the library's own
  // kernel would step the physics and leave observation, reward, flags and step counters as they were, without a word
  if (b->task_on && mode == MODE_STEP && !spec)
    return fail("the task kernel was built without the optional launch features this launch needs (a substep probe, legacy_step 2 or the "
                "implicitfast integrator): it cannot take the launch, and no other kernel runs the task layer");
  // longest-first hand-out pays for whole items only: with pieces a launch ends within one piece of the last claim whatever
  // the order (round 6, one box: config 3 +1.4 % without the 16 us ordering kernel in front of every launch, config 4 -0.2 %)
  if (b->lpt && slices <= 1) hipLaunchKernelGGL(order_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const int*)b->d_cost, b->d_order, b->nitems);
  StepIO<T> io; fill_io(b, &io);
  if (slices > 1) { io.prog = b->d_prog; io.slices = slices; io.cost = nullptr; io.order = nullptr; }
  io.ctrl_seq = sq ? (const T*)sq->ctrl : nullptr; io.qpos_seq = sq ? (T*)sq->qpos : nullptr;
  io.qvel_seq = sq ? (T*)sq->qvel : nullptr; io.sensor_seq = sq ? (T*)sq->sensor : nullptr;
  constexpr bool f64 = sizeof(T) == sizeof(double);
  StepOpts<T> cast; const StepOpts<T>* o;      // (fp64: the batch's own options, as they are)
  if constexpr (f64) o = &opts; else { cast = step_opts_cast<T>(opts); o = &cast; }
  hipError_t e;
  if (spec) {
    typedef int (*fn_t)(const LaunchGeom*, void*, const StepLayout*, const StepOpts<T>*, const int*, const T*, const int*, const StepIO<T>*, int, int, int, int, int);
    e = (hipError_t)((fn_t)b->spec_launch)(&b->geom, stream, b->d_layout, o, b->d_mi, (const T*)b->d_mr, b->d_mc, &io, nstep, legacy, mode, b->outmask, nsub);
  } else if constexpr (f64) e = launch_step_f64(b->geom, (hipStream_t)stream, b->d_layout, *o, b->d_mi, (const T*)b->d_mr, b->d_mc, io, nstep, legacy, mode, b->outmask, nsub);
  else e = launch_step_f32(b->geom, (hipStream_t)stream, b->d_layout, *o, b->d_mi, (const T*)b->d_mr, b->d_mc, io, nstep, legacy, mode, b->outmask, nsub);
  if (e != hipSuccess) return fail(std::string("kernel launch: ") + hipGetErrorString(e), -2);
  return 0;
}
static int launch_untimed(dmc_batch* b, int nstep, int legacy, LaunchMode mode, void* stream, const SeqArgs* sq) {
  HIP_TRY(hipSetDevice(b->device));
  b->launched_mask = b->outmask;      // what the derived arrays in HBM hold from now on (dmc_camera_render checks it)
  return b->precision == 64 ? launch_t<double>(b, nstep, legacy, mode, stream, sq) : launch_t<float>(b, nstep, legacy, mode, stream, sq);
}
static int launch(dmc_batch* b, int nstep, int legacy, LaunchMode mode, void* stream, const SeqArgs* sq = nullptr) {
  HIP_TRY(hipSetDevice(b->device));
  TimerPair t;
  const bool timed = prof_begin(b, (hipStream_t)stream, &t);
  const int rc = launch_untimed(b, nstep, legacy, mode, stream, sq);
  // mjTIMER_STEP counts mj_step calls: a step / rollout launch runs nstep (x n_sub_steps) of them; mj_step1 / mj_step2
  // launches count as one step per pair (on the mj_step2 half); mj_forward launches go to mjTIMER_FORWARD
  const bool fwd = mode == MODE_FORWARD || mode == MODE_FORWARD_NOACT;
  if (timed) prof_end(b, (hipStream_t)stream, t, fwd ? 1 : 0,
                      mode == MODE_STEP ? nstep : mode == MODE_ROLLOUT ? nstep * (sq ? sq->nsub : 1) : mode == MODE_STEP1 ? 0 : 1);
  return rc;
}

static int bump_epoch(dmc_batch* b, hipStream_t stream, bool wait);
extern "C" int dmc_batch_attach_specialised(dmc_batch* b, const char* so_path) {
  if (!b || !so_path) return fail("null argument");
  void* h = dlopen(so_path, RTLD_NOW | RTLD_LOCAL);
  if (!h) return fail(std::string("cannot load ") + so_path + ": " + dlerror());
  typedef const StepLayout* (*layout_t)();
  typedef void (*info_t)(int*);
  layout_t fl = (layout_t)dlsym(h, "dmc_spec_layout");
  info_t fi = (info_t)dlsym(h, "dmc_spec_info");
  void* launch = dlsym(h, "dmc_spec_launch");
  if (!fl || !fi || !launch) { dlclose(h); return fail("not a specialisation plugin (dmc_spec_* symbols missing)"); }
  int info[8]; fi(info);
  if (info[4] != b->precision) { dlclose(h); return fail("the plugin was built for another precision"); }
  const int so = b->precision == 64 ? (int)sizeof(StepOpts<double>) : (int)sizeof(StepOpts<float>);
  const int sio = b->precision == 64 ? (int)sizeof(StepIO<double>) : (int)sizeof(StepIO<float>);
  if (info[0] != (int)sizeof(StepLayout) || info[1] != so || info[2] != sio || info[3] != DMC_MODEL_VERSION || info[7] != (int)sizeof(LaunchGeom)) {
    dlclose(h); return fail("the plugin was built from other sources than this library (struct sizes / model version differ)");
  }
  if (info[5] != b->geom.lpe) { dlclose(h); return fail("the plugin was built for another lanes-per-environment shape"); }
  if (memcmp(fl(), &b->tb.L, sizeof(StepLayout)) != 0) { dlclose(h); return fail("the plugin's layout is not this batch's (another model or other caps)"); }
  if (b->spec_so) dlclose(b->spec_so);
  b->spec_so = h; b->spec_launch = launch; b->spec_features = info[6];
  typedef int (*tb_t)();
  tb_t tb = (tb_t)dlsym(h, "dmc_spec_task_args_bytes");
  b->spec_task_bytes = tb ? tb() : 0;
  tb_t fc = (tb_t)dlsym(h, "dmc_spec_coop_open");
  b->spec_coop = fc ? fc() : 0;
  b->task_on = 0;
  // the record of the kinematic stash is the kernel's choice (StepCore::krec: packed in a -DDMC_NO_WIDE_IO build): what
  // the kernel that ran so far left behind is not for the one that runs from here on
  return bump_epoch(b, 0, true);
}

extern "C" int dmc_batch_set_task_args(dmc_batch* b, const void* args, int nbytes) {
  if (!b || !args) return fail("null argument");
  if (!b->spec_task_bytes) return fail("the batch's kernel carries no task epilogue (attach a plugin built with a task header)");
  if (nbytes != b->spec_task_bytes) return fail("task argument block: size differs from the one the kernel was generated with");
  HIP_TRY(hipSetDevice(b->device));
  if (!b->d_task_args && dev_alloc(b, &b->d_task_args, (size_t)nbytes, false, "task arguments")) return -2;
  HIP_TRY(hipMemcpy(b->d_task_args, args, (size_t)nbytes, hipMemcpyHostToDevice));
  return 0;
}
extern "C" int dmc_batch_enable_task(dmc_batch* b, int on) {
  if (!b) return fail("null batch");
  if (on && (!b->spec_task_bytes || !b->d_task_args)) return fail("no task epilogue to enable (dmc_batch_set_task_args first)");
  b->task_on = on ? 1 : 0;
  return 0;
}

extern "C" int dmc_batch_step(dmc_batch* b, int nstep, int legacy_step, void* hip_stream) {
  if (!b) return fail("null batch");
  if (nstep < 1) return fail("nstep must be >= 1");
  if (legacy_step == 2 && b->tb.opts.integrator == DMC_INT_RK4) return fail("legacy_step 2 (step + mj_forward) is not implemented for RK4 models");
  return launch(b, nstep, legacy_step == 2 ? 2 : (legacy_step ? 1 : 0), MODE_STEP, hip_stream);
}
extern "C" int dmc_batch_set_step_probe(dmc_batch* b, int geom_id, void* out_dev, int capacity) {
  if (!b) return fail("null batch");
  if (!out_dev || capacity < 1) { b->d_probe = nullptr; b->probe_cap = 0; return 0; }
  if (geom_id < 0 || geom_id >= b->tb.L.d.ngeom) return fail("geom id out of range");
  b->d_probe = out_dev; b->probe_geom = geom_id; b->probe_cap = capacity;
  return 0;
}
// The stash epoch (StepIO::epoch) is a device int: every edit that can change what the stashed stages depend on bumps
// it with a one-thread kernel.  Host-synchronous entry points bump on the null stream and wait; dmc_batch_invalidate_async
// bumps on the caller's stream, which makes the invalidation capturable into a HIP graph together with the edit.
__global__ void epoch_bump_kernel(int* epoch) { *epoch = (*epoch == 0x7ffffff0) ? 1 : *epoch + 1; }
static int bump_epoch(dmc_batch* b, hipStream_t stream, bool wait) {
  HIP_TRY(hipSetDevice(b->device));
  hipLaunchKernelGGL(epoch_bump_kernel, dim3(1), dim3(1), 0, stream, b->d_epoch);
  HIP_TRY(hipGetLastError());
  if (wait) HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

// mj_step1 / mj_step2 as separate launches: the stage mj_step1 computes travels to mj_step2 through the per-env
// stash in HBM (allocated on first use)
static int ensure_stash(dmc_batch* b) {
  if (b->stash_on) return 0;
  if (dmc_batch_set_opt_int(b, "stash", 1)) return -2;
  b->stash_auto = 1;      // switched on by a step1 / step2 call, not by the caller's option: the step2 that consumes it switches it off again
  return 0;
}
extern "C" int dmc_batch_step1(dmc_batch* b, void* hip_stream) {
  if (!b) return fail("null batch");
  if (ensure_stash(b)) return -2;
  return launch(b, 1, 0, MODE_STEP1, hip_stream);
}
extern "C" int dmc_batch_step2(dmc_batch* b, void* hip_stream) {
  if (!b) return fail("null batch");
  if (b->tb.opts.integrator == DMC_INT_RK4) return fail("mj_step2 integrates with Euler only; RK4 models step through dmc_batch_step");
  if (ensure_stash(b)) return -2;
  const int rc = launch(b, 1, 0, MODE_STEP2, hip_stream);
  // a stash this pair switched on is not left on for every later launch (2 x n_keep reals per env of traffic each)
  if (b->stash_auto) { b->stash_on = 0; b->stash_auto = 0; }
  return rc;
}
extern "C" int dmc_batch_forward(dmc_batch* b, int disable_actuation, void* hip_stream) {
  if (!b) return fail("null batch");
  return launch(b, 0, 0, disable_actuation ? MODE_FORWARD_NOACT : MODE_FORWARD, hip_stream);
}
extern "C" int dmc_batch_rollout(dmc_batch* b, int nsteps, int n_sub_steps, const void* ctrl_seq, void* qpos_seq,
                                 void* qvel_seq, void* sensordata_seq, void* hip_stream) {
  if (!b) return fail("null batch");
  if (nsteps < 1 || n_sub_steps < 1) return fail("nsteps and n_sub_steps must be >= 1");
  SeqArgs sq = {ctrl_seq, qpos_seq, qvel_seq, sensordata_seq, n_sub_steps};
  return launch(b, nsteps, 1, MODE_ROLLOUT, hip_stream, &sq);
}
// ---- observation gather table (composer/observation/updater.py:285-295, observable/mjcf.py:43) ---------------
// An MJCFFeature observable is a named slice of an mjData field; a task's enabled observables resolve once into a
// table of (field, row, corruptor) triples, and every control step ONE launch gathers them out of the SoA field
// arrays into the (B, nobs) env-major observation matrix a policy consumes.  Reads are coalesced along the env
// index (SoA rows), writes along the observation index (a 64 x 64 tile transposed through LDS).
enum { GOP_NONE = 0, GOP_GREATER = 1, GOP_TANH2 = 2, GOP_LOG1P = 3, GOP_ASINH = 4 };
struct GatherRow { int field, row, op; float prm; };
struct GatherPtrs { const void* p[16]; };
struct dmc_gather {
  dmc_batch* batch;
  int nrows;
  std::vector<Field*> fields;   // distinct fields, slot order
  GatherRow* d_rows;
};
template <typename T>
__global__ void __launch_bounds__(256) gather_kernel(GatherPtrs ptrs, const GatherRow* __restrict__ rows, int nrows, int B, T* __restrict__ out) {
  __shared__ T tile[64][65];
  const int tx = threadIdx.x, ty = threadIdx.y;      // (64, 4)
  const int env0 = blockIdx.x * 64;
  // one 64 x 64 tile per workgroup: blockIdx.y walks the observation rows (a small batch -- soccer, B = 256: four
  // workgroups -- used to walk all its row tiles inside each of them: 61 us per control step)
  for (int k0 = blockIdx.y * 64; k0 < nrows; k0 += 64 * gridDim.y) {
    for (int kk = ty; kk < 64; kk += 4) {
      const int k = k0 + kk, env = env0 + tx;
      T v = 0;
      if (k < nrows && env < B) {
        const GatherRow r = rows[k];
        v = ((const T*)ptrs.p[r.field])[(size_t)r.row * B + env];
        if (r.op == GOP_GREATER) v = v > (T)r.prm ? (T)1 : (T)0;
        else if (r.op == GOP_TANH2) v = (T)tanh((double)(2 * v / (T)r.prm));
        else if (r.op == GOP_LOG1P) v = (T)log1p((double)v);
        else if (r.op == GOP_ASINH) v = (T)asinh((double)v);
      }
      tile[kk][tx] = v;
    }
    __syncthreads();
    for (int ee = ty; ee < 64; ee += 4) {
      const int env = env0 + ee, k = k0 + tx;
      if (env < B && k < nrows) out[(size_t)env * nrows + k] = tile[tx][ee];
    }
    __syncthreads();
  }
}
extern "C" int dmc_gather_create(dmc_batch* b, int nrows, const char* const* field_names, const int* rows, const int* ops,
                                 const double* params, dmc_gather** out) {
  if (!b || !out || nrows < 1 || !field_names || !rows) return fail("null argument");
  dmc_gather* g = new dmc_gather();
  g->batch = b; g->nrows = nrows; g->d_rows = nullptr;
  std::vector<GatherRow> h(nrows);
  for (int k = 0; k < nrows; k++) {
    Field* f = field_names[k] ? find_field(b, field_names[k]) : nullptr;
    if (!f) { delete g; return fail(std::string("unknown field: ") + (field_names[k] ? field_names[k] : "(null)")); }
    if (f->is_int || (f->flags & DMC_FIELD_F64)) { delete g; return fail(std::string("field cannot be gathered (not in batch precision): ") + f->name); }
    if (rows[k] < 0 || rows[k] >= f->rows) { delete g; return fail(std::string("row out of range for field ") + f->name); }
    int slot = -1;
    for (size_t q = 0; q < g->fields.size(); q++) if (g->fields[q] == f) slot = (int)q;
    if (slot < 0) { slot = (int)g->fields.size(); g->fields.push_back(f); }
    if (slot >= 16) { delete g; return fail("at most 16 distinct fields per gather table"); }
    const int op = ops ? ops[k] : GOP_NONE;
    if (op < GOP_NONE || op > GOP_ASINH) { delete g; return fail("unknown gather op"); }
    h[k].field = slot; h[k].row = rows[k]; h[k].op = op; h[k].prm = params ? (float)params[k] : 0.f;
  }
  hipError_t e = hipSetDevice(b->device);
  if (e == hipSuccess) e = hipMalloc((void**)&g->d_rows, sizeof(GatherRow) * nrows);
  if (e == hipSuccess) e = hipMemcpy(g->d_rows, h.data(), sizeof(GatherRow) * nrows, hipMemcpyHostToDevice);
  if (e != hipSuccess) { if (g->d_rows) (void)hipFree(g->d_rows); delete g; return fail(hipGetErrorString(e), -2); }
  *out = g;
  return 0;
}
extern "C" void dmc_gather_destroy(dmc_gather* g) {
  if (!g) return;
  if (g->d_rows) (void)hipFree(g->d_rows);
  delete g;
}
extern "C" int dmc_gather_run(dmc_gather* g, void* out, void* hip_stream) {
  if (!g || !out) return fail("null argument");
  dmc_batch* b = g->batch;
  GatherPtrs ptrs;
  for (int q = 0; q < 16; q++) ptrs.p[q] = nullptr;
  for (size_t q = 0; q < g->fields.size(); q++) ptrs.p[q] = g->fields[q]->dev;   // honours rebinding
  HIP_TRY(hipSetDevice(b->device));
  // (row tiles across blockIdx.y while the batch alone does not fill the chip: at least ~2 workgroups per CU in flight)
  const int gx = (b->B + 63) / 64, ktiles = (g->nrows + 63) / 64;
  const int gy = std::max(1, std::min(ktiles, (2 * b->ncu + gx - 1) / gx));
  const dim3 grid(gx, gy), block(64, 4);
  if (b->precision == 64) hipLaunchKernelGGL(gather_kernel<double>, grid, block, 0, (hipStream_t)hip_stream, ptrs, g->d_rows, g->nrows, b->B, (double*)out);
  else hipLaunchKernelGGL(gather_kernel<float>, grid, block, 0, (hipStream_t)hip_stream, ptrs, g->d_rows, g->nrows, b->B, (float*)out);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int dmc_batch_sync(dmc_batch* b) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

// ---- host <-> device field transfer (env-major host, SoA device) ------------------
// ---- asynchronous host transfers -------------------------------------------------------------------------------
// The host side of the boundary is env-major ((B, rows): what numpy callers hold), the device fields are SoA
// ((rows, B)).  dmc_batch_set / dmc_batch_get transpose and convert element by element on one host thread around
// synchronous pageable copies.  Here: the host only converts contiguously into PINNED staging (or not at all: fp32 on
// the wire for fp32 batches), copies are hipMemcpyAsync on the caller's stream, the transposition is a device kernel
// (LDS tile, coalesced on both sides), and a get of several fields is ONE device-to-host copy and one wait.
// out[c * ldo + r] = in[r * ldi + c] for r < nr, c < nc  (32 x 32 tiles through LDS).  `in` / `out` may be PINNED HOST
// memory (device-mapped): the set kernel reads the caller's staged (B, rows) array over PCIe and the get kernel writes
// the (B, rows) arrays straight into the host staging -- no separate hipMemcpyAsync on either side.
template <typename T>
__device__ inline void transpose_tile(const T* __restrict__ in, T* __restrict__ out, int nr, int nc, int ldi, int ldo, int bx, int by, T (*tile)[33]) {
  const int c0 = bx * 32, r0 = by * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) { const int r = r0 + k, c = c0 + tx; if (r < nr && c < nc) tile[k][tx] = in[(size_t)r * ldi + c]; }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) { const int c = c0 + k, r = r0 + tx; if (r < nr && c < nc) out[(size_t)c * ldo + r] = tile[tx][k]; }
}
template <typename T>
__global__ void __launch_bounds__(256) transpose_kernel(const T* __restrict__ in, T* __restrict__ out, int nr, int nc, int ldi, int ldo) {
  __shared__ T tile[32][33];
  transpose_tile<T>(in, out, nr, nc, ldi, ldo, blockIdx.x, blockIdx.y, tile);
}
template <typename T>
static void launch_transpose(const void* in, void* out, int nr, int nc, int ldi, int ldo, hipStream_t s) {
  hipLaunchKernelGGL(transpose_kernel<T>, dim3((nc + 31) / 32, (nr + 31) / 32), dim3(256), 0, s, (const T*)in, (T*)out, nr, nc, ldi, ldo);
}
// every field of a get in ONE launch: blockIdx.z = field
struct GetTable { const void* src[8]; void* dst[8]; int rows[8]; int wide[8]; int n; };
__global__ void __launch_bounds__(256) get_pack_kernel(GetTable t, int B) {
  __shared__ double tile64[32][33];
  const int f = blockIdx.z;
  if ((int)blockIdx.y * 32 >= t.rows[f]) return;
  if (t.wide[f]) transpose_tile<double>((const double*)t.src[f], (double*)t.dst[f], t.rows[f], B, B, t.rows[f], blockIdx.x, blockIdx.y, tile64);
  else transpose_tile<float>((const float*)t.src[f], (float*)t.dst[f], t.rows[f], B, B, t.rows[f], blockIdx.x, blockIdx.y, (float (*)[33])tile64);
}
static bool get_in_flight(const dmc_batch* b) { return b->xfer && b->xfer->out_in_flight; }
static size_t field_elem(const dmc_batch* b, const Field* f) { return f->is_int ? sizeof(int32_t) : (b->precision == 64 || (f->flags & DMC_FIELD_F64)) ? sizeof(double) : sizeof(float); }
extern "C" int dmc_batch_set_async(dmc_batch* b, const char* name, const void* src, int host_bits, void* hip_stream) {
  if (!b || !name || !src) return fail("null argument");
  if (host_bits != 64 && host_bits != 32) return fail("host_bits must be 64 or 32");
  Field* f = find_field(b, name);
  if (!f || f->is_int) return fail(std::string("unknown real field: ") + name);
  const size_t n = (size_t)f->rows * b->B;
  if (!n) return 0;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(hipSetDevice(b->device));
  if (!b->xfer) b->xfer = new Xfer();
  Xfer* x = b->xfer;
  const int k = x->next; x->next = (k + 1) % Xfer::kSlots;
  const size_t es = field_elem(b, f), bytes = n * es;
  if (x->cap_in[k] < bytes) {
    if (x->ev_in[k]) HIP_TRY(hipEventSynchronize(x->ev_in[k]));
    if (x->h_in[k]) (void)hipHostFree(x->h_in[k]);
    if (x->d_in[k]) (void)hipFree(x->d_in[k]);
    x->h_in[k] = nullptr; x->d_in[k] = nullptr; x->cap_in[k] = 0;
    HIP_TRY(hipHostMalloc(&x->h_in[k], bytes, hipHostMallocMapped));
    x->cap_in[k] = bytes;
    if (!x->ev_in[k]) HIP_TRY(hipEventCreateWithFlags(&x->ev_in[k], hipEventDisableTiming));
  } else HIP_TRY(hipEventSynchronize(x->ev_in[k]));      // the copy that last used this slot (four sets ago) has left the staging
  // host: contiguous conversion into the pinned slot (no transposition); the caller's array is free again on return
  if (es == 8) { double* d = (double*)x->h_in[k]; if (host_bits == 64) std::memcpy(d, src, bytes); else { const float* p = (const float*)src; for (size_t i = 0; i < n; i++) d[i] = p[i]; } }
  else { float* d = (float*)x->h_in[k]; if (host_bits == 32) std::memcpy(d, src, bytes); else { const double* p = (const double*)src; for (size_t i = 0; i < n; i++) d[i] = (float)p[i]; } }
  void* hin = nullptr;
  HIP_TRY(hipHostGetDevicePointer(&hin, x->h_in[k], 0));
  if (es == 8) launch_transpose<double>(hin, f->dev, b->B, f->rows, f->rows, b->B, st); else launch_transpose<float>(hin, f->dev, b->B, f->rows, f->rows, b->B, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(x->ev_in[k], st));
  if (f == &b->fields[F_xfrc_applied]) b->xfrc_on = 1;
  if (!(f->flags & DMC_FIELD_ACC_IN)) return bump_epoch(b, st, false);      // stream-ordered with the edit
  return 0;
}
extern "C" int dmc_batch_get_async(dmc_batch* b, int n, const char* const* names, void* hip_stream) {
  if (!b || n < 1 || !names) return fail("null argument");
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(hipSetDevice(b->device));
  if (!b->xfer) b->xfer = new Xfer();
  Xfer* x = b->xfer;
  if (x->out_in_flight) return fail("a get is already enqueued: call dmc_batch_get_wait first");
  x->pending.clear();
  size_t bytes = 0;
  for (int i = 0; i < n; i++) {
    Field* f = find_field(b, names[i]);
    if (!f) return fail(std::string("unknown field: ") + (names[i] ? names[i] : "(null)"));      // (int32 fields travel as they are)
    bytes = (bytes + 7) / 8 * 8;
    x->pending.push_back({f, bytes});
    bytes += (size_t)f->rows * b->B * field_elem(b, f);
  }
  if (n > 8) return fail("at most 8 fields per get");
  if (x->cap_out < bytes) {
    if (x->h_out) (void)hipHostFree(x->h_out);
    x->h_out = nullptr; x->cap_out = 0;
    HIP_TRY(hipHostMalloc(&x->h_out, bytes, hipHostMallocMapped));
    x->cap_out = bytes;
  }
  if (!x->ev_out) HIP_TRY(hipEventCreateWithFlags(&x->ev_out, hipEventDisableTiming));
  void* hout = nullptr;
  if (bytes) HIP_TRY(hipHostGetDevicePointer(&hout, x->h_out, 0));
  GetTable t; t.n = n;
  int maxrows = 0;
  for (int i = 0; i < 8; i++) { t.src[i] = nullptr; t.dst[i] = nullptr; t.rows[i] = 0; t.wide[i] = 0; }
  for (int i = 0; i < n; i++) {
    Field* f = x->pending[i].first;
    t.src[i] = f->dev; t.dst[i] = (char*)hout + x->pending[i].second; t.rows[i] = f->rows; t.wide[i] = field_elem(b, f) == 8;
    maxrows = std::max(maxrows, f->rows);
  }
  if (maxrows) hipLaunchKernelGGL(get_pack_kernel, dim3((b->B + 31) / 32, (maxrows + 31) / 32, n), dim3(256), 0, st, t, b->B);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(x->ev_out, st));
  x->out_in_flight = true;
  return 0;
}
extern "C" int dmc_batch_get_wait(dmc_batch* b, int n, void* const* dsts, int host_bits) {
  if (!b || !dsts) return fail("null argument");
  if (host_bits != 64 && host_bits != 32) return fail("host_bits must be 64 or 32");
  Xfer* x = b->xfer;
  if (!x || !x->out_in_flight) return fail("no get is enqueued");
  if ((size_t)n != x->pending.size()) return fail("dmc_batch_get_wait: the number of destinations differs from the enqueued get");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipEventSynchronize(x->ev_out));
  x->out_in_flight = false;
  for (int i = 0; i < n; i++) {
    Field* f = x->pending[i].first;
    const size_t cnt = (size_t)f->rows * b->B, es = field_elem(b, f);
    if (!cnt || !dsts[i]) continue;
    const void* srcp = (const char*)x->h_out + x->pending[i].second;
    if (f->is_int) { std::memcpy(dsts[i], srcp, cnt * 4); continue; }      // int32 whatever host_bits says
    if (es == 8) { const double* p = (const double*)srcp; if (host_bits == 64) std::memcpy(dsts[i], p, cnt * 8); else { float* d = (float*)dsts[i]; for (size_t k = 0; k < cnt; k++) d[k] = (float)p[k]; } }
    else { const float* p = (const float*)srcp; if (host_bits == 32) std::memcpy(dsts[i], p, cnt * 4); else { double* d = (double*)dsts[i]; for (size_t k = 0; k < cnt; k++) d[k] = p[k]; } }
  }
  return 0;
}
extern "C" const void* dmc_batch_get_staged(dmc_batch* b, int i) {
  if (!b || !b->xfer || b->xfer->out_in_flight || i < 0 || (size_t)i >= b->xfer->pending.size()) { fail("no completed get holds that field"); return nullptr; }
  return (const char*)b->xfer->h_out + b->xfer->pending[i].second;
}
// (B, rows) doubles from the (rows, B) device array of T
template <typename T>
static int get_transposed(const dmc_batch* b, const Field* f, double* dst) {
  std::vector<T> tmp((size_t)f->rows * b->B);
  HIP_TRY(hipMemcpy(tmp.data(), f->dev, tmp.size() * sizeof(T), hipMemcpyDeviceToHost));
  for (int k = 0; k < f->rows; k++) for (int e = 0; e < b->B; e++) dst[(size_t)e * f->rows + k] = tmp[(size_t)k * b->B + e];
  return 0;
}
static int get_real(dmc_batch* b, Field* f, double* dst) {
  const size_t n = (size_t)f->rows * b->B;
  if (!n) return 0;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipDeviceSynchronize());
  if (!get_in_flight(b)) {      // the pinned / device-transposed path, completed before returning
    if (dmc_batch_get_async(b, 1, &f->name, nullptr)) return -2;
    void* d = dst;
    return dmc_batch_get_wait(b, 1, &d, 64);
  }
  return field_elem(b, f) == 8 ? get_transposed<double>(b, f, dst) : get_transposed<float>(b, f, dst);
}
static int set_real(dmc_batch* b, Field* f, const double* src) {
  const size_t n = (size_t)f->rows * b->B;
  if (!n) return 0;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipDeviceSynchronize());
  // (inputs of the acceleration stage only, DMC_FIELD_ACC_IN, leave the stash epoch alone; every other field bumps it)
  // the synchronous form of dmc_batch_set_async: pinned staging, device-side transposition, done before returning
  if (dmc_batch_set_async(b, f->name, src, 64, nullptr)) return -2;
  HIP_TRY(hipStreamSynchronize(nullptr));
  return 0;
}
extern "C" int dmc_batch_field_rows(const dmc_batch* b, const char* name, int* rows, int* is_int) {
  if (!b || !name) return fail("null argument");
  Field* f = find_field(const_cast<dmc_batch*>(b), name);
  if (!f) return fail(std::string("unknown field: ") + name);
  if (rows) *rows = f->rows;
  if (is_int) *is_int = f->is_int;
  return 0;
}
extern "C" int dmc_batch_get(dmc_batch* b, const char* name, double* dst) {
  if (!b || !name || !dst) return fail("null argument");
  Field* f = find_field(b, name);
  if (!f || f->is_int) return fail(std::string("unknown real field: ") + name);
  return get_real(b, f, dst);
}
extern "C" int dmc_batch_set(dmc_batch* b, const char* name, const double* src) {
  if (!b || !name || !src) return fail("null argument");
  Field* f = find_field(b, name);
  if (!f || f->is_int) return fail(std::string("unknown real field: ") + name);
  return set_real(b, f, src);
}
static int get_int(dmc_batch* b, const Field* f, int32_t* dst) {
  const size_t n = (size_t)f->rows * b->B;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<int32_t> tmp(n);
  HIP_TRY(hipMemcpy(tmp.data(), f->dev, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int k = 0; k < f->rows; k++) for (int e = 0; e < b->B; e++) dst[(size_t)e * f->rows + k] = tmp[(size_t)k * b->B + e];
  return 0;
}
static int set_int(dmc_batch* b, Field* f, const int32_t* src) {
  const size_t n = (size_t)f->rows * b->B;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<int32_t> tmp(n);
  for (int k = 0; k < f->rows; k++) for (int e = 0; e < b->B; e++) tmp[(size_t)k * b->B + e] = src[(size_t)e * f->rows + k];
  HIP_TRY(hipMemcpy(f->dev, tmp.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
  return 0;
}
extern "C" int dmc_batch_get_int(dmc_batch* b, const char* name, int32_t* dst) {
  if (!b || !name || !dst) return fail("null argument");
  Field* f = find_field(b, name);
  if (!f || !f->is_int) return fail(std::string("unknown int field: ") + name);
  return get_int(b, f, dst);
}
extern "C" int dmc_batch_set_int(dmc_batch* b, const char* name, const int32_t* src) {
  if (!b || !name || !src) return fail("null argument");
  Field* f = find_field(b, name);
  if (!f || !f->is_int) return fail(std::string("unknown int field: ") + name);
  return set_int(b, f, src);
}
extern "C" void* dmc_batch_device_ptr(dmc_batch* b, const char* name) {
  if (!b || !name) { fail("null argument"); return nullptr; }
  Field* f = find_field(b, name);
  if (!f) { fail(std::string("unknown field: ") + name); return nullptr; }
  if (f == &b->fields[F_xfrc_applied]) b->xfrc_on = 1;
  return f->dev;
}
extern "C" int dmc_batch_bind(dmc_batch* b, const char* name, void* device_ptr) {
  if (!b || !name) return fail("null argument");
  Field* f = find_field(b, name);
  if (!f) return fail(std::string("unknown field: ") + name);
  f->dev = device_ptr ? device_ptr : f->owned;
  const bool xfrc = f == &b->fields[F_xfrc_applied];
  if (xfrc) b->xfrc_on = 1;
  // (the one exception to DMC_FIELD_ACC_IN: binding xfrc_applied bumps the epoch, writing it does not)
  if (!(f->flags & DMC_FIELD_ACC_IN) || xfrc) { if (bump_epoch(b, 0, true)) return -2; }
  return 0;
}
extern "C" int dmc_batch_invalidate(dmc_batch* b) {
  if (!b) return fail("null batch");
  return bump_epoch(b, 0, true);
}
extern "C" int dmc_batch_invalidate_async(dmc_batch* b, void* hip_stream) {
  if (!b) return fail("null batch");
  return bump_epoch(b, (hipStream_t)hip_stream, false);
}
extern "C" int dmc_batch_set_output_mask(dmc_batch* b, int mask) {
  if (!b) return fail("null batch");
  if (bump_epoch(b, 0, true)) return -2;
  b->outmask = mask;
  return 0;
}
// ---- per-environment model deltas: world-fixed geoms with per-env pose / size ---------------------------------
// The reference randomises scenery per episode by editing the MJCF and recompiling (soccer RandomizedPitch,
// locomotion/soccer/pitch.py:612-690 through composer's initialize_episode_mjcf); a batch shares one compiled model,
// so the geoms that differ between environments get their pose and size from a per-env array instead of the tables.
static double geom_rbound_of(int type, const double* size) {
  switch (type) {
    case DMC_GEOM_SPHERE: return size[0];
    case DMC_GEOM_CAPSULE: return size[0] + size[1];
    case DMC_GEOM_CYLINDER: return sqrt(size[0]*size[0] + size[1]*size[1]);
    case DMC_GEOM_ELLIPSOID: return std::max(size[0], std::max(size[1], size[2]));
    case DMC_GEOM_BOX: return sqrt(size[0]*size[0] + size[1]*size[1] + size[2]*size[2]);
    default: return 0;
  }
}
extern "C" int dmc_batch_set_env_geoms(dmc_batch* b, int n, const int* geom_ids) {
  if (!b || n < 1 || !geom_ids) return fail("null argument");
  Field& f = b->fields[F_env_geom];
  if (f.name) return fail("per-environment geoms were already declared for this batch");
  const HostModel& m = b->model->hm;
  std::vector<int> slot(m.ngeom, -1);
  for (int k = 0; k < n; k++) {
    const int g = geom_ids[k];
    if (g < 0 || g >= m.ngeom) return fail("geom id out of range");
    // world-fixed: on the worldbody, or on a jointless child of it whose frame is the world frame (PyMJCF attaches a
    // static entity -- a goal -- as such a body; the per-environment row holds the geom's WORLD pose either way)
    const int gb = m.geom_bodyid[g];
    bool fixed = gb == 0;
    if (!fixed && m.body_weldid[gb] == 0 && m.body_parentid[gb] == 0) {
      const double* bp = &m.body_pos[3*gb]; const double* bq = &m.body_quat[4*gb];
      fixed = bp[0] == 0 && bp[1] == 0 && bp[2] == 0 && bq[0] == 1 && bq[1] == 0 && bq[2] == 0 && bq[3] == 0;
    }
    if (!fixed) return fail("only world-fixed geoms (on the worldbody or on a jointless body at the world frame) can differ between environments");
    if (slot[g] >= 0) return fail("geom listed twice");
    slot[g] = k;
  }
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipDeviceSynchronize());
  // (the field is declared last: a failed allocation leaves the batch as it was)
  if (dev_alloc(b, &f.owned, (size_t)16 * n * b->B * b->elem, false, "per-environment geoms")) return -2;
  if (dev_alloc(b, &b->d_eg_slot, sizeof(int) * m.ngeom, false, "per-environment geoms", slot.data())) { dev_free(b, &f.owned); return -2; }
  f.name = "env_geom"; f.rows = 16*n; f.dev = f.owned;
  // initial values: the model's own
  std::vector<double> host((size_t)b->B * f.rows);
  for (int k = 0; k < n; k++) {
    const int g = geom_ids[k];
    const double* q = &m.geom_quat[4*g];
    double mat[9];
    { const double w = q[0], x = q[1], y = q[2], z = q[3];
      mat[0] = w*w + x*x - y*y - z*z; mat[4] = w*w - x*x + y*y - z*z; mat[8] = w*w - x*x - y*y + z*z;
      mat[1] = 2*(x*y - w*z); mat[2] = 2*(x*z + w*y); mat[3] = 2*(x*y + w*z); mat[5] = 2*(y*z - w*x); mat[6] = 2*(x*z - w*y); mat[7] = 2*(y*z + w*x); }
    double row[16];
    for (int j = 0; j < 3; j++) row[j] = m.geom_pos[3*g + j];
    for (int j = 0; j < 9; j++) row[3 + j] = mat[j];
    for (int j = 0; j < 3; j++) row[12 + j] = m.geom_size[3*g + j];
    row[15] = m.geom_rbound[g];
    for (int e = 0; e < b->B; e++) for (int j = 0; j < 16; j++) host[(size_t)e * f.rows + 16*k + j] = row[j];
  }
  b->tb.opts.eg_slot = b->d_eg_slot; b->tb.opts.eg_n = n; b->tb.opts.eg_B = b->B;
  if (bump_epoch(b, 0, true)) return -2;
  return set_real(b, &f, host.data());
}
// rows of one geom slot from (pos, quat, size): what a caller writes into "env_geom" (host helper, no device work)
extern "C" int dmc_env_geom_pack(int geom_type, const double* pos, const double* quat, const double* size, double* out16) {
  if (!pos || !quat || !size || !out16) return fail("null argument");
  const double n = sqrt(quat[0]*quat[0] + quat[1]*quat[1] + quat[2]*quat[2] + quat[3]*quat[3]);
  if (!(n > 0)) return fail("zero quaternion");
  const double w = quat[0]/n, x = quat[1]/n, y = quat[2]/n, z = quat[3]/n;
  for (int j = 0; j < 3; j++) out16[j] = pos[j];
  double* mat = out16 + 3;
  mat[0] = w*w + x*x - y*y - z*z; mat[4] = w*w - x*x + y*y - z*z; mat[8] = w*w - x*x - y*y + z*z;
  mat[1] = 2*(x*y - w*z); mat[2] = 2*(x*z + w*y); mat[3] = 2*(x*y + w*z); mat[5] = 2*(y*z - w*x); mat[6] = 2*(x*z - w*y); mat[7] = 2*(y*z + w*x);
  for (int j = 0; j < 3; j++) out16[12 + j] = size[j];
  out16[15] = geom_rbound_of(geom_type, size);
  return 0;
}
extern "C" int dmc_batch_set_opt_int(dmc_batch* b, const char* name, int value) {
  if (!b || !name) return fail("null argument");
  StepOpts<double>& o = b->tb.opts;
  if (bump_epoch(b, 0, true)) return -2;
  if (!strcmp(name, "stash")) {
    if (value && !b->d_stash_r) {
      const StepLayout& L = b->tb.L;
      HIP_TRY(hipSetDevice(b->device));
      const size_t nr = (size_t)std::max(1, L.n_keep) * b->B * b->elem, ni = (size_t)(L.n_si + 4) * b->B * sizeof(int);
      if (dev_alloc(b, &b->d_stash_i, ni, true, "stash") || dev_alloc(b, &b->d_stash_r, nr, false, "stash")) return -2;
    }
    b->stash_on = value ? 1 : 0;
    return 0;
  }
  if (!strcmp(name, "disableflags")) {
    if (b->tb.has_unsupported_pairs && !(value & (DMC_DSBL_CONTACT | DMC_DSBL_CONSTRAINT)))
      return fail("cannot enable contacts: the model has geom pair types the collision kernel does not implement");
    o.disableflags = value;
  }
  else if (!strcmp(name, "islands")) o.islands = value < 0 ? -1 : (value ? 1 : 0);      // per-island solves: 1 / 0 / -1 = by precision
  else if (!strcmp(name, "iterations")) o.iterations = value;
  else if (!strcmp(name, "ls_iterations")) o.ls_iterations = value;
  else if (!strcmp(name, "noslip_iterations")) {
    if (value > 0 && !b->tb.L.d.nslip) return fail("noslip needs scratch the batch was created without: compile the model with noslip_iterations > 0");
    o.noslip_iterations = value;
  }
  else return fail(std::string("unknown int option: ") + name);
  return 0;
}
extern "C" int dmc_batch_set_opt_real(dmc_batch* b, const char* name, double value) {
  if (!b || !name) return fail("null argument");
  StepOpts<double>& o = b->tb.opts;
  if (bump_epoch(b, 0, true)) return -2;
  if (!strcmp(name, "timestep")) { o.timestep = value; o.timestep_d = value; }   // timestep_d: what data.time advances by
  else if (!strcmp(name, "tolerance")) o.tolerance = value;
  else if (!strcmp(name, "ls_tolerance")) o.ls_tolerance = value;
  else if (!strcmp(name, "noslip_tolerance")) o.noslip_tolerance = value;
  else if (!strcmp(name, "gravity_x")) o.gravity[0] = value;
  else if (!strcmp(name, "gravity_y")) o.gravity[1] = value;
  else if (!strcmp(name, "gravity_z")) o.gravity[2] = value;
  else return fail(std::string("unknown real option: ") + name);
  return 0;
}

// Model constants that tasks rewrite between episodes (straight copies of mjModel arrays
// in the kernel's tables; anything the tables derive -- contact-pair mixing, inertias,
// invweight0 -- is fixed at batch creation, as mj_setConst-dependent fields are in MuJoCo).
extern "C" int dmc_batch_set_model_real(dmc_batch* b, const char* name, const double* values, int count) {
  if (!b || !name || !values) return fail("null argument");
  const StepLayout& L = b->tb.L;
  const StepDims& d = L.d;
  struct Slot { const char* name; int off, cnt, stride, ncopy; };   // stride: source elements per table element group
  const Slot slots[] = {
      {"dof_damping", L.mr_dof_damping, d.nv, 1, 1},   {"jnt_stiffness", L.mr_jnt_stiffness, d.njnt, 1, 1},
      {"jnt_range", L.mr_jnt_range, 2 * d.njnt, 1, 1}, {"jnt_margin", L.mr_jnt_margin, d.njnt, 1, 1},
      {"qpos_spring", L.mr_qpos_spring, d.nq, 1, 1},   {"site_pos", L.mr_site_pos, 3 * d.nsite, 1, 1},
      {"site_quat", L.mr_site_quat, 4 * d.nsite, 1, 1}, {"site_size", L.mr_site_size, 3 * d.nsite, 1, 1},
      {"actuator_ctrlrange", L.mr_act_ctrlrange, 2 * d.nu, 1, 1},
      {"actuator_forcerange", L.mr_act_forcerange, 2 * d.nu, 1, 1},
      {"wrap_prm", L.mr_wrap_prm, d.nwrap, 1, 1},
      {"body_pos", L.mr_body_pos, 3 * d.nbody, 1, 1}, {"body_quat", L.mr_body_quat, 4 * d.nbody, 1, 1},
      // geom frames / sizes (suite/reacher.py:88-94, suite/fish.py:150-154 move and resize their target geom); like a
      // write to mjModel, nothing derived at compile time follows (body inertias, geom_rbound, contact-pair mixing)
      {"geom_pos", L.mr_geom_pos, 3 * d.ngeom, 1, 1}, {"geom_quat", L.mr_geom_quat, 4 * d.ngeom, 1, 1},
      {"geom_size", L.mr_geom_size, 3 * d.ngeom, 1, 1},
  };
  for (const Slot& s : slots) {
    if (strcmp(name, s.name)) continue;
    if (count != s.cnt) return fail(std::string("wrong element count for model field ") + name);
    for (int i = 0; i < count; i++) b->tb.mr[s.off + i] = values[i];
    if (bump_epoch(b, 0, true)) return -2;
    if (!strcmp(name, "dof_damping")) {
      b->tb.opts.any_damping = 0;
      for (int i = 0; i < count; i++) { if (values[i] < 0) return fail("negative dof_damping"); if (values[i] > 0) b->tb.opts.any_damping = 1; }
    }
    hipError_t e = hipSetDevice(b->device);
    if (e != hipSuccess) return fail(hipGetErrorString(e));
    if (dmc_batch_sync(b)) return -2;
    return upload_tables(b);
  }
  return fail(std::string("model field cannot be changed after batch creation: ") + name);
}

extern "C" int dmc_batch_reset(dmc_batch* b, const uint8_t* env_mask, int keyframe) {
  if (!b) return fail("null batch");
  const HostModel& m = b->model->hm;
  if (keyframe >= m.nkey) return fail("keyframe out of range");
  const int B = b->B;
  auto reset_real = [&](FieldId id, const double* init, int rows) -> int {
    Field* f = &b->fields[id];
    if (!rows) return 0;
    std::vector<double> host((size_t)B * rows);
    if (env_mask) { if (get_real(b, f, host.data())) return -2; }
    for (int e = 0; e < B; e++) if (!env_mask || env_mask[e]) for (int k = 0; k < rows; k++) host[(size_t)e * rows + k] = init ? init[k] : 0.0;
    return set_real(b, f, host.data());
  };
  const double* q0 = keyframe >= 0 ? &m.key_qpos[(size_t)keyframe * m.nq] : m.qpos0.data();
  const double* v0 = keyframe >= 0 ? &m.key_qvel[(size_t)keyframe * m.nv] : nullptr;
  const double* c0 = keyframe >= 0 ? &m.key_ctrl[(size_t)keyframe * m.nu] : nullptr;
  if (reset_real(F_qpos, q0, m.nq)) return -2;
  if (reset_real(F_qvel, v0, m.nv)) return -2;
  if (reset_real(F_ctrl, c0, m.nu)) return -2;
  if (reset_real(F_qacc_warmstart, nullptr, m.nv)) return -2;
  if (reset_real(F_qfrc_applied, nullptr, m.nv)) return -2;
  if (b->xfrc_on && reset_real(F_xfrc_applied, nullptr, 6*m.nbody)) return -2;
  // mj_resetDataKeyframe restores time, the activations and the mocap poses of the keyframe as well
  if (reset_real(F_time, keyframe >= 0 ? &m.key_time[keyframe] : nullptr, 1)) return -2;
  if (reset_real(F_act, keyframe >= 0 && m.na ? &m.key_act[(size_t)keyframe * m.na] : nullptr, m.na)) return -2;
  if (m.nmocap) {      // mj_resetData: the mocap poses start at the bodies' model poses
    std::vector<double> mp(3 * (size_t)m.nmocap), mq(4 * (size_t)m.nmocap);
    for (int i = 0; i < m.nbody; i++) if (m.body_mocapid[i] >= 0) {
      for (int k = 0; k < 3; k++) mp[3*m.body_mocapid[i] + k] = m.body_pos[3*i + k];
      for (int k = 0; k < 4; k++) mq[4*m.body_mocapid[i] + k] = m.body_quat[4*i + k];
    }
    if (keyframe >= 0) {
      std::copy(m.key_mpos.begin() + (size_t)keyframe * 3 * m.nmocap, m.key_mpos.begin() + (size_t)(keyframe + 1) * 3 * m.nmocap, mp.begin());
      std::copy(m.key_mquat.begin() + (size_t)keyframe * 4 * m.nmocap, m.key_mquat.begin() + (size_t)(keyframe + 1) * 4 * m.nmocap, mq.begin());
    }
    if (reset_real(F_mocap_pos, mp.data(), 3*m.nmocap)) return -2;
    if (reset_real(F_mocap_quat, mq.data(), 4*m.nmocap)) return -2;
  }
  // mj_resetData clears warnings as well
  Field* w = &b->fields[F_warning];
  std::vector<int32_t> wh((size_t)B * DMC_NWARNING, 0);
  if (env_mask) { if (get_int(b, w, wh.data())) return -2; for (int e = 0; e < B; e++) if (env_mask[e]) for (int k = 0; k < DMC_NWARNING; k++) wh[(size_t)e * DMC_NWARNING + k] = 0; }
  return set_int(b, w, wh.data());
}

extern "C" int dmc_batch_info(const dmc_batch* b, int* info) {
  if (!b || !info) return fail("null argument");
  const StepLayout& L = b->tb.L;
  info[0] = b->B; info[1] = b->precision; info[2] = b->geom.lpe; info[3] = b->geom.waves; info[4] = b->geom.envs_per_block;
  info[5] = b->geom.lds_bytes; info[6] = b->geom.grid; info[7] = L.d.nconmax; info[8] = L.d.njmax;
  info[9] = (int)((size_t)L.n_sr * b->elem + (size_t)L.n_si * sizeof(int));
  info[10] = b->spec_launch ? 1000 : b->geom.static_id;      // 1000: a specialisation plugin is attached
  info[11] = L.d.kmax;
  info[12] = b->geom.lds_bytes - b->geom.envs_per_block * info[9];
  { long blocks = (160L * 1024) / b->geom.lds_bytes; if (blocks * b->geom.waves > 8) blocks = 8 / b->geom.waves; info[13] = (int)(blocks * b->geom.envs_per_block); }
  info[14] = L.d.njdense; info[15] = L.d.njcon; info[16] = b->stash_on; info[17] = (int)((size_t)L.n_keep * b->elem + (size_t)(L.n_si + 4) * sizeof(int));
  info[18] = (int)((size_t)L.n_gs * b->elem);
  info[19] = b->geom.queue;
  info[20] = b->geom.queue ? b->max_slices : 0;      // pieces a queued Physics.step(nstep > 1) launch cuts an item into, at most (<= 1: whole items)
  // 1: the batch's step launches open with the stage split across wave pairs (step_kernel_body's `coop`: a kernel that has
  // it, whole wave pairs per workgroup, no work queue, a kinematic stash and no full stash)
  const int coop_kernel = b->spec_launch ? b->spec_coop : (b->precision == 32 ? step_coop_open_f32(b->geom) : 0);
  info[21] = (coop_kernel && b->geom.waves % 2 == 0 && !b->geom.queue && b->d_kstash && !b->stash_on) ? 1 : 0;
  return 0;
}

extern "C" int dmc_batch_enable_profiling(dmc_batch* b, int enabled) {
  if (!b) return fail("null batch");
  if (!b->prof) b->prof = new Profiler();
  b->prof->on = enabled != 0;
  return 0;
}
extern "C" int dmc_batch_get_timer(dmc_batch* b, int timer, double* duration_s, long long* number) {
  if (!b || !duration_s || !number) return fail("null argument");
  if (timer != 0 && timer != 1) return fail("timer must be 0 (mjTIMER_STEP) or 1 (mjTIMER_FORWARD)");
  *duration_s = 0; *number = 0;
  if (!b->prof) return 0;
  HIP_TRY(hipSetDevice(b->device));
  prof_drain(b->prof, true);
  *duration_s = b->prof->duration[timer]; *number = b->prof->number[timer];
  return 0;
}
extern "C" int dmc_batch_time_steps(dmc_batch* b, int nstep, int legacy_step, int reps, void* hip_stream, float* ms_per_launch) {
  if (!b || !ms_per_launch || reps < 1) return fail("bad argument");
  HIP_TRY(hipSetDevice(b->device));
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  HIP_TRY(hipEventRecord(e0, (hipStream_t)hip_stream));
  for (int r = 0; r < reps; r++) { int rc = dmc_batch_step(b, nstep, legacy_step, hip_stream); if (rc) return rc; }
  HIP_TRY(hipEventRecord(e1, (hipStream_t)hip_stream));
  HIP_TRY(hipEventSynchronize(e1));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  *ms_per_launch = ms / reps;
  return 0;
}

extern "C" int dmc_batch_debug_enable(dmc_batch* b, int n) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->device));
  dev_free(b, &b->d_debug); dev_free(b, &b->d_debug_i);
  b->ndebug = 0;
  if (n <= 0) return 0;
  if (n > b->B) n = b->B;
  const StepLayout& L = b->tb.L;
  if (dev_alloc(b, &b->d_debug, (size_t)(L.n_sr + L.n_gs) * n * b->elem, true, "debug window") ||
      dev_alloc(b, &b->d_debug_i, (size_t)L.n_si * n * sizeof(int), true, "debug window")) return -2;
  b->ndebug = n;
  return 0;
}
// dst[i] = element (off + i, env) of the (rows, n) dump of T
template <typename T>
static int debug_column(const void* dump, int off, int cnt, int n, int env, double* dst, int* count) {
  std::vector<T> tmp((size_t)cnt * n);
  HIP_TRY(hipMemcpy(tmp.data(), (const T*)dump + (size_t)off * n, tmp.size() * sizeof(T), hipMemcpyDeviceToHost));
  for (int i = 0; i < cnt; i++) dst[i] = tmp[(size_t)i * n + env];
  *count = cnt;
  return 0;
}
extern "C" int dmc_batch_debug_get(dmc_batch* b, const char* scratch_name, int env, double* dst, int* count) {
  if (!b || !scratch_name || !dst || !count) return fail("null argument");
  if (env < 0 || env >= b->ndebug) return fail("env outside the debug window");
  int off, cnt, kind;
  if (!step_layout_find(&b->tb.L, scratch_name, &off, &cnt, &kind)) return fail(std::string("unknown scratch array: ") + scratch_name);
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipDeviceSynchronize());
  if (kind) return debug_column<int>(b->d_debug_i, off, cnt, b->ndebug, env, dst, count);
  return b->precision == 64 ? debug_column<double>(b->d_debug, off, cnt, b->ndebug, env, dst, count)
                            : debug_column<float>(b->d_debug, off, cnt, b->ndebug, env, dst, count);
}

// ---- per-episode joint randomisation on the device -------------------------------------------------------------
// suite/utils/randomizers.py:35-88 (randomize_limited_and_rotational_joints) and the draws of
// suite/cheetah.py:66-69 / suite/quadruped.py:_find_non_contacting_height for a whole batch, without a host round
// trip and without a finite pool of start states: a counter-based generator (Philox4x32-10, Salmon et al. 2011) keyed
// by the 64-bit seed with counter (draw number of the env, joint, block, env) -- every (env, episode, joint) has its own
// stream whatever the batch size, launch order or mask, and different seeds give different streams for every env
// (keying by seed ^ env made seeds below B permutations of one another).
struct Philox { uint32_t c[4]; };
__host__ __device__ inline Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  Philox o = {{c0, c1, c2, c3}};
  return o;
}
__device__ inline double philox_u01(uint32_t x) { return ((double)x + 0.5) * (1.0 / 4294967296.0); }      // in (0, 1)
__device__ inline void box_muller(double u0, double u1, double* n0, double* n1) {
  const double r = sqrt(-2.0 * log(u0)), a = 6.283185307179586476925286766559 * u1;
  *n0 = r * cos(a); *n1 = r * sin(a);
}
template <typename T>
__global__ void __launch_bounds__(256) randomize_joints_kernel(T* __restrict__ qpos, int B, int njnt, const int* __restrict__ ji,
                                                               const double* __restrict__ jr, uint32_t seed_lo, uint32_t seed_hi,
                                                               int* __restrict__ draw, const int* __restrict__ mask, int flags) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= B || (mask && !mask[env])) return;
  const uint32_t k = (uint32_t)draw[env];
  draw[env] = (int)(k + 1);
  const uint32_t key0 = seed_lo, key1 = seed_hi, cenv = (uint32_t)env;   // key = the seed alone; env is a counter word
  for (int j = 0; j < njnt; j++) {
    const int type = ji[j], adr = ji[njnt + j], limited = ji[2*njnt + j];
    const double lo = jr[2*j], hi = jr[2*j + 1];
    const Philox x = philox4x32_10(k, (uint32_t)j, 0u, cenv, key0, key1);
    if (type == DMC_JNT_HINGE || type == DMC_JNT_SLIDE) {
      if (limited) { if (flags & DMC_RAND_LIMITED) qpos[(size_t)adr*B + env] = (T)(lo + (hi - lo) * philox_u01(x.c[0])); }
      else if (type == DMC_JNT_HINGE && (flags & DMC_RAND_UNLIMITED_HINGE))
        qpos[(size_t)adr*B + env] = (T)(-3.14159265358979323846 + 6.283185307179586476925286766559 * philox_u01(x.c[0]));
    } else if (type == DMC_JNT_BALL && limited) {
      if (!(flags & DMC_RAND_LIMITED)) continue;
      // random_limited_quaternion: axis ~ normalised N(0, I), angle ~ U(0, range max)
      const Philox y = philox4x32_10(k, (uint32_t)j, 1u, cenv, key0, key1);
      double n[4];
      box_muller(philox_u01(x.c[0]), philox_u01(x.c[1]), &n[0], &n[1]);
      box_muller(philox_u01(x.c[2]), philox_u01(x.c[3]), &n[2], &n[3]);
      const double nn = sqrt(n[0]*n[0] + n[1]*n[1] + n[2]*n[2]), ang = philox_u01(y.c[0]) * hi, sn = sin(0.5 * ang) / nn;
      qpos[(size_t)adr*B + env] = (T)cos(0.5 * ang);
      for (int c = 0; c < 3; c++) qpos[(size_t)(adr + 1 + c)*B + env] = (T)(n[c] * sn);
    } else if (type == DMC_JNT_BALL || type == DMC_JNT_FREE) {
      if (!(flags & DMC_RAND_QUATERNION)) continue;
      // ball joints: normalised N(0, I) (uniform on the 3-sphere); free joints: normalised U(0, 1)^4 as the reference
      // draws them (randomizers.py:84-88 keeps `rand` on purpose) unless DMC_RAND_FREE_NORMAL asks for the sphere
      double q[4];
      if (type == DMC_JNT_BALL || (flags & DMC_RAND_FREE_NORMAL)) {
        box_muller(philox_u01(x.c[0]), philox_u01(x.c[1]), &q[0], &q[1]);
        box_muller(philox_u01(x.c[2]), philox_u01(x.c[3]), &q[2], &q[3]);
      } else {
        for (int c = 0; c < 4; c++) q[c] = philox_u01(x.c[c]);
      }
      const double inv = 1.0 / sqrt(q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3]);
      const int a0 = adr + (type == DMC_JNT_FREE ? 3 : 0);
      for (int c = 0; c < 4; c++) qpos[(size_t)(a0 + c)*B + env] = (T)(q[c] * inv);
    }
  }
}
extern "C" int dmc_batch_randomize_joints(dmc_batch* b, uint64_t seed, int32_t* d_draw, const int32_t* d_env_mask, int flags,
                                          void* hip_stream) {
  if (!b || !d_draw) return fail("null argument");
  HIP_TRY(hipSetDevice(b->device));
  const HostModel& m = b->model->hm;
  const int nj = m.njnt;
  if (!b->d_rj_i) {
    std::vector<int> ji(3 * (size_t)std::max(1, nj));
    for (int j = 0; j < nj; j++) { ji[j] = m.jnt_type[j]; ji[nj + j] = m.jnt_qposadr[j]; ji[2*nj + j] = m.jnt_limited[j]; }
    std::vector<double> jr(2 * (size_t)std::max(1, nj));
    std::copy(m.jnt_range.begin(), m.jnt_range.begin() + 2 * (size_t)nj, jr.begin());
    if (dev_alloc(b, &b->d_rj_r, jr.size() * sizeof(double), false, "joint ranges", jr.data()) ||
        dev_alloc(b, &b->d_rj_i, ji.size() * sizeof(int), false, "joint ranges", ji.data())) return -2;
  }
  const dim3 grid((b->B + 255) / 256), block(256);
  void* q = b->fields[F_qpos].dev;
  auto run = [&](auto* qpos) {
    hipLaunchKernelGGL(randomize_joints_kernel, grid, block, 0, (hipStream_t)hip_stream, qpos, b->B, nj, (const int*)b->d_rj_i,
                       (const double*)b->d_rj_r, (uint32_t)seed, (uint32_t)(seed >> 32), d_draw, d_env_mask, flags);
  };
  if (b->precision == 64) run((double*)q); else run((float*)q);
  HIP_TRY(hipGetLastError());
  // qpos was edited behind the stashes' back
  return dmc_batch_invalidate_async(b, hip_stream);
}

// ---- wave trace: when every wave of the LAST launch started / finished its item (100 MHz constant clock) -------
extern "C" int dmc_batch_wave_trace(dmc_batch* b, int enable, int32_t* dst, int* nitems) {
  if (!b) return fail("null batch");
  HIP_TRY(hipSetDevice(b->device));
  const int n = (b->B * b->geom.lpe + 63) / 64;
  if (nitems) *nitems = n;
  if (dst) {
    if (!b->d_trace) return fail("wave trace not enabled");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dst, b->d_trace, (size_t)64 * n * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
  }
  HIP_TRY(hipDeviceSynchronize());
  dev_free(b, &b->d_trace);
  b->trace_launch = 0;
  return enable ? dev_alloc(b, &b->d_trace, (size_t)64 * n * sizeof(int), true, "wave trace") : 0;
}

// ---- per-phase cycle profile (only meaningful in -DDMC_PROFILE builds) -----------
extern "C" int dmc_batch_prof_enable(dmc_batch* b, int enable) {
  if (!b) return fail("null batch");
#ifndef DMC_PROFILE
  if (enable) return fail("library built without DMC_PROFILE");
#endif
  HIP_TRY(hipSetDevice(b->device));
  dev_free(b, &b->d_prof);
  if (!enable) return 0;
  return dev_alloc(b, &b->d_prof, (size_t)32 * b->B * sizeof(long long), true, "phase counters");
}
// dst: (PROF_N) mean cycles per env, accumulated since enable; returns PROF_N in *n
extern "C" int dmc_batch_prof_get(dmc_batch* b, double* dst, int* n) {
  if (!b || !dst || !n) return fail("null argument");
  if (!b->d_prof) return fail("profiling not enabled");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<long long> tmp((size_t)32 * b->B);
  HIP_TRY(hipMemcpy(tmp.data(), b->d_prof, tmp.size() * sizeof(long long), hipMemcpyDeviceToHost));
  for (int k = 0; k < 32; k++) { double s = 0; for (int e = 0; e < b->B; e++) s += (double)tmp[(size_t)k * b->B + e]; dst[k] = s / b->B; }
  *n = 32;
  return 0;
}

// ---- batched ray-cast cameras (camera_core.h, camera_kernels.hip) ----------------------------------------------
#include "camera_core.h"

// ---- what the add-on units of a batch (cameras, rays) share ------------------------------------------------------
// f(T()) with the batch's real type: `by_precision(b, [&](auto t) { using T = decltype(t); ... })`
template <class F>
static auto by_precision(const dmc_batch* b, F&& f) { return b->precision == 64 ? f(double()) : f(float()); }
// The batch's poses and geometry as a unit's kernel reads them: the members CamArgs and RayArgs share by name.
template <class Args>
static void fill_pose_args(const dmc_batch* b, Args* a) {
  using P = decltype(a->geom_xpos);      // const T*
  a->geom_xpos = (P)b->fields[F_geom_xpos].dev; a->geom_xmat = (P)b->fields[F_geom_xmat].dev;
  a->xpos = (P)b->fields[F_xpos].dev; a->xmat = (P)b->fields[F_xmat].dev;
  a->geom_size = (P)b->d_mr + b->tb.L.mr_geom_size;
  const Field* eg = b->tb.opts.eg_n ? &b->fields[F_env_geom] : nullptr;
  a->eg_data = eg ? (P)eg->dev : nullptr; a->eg_slot = eg ? b->d_eg_slot : nullptr;
  a->B = b->B;
}
// 0 when the derived arrays of `need` (OUT_*) in device memory are those of the last step / forward launch, else -3
static int poses_fresh(const dmc_batch* b, int need, const char* who) {
  if ((b->outmask & b->launched_mask & need) == need) return 0;
  return fail(std::string(who) + ": the batch's output mask excludes arrays it reads (geom / xpos / xmat / subtree_com / site), or "
              "did when the last step / forward launch ran (or none has run yet): the poses in device memory would be stale", -3);
}

struct dmc_camera {
  dmc_batch* b;
  std::vector<void*> dev_bufs;      // dev_alloc / dev_free_all
  int ncam, H, W, ngeom, nmat, need_mask, cull, pretransform;
  double near_, far_, ambient, diffuse, bg[3];
  std::vector<int> matid;
  void* d_cams; int* d_type; int* d_skip; float* d_color;
  // textures (dmc_camera_set_materials): off until set, and off again when cleared
  int tex_on, tex_filter, sky; float sky1[3], sky2[3];
  void* d_mat;      // CamMat<T>[ngeom] in the batch precision
  std::vector<double> mat_rgba_own;      // (ngeom, 4): a material record's own rgba, NaN where it has none
};
template <typename T>
static void cam_spec_to_dev(const dmc_camera_spec& s, int H, CamDev<T>* d) {
  d->mode = s.mode; d->body = s.bodyid; d->target = s.targetbodyid; d->pad = 0;
  for (int k = 0; k < 3; k++) { d->pos[k] = (T)s.pos[k]; d->pos0[k] = (T)s.pos0[k]; d->poscom0[k] = (T)s.poscom0[k]; }
  for (int k = 0; k < 9; k++) { d->mat[k] = (T)s.mat[k]; d->mat0[k] = (T)s.mat0[k]; }
  d->inv_f = (T)(tan(0.5*s.fovy*3.14159265358979323846/180.0)/(0.5*H));
}
extern "C" int dmc_camera_create(dmc_batch* b, int ncam, const dmc_camera_spec* specs, int height, int width,
                                 const dmc_camera_options* opt, dmc_camera** out) {
  if (!b || !specs || !out || !opt) return fail("null argument");
  if (ncam < 1 || height < 1 || width < 1) return fail("camera count and image size must be positive");
  const HostModel& m = b->model->hm;
  int need = OUT_GEOM;
  for (int i = 0; i < ncam; i++) {
    const dmc_camera_spec& s = specs[i];
    if (s.mode < CAM_FIXED || s.mode > CAM_TARGETBODYCOM) return fail("camera mode out of range");
    if (s.bodyid < 0 || s.bodyid >= m.nbody) return fail("camera body out of range");
    if (s.mode >= CAM_TARGETBODY && (s.targetbodyid < 0 || s.targetbodyid >= m.nbody)) return fail("a targetbody camera needs a target body");
    if (!(s.fovy > 0 && s.fovy < 180)) return fail("camera fovy must lie in (0, 180) degrees");
    if (s.mode == CAM_TRACK) need |= OUT_XPOS;
    else if (s.mode == CAM_TRACKCOM) need |= OUT_SUBTREE_COM;
    else need |= OUT_XPOS | OUT_XMAT | (s.mode == CAM_TARGETBODYCOM ? OUT_SUBTREE_COM : 0);
  }
  if (!(opt->near_m >= 0) || !(opt->far_m > opt->near_m)) return fail("camera clip range: need 0 <= near < far");
  HIP_TRY(hipSetDevice(b->device));
  dmc_camera* c = new dmc_camera();      // (zeroed)
  c->b = b; c->ncam = ncam; c->H = height; c->W = width; c->ngeom = m.ngeom; c->nmat = opt->nmat; c->need_mask = need;
  c->cull = 1; c->pretransform = 1;
  c->near_ = opt->near_m; c->far_ = opt->far_m; c->ambient = opt->ambient; c->diffuse = opt->diffuse;
  for (int k = 0; k < 3; k++) c->bg[k] = opt->background[k];
  c->matid.assign(m.ngeom, -1);
  std::vector<int> type(std::max(1, m.ngeom)), skip(std::max(1, m.ngeom));
  for (int g = 0; g < m.ngeom; g++) {
    type[g] = m.geom_type[g];
    const int grp = opt->geom_group ? opt->geom_group[g] : 0;
    skip[g] = !cam_primitive(type[g]) || m.geom_invisible[g] || grp < 0 || grp > 30 || !((opt->group_mask >> grp) & 1);
    if (opt->geom_matid && opt->geom_matid[g] >= 0) {
      if (opt->geom_matid[g] >= opt->nmat) { delete c; return fail("geom_matid out of range"); }
      c->matid[g] = opt->geom_matid[g];
    }
  }
  const size_t ni = sizeof(int)*type.size();
  int rc = dev_alloc(c, &c->d_type, ni, false, "camera geom types", type.data());
  rc = rc ? rc : dev_alloc(c, &c->d_skip, ni, false, "camera geom mask", skip.data());
  rc = rc ? rc : dev_alloc(c, &c->d_color, sizeof(float)*3*type.size(), true, "camera geom colours");
  rc = rc ? rc : by_precision(b, [&](auto t) {
    std::vector<CamDev<decltype(t)>> d(ncam);
    for (int i = 0; i < ncam; i++) cam_spec_to_dev(specs[i], height, &d[i]);
    return dev_alloc(c, &c->d_cams, sizeof(d[0])*ncam, false, "cameras", d.data());
  });
  if (rc) { dmc_camera_destroy(c); return rc; }
  *out = c;
  return 0;
}
extern "C" void dmc_camera_destroy(dmc_camera* c) {
  if (!c) return;
  dev_free_all(c);
  delete c;
}
extern "C" int dmc_camera_set_colors(dmc_camera* c, const double* geom_rgba, const double* mat_rgba) {
  if (!c || !geom_rgba) return fail("null argument");
  std::vector<float> col(3*(size_t)std::max(1, c->ngeom));
  for (int g = 0; g < c->ngeom; g++) {
    const double* s = geom_rgba + 4*g;
    // mjv's setMaterial: a material's colour takes over only where the geom's own rgba is the default grey
    const bool grey = s[0] == 0.5 && s[1] == 0.5 && s[2] == 0.5 && s[3] == 1.0;
    if (grey && c->tex_on && !c->mat_rgba_own.empty() && c->mat_rgba_own[4*g] == c->mat_rgba_own[4*g]) s = &c->mat_rgba_own[4*g];
    else if (c->matid[g] >= 0 && mat_rgba && grey) s = mat_rgba + 4*c->matid[g];
    for (int k = 0; k < 3; k++) col[3*g + k] = (float)s[k];
  }
  HIP_TRY(hipSetDevice(c->b->device));
  HIP_TRY(hipMemcpy(c->d_color, col.data(), sizeof(float)*col.size(), hipMemcpyHostToDevice));
  return 0;
}
template <typename T>
static int upload_materials(dmc_camera* c, const dmc_camera_material* mats) {
  std::vector<CamMat<T>> d((size_t)std::max(1, c->ngeom));
  memset(d.data(), 0, sizeof(d[0])*d.size());
  for (int g = 0; g < c->ngeom; g++) {
    const dmc_camera_material& s = mats[g];
    CamMat<T>& m = d[g];
    m.mapping = s.mapping; m.builtin = s.builtin; m.mark = s.mark; m.W = s.width; m.H = s.height; m.uniform = s.texuniform ? 1 : 0;
    for (int k = 0; k < 2; k++) m.rep[k] = (T)s.texrepeat[k];
    for (int k = 0; k < 3; k++) { m.rgb1[k] = (float)s.rgb1[k]; m.rgb2[k] = (float)s.rgb2[k]; m.markrgb[k] = (float)s.markrgb[k]; }
  }
  if (!c->d_mat) return dev_alloc(c, &c->d_mat, sizeof(d[0])*d.size(), false, "camera materials", d.data());
  HIP_TRY(hipMemcpy(c->d_mat, d.data(), sizeof(d[0])*d.size(), hipMemcpyHostToDevice));
  return 0;
}
extern "C" int dmc_camera_set_materials(dmc_camera* c, const dmc_camera_material* per_geom, const dmc_camera_sky* sky, int filter) {
  if (!c) return fail("null camera");
  if (filter != CAM_FILTER_NEAREST && filter != CAM_FILTER_BOX) return fail("camera materials: filter must be 0 (nearest) or 1 (box)");
  if (!per_geom && !sky) {      // cleared: the next render launches the flat-colour kernel again
    c->tex_on = 0; c->sky = 0; c->mat_rgba_own.clear();
    return 0;
  }
  const HostModel& hm = c->b->model->hm;
  std::vector<dmc_camera_material> none;
  if (!per_geom) { none.assign((size_t)std::max(1, c->ngeom), dmc_camera_material()); per_geom = none.data(); }
  for (int g = 0; g < c->ngeom; g++) {
    const dmc_camera_material& s = per_geom[g];
    if (s.mapping < CAM_MAP_NONE || s.mapping > CAM_MAP_CUBE) return fail("camera materials: mapping out of range");
    if (s.mapping == CAM_MAP_NONE) continue;
    if (s.builtin < CAM_TEX_FLAT || s.builtin > CAM_TEX_GRADIENT) return fail("camera materials: builtin out of range");
    if (s.mark < CAM_MARK_NONE || s.mark > CAM_MARK_CROSS) return fail("camera materials: mark out of range");
    if (s.width < 1 || s.height < 1 || s.width > (1 << 24) || s.height > (1 << 24)) return fail("camera materials: a texture needs 1 <= width, height <= 2^24 texels");
    const int type = hm.geom_type[g];
    if ((s.mapping == CAM_MAP_PLANE) != (type == DMC_GEOM_PLANE)) return fail("camera materials: a 2d texture maps onto planes and a cube texture onto solids only");
    if (s.mapping == CAM_MAP_CUBE && !cam_primitive(type)) return fail("camera materials: a cube texture on a geom the camera does not draw");
  }
  if (sky && (sky->builtin != CAM_TEX_FLAT && sky->builtin != CAM_TEX_GRADIENT)) return fail("camera materials: the skybox is flat or gradient");
  HIP_TRY(hipSetDevice(c->b->device));
  if (int rc = by_precision(c->b, [&](auto t) { return upload_materials<decltype(t)>(c, per_geom); })) return rc;
  c->mat_rgba_own.assign(4*(size_t)std::max(1, c->ngeom), (double)NAN);
  for (int g = 0; g < c->ngeom; g++) if (per_geom[g].has_rgba) for (int k = 0; k < 4; k++) c->mat_rgba_own[4*g + k] = per_geom[g].rgba[k];
  c->sky = sky ? 1 + sky->builtin : 0;
  for (int k = 0; k < 3; k++) { c->sky1[k] = sky ? (float)sky->rgb1[k] : 0.f; c->sky2[k] = sky ? (float)sky->rgb2[k] : 0.f; }
  c->tex_filter = filter; c->tex_on = 1;
  return 0;
}
extern "C" int dmc_camera_set_tuning(dmc_camera* c, int cull, int pretransform) {
  if (!c) return fail("null camera");
  c->cull = cull ? 1 : 0;
  c->pretransform = pretransform ? 1 : 0;
  return 0;
}
template <typename T>
static int camera_render_t(dmc_camera* c, int what, void* rgb, void* depth, void* seg, void* stream) {
  dmc_batch* b = c->b;
  CamArgs<T> a;
  fill_pose_args(b, &a);
  a.subtree_com = (const T*)b->fields[F_subtree_com].dev;
  a.geom_type = c->d_type; a.geom_skip = c->d_skip; a.geom_color = c->d_color;
  a.cams = (const CamDev<T>*)c->d_cams;
  a.ngeom = c->ngeom; a.ncam = c->ncam; a.H = c->H; a.W = c->W; a.cull = c->cull; a.pretransform = c->pretransform;
  a.near_ = (T)c->near_; a.far_ = (T)c->far_; a.ambient = (T)c->ambient; a.diffuse = (T)c->diffuse;
  for (int k = 0; k < 3; k++) {
    const double v = std::min(1.0, std::max(0.0, c->bg[k]));
    a.bg[k] = (uint8_t)(int)floor(255*v + 0.5);
  }
  a.bg[3] = 0;
  a.rgb = (what & CAM_RGB) ? (uint8_t*)rgb : nullptr; a.depth = (what & CAM_DEPTH) ? (T*)depth : nullptr;
  a.seg = (what & CAM_SEG) ? (int*)seg : nullptr;
  int rc;
  if (c->tex_on) {
    CamTexArgs<T> t;
    t.mat = (const CamMat<T>*)c->d_mat; t.filter = c->tex_filter; t.sky = c->sky;
    for (int k = 0; k < 3; k++) { t.sky1[k] = c->sky1[k]; t.sky2[k] = c->sky2[k]; }
    if constexpr (std::is_same_v<T, double>) rc = launch_camera_tex_f64(a, t, stream);
    else rc = launch_camera_tex_f32(a, t, stream);
  } else if constexpr (std::is_same_v<T, double>) rc = launch_camera_f64(a, stream);
  else rc = launch_camera_f32(a, stream);
  if (rc) return fail(rc == -1 ? "camera render: the launch grid does not fit" : "camera render: launch failed", -2);
  return 0;
}
extern "C" int dmc_camera_render(dmc_camera* c, int what_mask, void* rgb_dev, void* depth_dev, void* seg_dev, void* hip_stream) {
  if (!c) return fail("null camera");
  if (!(what_mask & (CAM_RGB | CAM_DEPTH | CAM_SEG))) return fail("camera render: nothing asked for");
  if (((what_mask & CAM_RGB) && !rgb_dev) || ((what_mask & CAM_DEPTH) && !depth_dev) || ((what_mask & CAM_SEG) && !seg_dev))
    return fail("camera render: null output array");
  if (int rc = poses_fresh(c->b, c->need_mask, "camera render")) return rc;
  HIP_TRY(hipSetDevice(c->b->device));
  return by_precision(c->b, [&](auto t) { return camera_render_t<decltype(t)>(c, what_mask, rgb_dev, depth_dev, seg_dev, hip_stream); });
}

// ---- batched ray casts (ray_core.h, ray_kernels.hip; include/dmc_ray.h) ------------------------------------------
#include "../../include/dmc_ray.h"
#include "ray_core.h"
struct dmc_rays {
  dmc_batch* b;
  std::vector<void*> dev_bufs;      // dev_alloc / dev_free_all
  int ngeom, nlist, nscan, ndir, scan_mask;
  double cutoff;
  int *d_type, *d_body, *d_list;
  void* d_scans; void* d_dirs;      // RayScan<T>[nscan], T (nscan, ndir, 3) in the batch precision
  std::vector<dmc::RayScan<double>> scans;
  std::vector<double> dirs;
};
extern "C" int dmc_rays_create(dmc_batch* b, const dmc_rays_options* opt, dmc_rays** out) {
  if (!b || !opt || !out) return fail("null argument");
  const HostModel& m = b->model->hm;
  if (m.ngeom > 0 && (!opt->geom_group || opt->ngeom_group != m.ngeom)) return fail("rays: geom_group must hold one group per geom of the model");
  if (opt->cutoff != opt->cutoff) return fail("rays: cutoff is NaN");
  std::vector<int> type(std::max(1, m.ngeom)), body(std::max(1, m.ngeom)), list;
  for (int g = 0; g < m.ngeom; g++) {
    type[g] = m.geom_type[g];
    body[g] = m.geom_bodyid[g];
    if (body[g] < 0 || body[g] >= m.nbody) return fail("rays: geom body out of range");
    const int grp = std::min(5, std::max(0, opt->geom_group[g]));
    if (!cam_primitive(type[g]) || m.geom_invisible[g] || (opt->has_geomgroup && !opt->geomgroup[grp]) ||
        (!opt->flg_static && m.body_weldid[body[g]] == 0)) continue;
    list.push_back(g);
  }
  HIP_TRY(hipSetDevice(b->device));
  dmc_rays* r = new dmc_rays();      // (zeroed)
  r->b = b; r->ngeom = m.ngeom; r->nlist = (int)list.size(); r->nscan = 0; r->ndir = 0; r->scan_mask = 0;
  r->cutoff = (opt->cutoff > 0 && opt->cutoff < 1e30) ? opt->cutoff : (double)INFINITY;
  list.resize(std::max<size_t>(1, list.size()), 0);
  const size_t ni = sizeof(int)*type.size();
  int rc = dev_alloc(r, &r->d_type, ni, false, "rays geom types", type.data());
  rc = rc ? rc : dev_alloc(r, &r->d_body, ni, false, "rays geom bodies", body.data());
  rc = rc ? rc : dev_alloc(r, &r->d_list, sizeof(int)*list.size(), false, "rays geom list", list.data());
  if (rc) { dmc_rays_destroy(r); return rc; }
  *out = r;
  return 0;
}
extern "C" void dmc_rays_destroy(dmc_rays* r) {
  if (!r) return;
  dev_free_all(r);
  delete r;
}
extern "C" int dmc_rays_info(const dmc_rays* r, int* info) {
  if (!r || !info) return fail("null argument");
  const int v[8] = {r->b->B, r->b->precision, r->nlist, r->nscan, r->ndir, kRayBlock, kRayTile, kRayPass};
  for (int k = 0; k < 8; k++) info[k] = v[k];
  return 0;
}
template <typename T>
static int rays_upload_scans(dmc_rays* r) {
  std::vector<RayScan<T>> s(r->scans.size());
  for (size_t i = 0; i < s.size(); i++) {
    const RayScan<double>& h = r->scans[i];
    s[i].frame_type = h.frame_type; s[i].frame_id = h.frame_id; s[i].bodyexclude = h.bodyexclude; s[i].pad = 0; s[i].pad2 = 0;
    for (int k = 0; k < 3; k++) s[i].offset[k] = (T)h.offset[k];
  }
  std::vector<T> d(r->dirs.begin(), r->dirs.end());
  void *ds = nullptr, *dd = nullptr;
  if (dev_alloc(r, &ds, sizeof(s[0])*s.size(), false, "rays scans", s.data()) ||
      dev_alloc(r, &dd, sizeof(T)*d.size(), false, "rays scan directions", d.data())) { dev_free(r, &ds); return -2; }
  HIP_TRY(hipDeviceSynchronize());      // (a launch in flight may still read the tables this replaces)
  dev_free(r, &r->d_scans); dev_free(r, &r->d_dirs);
  r->d_scans = ds; r->d_dirs = dd;
  return 0;
}
extern "C" int dmc_rays_add_scan(dmc_rays* r, int frame_type, int frame_id, const double* offset, int bodyexclude, int ndir,
                                 const double* dirs_host) {
  if (!r || !offset || !dirs_host) return fail("null argument");
  const HostModel& m = r->b->model->hm;
  if (frame_type < RAY_FRAME_WORLD || frame_type > RAY_FRAME_GEOM) return fail("rays scan: frame type must be 0 world, 1 body, 2 site or 3 geom");
  const int nframe = frame_type == RAY_FRAME_BODY ? m.nbody : frame_type == RAY_FRAME_SITE ? m.nsite : frame_type == RAY_FRAME_GEOM ? m.ngeom : 1;
  if (frame_type == RAY_FRAME_WORLD) frame_id = 0;
  if (frame_id < 0 || frame_id >= nframe) return fail("rays scan: frame id out of range");
  if (bodyexclude < -1 || bodyexclude >= m.nbody) return fail("rays scan: bodyexclude out of range");
  if (ndir < 1) return fail("rays scan: no directions");
  if (r->nscan && ndir != r->ndir) return fail("rays scan: every scan of one object has the same number of directions");
  for (int k = 0; k < 3*ndir; k++) if (!(fabs(dirs_host[k]) < 1e30)) return fail("rays scan: a direction is not finite");
  for (int k = 0; k < 3; k++) if (!(fabs(offset[k]) < 1e30)) return fail("rays scan: the offset is not finite");
  RayScan<double> s;
  s.frame_type = frame_type; s.frame_id = frame_id; s.bodyexclude = bodyexclude; s.pad = 0; s.pad2 = 0;
  for (int k = 0; k < 3; k++) s.offset[k] = offset[k];
  r->scans.push_back(s);
  r->dirs.insert(r->dirs.end(), dirs_host, dirs_host + 3*(size_t)ndir);
  HIP_TRY(hipSetDevice(r->b->device));
  if (int rc = by_precision(r->b, [&](auto t) { return rays_upload_scans<decltype(t)>(r); })) { r->scans.pop_back(); r->dirs.resize(r->dirs.size() - 3*(size_t)ndir); return rc; }
  r->nscan = (int)r->scans.size(); r->ndir = ndir;
  r->scan_mask |= frame_type == RAY_FRAME_BODY ? (OUT_XPOS | OUT_XMAT) : frame_type == RAY_FRAME_SITE ? OUT_SITE : 0;
  return 0;
}
template <typename T>
static int rays_launch_t(dmc_rays* r, bool scan, int nray, const void* pnt, const void* vec, int bex, const int32_t* bex_dev,
                         int per_ray, void* dist, int32_t* geomid, void* normal, void* stream) {
  dmc_batch* b = r->b;
  RayArgs<T> a;
  fill_pose_args(b, &a);
  a.site_xpos = (const T*)b->fields[F_site_xpos].dev; a.site_xmat = (const T*)b->fields[F_site_xmat].dev;
  a.geom_type = r->d_type; a.geom_body = r->d_body; a.list = r->d_list;
  a.ngeom = r->ngeom; a.nlist = r->nlist; a.cutoff = (T)r->cutoff;
  a.nray = nray; a.bodyexclude = bex; a.bodyexclude_per_ray = per_ray; a.pnt = (const T*)pnt; a.vec = (const T*)vec;
  a.bodyexclude_dev = bex_dev;
  a.nscan = r->nscan; a.ndir = r->ndir; a.scans = (const RayScan<T>*)r->d_scans; a.dirs = (const T*)r->d_dirs;
  a.dist = (T*)dist; a.geomid = geomid; a.normal = (T*)normal;
  int rc;
  if constexpr (std::is_same_v<T, double>) rc = scan ? launch_ray_scan_f64(a, stream) : launch_ray_cast_f64(a, stream);
  else rc = scan ? launch_ray_scan_f32(a, stream) : launch_ray_cast_f32(a, stream);
  if (rc) return fail(rc == -1 ? "rays: the launch grid does not fit" : "rays: launch failed", -2);
  return 0;
}
extern "C" int dmc_rays_cast(dmc_rays* r, int nray, const void* pnt_dev, const void* vec_dev, int bodyexclude,
                             const int32_t* bodyexclude_dev, int bodyexclude_per_ray, void* dist_out, int32_t* geomid_out,
                             void* normal_out, void* hip_stream) {
  if (!r) return fail("null rays");
  if (!pnt_dev || !vec_dev) return fail("rays cast: null input array");
  if (!dist_out && !geomid_out && !normal_out) return fail("rays cast: nothing asked for");
  if (nray < 1) return fail("rays cast: the number of rays must be positive");
  if (!bodyexclude_dev && (bodyexclude < -1 || bodyexclude >= r->b->model->hm.nbody)) return fail("rays cast: bodyexclude out of range");
  if (int rc = poses_fresh(r->b, OUT_GEOM, "rays")) return rc;
  HIP_TRY(hipSetDevice(r->b->device));
  return by_precision(r->b, [&](auto t) {
    return rays_launch_t<decltype(t)>(r, false, nray, pnt_dev, vec_dev, bodyexclude, bodyexclude_dev, bodyexclude_per_ray ? 1 : 0, dist_out, geomid_out, normal_out, hip_stream);
  });
}
extern "C" int dmc_rays_scan(dmc_rays* r, void* dist_out, int32_t* geomid_out, void* normal_out, void* hip_stream) {
  if (!r) return fail("null rays");
  if (!r->nscan) return fail("rays scan: no scan was added");
  if (!dist_out && !geomid_out && !normal_out) return fail("rays scan: nothing asked for");
  if (int rc = poses_fresh(r->b, OUT_GEOM | r->scan_mask, "rays")) return rc;
  HIP_TRY(hipSetDevice(r->b->device));
  return by_precision(r->b, [&](auto t) {
    return rays_launch_t<decltype(t)>(r, true, 0, nullptr, nullptr, -1, nullptr, 0, dist_out, geomid_out, normal_out, hip_stream);
  });
}

// ---- batched geom distances (dist_core.h, dist_kernels.hip; include/dmc_dist.h) -----------------------------------
#include "../../include/dmc_dist.h"
#include "dist_core.h"
struct dmc_dist {
  dmc_batch* b;
  std::vector<void*> dev_bufs;      // dev_alloc / dev_free_all
  int ngeom, npair, nmember, iterations;
  double tolerance;
  int *d_type, *d_adr, *d_member;
  void* d_distmax;      // T (npair) in the batch precision
};
extern "C" int dmc_dist_create(dmc_batch* b, int npair, const int32_t* pair_adr, const int32_t* member, int nmember,
                               const double* distmax, const dmc_dist_options* opt, dmc_dist** out) {
  if (!b || !pair_adr || !member || !distmax || !opt || !out) return fail("null argument");
  const HostModel& m = b->model->hm;
  if (npair < 1 || nmember < 2) return fail("dist: no pairs");
  if (!(opt->tolerance > 0) || !(opt->tolerance < 1)) return fail("dist: tolerance must lie in (0, 1)");
  if (opt->iterations < 1 || opt->iterations > 10000) return fail("dist: iterations must lie in [1, 10000]");
  for (int i = 0; i < nmember; i++) {
    if (member[i] < 0 || member[i] >= m.ngeom) return fail("dist: a member geom id is out of range");
    if (!dist_supported(m.geom_type[member[i]]))
      return fail("dist: geom " + std::to_string(member[i]) + " is a mesh or a height field: no distance to those");
  }
  for (int p = 0; p < npair; p++) {
    const int32_t* a = pair_adr + 4*p;
    if (a[1] < 1 || a[3] < 1) return fail("dist: pair " + std::to_string(p) + " has a member without geoms");
    if (a[0] < 0 || a[2] < 0 || (long long)a[0] + a[1] > nmember || (long long)a[2] + a[3] > nmember)
      return fail("dist: the member table of pair " + std::to_string(p) + " leaves the member list");
    if (distmax[p] != distmax[p]) return fail("dist: distmax is NaN");
  }
  std::vector<int> type(std::max(1, m.ngeom));
  for (int g = 0; g < m.ngeom; g++) type[g] = m.geom_type[g];
  HIP_TRY(hipSetDevice(b->device));
  dmc_dist* d = new dmc_dist();      // (zeroed)
  d->b = b; d->ngeom = m.ngeom; d->npair = npair; d->nmember = nmember; d->iterations = opt->iterations; d->tolerance = opt->tolerance;
  int rc = dev_alloc(d, &d->d_type, sizeof(int)*type.size(), false, "dist geom types", type.data());
  rc = rc ? rc : dev_alloc(d, &d->d_adr, sizeof(int)*4*npair, false, "dist pair table", pair_adr);
  rc = rc ? rc : dev_alloc(d, &d->d_member, sizeof(int)*nmember, false, "dist member list", member);
  rc = rc ? rc : by_precision(b, [&](auto t) {
    using T = decltype(t);
    std::vector<T> dm(npair);
    for (int p = 0; p < npair; p++) dm[p] = (T)distmax[p];      // (infinity stays infinity: an unreached pair reads inf)
    return dev_alloc(d, &d->d_distmax, sizeof(T)*npair, false, "dist cutoffs", dm.data());
  });
  if (rc) { dmc_dist_destroy(d); return rc; }
  *out = d;
  return 0;
}
extern "C" void dmc_dist_destroy(dmc_dist* d) {
  if (!d) return;
  dev_free_all(d);
  delete d;
}
extern "C" int dmc_dist_info(const dmc_dist* d, int* info) {
  if (!d || !info) return fail("null argument");
  const bool f64 = d->b->precision == 64;
  const int V = f64 ? DistCaps<double>::V : DistCaps<float>::V, F = f64 ? DistCaps<double>::F : DistCaps<float>::F,
            K = f64 ? DistCaps<double>::K : DistCaps<float>::K, es = f64 ? 8 : 4;
  const int v[10] = {d->b->B, d->b->precision, d->npair, d->nmember, d->iterations, kDistBlock, V, F, K,
                     es*((3*V + F)*K + kDistGeomReals*kDistBlock) + 4*F*K};
  for (int k = 0; k < 10; k++) info[k] = v[k];
  return 0;
}
extern "C" int dmc_dist_query(dmc_dist* d, void* dist_out, void* fromto_out, void* normal_out, int32_t* status_out, void* hip_stream) {
  if (!d) return fail("null dist");
  if (!dist_out && !fromto_out && !normal_out && !status_out) return fail("dist query: nothing asked for");
  if (int rc = poses_fresh(d->b, OUT_GEOM, "dist")) return rc;
  HIP_TRY(hipSetDevice(d->b->device));
  return by_precision(d->b, [&](auto t) {
    using T = decltype(t);
    DistArgs<T> a;
    fill_pose_args(d->b, &a);
    a.geom_type = d->d_type; a.adr = d->d_adr; a.member = d->d_member; a.distmax = (const T*)d->d_distmax;
    a.npair = d->npair; a.iterations = d->iterations; a.tolerance = (T)d->tolerance;
    a.dist = (T*)dist_out; a.fromto = (T*)fromto_out; a.normal = (T*)normal_out; a.status = status_out;
    int rc;
    if constexpr (std::is_same_v<T, double>) rc = launch_dist_f64(a, hip_stream);
    else rc = launch_dist_f32(a, hip_stream);
    if (rc) return fail(rc == -1 ? "dist: the launch grid does not fit" : "dist: launch failed", -2);
    return 0;
  });
}
// one pair on the host in fp64, from the same dist_core.h (no device, no batch)
extern "C" double dmc_geom_distance_host(int type1, const double* size1, const double* pos1, const double* mat1, int type2,
                                         const double* size2, const double* pos2, const double* mat2, double distmax,
                                         double tolerance, int iterations, double* fromto, int32_t* status) {
  if (status) *status = -1;
  if (fromto) for (int k = 0; k < 6; k++) fromto[k] = 0;
  if (!size1 || !pos1 || !mat1 || !size2 || !pos2 || !mat2) { fail("null argument"); return distmax; }
  if (!dist_supported(type1) || !dist_supported(type2)) { fail("geom distance: a mesh or a height field has no distance"); return distmax; }
  if (!(tolerance > 0) || iterations < 1) { fail("geom distance: tolerance and iterations must be positive"); return distmax; }
  DistGeom<double> g1, g2;
  g1.type = type1; g2.type = type2;
  for (int k = 0; k < 3; k++) { g1.size[k] = size1[k]; g1.pos[k] = pos1[k]; g2.size[k] = size2[k]; g2.pos[k] = pos2[k]; }
  for (int k = 0; k < 9; k++) { g1.mat[k] = mat1[k]; g2.mat[k] = mat2[k]; }
  std::vector<double> vtx(3*DistCaps<double>::V), fdist(DistCaps<double>::F);
  std::vector<int> fidx(DistCaps<double>::F);
  DistEpaMem<double> mem;
  mem.vtx = vtx.data(); mem.fdist = fdist.data(); mem.fidx = fidx.data(); mem.stride = 1;
  DistResult<double> r;
  dist_pair_host(g1, g2, distmax, tolerance, iterations, mem, &r);
  if (fromto) { fromto[0] = r.from.x; fromto[1] = r.from.y; fromto[2] = r.from.z; fromto[3] = r.to.x; fromto[4] = r.to.y; fromto[5] = r.to.z; }
  if (status) *status = r.status != 0;
  return r.dist;
}

// ---- batched Jacobians (jac_core.h, jac_kernels.hip; include/dmc_jac.h) --------------------------------------------
#include "../../include/dmc_jac.h"
#include "jac_core.h"
struct dmc_jac {
  dmc_batch* b;
  std::vector<void*> dev_bufs;      // dev_alloc / dev_free_all
  int ntarget, ncol, maxdof, epb;
  int *d_head, *d_ints;
  void* d_reals;      // T in the batch precision
};
extern "C" int dmc_jac_create(dmc_batch* b, const dmc_jac_tables* tb, dmc_jac** out) {
  if (!b || !tb || !out || !tb->dims || !tb->ints || !tb->reals) return fail("null argument");
  *out = nullptr;
  const HostModel& m = b->model->hm;
  const int T = tb->ntarget, C = tb->ncol;
  if (T < 1 || T > 65535) return fail("jac: between 1 and 65535 targets are needed");
  if (C < 1 || C > m.nv) return fail("jac: the number of columns must lie in [1, nv]");
  // every index the kernels follow is checked here, once
  static const int qw[4] = {7, 4, 1, 1}, dw[4] = {6, 3, 1, 1};
  std::vector<int> head((size_t)T*kJacHead, 0);
  long long io = 0, ro = 0;
  int maxdof = 0;
  for (int t = 0; t < T; t++) {
    const std::string who = "jac: target " + std::to_string(t) + ": ";
    const JacDims d = {tb->dims[3*t], tb->dims[3*t + 1], tb->dims[3*t + 2]};
    if (d.nb < 1 || d.nb > m.nbody || d.nj < 0 || d.nd < 0 || d.nj > d.nd) return fail(who + "inconsistent chain sizes");
    if (d.nd > kJacMaxDof) return fail(who + std::to_string(d.nd) + " chain dofs, at most " + std::to_string(kJacMaxDof));
    if (io + jac_nints(d) > tb->nints || ro + jac_nreals(d) > tb->nreals) return fail(who + "the tables are shorter than their sizes say");
    const int32_t* bj = tb->ints + io; const int32_t* bn = bj + d.nb; const int32_t* jt = bn + d.nb; const int32_t* jq = jt + d.nj;
    const int32_t* jd = jq + d.nj; const int32_t* dof = jd + d.nj; const int32_t* col = dof + d.nd;
    std::vector<int> seen(d.nj, 0), covered(d.nd, 0);
    for (int k = 0; k < d.nb; k++) {
      const int j0 = bj[k], jn = bn[k];
      int nball = 0;
      if (jn < 0 || (jn > 0 && (j0 < 0 || (long long)j0 + jn > d.nj))) return fail(who + "body joint range outside the chain");
      for (int j = j0; j < j0 + jn; j++) {
        seen[j]++;
        if (jt[j] == DMC_JNT_FREE && jn != 1) return fail(who + "a free joint must be its body's only joint");
        nball += jt[j] == DMC_JNT_BALL;
      }
      if (nball > 1) return fail(who + "a body with two ball joints is not supported");
    }
    for (int j = 0; j < d.nj; j++) {
      const int ty = jt[j];
      if (seen[j] != 1) return fail(who + "every chain joint must belong to exactly one chain body");
      if (ty < 0 || ty > 3) return fail(who + "unknown joint type");
      if (jq[j] < 0 || jq[j] + qw[ty] > m.nq) return fail(who + "qpos address outside the model");
      if (jd[j] < 0 || jd[j] + dw[ty] > d.nd) return fail(who + "dof slot outside the chain");
      for (int i = 0; i < dw[ty]; i++) covered[jd[j] + i]++;
    }
    for (int k = 0; k < d.nd; k++) {
      if (covered[k] != 1) return fail(who + "every chain dof must belong to exactly one chain joint");
      if (dof[k] < 0 || dof[k] >= m.nv) return fail(who + "dof id outside the model");
      if (col[k] < -1 || col[k] >= C) return fail(who + "output column outside [0, C)");
    }
    for (long long k = ro; k < ro + jac_nreals(d); k++) if (!std::isfinite(tb->reals[k])) return fail(who + "a table entry is not finite");
    int* h = &head[(size_t)t*kJacHead];
    h[0] = d.nb; h[1] = d.nj; h[2] = d.nd; h[4] = (int)io; h[5] = (int)ro;
    io += jac_nints(d); ro += jac_nreals(d);
    if (io > 0x7fffffffLL || ro > 0x7fffffffLL) return fail("jac: the tables are too long");
    maxdof = std::max(maxdof, d.nd);
  }
  if (io != tb->nints || ro != tb->nreals) return fail("jac: the tables are longer than their sizes say");
  const int rb = b->precision == 64 ? 8 : 4;
  const int epb = std::min(kJacBlock, kJacForceLds/rb/C);
  if (epb < 1) return fail("jac: " + std::to_string(C) + " columns do not fit one workgroup's LDS");
  HIP_TRY(hipSetDevice(b->device));
  dmc_jac* j = new dmc_jac();      // (zeroed)
  j->b = b; j->ntarget = T; j->ncol = C; j->maxdof = maxdof; j->epb = epb;
  int rc = dev_alloc(j, &j->d_head, sizeof(int)*head.size(), false, "jac head table", head.data());
  rc = rc ? rc : dev_alloc(j, &j->d_ints, sizeof(int)*std::max<size_t>(1, (size_t)io), false, "jac int tables", io ? tb->ints : nullptr);
  rc = rc ? rc : by_precision(b, [&](auto t) {
    using R = decltype(t);
    std::vector<R> r(tb->reals, tb->reals + ro);
    return dev_alloc(j, &j->d_reals, sizeof(R)*r.size(), false, "jac real tables", r.data());
  });
  if (rc) { dmc_jac_destroy(j); return rc; }
  *out = j;
  return 0;
}
extern "C" void dmc_jac_destroy(dmc_jac* j) {
  if (!j) return;
  dev_free_all(j);
  delete j;
}
extern "C" int dmc_jac_info(const dmc_jac* j, int* info) {
  if (!j || !info) return fail("null argument");
  const int rb = j->b->precision == 64 ? 8 : 4;
  const int v[10] = {j->b->B, j->b->precision, j->ntarget, j->ncol, kJacBlock, 128/rb, jac_tile_bytes(rb), j->epb,
                     kJacForceLds, j->maxdof};
  for (int k = 0; k < 10; k++) info[k] = v[k];
  return 0;
}
template <typename T>
static void jac_fill(const dmc_jac* j, JacArgs<T>* a) {
  *a = JacArgs<T>();
  a->head = j->d_head; a->ints = j->d_ints; a->reals = (const T*)j->d_reals;
  a->qpos = (const T*)j->b->fields[F_qpos].dev; a->qvel = (const T*)j->b->fields[F_qvel].dev;      // (every call: a field can be rebound)
  a->B = j->b->B; a->ntarget = j->ntarget; a->ncol = j->ncol; a->epb = j->epb;
}
extern "C" int dmc_jac_jacobian(dmc_jac* j, const void* point, void* jacp_out, void* jacr_out, void* hip_stream) {
  if (!j) return fail("null jac");
  if (!jacp_out && !jacr_out) return fail("jac: nothing asked for");
  HIP_TRY(hipSetDevice(j->b->device));
  return by_precision(j->b, [&](auto t) {
    using T = decltype(t);
    JacArgs<T> a;
    jac_fill(j, &a);
    a.point = (const T*)point; a.jacp = (T*)jacp_out; a.jacr = (T*)jacr_out;
    a.vec = j->ncol % (16/(int)sizeof(T)) == 0 && ((uintptr_t)jacp_out | (uintptr_t)jacr_out) % 16 == 0;
    int rc;
    if constexpr (std::is_same_v<T, double>) rc = launch_jac_f64(a, hip_stream);
    else rc = launch_jac_f32(a, hip_stream);
    if (rc) return fail(rc == -1 ? "jac: the launch grid does not fit" : "jac: launch failed", -2);
    return 0;
  });
}
extern "C" int dmc_jac_velocity(dmc_jac* j, int local, void* vel_out, void* hip_stream) {
  if (!j || !vel_out) return fail("null argument");
  HIP_TRY(hipSetDevice(j->b->device));
  return by_precision(j->b, [&](auto t) {
    using T = decltype(t);
    JacArgs<T> a;
    jac_fill(j, &a);
    a.vel = (T*)vel_out; a.local = local != 0;
    int rc;
    if constexpr (std::is_same_v<T, double>) rc = launch_jac_vel_f64(a, hip_stream);
    else rc = launch_jac_vel_f32(a, hip_stream);
    if (rc) return fail(rc == -1 ? "jac: the launch grid does not fit" : "jac: launch failed", -2);
    return 0;
  });
}
extern "C" int dmc_jac_force(dmc_jac* j, const void* force, int64_t force_env_stride, int64_t force_target_stride, const void* torque,
                             int64_t torque_env_stride, int64_t torque_target_stride, void* qfrc_out, void* hip_stream) {
  if (!j || !qfrc_out) return fail("null argument");
  if (force_env_stride < 0 || force_target_stride < 0 || torque_env_stride < 0 || torque_target_stride < 0) return fail("jac: negative stride");
  HIP_TRY(hipSetDevice(j->b->device));
  return by_precision(j->b, [&](auto t) {
    using T = decltype(t);
    JacArgs<T> a;
    jac_fill(j, &a);
    a.force = (const T*)force; a.f_se = force_env_stride; a.f_st = force_target_stride;
    a.torque = (const T*)torque; a.t_se = torque_env_stride; a.t_st = torque_target_stride;
    a.qfrc = (T*)qfrc_out;
    int rc;
    if constexpr (std::is_same_v<T, double>) rc = launch_jac_force_f64(a, hip_stream);
    else rc = launch_jac_force_f32(a, hip_stream);
    if (rc) return fail(rc == -1 ? "jac: the launch grid does not fit" : "jac: launch failed", -2);
    return 0;
  });
}

// ---- batched dynamics (dyn_core.h, dyn_kernels.hip; include/dmc_dyn.h) ---------------------------------------------
#include "../../include/dmc_dyn.h"
#include "dyn_core.h"
struct dmc_dyn {
  dmc_batch* b;
  std::vector<void*> dev_bufs;      // dev_alloc / dev_free_all
  DynDims d;
  int W;
  int* d_ints;
  void* d_reals;      // T in the batch precision
};
extern "C" int dmc_dyn_create(dmc_batch* b, const dmc_dyn_tables* tb, int lanes_per_env, dmc_dyn** out) {
  if (!b || !tb || !out || !tb->ints || !tb->reals) return fail("null argument");
  *out = nullptr;
  const HostModel& m = b->model->hm;
  const DynDims d = {tb->nb, tb->nj, tb->nv, tb->nq, tb->nlevel, tb->nsub};
  const int W = lanes_per_env;
  if (W != 16 && W != 32 && W != 64) return fail("dyn: lanes_per_env must be 16, 32 or 64");
  if (d.nv < 1 || d.nv > kDynMaxDof) return fail("dyn: nv must lie in [1, " + std::to_string(kDynMaxDof) + "]");
  if (d.nv != m.nv || d.nq != m.nq) return fail("dyn: nv and nq must be the model's");
  if (d.nb < 2 || d.nb > m.nbody || d.nj < 1 || d.nj > d.nv || d.nlevel < 1 || d.nlevel >= d.nb || d.nsub < d.nb ||
      (long long)d.nsub > (long long)d.nb*d.nb)
    return fail("dyn: inconsistent table sizes");
  if (tb->nints != dyn_nints(d) || tb->nreals != dyn_nreals(d)) return fail("dyn: the tables do not have the length their sizes say");
  // every index the kernels follow is checked here, once
  const DynTab<double> t = dyn_tab<double>(d, tb->ints, tb->reals);
  static const int qw[4] = {7, 4, 1, 1}, dw[4] = {6, 3, 1, 1};
  std::vector<int> jseen(d.nj, 0), dseen(d.nv, 0), level(d.nb, -1);
  if (t.level_adr[0] != 0 || t.level_adr[d.nlevel] != d.nb - 1) return fail("dyn: the levels must cover every body below the world");
  for (int l = 0; l < d.nlevel; l++) {
    if (t.level_adr[l + 1] < t.level_adr[l]) return fail("dyn: level_adr must not decrease");
    for (int k = t.level_adr[l]; k < t.level_adr[l + 1]; k++) {
      const int body = t.level_body[k];
      if (body < 1 || body >= d.nb || level[body] >= 0) return fail("dyn: every body below the world belongs to exactly one level");
      level[body] = l;
    }
  }
  if (t.body_parent[0] != 0 || t.body_jntnum[0] != 0 || t.sub_adr[0] != 0 || t.sub_adr[d.nb] != d.nsub) return fail("dyn: inconsistent world body or subtree lists");
  for (int k = 0; k < d.nb; k++) {
    const std::string who = "dyn: body " + std::to_string(k) + ": ";
    const int p = t.body_parent[k], j0 = t.body_jntadr[k], jn = t.body_jntnum[k];
    if (k > 0 && (p < 0 || p >= k || (p > 0 && level[p] >= level[k]))) return fail(who + "a parent precedes its children, on an earlier level");
    if (t.body_root[k] < 0 || t.body_root[k] >= d.nb || t.body_lastdof[k] < -1 || t.body_lastdof[k] >= d.nv) return fail(who + "root or last dof out of range");
    if (t.sub_adr[k + 1] < t.sub_adr[k] || t.sub_adr[k + 1] > d.nsub) return fail(who + "subtree list out of range");
    for (int s = t.sub_adr[k]; s < t.sub_adr[k + 1]; s++) if (t.sub_body[s] < 0 || t.sub_body[s] >= d.nb) return fail(who + "subtree member out of range");
    if (jn < 0 || (jn > 0 && (j0 < 0 || (long long)j0 + jn > d.nj))) return fail(who + "joint range outside the model");
    int nball = 0;
    for (int j = j0; j < j0 + jn; j++) {
      jseen[j]++;
      if (t.jnt_type[j] == DMC_JNT_FREE && jn != 1) return fail(who + "a free joint must be its body's only joint");
      nball += t.jnt_type[j] == DMC_JNT_BALL;
    }
    if (nball > 1) return fail(who + "a body with two ball joints is not supported");
  }
  for (int j = 0; j < d.nj; j++) {
    const int ty = t.jnt_type[j];
    if (jseen[j] != 1) return fail("dyn: every joint must belong to exactly one body");
    if (ty < 0 || ty > 3) return fail("dyn: unknown joint type");
    if (t.jnt_qadr[j] < 0 || t.jnt_qadr[j] + qw[ty] > d.nq) return fail("dyn: qpos address outside the model");
    if (t.jnt_dadr[j] < 0 || t.jnt_dadr[j] + dw[ty] > d.nv) return fail("dyn: dof address outside the model");
    for (int i = 0; i < dw[ty]; i++) dseen[t.jnt_dadr[j] + i]++;
  }
  for (int k = 0; k < d.nv; k++) {
    if (dseen[k] != 1) return fail("dyn: every dof must belong to exactly one joint");
    if (t.dof_body[k] < 1 || t.dof_body[k] >= d.nb) return fail("dyn: dof body out of range");
    if (t.dof_parent[k] < -1 || t.dof_parent[k] >= k || t.dof_pred[k] < -1 || t.dof_pred[k] >= k) return fail("dyn: a dof's parent and predecessor precede it");
    if (t.dof_rot[k] != 0 && t.dof_rot[k] != 1) return fail("dyn: dof_rot is 0 or 1");
  }
  for (int k = 0; k < tb->nreals; k++) if (!std::isfinite(tb->reals[k])) return fail("dyn: a table entry is not finite");
  const int rb = b->precision == 64 ? 8 : 4;
  if (dyn_tier(d.nb, d.nv, 0, W, rb) < 0 || dyn_tier(d.nb, d.nv, 1, W, rb) < 0)
    return fail("dyn: " + std::to_string(kDynBlock/W) + " environments of nv = " + std::to_string(d.nv) + ", " + std::to_string(d.nb) +
                " bodies do not fit one workgroup's LDS at " + std::to_string(W) + " lanes per environment");
  HIP_TRY(hipSetDevice(b->device));
  dmc_dyn* y = new dmc_dyn();      // (zeroed)
  y->b = b; y->d = d; y->W = W;
  int rc = dev_alloc(y, &y->d_ints, sizeof(int)*(size_t)tb->nints, false, "dyn int tables", tb->ints);
  rc = rc ? rc : by_precision(b, [&](auto z) {
    using R = decltype(z);
    std::vector<R> r(tb->reals, tb->reals + tb->nreals);
    return dev_alloc(y, &y->d_reals, sizeof(R)*r.size(), false, "dyn real tables", r.data());
  });
  if (rc) { dmc_dyn_destroy(y); return rc; }
  *out = y;
  return 0;
}
extern "C" void dmc_dyn_destroy(dmc_dyn* y) {
  if (!y) return;
  dev_free_all(y);
  delete y;
}
extern "C" int dmc_dyn_info(const dmc_dyn* y, int* info) {
  if (!y || !info) return fail("null argument");
  const int rb = y->b->precision == 64 ? 8 : 4;
  const int v[10] = {y->b->B, y->b->precision, y->d.nv, y->d.nb, y->W, kDynBlock/y->W, kDynTierBytes[dyn_tier(y->d.nb, y->d.nv, 0, y->W, rb)],
                     kDynTierBytes[dyn_tier(y->d.nb, y->d.nv, 1, y->W, rb)], kDynChunk, y->d.nlevel};
  for (int k = 0; k < 10; k++) info[k] = v[k];
  return 0;
}
// kind 0: the crb launch in `mode`; kind 1: the rne launch
static int dyn_launch(dmc_dyn* y, int kind, int mode, const void* in, int64_t in_se, int K, void* out, void* hip_stream) {
  if (!y || !out) return fail("null argument");
  HIP_TRY(hipSetDevice(y->b->device));
  return by_precision(y->b, [&](auto z) {
    using T = decltype(z);
    DynArgs<T> a = DynArgs<T>();
    a.d = y->d; a.ints = y->d_ints; a.reals = (const T*)y->d_reals;
    a.qpos = (const T*)y->b->fields[F_qpos].dev; a.qvel = (const T*)y->b->fields[F_qvel].dev;      // (every call: a field can be rebound)
    a.B = y->b->B; a.W = y->W; a.mode = mode; a.in = (const T*)in; a.in_se = in_se; a.K = K; a.out = (T*)out;
    int rc;
    if constexpr (std::is_same_v<T, double>) rc = kind ? launch_dyn_rne_f64(a, hip_stream) : launch_dyn_crb_f64(a, hip_stream);
    else rc = kind ? launch_dyn_rne_f32(a, hip_stream) : launch_dyn_crb_f32(a, hip_stream);
    if (rc) return fail(rc == -1 ? "dyn: the launch does not fit" : "dyn: launch failed", -2);
    return 0;
  });
}
extern "C" int dmc_dyn_mass_matrix(dmc_dyn* y, void* M_out, void* hip_stream) { return dyn_launch(y, 0, DYN_MASS, nullptr, 0, 0, M_out, hip_stream); }
extern "C" int dmc_dyn_bias(dmc_dyn* y, void* bias_out, void* hip_stream) { return dyn_launch(y, 1, 0, nullptr, 0, 0, bias_out, hip_stream); }
extern "C" int dmc_dyn_inverse(dmc_dyn* y, const void* qacc, int64_t qacc_env_stride, void* tau_out, void* hip_stream) {
  if (!qacc) return fail("null argument");
  if (qacc_env_stride < 0) return fail("dyn: negative stride");
  return dyn_launch(y, 1, 0, qacc, qacc_env_stride, 0, tau_out, hip_stream);
}
extern "C" int dmc_dyn_mul(dmc_dyn* y, const void* vec, int K, void* out, void* hip_stream) {
  if (!vec) return fail("null argument");
  if (K < 1) return fail("dyn: at least one vector per environment is needed");
  return dyn_launch(y, 0, DYN_MUL, vec, 0, K, out, hip_stream);
}
extern "C" int dmc_dyn_solve(dmc_dyn* y, const void* vec, int K, void* out, void* hip_stream) {
  if (!vec) return fail("null argument");
  if (K < 1) return fail("dyn: at least one right-hand side per environment is needed");
  return dyn_launch(y, 0, DYN_SOLVE, vec, 0, K, out, hip_stream);
}

// ---- batched linearisation (lin_core.h, lin_kernels.hip; include/dmc_lin.h) -----------------------------------------
#include "../../include/dmc_lin.h"
#include "lin_core.h"
struct dmc_lin {
  dmc_batch *src, *scr;
  std::vector<void*> dev_bufs;      // dev_alloc / dev_free_all
  LinDims d;
  int P, nstep;
  double eps;
  int* d_ints;
  double* d_reals;    // ctrlrange, fp64 in every precision pair
  int* d_flags;       // (B, nu)
  int* d_warn;        // (B)
};
extern "C" int dmc_lin_create(dmc_batch* src, dmc_batch* scr, const dmc_lin_tables* tb, double eps, int centered, int nstep,
                              dmc_lin** out) {
  if (!src || !scr || !tb || !out || !tb->ints) return fail("null argument");
  *out = nullptr;
  if (src == scr) return fail("lin: the scratch batch must be a batch of its own");
  const HostModel &m = src->model->hm, &ms = scr->model->hm;
  if (src->device != scr->device) return fail("lin: the scratch batch must live on the source batch's device");
  if (ms.nq != m.nq || ms.nv != m.nv || ms.na != m.na || ms.nu != m.nu || ms.njnt != m.njnt || ms.nbody != m.nbody ||
      ms.nmocap != m.nmocap || ms.nsensordata != m.nsensordata)
    return fail("lin: the scratch batch must hold the source batch's model");
  if (scr->precision < src->precision) return fail("lin: an fp32 scratch batch cannot linearise an fp64 batch");
  if (src->tb.opts.eg_n) return fail("lin: the source batch declares per-environment geoms, which are not mirrored to the scratch batch");
  if (!(eps > 0) || !std::isfinite(eps)) return fail("lin: eps must be positive");
  if (nstep < 1) return fail("lin: nstep must be >= 1");
  if (tb->nj != m.njnt || tb->nq != m.nq || tb->nv != m.nv || tb->na != m.na || tb->nu != m.nu) return fail("lin: the table sizes must be the model's");
  LinDims d = {m.njnt, m.nq, m.nv, m.na, m.nu, m.nbody, m.nmocap, m.nsensordata, 0, centered ? 1 : 0};
  if (lin_nx(d) < 1) return fail("lin: the model has no state (nx = 0)");
  if (tb->nints != lin_nints(d) || tb->nreals != lin_nreals(d) || (tb->nreals && !tb->reals)) return fail("lin: the tables do not have the length their sizes say");
  // every address the kernels follow is checked here, once
  const LinTab t = lin_tab(d, tb->ints, tb->reals);
  static const int qw[4] = {7, 4, 1, 1}, dw[4] = {6, 3, 1, 1};
  std::vector<int> qseen(d.nq, 0), dseen(d.nv, 0);
  for (int j = 0; j < d.nj; j++) {
    const int ty = t.jnt_type[j];
    if (ty < 0 || ty > 3) return fail("lin: unknown joint type");
    if (t.jnt_qadr[j] < 0 || t.jnt_qadr[j] + qw[ty] > d.nq) return fail("lin: qpos address outside the model");
    if (t.jnt_dadr[j] < 0 || t.jnt_dadr[j] + dw[ty] > d.nv) return fail("lin: dof address outside the model");
    for (int i = 0; i < qw[ty]; i++) qseen[t.jnt_qadr[j] + i]++;
    for (int i = 0; i < dw[ty]; i++) dseen[t.jnt_dadr[j] + i]++;
  }
  for (int k = 0; k < d.nq; k++) if (qseen[k] != 1) return fail("lin: every qpos entry must belong to exactly one joint");
  for (int k = 0; k < d.nv; k++) if (dseen[k] != 1) return fail("lin: every dof must belong to exactly one joint");
  for (int k = 0; k < d.nu; k++) {
    if (t.ctrllimited[k] != 0 && t.ctrllimited[k] != 1) return fail("lin: ctrllimited is 0 or 1");
    if (!std::isfinite(t.ctrlrange[2*k]) || !std::isfinite(t.ctrlrange[2*k + 1])) return fail("lin: a table entry is not finite");
  }
  const int P = lin_ncol(d);
  if (scr->B < P) return fail("lin: the scratch batch holds " + std::to_string(scr->B) + " environments, one linearisation needs " + std::to_string(P));
  HIP_TRY(hipSetDevice(src->device));
  dmc_lin* l = new dmc_lin();      // (zeroed)
  l->src = src; l->scr = scr; l->d = d; l->P = P; l->nstep = nstep; l->eps = eps;
  int rc = dev_alloc(l, &l->d_ints, sizeof(int)*(size_t)std::max(1, tb->nints), false, "lin int tables", tb->nints ? tb->ints : nullptr);
  std::vector<double> reals(tb->reals, tb->reals + tb->nreals);
  reals.push_back(0);      // (never empty)
  rc = rc ? rc : dev_alloc(l, &l->d_reals, sizeof(double)*reals.size(), false, "lin real tables", reals.data());
  rc = rc ? rc : dev_alloc(l, &l->d_flags, sizeof(int)*(size_t)src->B*std::max(1, d.nu), true, "lin nudge flags");
  rc = rc ? rc : dev_alloc(l, &l->d_warn, sizeof(int)*(size_t)src->B, true, "lin warnings");
  if (rc) { dmc_lin_destroy(l); return rc; }
  *out = l;
  return 0;
}
extern "C" void dmc_lin_destroy(dmc_lin* l) {
  if (!l) return;
  dev_free_all(l);
  delete l;
}
extern "C" int dmc_lin_info(const dmc_lin* l, int* info) {
  if (!l || !info) return fail("null argument");
  const int v[12] = {l->src->B, l->P, lin_nx(l->d), l->d.nu, l->d.nsensordata, l->scr->B, l->scr->B/l->P, l->src->precision,
                     l->scr->precision, l->nstep, l->d.centered, kLinBlock};
  for (int k = 0; k < 12; k++) info[k] = v[k];
  return 0;
}
extern "C" int dmc_lin_warnings(dmc_lin* l, int32_t* warn_out, void* hip_stream) {
  if (!l || !warn_out) return fail("null argument");
  HIP_TRY(hipSetDevice(l->src->device));
  HIP_TRY(hipMemcpyAsync(warn_out, l->d_warn, sizeof(int)*(size_t)l->src->B, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
  return 0;
}
template <typename Ts, typename Tc>
static void lin_fill(dmc_lin* l, LinArgs<Ts, Tc>* a) {
  static const FieldId ids[LIN_NFIELD] = {F_qpos, F_qvel, F_act, F_ctrl, F_qacc_warmstart, F_qfrc_applied, F_xfrc_applied, F_mocap_pos,
                                          F_mocap_quat, F_sensordata};
  *a = LinArgs<Ts, Tc>();
  a->d = l->d; a->d.xfrc = l->src->xfrc_on ? 1 : 0;
  a->ints = l->d_ints; a->reals = l->d_reals;
  for (int f = 0; f < LIN_NFIELD; f++) {      // (every call: a field can be rebound)
    a->src[f] = (const Ts*)l->src->fields[ids[f]].dev;
    a->scr[f] = (Tc*)l->scr->fields[ids[f]].dev;
  }
  a->src_time = (const double*)l->src->fields[F_time].dev; a->scr_time = (double*)l->scr->fields[F_time].dev;
  a->scr_warning = (int*)l->scr->fields[F_warning].dev;
  a->flags = l->d_flags; a->warn = l->d_warn;
  a->B = l->src->B; a->Bs = l->scr->B; a->P = l->P;
  a->eps = (Tc)l->eps; a->ch = (Tc)cos(0.5*l->eps); a->sh = (Tc)sin(0.5*l->eps);
}
// fan_only: the first launch of a transition alone (dmc_lin_fan_out)
static int lin_run(dmc_lin* l, int first_env, int nenv, void* A, void* Bm, void* C, void* D, void* hip_stream, bool fan_only) {
  if (!l || (!fan_only && (!A || (!Bm && l->d.nu)))) return fail("null argument");
  if ((C == nullptr) != (D == nullptr) && l->d.nu) return fail("lin: C and D come together");
  if (C && !(l->scr->outmask & OUT_SENSOR)) return fail("lin: sensor derivatives need the sensors in the scratch batch's output mask");
  if (nenv < 1 || first_env < 0 || (long long)first_env + nenv > l->src->B) return fail("lin: the chunk lies outside the source batch");
  if ((long long)nenv*l->P > l->scr->B)
    return fail("lin: " + std::to_string(nenv) + " environments need " + std::to_string((long long)nenv*l->P) + " scratch environments, the scratch batch holds " +
                std::to_string(l->scr->B));
  HIP_TRY(hipSetDevice(l->src->device));
  auto run = [&](auto zs, auto zc) {
    using Ts = decltype(zs);
    using Tc = decltype(zc);
    LinArgs<Ts, Tc> a;
    lin_fill(l, &a);
    a.first_env = first_env; a.nenv = nenv;
    a.A = (Ts*)A; a.Bm = (Ts*)Bm; a.C = (Ts*)C; a.D = (Ts*)D;
    auto go = [&](int which) {
      if constexpr (std::is_same_v<Tc, float>) return launch_lin_f32_f32(a, which, hip_stream);
      else if constexpr (std::is_same_v<Ts, float>) return launch_lin_f32_f64(a, which, hip_stream);
      else return launch_lin_f64_f64(a, which, hip_stream);
    };
    int rc = go(0);
    if (rc) return fail(rc == -1 ? "lin: the launch does not fit" : "lin: launch failed", -2);
    // the scratch state was written behind the batch's back: whatever its stashes hold is stale
    if (a.d.xfrc) l->scr->xfrc_on = 1;
    if ((rc = dmc_batch_invalidate_async(l->scr, hip_stream))) return rc;
    if (fan_only) return 0;
    if ((rc = dmc_batch_step(l->scr, l->nstep, 0, hip_stream))) return rc;
    rc = go(1);
    if (rc) return fail(rc == -1 ? "lin: the launch does not fit" : "lin: launch failed", -2);
    return 0;
  };
  if (l->src->precision == 64) return run(double(), double());
  return l->scr->precision == 64 ? run(float(), double()) : run(float(), float());
}
extern "C" int dmc_lin_transition(dmc_lin* l, int first_env, int nenv, void* A, void* Bm, void* C, void* D, void* hip_stream) {
  return lin_run(l, first_env, nenv, A, Bm, C, D, hip_stream, false);
}
extern "C" int dmc_lin_fan_out(dmc_lin* l, int first_env, int nenv, void* hip_stream) {
  return lin_run(l, first_env, nenv, nullptr, nullptr, nullptr, nullptr, hip_stream, true);
}

// ---- batched contact wrenches (con_core.h, con_kernels.hip; include/dmc_con.h) -------------------------------------
#include "../../include/dmc_con.h"
#include "con_core.h"
struct dmc_con {
  dmc_batch* b;
  std::vector<void*> dev_bufs;      // dev_alloc / dev_free_all
  int ntarget, words, about, nconmax;
  int* d_head;
  uint32_t* d_masks;
  void* d_warm;      // (nv, B) reals: the warm start across a refresh (dmc_con_warmstart)
};
extern "C" int dmc_con_create(dmc_batch* b, const dmc_con_tables* tb, dmc_con** out) {
  if (!b || !tb || !out || !tb->body || !tb->masks) return fail("null argument");
  *out = nullptr;
  const HostModel& m = b->model->hm;
  const int T = tb->ntarget, W = tb->words, nconmax = b->tb.L.d.nconmax;
  if (nconmax < 1) return fail("con: the batch holds no contacts (nconmax == 0)");
  if (T < 1) return fail("con: at least one target is needed");
  if (T > kConMaxTargets) return fail("con: " + std::to_string(T) + " targets, at most " + std::to_string(kConMaxTargets) + " per object");
  if (tb->ngeom != m.ngeom || W != con_words(m.ngeom)) return fail("con: the masks are not sized for the model's " + std::to_string(m.ngeom) + " geoms");
  if (W < 1 || W > kConMaxWords) return fail("con: a model of " + std::to_string(m.ngeom) + " geoms does not fit the mask (at most " + std::to_string(32*kConMaxWords) + ")");
  if (tb->about < CON_ABOUT_COM || tb->about > CON_ABOUT_WORLD) return fail("con: about must be 0 (com), 1 (origin) or 2 (world)");
  std::vector<int> head((size_t)T*kConHead, 0);
  for (int t = 0; t < T; t++) {
    const std::string who = "con: target " + std::to_string(t) + ": ";
    if (tb->body[t] < 0 || tb->body[t] >= m.nbody) return fail(who + "body id outside the model");
    const uint32_t* S = tb->masks + (size_t)t*2*W;
    bool any = false;
    for (int k = 0; k < 2*W; k++) {
      const int w = k % W, bits = m.ngeom - 32*w;      // bits of this word that name a geom
      if (bits < 32 && (S[k] >> bits)) return fail(who + "a mask bit names a geom outside the model");
      any = any || (k < W && S[k]);
    }
    if (!any) return fail(who + "the set of geoms is empty");
    head[(size_t)t*kConHead] = tb->body[t];
  }
  HIP_TRY(hipSetDevice(b->device));
  dmc_con* c = new dmc_con();      // (zeroed)
  c->b = b; c->ntarget = T; c->words = W; c->about = tb->about; c->nconmax = nconmax;
  int rc = dev_alloc(c, &c->d_head, sizeof(int)*head.size(), false, "con head table", head.data());
  rc = rc ? rc : dev_alloc(c, &c->d_masks, sizeof(uint32_t)*(size_t)T*2*W, false, "con masks", tb->masks);
  rc = rc ? rc : dev_alloc(c, &c->d_warm, std::max<size_t>(1, (size_t)m.nv)*b->B*b->elem, true, "con warm start");
  if (rc) { dmc_con_destroy(c); return rc; }
  *out = c;
  return 0;
}
extern "C" void dmc_con_destroy(dmc_con* c) {
  if (!c) return;
  dev_free_all(c);
  delete c;
}
static int con_need(const dmc_con* c, int local) {
  return OUT_CONTACT | (c->about == CON_ABOUT_COM ? OUT_XIPOS : c->about == CON_ABOUT_ORIGIN ? OUT_XPOS : 0) | (local ? OUT_XMAT : 0);
}
extern "C" int dmc_con_info(const dmc_con* c, int* info) {
  if (!c || !info) return fail("null argument");
  const int v[8] = {c->b->B, c->b->precision, c->ntarget, c->nconmax, kConBlock, c->words, 2*kConMaxWords*(int)sizeof(uint32_t), con_need(c, 0)};
  for (int k = 0; k < 8; k++) info[k] = v[k];
  return 0;
}
static int con_fresh(const dmc_con* c, int need) {
  const dmc_batch* b = c->b;
  if ((b->outmask & b->launched_mask & need) == need) return 0;
  return fail("con: the batch's output mask lacks the contact arrays (OUT_CONTACT) or the pose arrays `about` / `local` read (xipos / xpos / "
              "xmat), or did when the last step / forward launch ran (or none has run yet): the arrays in device memory would be stale", -3);
}
template <typename T>
static void con_fill(const dmc_con* c, ConArgs<T>* a) {
  *a = ConArgs<T>();
  const dmc_batch* b = c->b;
  auto R = [&](int f) { return (const T*)b->fields[f].dev; };      // (every call: a field can be rebound)
  auto I = [&](int f) { return (const int*)b->fields[f].dev; };
  a->in.ncon = I(F_ncon); a->in.geom1 = I(F_contact_geom1); a->in.geom2 = I(F_contact_geom2);
  a->in.dist = R(F_contact_dist); a->in.pos = R(F_contact_pos); a->in.frame = R(F_contact_frame); a->in.force = R(F_contact_force);
  a->in.xpos = R(F_xpos); a->in.xipos = R(F_xipos); a->in.xmat = R(F_xmat);
  a->in.B = (size_t)b->B; a->in.nconmax = c->nconmax; a->in.ngeom = b->model->hm.ngeom;
  a->head = c->d_head; a->masks = c->d_masks; a->ntarget = c->ntarget; a->words = c->words; a->about = c->about;
}
extern "C" int dmc_con_wrench(dmc_con* c, void* wrench_out, void* hip_stream) {
  if (!c || !wrench_out) return fail("null argument");
  if (int rc = con_fresh(c, OUT_CONTACT)) return rc;
  HIP_TRY(hipSetDevice(c->b->device));
  return by_precision(c->b, [&](auto t) {
    using T = decltype(t);
    ConArgs<T> a;
    con_fill(c, &a);
    a.wrench = (T*)wrench_out;
    int rc;
    if constexpr (std::is_same_v<T, double>) rc = launch_con_wrench_f64(a, hip_stream);
    else rc = launch_con_wrench_f32(a, hip_stream);
    if (rc) return fail(rc == -1 ? "con: the launch grid does not fit" : "con: launch failed", -2);
    return 0;
  });
}
extern "C" int dmc_con_net(dmc_con* c, int local, void* force_out, void* torque_out, void* normal_out, void* count_out, void* dist_out,
                           void* hip_stream) {
  if (!c) return fail("null con");
  if (!force_out && !torque_out && !normal_out && !count_out && !dist_out) return fail("con: nothing asked for");
  // (the pose arrays are read only for the torque's lever arm and the local frame)
  const bool rot = local && (force_out || torque_out);
  if (int rc = con_fresh(c, (torque_out ? con_need(c, 0) : OUT_CONTACT) | (rot ? OUT_XMAT : 0))) return rc;
  HIP_TRY(hipSetDevice(c->b->device));
  return by_precision(c->b, [&](auto t) {
    using T = decltype(t);
    ConArgs<T> a;
    con_fill(c, &a);
    if (!torque_out) a.about = CON_ABOUT_WORLD;      // no lever arm is needed: no pose is read
    a.local = rot;
    a.force = (T*)force_out; a.torque = (T*)torque_out; a.normal = (T*)normal_out; a.count = (int*)count_out; a.mindist = (T*)dist_out;
    int rc;
    if constexpr (std::is_same_v<T, double>) rc = launch_con_net_f64(a, hip_stream);
    else rc = launch_con_net_f32(a, hip_stream);
    if (rc) return fail(rc == -1 ? "con: the launch grid does not fit" : "con: launch failed", -2);
    return 0;
  });
}
extern "C" int dmc_con_warmstart(dmc_con* c, int restore, void* hip_stream) {
  if (!c) return fail("null con");
  dmc_batch* b = c->b;
  const size_t bytes = (size_t)b->model->hm.nv*b->B*b->elem;
  if (!bytes) return 0;
  HIP_TRY(hipSetDevice(b->device));
  void* field = b->fields[F_qacc_warmstart].dev;
  HIP_TRY(hipMemcpyAsync(restore ? field : c->d_warm, restore ? c->d_warm : field, bytes, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
  return 0;
}
