// dyn_kernels.hip -- batched dynamics (include/dmc_dyn.h): mj_fullM, mj_mulM, mj_solveM and mj_rne for every environment
// of a batch.  The arithmetic of one environment is dyn_core.h.
//
// Both kernels: one wave per workgroup; a group of W = 16 / 32 / 64 lanes of the wave works on one environment, so 64 / W
// environments share the workgroup and every hand-off between phases is a wave-level fence (the step kernel's scheme).
// The working set of an environment -- frames, cdof, cinert, and either crb + the dense M + a chunk of right-hand sides or
// the arrays of mj_rne -- lives in LDS: a static array of 16, 32 or 64 KB, the smallest the workgroup's workspaces fit
// (dyn_tier; dmc_dyn_create refuses a model that fits none).  What the kinematics are computed from is the qpos in device memory: no pose array is read.
//
// dyn_crb_kernel: frames, crb, M; then by mode: M leaves as (B, nv, nv); or the K vectors of (B, K, nv) pass through the
// workspace in chunks of 8 and M v leaves; or M is factorised once and the chunks are solved in place.
// dyn_rne_kernel: frames, mj_comVel, mj_rne with qacc = 0 (bias) or the caller's (inverse); (B, nv) leaves.
//
// An environment's outputs are one contiguous run; the lanes of its group store consecutive addresses, 16 bytes each
// between the first and the last 16-byte boundary of the run, single reals before and after.
#include <hip/hip_runtime.h>

#include "dyn_core.h"

namespace dmc {

template <typename T, int P>
struct alignas(sizeof(T)*P) DynVec { T v[P]; };

struct DynPar {      // dyn_core.h's executor: the group's lanes stride over the items, a wave-level fence ends the phase
  int lane, W;
  template <class F>
  __device__ __forceinline__ void run(int n, F f) {
    for (int i = lane; i < n; i += W) f(i);
    DMC_WSYNC();
  }
};

// n reals from the workspace to the run at dst (the caller fences before: src is complete)
template <typename T>
__device__ __forceinline__ void dyn_store_run(T* dst, const T* src, int n, int lane, int W) {
  constexpr int V = 16/(int)sizeof(T);
  int head = (int)((V - (int)(((uintptr_t)dst/sizeof(T)) % V)) % V);
  head = head < n ? head : n;
  const int nvec = (n - head)/V, tail = head + nvec*V;
  if (lane < head) dst[lane] = src[lane];
  for (int i = lane; i < nvec; i += W) {
    DynVec<T, V> o;
#pragma unroll
    for (int j = 0; j < V; j++) o.v[j] = src[head + i*V + j];
    *reinterpret_cast<DynVec<T, V>*>(dst + head + i*V) = o;
  }
  if (lane < n - tail) dst[tail + lane] = src[tail + lane];
}
template <typename T>
__device__ __forceinline__ void dyn_load_run(T* dst, const T* src, int n, int lane, int W) {
  constexpr int V = 16/(int)sizeof(T);
  int head = (int)((V - (int)(((uintptr_t)src/sizeof(T)) % V)) % V);
  head = head < n ? head : n;
  const int nvec = (n - head)/V, tail = head + nvec*V;
  if (lane < head) dst[lane] = src[lane];
  for (int i = lane; i < nvec; i += W) {
    const DynVec<T, V> o = *reinterpret_cast<const DynVec<T, V>*>(src + head + i*V);
#pragma unroll
    for (int j = 0; j < V; j++) dst[head + i*V + j] = o.v[j];
  }
  if (lane < n - tail) dst[tail + lane] = src[tail + lane];
}

template <typename T, int TIER>
__global__ void __launch_bounds__(kDynBlock) dyn_crb_kernel(const DynArgs<T> a) {
  __shared__ __attribute__((aligned(16))) T lds[kDynTierBytes[TIER]/(int)sizeof(T)];
  static_assert(kDynTierBytes[TIER] <= 65536, "the workspaces of a workgroup fit 64 KB of LDS");
  const int W = a.W, epb = kDynBlock/W, g = (int)threadIdx.x/W, nv = a.d.nv;
  const size_t B = (size_t)a.B, env = (size_t)blockIdx.x*epb + g;
  const bool live = env < B;
  const size_t le = live ? env : B - 1;      // (a group past the batch works on the last environment and stores nothing)
  const DynLayout L = dyn_layout(a.d.nb, nv, 0);
  T* ws = lds + (size_t)g*L.total;
  DynPar par = {(int)threadIdx.x % W, W};
  const DynTab<T> t = dyn_tab(a.d, a.ints, a.reals);
  dyn_frames(t, ws, L, [&](int adr) { return a.qpos[(size_t)adr*B + le]; }, [](int) {}, par);
  dyn_crb(t, ws, L, par);
  if (a.mode == DYN_MASS) {
    if (live) dyn_store_run(a.out + env*nv*nv, ws + L.M, nv*nv, par.lane, W);
    return;
  }
  if (a.mode == DYN_SOLVE) dyn_factor(ws, L, nv, par);
#pragma unroll 1
  for (int c0 = 0; c0 < a.K; c0 += kDynChunk) {
    const int kc = a.K - c0 < kDynChunk ? a.K - c0 : kDynChunk;
    const size_t at = (le*a.K + c0)*nv;
    dyn_load_run(ws + L.rhs, a.in + at, kc*nv, par.lane, W);
    DMC_WSYNC();
    if (a.mode == DYN_SOLVE) dyn_solve_chunk(ws, L, nv, kc, par);
    else dyn_mul_chunk(ws, L, nv, kc, par);
    if (live) dyn_store_run(a.out + at, ws + (a.mode == DYN_SOLVE ? L.rhs : L.res), kc*nv, par.lane, W);
    DMC_WSYNC();      // the chunk's workspace is free again
  }
}

template <typename T, int TIER>
__global__ void __launch_bounds__(kDynBlock) dyn_rne_kernel(const DynArgs<T> a) {
  __shared__ __attribute__((aligned(16))) T lds[kDynTierBytes[TIER]/(int)sizeof(T)];
  static_assert(kDynTierBytes[TIER] <= 65536, "the workspaces of a workgroup fit 64 KB of LDS");
  const int W = a.W, epb = kDynBlock/W, g = (int)threadIdx.x/W, nv = a.d.nv;
  const size_t B = (size_t)a.B, env = (size_t)blockIdx.x*epb + g;
  const bool live = env < B;
  const size_t le = live ? env : B - 1;
  const DynLayout L = dyn_layout(a.d.nb, nv, 1);
  T* ws = lds + (size_t)g*L.total;
  DynPar par = {(int)threadIdx.x % W, W};
  const DynTab<T> t = dyn_tab(a.d, a.ints, a.reals);
  dyn_frames(t, ws, L, [&](int adr) { return a.qpos[(size_t)adr*B + le]; },
             [&](int k) {
               ws[L.qvel + k] = a.qvel[(size_t)k*B + le];
               ws[L.qacc + k] = a.in ? a.in[le*a.in_se + k] : (T)0;
             }, par);
  dyn_rne(t, ws, L, par);
  if (live) dyn_store_run(a.out + env*nv, ws + L.res, nv, par.lane, W);
}

template <typename T>
static bool dyn_grid(const DynArgs<T>& a, int kind, dim3* grid, int* tier) {
  if (a.B < 1 || (a.W != 16 && a.W != 32 && a.W != 64) || a.d.nv < 1 || a.d.nv > kDynMaxDof || a.d.nb < 2) return false;
  const int epb = kDynBlock/a.W;
  const long long gx = ((long long)a.B + epb - 1)/epb;
  *tier = dyn_tier(a.d.nb, a.d.nv, kind, a.W, (int)sizeof(T));      // the smallest static LDS array the workspaces fit
  if (*tier < 0 || gx > 0x7fffffffLL) return false;
  *grid = dim3((unsigned)gx);
  return true;
}
template <typename T>
static int launch_dyn_crb(const DynArgs<T>& a, void* stream) {
  dim3 grid;
  int tier;
  if (!dyn_grid(a, 0, &grid, &tier) || a.mode < DYN_MASS || a.mode > DYN_SOLVE || (a.mode != DYN_MASS && (a.K < 1 || !a.in)) || !a.out) return -1;
  hipStream_t s = (hipStream_t)stream;
  if (tier == 0) hipLaunchKernelGGL((dyn_crb_kernel<T, 0>), grid, dim3(kDynBlock), 0, s, a);
  else if (tier == 1) hipLaunchKernelGGL((dyn_crb_kernel<T, 1>), grid, dim3(kDynBlock), 0, s, a);
  else hipLaunchKernelGGL((dyn_crb_kernel<T, 2>), grid, dim3(kDynBlock), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template <typename T>
static int launch_dyn_rne(const DynArgs<T>& a, void* stream) {
  dim3 grid;
  int tier;
  if (!dyn_grid(a, 1, &grid, &tier) || !a.out || a.in_se < 0) return -1;
  hipStream_t s = (hipStream_t)stream;
  if (tier == 0) hipLaunchKernelGGL((dyn_rne_kernel<T, 0>), grid, dim3(kDynBlock), 0, s, a);
  else if (tier == 1) hipLaunchKernelGGL((dyn_rne_kernel<T, 1>), grid, dim3(kDynBlock), 0, s, a);
  else hipLaunchKernelGGL((dyn_rne_kernel<T, 2>), grid, dim3(kDynBlock), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
int launch_dyn_crb_f32(const DynArgs<float>& a, void* stream) { return launch_dyn_crb<float>(a, stream); }
int launch_dyn_crb_f64(const DynArgs<double>& a, void* stream) { return launch_dyn_crb<double>(a, stream); }
int launch_dyn_rne_f32(const DynArgs<float>& a, void* stream) { return launch_dyn_rne<float>(a, stream); }
int launch_dyn_rne_f64(const DynArgs<double>& a, void* stream) { return launch_dyn_rne<double>(a, stream); }

}  // namespace dmc
