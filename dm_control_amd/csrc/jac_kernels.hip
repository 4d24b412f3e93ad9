// jac_kernels.hip -- batched Jacobians (include/dmc_jac.h): mj_jac, J qvel and J' f for every (environment, target) of
// a batch.  The arithmetic of one (environment, target) is jac_core.h.
//
// All three kernels: one wave per workgroup, one environment per lane, the target uniform over the workgroup -- the
// chain tables are read at uniform addresses and the SoA state loads qpos[a B + env] coalesce.  What the kinematics are
// computed from is the qpos in device memory: no pose array is read, so nothing can be stale.
//
// jac_kernel, grid (ceil(B / 64), T).  The outputs are torch-contiguous (B, T, 3, C): a lane that stored its own rows
// would write 8 or 4 bytes every 6 C reals.  Instead the columns go through LDS in chunks of 16 (fp64) / 32 (fp32)
// columns: tile[(row, column), lane] with a lane stride of 65, written by the lane that walks the chain, read back
// transposed so that consecutive lanes store consecutive addresses of one (environment, row) run of the chunk -- 128
// bytes per run, 16 bytes per lane where the bases and C allow; which (row, column) a lane stores is the same for every
// environment and worked out once per chunk.  The chunk bounds the static LDS at 49920 B whatever C is; the price is one
// more walk per chunk that holds a chain dof.  A chunk no chain dof falls in (most of them for a
// model of many free bodies) is stored as zeros without a walk.  Every element of the outputs is written.
//
// jac_vel_kernel, same grid: two walks, six sums in registers, (B, T, 6) through a small tile.
// jac_force_kernel, grid ceil(B / epb): a lane takes its environment through the targets IN ORDER and adds each one's
// J' f into its own C accumulators in LDS (runtime-indexed by the column, so never registers): plain sequential sums, no
// atomics, the same bits on every launch.  epb = min(64, 60 KB / (C reals)) environments share a workgroup.
#include <hip/hip_runtime.h>

#include "jac_core.h"

namespace dmc {

template <typename T, int P>
struct alignas(sizeof(T)*P) JacVec { T v[P]; };

// A chunk leaves the workgroup: per environment it is 6 runs (3 rows of jacp, 3 of jacr) of w columns, and consecutive
// lanes store consecutive addresses of a run, P reals each.  A lane's share of one environment -- the (row, column) of
// its elements -- is the same for every environment, so it is worked out once and the loop over the environments holds no
// division.  row0 = (env0 T + t) 3: the first output row of the workgroup's first environment.
template <typename T, int P>
__device__ __forceinline__ void jac_flush(const JacArgs<T>& a, const T* tile, bool any, size_t row0, int nenv, int c0, int w, int tid) {
  constexpr int CH = JacTile<T>::kChunk, K = (6*CH/P + kJacBlock - 1)/kJacBlock;
  const int wp = w/P, n1 = 6*wp, C = a.ncol;
  int lds[K], off[K];
  T* dst[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int f = tid + k*kJacBlock;
    const bool ok = f < n1;
    const int r = ok ? f/wp : 0, cc = ok ? (f % wp)*P : 0;
    dst[k] = ok ? (r < 3 ? a.jacp : a.jacr) : nullptr;
    lds[k] = (r*CH + cc)*kJacPad;
    off[k] = (r % 3)*C + c0 + cc;
  }
  const size_t estride = (size_t)a.ntarget*3*C;
  for (int e = 0; e < nenv; e++) {
#pragma unroll
    for (int k = 0; k < K; k++) {
      if (!dst[k]) continue;
      JacVec<T, P> o;
#pragma unroll
      for (int j = 0; j < P; j++) o.v[j] = any ? tile[lds[k] + j*kJacPad + e] : (T)0;
      *reinterpret_cast<JacVec<T, P>*>(dst[k] + row0*C + e*estride + off[k]) = o;
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(kJacBlock) jac_kernel(const JacArgs<T> a) {
  constexpr int CH = JacTile<T>::kChunk, V = 16/(int)sizeof(T);
  __shared__ __attribute__((aligned(16))) T tile[6*CH*kJacPad];
  static_assert(sizeof(T)*6*CH*kJacPad <= 65536, "the transposing tile fits 64 KB of LDS");
  const int tid = threadIdx.x, t = blockIdx.y;
  const size_t B = (size_t)a.B, env0 = (size_t)blockIdx.x*kJacBlock, env = env0 + tid;
  const int nenv = (int)(B - env0 < (size_t)kJacBlock ? B - env0 : (size_t)kJacBlock);
  const bool live = env < B;
  const size_t le = live ? env : env0;      // (a lane past the batch reads nothing and writes nothing)
  const JacChain<T> ch = jac_chain(a.head, a.ints, a.reals, t);
  const int* dcol = ch.ints + 2*ch.d.nb + 3*ch.d.nj + ch.d.nd;
  const int C = a.ncol, nt = a.ntarget;
  auto q = [&](int adr) { return a.qpos[(size_t)adr*B + le]; };
  T p[3] = {0, 0, 0};
  if (live) {
    if (a.point) { for (int k = 0; k < 3; k++) p[k] = a.point[(env*nt + t)*3 + k]; }
    else { T tq[4]; jac_target(ch, q, p, tq); }
  }
#pragma unroll 1
  for (int c0 = 0; c0 < C; c0 += CH) {
    const int w = C - c0 < CH ? C - c0 : CH;
    bool any = false;      // uniform: does a chain dof of this target fall in the chunk?
    for (int c = 0; c < ch.d.nd; c++) { const int col = dcol[c]; any = any || (col >= c0 && col < c0 + w); }
    if (any) {
      for (int k = 0; k < 6*CH; k++) tile[k*kJacPad + tid] = 0;
      if (live) {
        jac_columns(ch, q, (const T*)p, [&](int, int col, const T* jp, const T* jr) {
          if (col < c0 || col >= c0 + w) return;
          for (int k = 0; k < 3; k++) {
            tile[(k*CH + col - c0)*kJacPad + tid] = jp[k];
            tile[((3 + k)*CH + col - c0)*kJacPad + tid] = jr[k];
          }
        });
      }
      __syncthreads();
    }
    // out of the workgroup, 16 bytes per lane where the bases and C allow
    if (a.vec) jac_flush<T, V>(a, tile, any, (env0*nt + t)*3, nenv, c0, w, tid);
    else jac_flush<T, 1>(a, tile, any, (env0*nt + t)*3, nenv, c0, w, tid);
    if (any) __syncthreads();      // the tile is free again
  }
}

template <typename T>
__global__ void __launch_bounds__(kJacBlock) jac_vel_kernel(const JacArgs<T> a) {
  __shared__ T tile[6*kJacPad];
  const int tid = threadIdx.x, t = blockIdx.y;
  const size_t B = (size_t)a.B, env0 = (size_t)blockIdx.x*kJacBlock, env = env0 + tid;
  const int nenv = (int)(B - env0 < (size_t)kJacBlock ? B - env0 : (size_t)kJacBlock);
  if (env < B) {
    const JacChain<T> ch = jac_chain(a.head, a.ints, a.reals, t);
    T res[6];
    jac_velocity(ch, [&](int adr) { return a.qpos[(size_t)adr*B + env]; }, [&](int dof) { return a.qvel[(size_t)dof*B + env]; },
                 a.local != 0, res);
#pragma unroll
    for (int k = 0; k < 6; k++) tile[k*kJacPad + tid] = res[k];
  }
  __syncthreads();
  for (int f = tid; f < nenv*6; f += kJacBlock) {
    const int e = f/6, k = f % 6;
    a.vel[((env0 + e)*a.ntarget + t)*6 + k] = tile[k*kJacPad + e];
  }
}

template <typename T>
__global__ void __launch_bounds__(kJacBlock) jac_force_kernel(const JacArgs<T> a) {
  __shared__ T acc[kJacForceLds/(int)sizeof(T)];
  const int tid = threadIdx.x, epb = a.epb, C = a.ncol;
  const size_t B = (size_t)a.B, env0 = (size_t)blockIdx.x*epb, env = env0 + tid;
  const int nenv = (int)(B - env0 < (size_t)epb ? B - env0 : (size_t)epb);
  if (tid < epb && env < B) {
    for (int c = 0; c < C; c++) acc[c*epb + tid] = 0;
#pragma unroll 1
    for (int t = 0; t < a.ntarget; t++) {
      const JacChain<T> ch = jac_chain(a.head, a.ints, a.reals, t);
      T f[3] = {0, 0, 0}, tau[3] = {0, 0, 0};
      if (a.force) for (int k = 0; k < 3; k++) f[k] = a.force[env*a.f_se + t*a.f_st + k];
      if (a.torque) for (int k = 0; k < 3; k++) tau[k] = a.torque[env*a.t_se + t*a.t_st + k];
      jac_force(ch, [&](int adr) { return a.qpos[(size_t)adr*B + env]; }, (const T*)f, (const T*)tau,
                [&](int col, T v) { acc[col*epb + tid] += v; });
    }
  }
  __syncthreads();
  const int n = nenv*C;      // the workgroup's rows of (B, C) are one run of memory
  for (int f = tid; f < n; f += kJacBlock) a.qfrc[env0*C + f] = acc[(f % C)*epb + f/C];
}

template <typename T>
static bool jac_grid(const JacArgs<T>& a, int per, dim3* grid, bool by_target) {
  const long long gx = ((long long)a.B + per - 1)/per;
  if (a.B < 1 || a.ntarget < 1 || a.ncol < 1 || per < 1 || gx > 0x7fffffffLL || a.ntarget > 65535) return false;
  *grid = dim3((unsigned)gx, by_target ? (unsigned)a.ntarget : 1u);
  return true;
}
template <typename T>
static int launch_jac(const JacArgs<T>& a, void* stream) {
  dim3 grid;
  if (!jac_grid(a, kJacBlock, &grid, true)) return -1;
  hipLaunchKernelGGL((jac_kernel<T>), grid, dim3(kJacBlock), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template <typename T>
static int launch_jac_vel(const JacArgs<T>& a, void* stream) {
  dim3 grid;
  if (!jac_grid(a, kJacBlock, &grid, true)) return -1;
  hipLaunchKernelGGL((jac_vel_kernel<T>), grid, dim3(kJacBlock), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template <typename T>
static int launch_jac_force(const JacArgs<T>& a, void* stream) {
  dim3 grid;
  if (a.epb < 1 || a.epb > kJacBlock || (long long)a.epb*a.ncol*(int)sizeof(T) > kJacForceLds) return -1;
  if (!jac_grid(a, a.epb, &grid, false)) return -1;
  hipLaunchKernelGGL((jac_force_kernel<T>), grid, dim3(kJacBlock), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
int launch_jac_f32(const JacArgs<float>& a, void* stream) { return launch_jac<float>(a, stream); }
int launch_jac_f64(const JacArgs<double>& a, void* stream) { return launch_jac<double>(a, stream); }
int launch_jac_vel_f32(const JacArgs<float>& a, void* stream) { return launch_jac_vel<float>(a, stream); }
int launch_jac_vel_f64(const JacArgs<double>& a, void* stream) { return launch_jac_vel<double>(a, stream); }
int launch_jac_force_f32(const JacArgs<float>& a, void* stream) { return launch_jac_force<float>(a, stream); }
int launch_jac_force_f64(const JacArgs<double>& a, void* stream) { return launch_jac_force<double>(a, stream); }

}  // namespace dmc
