// con_kernels.hip -- batched contact wrenches (include/dmc_con.h): the world wrench of every contact slot and the net
// contact wrench on every target of every environment of a batch.  The arithmetic of one environment is con_core.h.
//
// Both kernels: one wave per workgroup, one environment per lane, so every read field[row*B + env] of the step kernels'
// structure-of-arrays outputs coalesces; nothing is computed twice and nothing crosses lanes.
//
// con_wrench_kernel, grid (ceil(B / 64), nconmax): slot c of every environment; zeros past the lane's ncon.  Every
// element of (B, nconmax, 6) is written.
// con_net_kernel, grid (ceil(B / 64), T): the target is uniform over the workgroup; its two masks (S, O) are staged in LDS
// once per workgroup (2 x words x 4 bytes, at most 2 KB).  A lane walks its OWN ncon contacts in index order, reads the
// two geom ids first and loads frame, force, position and distance only of the contacts that count; the sums are plain
// sequential arithmetic in registers: no atomic, no cross-lane reduction, the same bits on every launch.
//
// The outputs are torch-contiguous and environment-major, (B, T, 3) / (B, T) / (B, nconmax, 6), so a lane's stores are
// strided by the row of its environment.  They are plain strided stores: an environment's whole output is 9 reals and one
// int per target, a few bytes against the contact arrays the lane reads, and with the target on the grid's second axis a
// workgroup holds no run of memory longer than those few reals that a transposing tile could gather.
// A lane past the end of the batch loads nothing and stores nothing.
#include <hip/hip_runtime.h>

#include "con_core.h"

namespace dmc {

template <typename T>
__global__ void __launch_bounds__(kConBlock) con_wrench_kernel(const ConArgs<T> a) {
  const size_t env = (size_t)blockIdx.x*kConBlock + threadIdx.x;
  const int c = blockIdx.y;
  if (env >= a.in.B || c >= a.in.nconmax) return;
  T w[6];
  con_wrench(a.in, env, c, w);
  T* dst = a.wrench + (env*(size_t)a.in.nconmax + c)*6;
#pragma unroll
  for (int k = 0; k < 6; k++) dst[k] = w[k];
}

template <typename T>
__global__ void __launch_bounds__(kConBlock) con_net_kernel(const ConArgs<T> a) {
  __shared__ uint32_t mask[2*kConMaxWords];
  const int tid = threadIdx.x, t = blockIdx.y, W = a.words;
  for (int k = tid; k < 2*W; k += kConBlock) mask[k] = a.masks[(size_t)t*2*W + k];
  __syncthreads();
  const size_t env = (size_t)blockIdx.x*kConBlock + tid;
  if (env >= a.in.B) return;
  ConNet<T> o;
  con_net(a.in, env, mask, mask + W, a.head[kConHead*t], a.about, a.local != 0, &o);
  const size_t row = env*(size_t)a.ntarget + t;
  if (a.force) { for (int k = 0; k < 3; k++) a.force[row*3 + k] = o.force[k]; }
  if (a.torque) { for (int k = 0; k < 3; k++) a.torque[row*3 + k] = o.torque[k]; }
  if (a.normal) a.normal[row] = o.normal;
  if (a.count) a.count[row] = o.count;
  if (a.mindist) a.mindist[row] = o.dist;
}

template <typename T>
static bool con_grid(const ConArgs<T>& a, int ny, dim3* grid) {
  const long long gx = ((long long)a.in.B + kConBlock - 1)/kConBlock;
  if (a.in.B < 1 || ny < 1 || ny > 65535 || gx > 0x7fffffffLL || a.words < 1 || a.words > kConMaxWords) return false;
  *grid = dim3((unsigned)gx, (unsigned)ny);
  return true;
}
template <typename T>
static int launch_con_wrench(const ConArgs<T>& a, void* stream) {
  dim3 grid;
  if (!a.wrench || !con_grid(a, a.in.nconmax, &grid)) return -1;
  hipLaunchKernelGGL((con_wrench_kernel<T>), grid, dim3(kConBlock), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
template <typename T>
static int launch_con_net(const ConArgs<T>& a, void* stream) {
  dim3 grid;
  if (a.ntarget > kConMaxTargets || !con_grid(a, a.ntarget, &grid)) return -1;
  hipLaunchKernelGGL((con_net_kernel<T>), grid, dim3(kConBlock), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
int launch_con_wrench_f32(const ConArgs<float>& a, void* stream) { return launch_con_wrench<float>(a, stream); }
int launch_con_wrench_f64(const ConArgs<double>& a, void* stream) { return launch_con_wrench<double>(a, stream); }
int launch_con_net_f32(const ConArgs<float>& a, void* stream) { return launch_con_net<float>(a, stream); }
int launch_con_net_f64(const ConArgs<double>& a, void* stream) { return launch_con_net<double>(a, stream); }

}  // namespace dmc
