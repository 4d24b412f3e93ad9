// lin_kernels.hip -- batched linearisation of the step (include/dmc_lin.h): the fan-out of a chunk of environments into
// the perturbed columns of a scratch batch, and the differencing of the stepped columns into A, B, C, D.  The arithmetic
// of one column is lin_core.h; the step in between is the scratch batch's own launch, untouched.
//
// Layout.  The scratch environment of (environment e of the chunk, column c) is e P + c, and a batch field is SoA
// (rows, Bscratch): for a fixed row the columns of one environment are contiguous.  Both kernels run one column per lane
// over the flat index e P + c (fan-out) or e n + j (difference, n = nx + nu inputs), so
//   * the fan-out's stores scr[row Bs + e P + c] are consecutive over the lanes; its loads src[row B + e] hit one address
//     per environment (a broadcast within the wave),
//   * the difference's loads scr[row Bs + e P + 1 + j] (and the minus column's, n further on) are consecutive, and so are
//     its stores A[e, i, j]: row-major outputs need no transposition.
// Every loop bound is uniform over the lanes (the joint table, nv, na, nu, nsensordata); only the few rows a column
// perturbs diverge.  No LDS, no private arrays indexed at run time.
//
// Precision pairs <Ts source and outputs, Tc scratch>: (double, double), (float, double), (float, float).  All arithmetic
// is in Tc (the range test of a clamped control compares in fp64); loads convert up, the stores of A .. D convert down.
//
// The per-environment warning mask is the one reduction across lanes: the warning counters of an environment's columns are
// ORed into warn[e] with atomicOr -- integer and commutative, so the result does not depend on the order.
#include <hip/hip_runtime.h>

#include "lin_core.h"

namespace dmc {

template <typename Ts, typename Tc>
struct LinFanIO {
  const LinArgs<Ts, Tc>& a;
  size_t es, cs;      // the environment in the source batch, the column in the scratch batch
  __device__ __forceinline__ Tc load(int f, int row) const { return (Tc)a.src[f][(size_t)row*a.B + es]; }
  __device__ __forceinline__ void store(int f, int row, Tc v) const { a.scr[f][(size_t)row*a.Bs + cs] = v; }
  __device__ __forceinline__ void copy(int f, int row) const { store(f, row, load(f, row)); }
  __device__ __forceinline__ void flags(int k, int v) const { a.flags[es*a.d.nu + k] = v; }
  __device__ __forceinline__ void rest() const {
    a.scr_time[cs] = a.src_time[es];
    for (int w = 0; w < DMC_NWARNING; w++) a.scr_warning[(size_t)w*a.Bs + cs] = 0;
  }
};

template <typename Ts, typename Tc>
__global__ void __launch_bounds__(kLinBlock) lin_fan_out(const LinArgs<Ts, Tc> a) {
  const size_t tid = (size_t)blockIdx.x*kLinBlock + threadIdx.x;
  if (tid >= (size_t)a.nenv*a.P) return;
  const int e = (int)(tid/a.P), c = (int)(tid - (size_t)e*a.P);
  const LinFanIO<Ts, Tc> io = {a, (size_t)a.first_env + e, tid};
  if (c == 0) a.warn[io.es] = 0;
  lin_fan_column<Tc>(a.d, lin_tab(a.d, a.ints, a.reals), c, a.eps, a.ch, a.sh, io);
}

template <typename Ts, typename Tc>
struct LinDiffIO {
  const LinArgs<Ts, Tc>& a;
  size_t es, c0;      // the environment in the source batch, its nominal column in the scratch batch
  int in, nx;
  __device__ __forceinline__ Tc x(int f, int row, int col) const { return a.scr[f][(size_t)row*a.Bs + c0 + col]; }
  __device__ __forceinline__ void out(int row, Tc v) const {
    if (in < nx) a.A[(es*nx + row)*nx + in] = (Ts)v;
    else a.Bm[(es*nx + row)*a.d.nu + (in - nx)] = (Ts)v;
  }
  __device__ __forceinline__ void sens(int row, Tc v) const {
    if (in < nx) a.C[(es*a.d.nsensordata + row)*nx + in] = (Ts)v;
    else a.D[(es*a.d.nsensordata + row)*a.d.nu + (in - nx)] = (Ts)v;
  }
  __device__ __forceinline__ int warned(int col) const {
    int m = 0;
    for (int w = 0; w < DMC_NWARNING; w++) m |= (a.scr_warning[(size_t)w*a.Bs + c0 + col] != 0) << w;
    return m;
  }
};

template <typename Ts, typename Tc>
__global__ void __launch_bounds__(kLinBlock) lin_difference(const LinArgs<Ts, Tc> a) {
  const int n = lin_nin(a.d), nx = lin_nx(a.d);
  const size_t tid = (size_t)blockIdx.x*kLinBlock + threadIdx.x;
  if (tid >= (size_t)a.nenv*n) return;
  const int e = (int)(tid/n), in = (int)(tid - (size_t)e*n);
  const LinDiffIO<Ts, Tc> io = {a, (size_t)a.first_env + e, (size_t)e*a.P, in, nx};
  const int flags = in < nx ? (LIN_FWD | (a.d.centered ? LIN_BACK : 0)) : a.flags[io.es*a.d.nu + (in - nx)];
  lin_diff_column<Tc>(a.d, lin_tab(a.d, a.ints, a.reals), in, flags, a.eps, a.C != nullptr, io);
  // the warnings of the columns this lane read or left unread: its plus column, its minus column where one exists, and
  // (input 0) the nominal one
  int m = io.warned(1 + in);
  if (a.d.centered || in >= nx) m |= io.warned(lin_minus_col(a.d, in));
  if (in == 0) m |= io.warned(0);
  if (m) atomicOr(a.warn + io.es, m);
}

template <typename Ts, typename Tc>
static int lin_launch(const LinArgs<Ts, Tc>& a, int which, void* stream) {
  const long long items = (long long)a.nenv*(which ? lin_nin(a.d) : a.P), gx = (items + kLinBlock - 1)/kLinBlock;
  if (a.nenv < 1 || a.P != lin_ncol(a.d) || (long long)a.nenv*a.P > a.Bs || a.first_env < 0 ||
      (long long)a.first_env + a.nenv > a.B || gx < 1 || gx > 0x7fffffffLL) return -1;
  if (which) hipLaunchKernelGGL((lin_difference<Ts, Tc>), dim3((unsigned)gx), dim3(kLinBlock), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((lin_fan_out<Ts, Tc>), dim3((unsigned)gx), dim3(kLinBlock), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
int launch_lin_f64_f64(const LinArgs<double, double>& a, int which, void* stream) { return lin_launch(a, which, stream); }
int launch_lin_f32_f64(const LinArgs<float, double>& a, int which, void* stream) { return lin_launch(a, which, stream); }
int launch_lin_f32_f32(const LinArgs<float, float>& a, int which, void* stream) { return lin_launch(a, which, stream); }

}  // namespace dmc
