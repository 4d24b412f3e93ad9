// dist_kernels.hip -- batched geom distances (dmc_dist_query): mj_geomDistance for every (environment, pair) of a batch
// from the geom poses a step / forward launch left in HBM.  See dist_core.h for the model.
//
// dist_kernel: one launch per query, one lane per (environment, pair) with the environment fastest, so that the SoA pose
// loads geom_xpos[(3 g + k) B + env] coalesce; where B is a multiple of 64 a wave shares one pair, its member lists and
// its geom types, so the dispatch on the types is wave-uniform and only the iteration counts diverge.  A member given as
// a body is a list of geoms: the lane walks the list pairs and keeps the smallest distance (the first on a tie).
//
// A pair of convex geoms is solved in the frame of the first: that one is a type and a size in registers, the second
// one's size and relative pose (15 reals) is staged in the lane's LDS slice, element e at [e 64 + lane], and read where a
// support point needs it -- a fp64 pair held in registers for the whole solve spills.  The first geom's pose is loaded
// again for the way back to the world frame.
//
// The EPA polytope of a lane lives in LDS too, never in private memory.  One that can hold the 50 iterations of the
// default options takes 2664 B (fp64) / 1552 B (fp32): 64 of them do not fit 64 KB.  Only lanes whose cores overlap need
// one, so the workgroup is one wave and runs those lanes in passes of K = DistCaps<T>::K (21 / 39): the lanes are ranked
// with a ballot, lane r of a pass owns slice r, element e of it at [e K + r] -- consecutive lanes, consecutive banks.
// One wave executes its LDS accesses in order, so the passes need no workgroup barrier (wave barriers fence them for the compiler).  63624 B / 64368 B of static LDS (63632 / 64384 with the compiler's padding).
#include <hip/hip_runtime.h>

#include "dist_core.h"

namespace dmc {

template <typename T>
__device__ __forceinline__ void dist_load_geom(const DistArgs<T>& a, int g, size_t env, DistGeom<T>* o) {
  const size_t B = a.B;
  const int slot = a.eg_slot ? a.eg_slot[g] : -1;
  o->type = a.geom_type[g];
#pragma unroll
  for (int k = 0; k < 3; k++) o->pos[k] = a.geom_xpos[(size_t)(3*g + k)*B + env];
#pragma unroll
  for (int k = 0; k < 9; k++) o->mat[k] = a.geom_xmat[(size_t)(9*g + k)*B + env];
  // size in force: the environment's own where the geom was declared per environment, else the live model table
#pragma unroll
  for (int k = 0; k < 3; k++) o->size[k] = slot >= 0 ? a.eg_data[(size_t)(16*slot + 12 + k)*B + env] : a.geom_size[3*g + k];
}

template <typename T>
struct DistGeomLds {      // the staged second geom: volatile, so that each use is a load and not a register held since the staging
  typedef T real;
  static constexpr bool kOrigin = false;
  const volatile T* base;      // the lane's slice: size 0..2, pos 3..5, mat 6..14
  int type;
  __device__ __forceinline__ int ty() const { return type; }
  __device__ __forceinline__ T sz(int k) const { return base[k*kDistBlock]; }
  __device__ __forceinline__ T ps(int k) const { return base[(3 + k)*kDistBlock]; }
  __device__ __forceinline__ T mt(int k) const { return base[(6 + k)*kDistBlock]; }
};

template <typename T>
__global__ void __launch_bounds__(kDistBlock) dist_kernel(const DistArgs<T> a) {
  constexpr int V = DistCaps<T>::V, F = DistCaps<T>::F, K = DistCaps<T>::K;
  __shared__ T s_vtx[3*V*K];
  __shared__ T s_fdist[F*K];
  __shared__ int s_fidx[F*K];
  __shared__ T s_geom[kDistGeomReals*kDistBlock];
  static_assert(sizeof(T)*((3*V + F)*K + kDistGeomReals*kDistBlock) + sizeof(int)*F*K <= 65536, "the polytopes of one pass and the staged geoms fit 64 KB of LDS");
  static_assert(kDistBlock == 64, "one wave: the ballot ranks the whole workgroup and LDS passes need no barrier");
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x*kDistBlock + tid, total = (long long)a.B*a.npair;
  if (i >= total) return;      // the last wave is ragged; no barrier follows
  const size_t env = (size_t)(i % a.B);
  const int pair = (int)(i / a.B);
  const int adr1 = a.adr[4*pair], n1 = a.adr[4*pair + 1], adr2 = a.adr[4*pair + 2], n2 = a.adr[4*pair + 3];
  const T distmax = a.distmax[pair];
  const size_t o = env*a.npair + pair, B = a.B;
  T best = distmax;      // the outputs are written as a smaller distance is found: nothing but it is carried
  if (a.fromto) {
#pragma unroll
    for (int k = 0; k < 6; k++) a.fromto[6*o + k] = 0;
  }
  if (a.normal) {
#pragma unroll
    for (int k = 0; k < 3; k++) a.normal[3*o + k] = 0;
  }
  int flags = 0;
  for (int j1 = 0; j1 < n1; j1++) {
    const int id1 = a.member[adr1 + j1];
    for (int j2 = 0; j2 < n2; j2++) {
      DistResult<T> r;
      bool convex;
      DistGeomOrigin<T> ga;
      DistGeomLds<T> gb;
      gb.base = s_geom + tid;
      {
        DistGeom<T> g1, g2, rel;
        dist_load_geom(a, id1, env, &g1);
        dist_load_geom(a, a.member[adr2 + j2], env, &g2);
        convex = !dist_pair_plane(g1, g2, distmax, &r);
        dist_relative(g1, g2, &ga, &rel);
        gb.type = rel.type;
        if (convex) {
#pragma unroll
          for (int k = 0; k < 3; k++) { s_geom[k*kDistBlock + tid] = rel.size[k]; s_geom[(3 + k)*kDistBlock + tid] = rel.pos[k]; }
#pragma unroll
          for (int k = 0; k < 9; k++) s_geom[(6 + k)*kDistBlock + tid] = rel.mat[k];
        }
      }
      if (convex) {
        dist_pair_convex(ga, gb, distmax, a.tolerance, a.iterations, [&](const DistSimplex<T>& s, const DistSetup<T>& u) {
          // the lanes that are here are the ones whose cores overlap: rank them, K per pass.  (Should the overlap lanes of
          // a wave not have reconverged here, each subset ballots for itself and the subsets run one after another -- a
          // subset is done with its slices before the next one starts, so sharing them stays safe.)
          const unsigned long long need = __ballot(1);
          const int rank = __popcll(need & ((1ull << tid) - 1)), npass = (__popcll(need) + K - 1)/K;
          DistEpaMem<T> mem;
          mem.vtx = s_vtx + rank % K; mem.fdist = s_fdist + rank % K; mem.fidx = s_fidx + rank % K; mem.stride = K;
          DistEpaOut<T> e;
          e.status = 1; e.depth = 0; e.nrm = dv((T)0, (T)0, (T)1); e.flat = true;
#pragma unroll 1
          for (int pass = 0; pass < npass; pass++) {
            // a wave barrier on either side of a pass: a convergent operation the optimiser may not move the solve across,
            // so that lanes r and r + K can never be folded into one pass on the slice they share
            __builtin_amdgcn_wave_barrier();
            if (rank/K == pass) e = dist_epa(ga, gb, u.scale, u.tol, u.tol_user, a.iterations, s, mem);
            __builtin_amdgcn_wave_barrier();
          }
          return e;
        }, &r);
        // back to the world with the first geom's pose, loaded again (the fence keeps the two loads apart)
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        T p1[3], m1[9];
#pragma unroll
        for (int k = 0; k < 3; k++) p1[k] = a.geom_xpos[(size_t)(3*id1 + k)*B + env];
#pragma unroll
        for (int k = 0; k < 9; k++) m1[k] = a.geom_xmat[(size_t)(9*id1 + k)*B + env];
        dist_to_world(p1, m1, distmax, &r);
      }
      flags |= (r.status != 0) | r.epa << 1;
      if (r.dist < best) {
        best = r.dist;
        if (a.fromto) {
          a.fromto[6*o] = r.from.x; a.fromto[6*o + 1] = r.from.y; a.fromto[6*o + 2] = r.from.z;
          a.fromto[6*o + 3] = r.to.x; a.fromto[6*o + 4] = r.to.y; a.fromto[6*o + 5] = r.to.z;
        }
        if (a.normal) {
          a.normal[3*o] = r.normal.x; a.normal[3*o + 1] = r.normal.y; a.normal[3*o + 2] = r.normal.z;
        }
      }
    }
  }
  if (a.dist) a.dist[o] = best;
  if (a.status) a.status[o] = flags;
}

template <typename T>
static int launch_dist(const DistArgs<T>& a, void* stream) {
  const long long grid = ((long long)a.B*a.npair + kDistBlock - 1)/kDistBlock;
  if (a.B < 1 || a.npair < 1 || grid <= 0 || grid > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL((dist_kernel<T>), dim3((unsigned)grid), dim3(kDistBlock), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
int launch_dist_f32(const DistArgs<float>& a, void* stream) { return launch_dist<float>(a, stream); }
int launch_dist_f64(const DistArgs<double>& a, void* stream) { return launch_dist<double>(a, stream); }

}  // namespace dmc
