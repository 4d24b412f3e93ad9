// step_dense.h -- dense factorisations of the step core: packed-triangle indexing, the Cholesky factor / solve routines
// in LDS, in registers (one lane per row), over the kinematic trees and on the matrix cores (CholTiles; device unit
// test: scripts/chol_mfma_probe.hip).
#pragma once
#include "step_defs.h"
#include "step_math.h"
#include "step_lanes.h"

namespace dmc {
// ---------------------------------------------------------------------------
// out-of-line LDS routines shared by several call sites
// ---------------------------------------------------------------------------
// Symmetric n x n matrices (the factor of M, H = M + J'DJ and its factor) are stored as their lower
// triangle packed BY COLUMNS: entry (i, j), i >= j, lives at tri_c0(j, n) + i - j.  Column k is
// contiguous, and the entries a right-looking Cholesky still has to touch at step k are a suffix.
DMC_DEV int tri_c0(int j, int n) { return j*n - ((j*(j - 1)) >> 1); }
DMC_DEV int tri_at(int i, int j, int n) { return tri_c0(j, n) + i - j; }
// inverse of tri_at for a packed index t of an m x m triangle: column j and row i
DMC_DEV void tri_unrank(int t, int m, int* i, int* j) {
  const float b = (float)(2*m + 1);
  int c = (int)((b - sqrtf(b*b - 8.0f*(float)t)) * 0.5f);
  c = c < 0 ? 0 : (c > m - 1 ? m - 1 : c);
  if (tri_c0(c, m) > t) c--;
  else if (c + 1 < m && tri_c0(c + 1, m) <= t) c++;
  *j = c; *i = c + (t - tri_c0(c, m));
}
// In-place Cholesky of a packed lower triangle, same operation order as the oracle.  On exit: strict
// lower part = L, diagonal = 1/L[k][k].  Two wave fences per column: scale column k, then every
// remaining entry (i, j), j > k, is updated by one lane with  A[i][j] -= L[i][k] L[j][k].
// a - b c: in the fp32 kernels ONE fused operation, said explicitly -- left to the contraction pass, the SLP vectoriser first
// pairs the products of neighbouring columns into v_pk_mul_f32 and the fusion is lost (two moves, a packed product and two
// subtractions where two FMAs do); in fp64 the two roundings of the oracle.
// (FUSE: the small row routines, N <= 16; the larger ones keep the expression the compiler has always seen -- on the 27-dof
// model the explicit form bought nothing and moved the mean iteration count, profiles/r05_s7_ab_large_models.log)
template <bool FUSE, typename T> DMC_DEV T nmsub(T a, T b, T c) {
#ifndef DMC_HOST_EMU
  if constexpr (FUSE && sizeof(T) == 4) return __builtin_fmaf(-b, c, a);
#endif
  return a - b * c;
}
#ifndef DMC_HOST_EMU
// Row-per-lane factor -> the packed triangle (column j at tri_c0(j, N), rows j .. N-1): lane i holds (i, j) for j <= i.
// Stored WITHOUT a predicate per column: the columns go out last to first, and a lane above the diagonal (i < j) aims
// its don't-care value at tri_c0(j, N) + i - j -- a slot of an EARLIER column (>= 0 because tri_c0(j, N) >= j), which that
// column's own store, issued later by the same wave, overwrites with the entry that belongs there.  One exec mask for
// the N row-holding lanes instead of a compare / mask / branch / restore sequence per column (9 x 8 instructions on the
// 9-dof model, a quarter of the factorisation).
template <typename T, int N> DMC_DEV void store_factor_rows(DMC_LDS T* A, const T* a, int lane) {
  if (lane < N) {
#pragma unroll
    for (int j = N - 1; j >= 0; j--) { A[tri_c0(j, N) + lane - j] = a[j]; asm volatile("" ::: "memory"); }      // (in THIS order: to one lane the nine addresses are unrelated)
  }
}
#endif
template <typename T, int LPE>
DMC_FN void chol_factor_lds(DMC_LDS T* A, int n, int lane) {
  const int ntri = (n*(n + 1)) >> 1;
  for (int k = 0; k < n; k++) {
    DMC_WSYNC();
    const int ck = tri_c0(k, n);
    T akk = A[ck];
    if (akk < (T)DMC_MINVAL) akk = (T)DMC_MINVAL;
    const T inv = t_rsqrt(akk);
    for (int i = k + 1 + lane; i < n; i += LPE) A[ck + i - k] *= inv;
    DMC_WSYNC();
    if (lane == 0) A[ck] = inv;
    const int c1 = ck + n - k, m = n - k - 1;   // trailing (n-k-1) x (n-k-1) triangle starts at c1
    for (int t = lane; t < ntri - c1; t += LPE) {
      int ii, jj;
      tri_unrank(t, m, &ii, &jj);
      A[c1 + t] -= A[ck + 1 + ii] * A[ck + 1 + jj];
    }
  }
  DMC_WSYNC();
}
// Model-specialised kernels know nv at compile time: lane i of the group keeps row i of the
// matrix in N registers, pivots and scaled columns travel by v_readlane -- no LDS round trip
// and no fence per column (N = 27: ~1.1 k instructions instead of 27 fenced LDS sweeps).
// Same arithmetic per entry, in the same order, as chol_factor_lds: identical results.
#ifndef DMC_HOST_EMU
template <typename T, int LPE, int N>
DMC_FN void chol_factor_rows(DMC_LDS T* A, int lane) {
  static_assert(N >= 1 && N <= LPE, "one lane per matrix row");
  DMC_WSYNC();
  T a[N];
  const bool own = lane < N;
#pragma unroll
  for (int j = 0; j < N; j++) {      // (N <= 16: unpredicated loads, the value selected afterwards -- a predicated load costs an exec-mask round trip each)
    if constexpr (N > 16) a[j] = (own && j <= lane) ? A[tri_c0(j, N) + lane - j] : (T)0;      // (27 dofs: 3 % faster predicated -- half the reads)
    else {
      const int i_ = own && j <= lane ? lane : j;
      const T v = A[tri_c0(j, N) + i_ - j];
      a[j] = (own && j <= lane) ? v : (T)0;
    }
  }
#pragma unroll
  for (int k = 0; k < N; k++) {
    T akk = bcast_rows<LPE, N>(a[k], k);
    if (akk < (T)DMC_MINVAL) akk = (T)DMC_MINVAL;
    const T inv = t_rsqrt(akk);
    const T lik = a[k] * inv;
#pragma unroll
    for (int j = k + 1; j < N; j++) { const T ljk = bcast_rows<LPE, N>(lik, j); a[j] = nmsub<(N <= 16)>(a[j], lik, ljk); }
    a[k] = lane == k ? inv : lik;
  }
  store_factor_rows<T, N>(A, a, lane);
  DMC_WSYNC();
}
#endif
// The same factorisation on the MATRIX CORES for the large fp32 models (32 < N <= 64, one environment per wave): blocked
// right-looking U'U on 16 x 16 tiles held in the accumulator layout of v_mfma_f32_16x16x4_f32 -- lane 16 g + c, register r
// of a tile = its element (4 g + r, c).  Fed as BOTH operands, register by register, two tiles X, Y in that layout give
// X'Y (operand A reads lane l as A[l & 15][l >> 4], operand B as B[l >> 4][l & 15]: register r of X is X'[i][4 k + r],
// register r of Y is Y[4 k + r][j], and the four instructions r = 0 .. 3 cover the sixteen k) -- which is the trailing update
// A_ij -= U_ki' U_kj of the upper-triangular form, in place, with no layout conversion: 40 matrix instructions do what
// 1 891 v_readlane + v_fma pairs do in chol_factor_rows<62>.  The sixteen columns of a diagonal tile are eliminated on
// the vector ALU, together with the rest of their block row (which is the panel solve): the pivot comes by v_readlane,
// the column below it by DPP row_newbcast (the diagonal tile is kept whole and symmetric, so column C0 of a row group is
// lane C0 of that row group), the scaled pivot row reaches the other row groups through one ds_bpermute per tile; rows at
// or above the pivot get a zero multiplier instead of a predicate.  Rows / columns N .. 63 enter as the identity.  The
// packed triangle leaves as chol_factor_rows leaves it (scaled columns, 1 / L_kk on the diagonal); the sums run in another
// order (the products of a tile update are added k-slot by k-slot), so the factor differs from chol_factor_rows' by
// rounding.  Measured (scripts/chol_mfma_probe.hip, profiles/r06_chol_mfma_probe.log): 2 191 instructions against 5 118,
// 17.0 k cycles per factorisation against 38.9 k with five waves per CU.
#if !defined(DMC_HOST_EMU)
typedef float dmc_f4 __attribute__((ext_vector_type(4)));
template <int N> struct CholTiles {
  static constexpr int NB = (N + 15) / 16;
  struct LaneInfo { int g, col4, lane; float fgt[3]; };      // fgt[q] = 1 where the lane's row group g > q, else 0
  // the value of the lane of the same column in row group GC, for every row group: on the diagonal tile (the critical
  // chain) by two VALU swaps, on the rest of the block row through the LDS crossbar (off the chain; 18.5 k -> 15.3 k cycles)
  template <int GC, bool DIAG> static DMC_DEV float bcast_rowgroup(float x, int col4) {
    if constexpr (!DIAG) return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(col4 + 64 * GC, __builtin_bit_cast(int, x)));
    else {
      const unsigned u = __builtin_bit_cast(unsigned, x);
      const auto h = __builtin_amdgcn_permlane32_swap(u, u, false, false);      // h[0]: row groups (0 1 0 1), h[1]: (2 3 2 3)
      const unsigned y = GC < 2 ? h[0] : h[1];
      const auto q = __builtin_amdgcn_permlane16_swap(y, y, false, false);      // q[0]: the even group everywhere, q[1]: the odd
      return __builtin_bit_cast(float, (GC & 1) ? q[1] : q[0]);
    }
  }
  template <int K, int C0> static DMC_DEV void eliminate_column(dmc_f4 (&t)[NB][NB], const LaneInfo& tl) {
    constexpr int GC = C0 >> 2, RC = C0 & 3;
    dmc_f4& D = t[K][K];
    const float inv = __builtin_amdgcn_rsqf(__builtin_amdgcn_fmed3f(readlane_t(D[RC], 16 * GC + C0), (float)DMC_MINVAL, __builtin_inff()));
    // the column below the pivot, scaled; rows at or above the pivot row get a zero multiplier, folded into the scale
    // (4 g + r > C0  <=>  r > RC ? g >= GC : g > GC)
    const float inv_ge = GC == 0 ? inv : inv * tl.fgt[GC > 0 ? GC - 1 : 0];
    const float inv_gt = GC == 3 ? 0.f : inv * tl.fgt[GC < 3 ? GC : 0];
    float ui[4];
#pragma unroll
    for (int r = 0; r < 4; r++) ui[r] = (GC == 3 && r <= RC) ? 0.f : dpp_all<0x150 + C0>(D[r]) * (r > RC ? inv_ge : inv_gt);
    const float scale = tl.g == GC ? inv : 1.f;      // the pivot row itself is scaled in place
#pragma unroll
    for (int j = K; j < NB; j++) {
      dmc_f4& P = t[K][j];
      P[RC] = P[RC] * scale;
      const float X = j == K ? bcast_rowgroup<GC, true>(P[RC], tl.col4) : bcast_rowgroup<GC, false>(P[RC], tl.col4);
#pragma unroll
      for (int r = 0; r < 4; r++) if (!(GC == 3 && r <= RC)) P[r] = P[r] - ui[r] * X;
    }
    D[RC] = (tl.lane == 16 * GC + C0) ? inv : D[RC];      // the packed form keeps 1 / L_kk on the diagonal
  }
  template <int K, int C0> struct Columns {
    static DMC_DEV void run(dmc_f4 (&t)[NB][NB], const LaneInfo& tl) {
      if constexpr (16 * K + C0 < N) eliminate_column<K, C0>(t, tl);      // (the columns past N are the identity's)
      if constexpr (C0 + 1 < 16) Columns<K, C0 + 1>::run(t, tl);
    }
  };
  template <int K> static DMC_DEV void block_column(dmc_f4 (&t)[NB][NB], const LaneInfo& tl) {
    Columns<K, 0>::run(t, tl);
#pragma unroll
    for (int i = K + 1; i < NB; i++) {
      const dmc_f4 nx = -t[K][i];
#pragma unroll
      for (int j = i; j < NB; j++) {
#pragma unroll
        for (int r = 0; r < 4; r++) t[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(nx[r], t[K][j][r], t[i][j], 0, 0, 0);
      }
    }
    if constexpr (K + 1 < NB) block_column<K + 1>(t, tl);
  }
  static DMC_DEV constexpr int c0(int j) { return j * N - ((j * (j - 1)) >> 1); }      // tri_c0(j, N)
  // Packed index of element (R, C), R <= C, of tile (bi, bj), register r, for the lane (g, c): tri_c0(R) + C - R with
  // R = R0 + G (R0 = 16 bi + r, G = 4 g)  =  [tri_c0(R0) + 16 bj - R0] + [tri_c0(G) - G + c] - R0 G
  static DMC_DEV void factor(DMC_LDS float* A, int lane) {
    static_assert(N > 32 && N <= 64, "three or four tiles a side (store()'s spare slot is an entry of column 16 + c: N >= 32; below 33 dofs the row form is as fast)");
    const int g = lane >> 4, c = lane & 15, G = 4 * g;
    LaneInfo tl; tl.g = g; tl.col4 = 4 * c; tl.lane = lane;
#pragma unroll
    for (int q = 0; q < 3; q++) tl.fgt[q] = g > q ? 1.f : 0.f;
    const int up = c0(G) - G + c;                      // lane part of the upper-triangle index
    const int tc = ((c * (2 * N + 1 - c)) >> 1) - c;   // tri_c0(c) - c: lane part of the mirrored (lower-triangle) index
    dmc_f4 t[NB][NB];
#pragma unroll
    for (int bi = 0; bi < NB; bi++)
#pragma unroll
      for (int bj = bi; bj < NB; bj++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int R0 = 16 * bi + r;
          int at = c0(R0) + 16 * bj - R0 + up - R0 * G;
          if (bi == bj) {      // the diagonal tiles enter whole (symmetric): below the diagonal the mirrored entry
            const int low = c0(16 * bi) + tc - 16 * bi * c + R0 - 16 * bi + G;
            at = (G + r <= c) ? at : low;
          }
          float v = A[at];      // (unpredicated: an index past the triangle reads a neighbouring array, the value is dropped)
          if (16 * bj + 15 >= N) { const bool in = (16 * bj + c < N) && (bi < bj || 16 * bi + G + r < N); v = in ? v : ((bi == bj && G + r == c) ? 1.f : 0.f); }
          t[bi][bj][r] = v;
        }
    block_column<0>(t, tl);
    // stores: an entry that does not exist (below the diagonal of a diagonal tile, past column N) aims at the slot of the
    // lane's entry (row 4 g, column 16 + c) -- which exists for every lane and is stored LAST, over whatever landed there
    const int safe = 16 + up;
#pragma unroll
    for (int bi = NB - 1; bi >= 0; bi--)
#pragma unroll
      for (int bj = NB - 1; bj >= bi; bj--)
#pragma unroll
        for (int r = 3; r >= 0; r--) {
          const int R0 = 16 * bi + r;
          int at = c0(R0) + 16 * bj - R0 + up - R0 * G;
          bool ok = true;
          if (bi == bj) ok = G + r <= c;
          if (16 * bj + 15 >= N) ok = ok && (16 * bj + c < N);
          if (bi == bj || 16 * bj + 15 >= N) at = ok ? at : safe;
          if (!(bi == 0 && bj == 1 && r == 0)) A[at] = t[bi][bj][r];
        }
    asm volatile("" ::: "memory");
    A[safe] = t[0][1][0];
  }
};
template <int LPE, int N>
DMC_FN void chol_factor_tiles(DMC_LDS float* A, int lane) {
  static_assert(LPE == 64, "one environment per wave");
  DMC_WSYNC();
  CholTiles<N>::factor(A, lane);
  DMC_WSYNC();
}
#endif
// Substitution for model-specialised kernels: lane i loads its row and its column of L up
// front (all loads in flight together), then both sweeps run on registers and v_readlane --
// no LDS access inside the 2 N dependent steps.  Same operations as chol_solve_lds.
#ifndef DMC_HOST_EMU
template <typename T, int LPE, int N>
DMC_FN void chol_solve_rows(DMC_LDS T* x, const DMC_LDS T* Lm, const DMC_LDS T* b, int lane) {
  static_assert(N >= 1 && N <= LPE, "one lane per unknown");
  const int i = lane;
  const bool own = i < N;
  const int ci = tri_c0(own ? i : 0, N);
  T row[N], col[N];
#pragma unroll
  for (int k = 0; k < N; k++) {      // (N <= 16: unpredicated loads from in-range addresses, the values selected afterwards)
    if constexpr (N > 16) { row[k] = (own && k < i) ? Lm[tri_c0(k, N) + i - k] : (T)0; col[k] = (own && k > i) ? Lm[ci + k - i] : (T)0; }
    else {
      const T r_ = Lm[tri_c0(k, N) + ((own && k < i) ? i - k : 0)], c_ = Lm[ci + ((own && k > i) ? k - i : 0)];
      row[k] = (own && k < i) ? r_ : (T)0; col[k] = (own && k > i) ? c_ : (T)0;
    }
  }
  const T dinv_ = Lm[ci], b_ = b[own ? i : 0];
  const T dinv = own ? dinv_ : (T)0;      // 1 / L[i][i]
  T sreg = own ? b_ : (T)0;
  // Step k needs x_k = s_k / L[k][k]: every lane forms its own s_i * dinv_i (one VALU op, and lane k's is the value),
  // ONE cross-lane read fetches it, and the update is an unconditional FMA -- row[k] / col[k] are zeros where the
  // step does not reach, so lane k keeps its finished s_k and its x_k is s_k * dinv_k again after the loop.  Three
  // instructions per step instead of ~20 (two broadcasts, a scalar product moved back to a VGPR, a write-lane and two
  // predicated updates: 2 603 instructions for N = 62, 8 % of the 62-dof step).  The same products and differences as
  // before, bit for bit.
#pragma unroll
  for (int k = 0; k < N; k++) { const T xk = bcast_rows<LPE, N>(sreg*dinv, k); sreg = nmsub<(N <= 16)>(sreg, row[k], xk); }
  sreg = sreg*dinv;
#pragma unroll
  for (int k = N - 1; k >= 0; k--) { const T xk = bcast_rows<LPE, N>(sreg*dinv, k); sreg = nmsub<(N <= 16)>(sreg, col[k], xk); }
  if (own) x[i] = sreg*dinv;
  DMC_WSYNC();
}
#endif
// ---- block diagonal over the kinematic trees (StepDims::treemax) ------------------------------------------------
// M -- and H = M + J'DJ as long as no constraint row moves two trees -- is block diagonal over the kinematic trees of a
// multi-body scene (soccer 2v2: five trees of six dofs).  The row-per-lane routines above run the N columns one after
// the other, N (N + 1) / 2 cross-lane broadcasts + FMAs, of which all but the in-tree ones multiply exact zeros; a lone
// wave per SIMD pays ~9 cycles per instruction, so the 30 x 30 factorisation was 16 k cycles, 8 % of the soccer step, and
// each substitution 11 k.  Here every tree eliminates ITS column kk = 0 .. TM-1 at the same time: the pivot lane differs
// per tree, so the broadcasts are per-lane-addressed (ds_bpermute) instead of v_readlane: TM (TM + 1) / 2 of them for
// the whole matrix.  Entry for entry the same operations in the same order as chol_factor_rows / chol_solve_rows --
// what is skipped is  a - 0 * x -- so the results are bit-identical.  t0 / t1: first dof / 1 + last dof of the lane's
// tree.  One environment per wave (LPE = 64).
#ifndef DMC_HOST_EMU
DMC_DEV float lane_read(float v, int src) { return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src << 2, __builtin_bit_cast(int, v))); }
DMC_DEV double lane_read(double v, int src) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)u);
  const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)(u >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <typename T, int LPE, int N, int TM>
DMC_FN void chol_factor_trees(DMC_LDS T* A, int lane, int t0, int t1) {
  static_assert(LPE == 64 && N <= LPE, "one lane per matrix row, one environment per wave");
  DMC_WSYNC();
  T a[TM];
  const bool own = lane < N;
#pragma unroll
  for (int kk = 0; kk < TM; kk++) { const int j = t0 + kk; a[kk] = (own && j <= lane) ? A[tri_c0(j, N) + lane - j] : (T)0; }
#pragma unroll
  for (int kk = 0; kk < TM; kk++) {
    const int src = t0 + kk;
    T akk = lane_read(a[kk], src);
    if (akk < (T)DMC_MINVAL) akk = (T)DMC_MINVAL;
    const T inv = t_rsqrt(akk);
    const T lik = (own && src < t1) ? a[kk] * inv : (T)0;      // (a tree with fewer than TM dofs sits these columns out)
#pragma unroll
    for (int jj = kk + 1; jj < TM; jj++) { const T ljk = lane_read(lik, t0 + jj); a[jj] = a[jj] - lik * ljk; }
    a[kk] = lane == src ? inv : lik;
  }
#pragma unroll
  for (int kk = 0; kk < TM; kk++) { const int j = t0 + kk; if (own && j <= lane) A[tri_c0(j, N) + lane - j] = a[kk]; }
  DMC_WSYNC();
}
template <typename T, int LPE, int N, int TM>
DMC_FN void chol_solve_trees(DMC_LDS T* x, const DMC_LDS T* Lm, const DMC_LDS T* b, int lane, int t0, int t1) {
  static_assert(LPE == 64 && N <= LPE, "one lane per unknown, one environment per wave");
  const int i = lane;
  const bool own = i < N;
  const int ci = tri_c0(own ? i : 0, N);
  T row[TM], col[TM], dk[TM];
  const T dinv = own ? Lm[ci] : (T)0;      // 1 / L[i][i]
#pragma unroll
  for (int kk = 0; kk < TM; kk++) {
    const int k = t0 + kk;
    row[kk] = (own && k < i) ? Lm[tri_c0(k, N) + i - k] : (T)0;
    col[kk] = (own && k > i && k < t1) ? Lm[ci + k - i] : (T)0;
    dk[kk] = lane_read(dinv, k);
  }
  T sreg = own ? b[i] : (T)0;
#pragma unroll
  for (int kk = 0; kk < TM; kk++) {
    const int k = t0 + kk;
    const T xk = lane_read(sreg, k) * dk[kk];
    if (i == k) sreg = xk;
    if (i > k && own) sreg -= row[kk]*xk;
  }
#pragma unroll
  for (int kk = TM - 1; kk >= 0; kk--) {
    const int k = t0 + kk;
    const T xk = lane_read(sreg, k) * dk[kk];
    if (i == k) sreg = xk;
    if (i < k && k < t1 && own) sreg -= col[kk]*xk;
  }
  if (own) x[i] = sreg;
  DMC_WSYNC();
}
#endif
// x = (L L')^-1 b (x may alias b); Lm as produced by chol_factor_lds
//   n <= LPE : lane i carries x[i] in a register; the pivot value travels by a
//              cross-lane broadcast, no LDS round trip, no fence inside the loops.
template <typename T, int LPE>
DMC_FN void chol_solve_lds(DMC_LDS T* x, const DMC_LDS T* Lm, const DMC_LDS T* b, int n, int lane) {
  if (n <= LPE && LPE > 1) {
    const int i = lane;
    const int ci = tri_c0(i < n ? i : 0, n);
    T sreg = i < n ? b[i] : (T)0;
    for (int k = 0; k < n; k++) {
      const int ck = tri_c0(k, n);
      const T lik = (i > k && i < n) ? Lm[ck + i - k] : (T)0;
      const T xk = wave_bcast<LPE>(sreg, k) * Lm[ck];
      if (i == k) sreg = xk;
      if (i > k && i < n) sreg -= lik*xk;
    }
    for (int k = n - 1; k >= 0; k--) {
      const T lki = i < k ? Lm[ci + k - i] : (T)0;
      const T xk = wave_bcast<LPE>(sreg, k) * Lm[tri_c0(k, n)];
      if (i == k) sreg = xk;
      if (i < k) sreg -= lki*xk;
    }
    if (i < n) x[i] = sreg;
    DMC_WSYNC();
    return;
  }
  for (int i = lane; i < n; i += LPE) x[i] = b[i];
  DMC_WSYNC();
  for (int k = 0; k < n; k++) {
    const int ck = tri_c0(k, n);
    const T xk = x[k] * Lm[ck];
    DMC_WSYNC();
    if (lane == 0) x[k] = xk;
    for (int i = k + 1 + lane; i < n; i += LPE) x[i] -= Lm[ck + i - k]*xk;
    DMC_WSYNC();
  }
  for (int k = n - 1; k >= 0; k--) {
    const T xk = x[k] * Lm[tri_c0(k, n)];
    DMC_WSYNC();
    if (lane == 0) x[k] = xk;
    for (int i = lane; i < k; i += LPE) x[i] -= Lm[tri_c0(i, n) + k - i]*xk;
    DMC_WSYNC();
  }
}
}  // namespace dmc
