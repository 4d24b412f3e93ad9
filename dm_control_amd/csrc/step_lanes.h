// step_lanes.h -- the cross-lane layer of the step core: DPP moves, row / half swaps, readlane broadcasts and the group
// reductions and scans built from them (device unit test: scripts/lane_primitives_probe.hip).
#pragma once
#include "step_defs.h"

namespace dmc {
// ---------------------------------------------------------------------------
// group primitives (LPE lanes of one wave)
// ---------------------------------------------------------------------------
#ifndef DMC_HOST_EMU
// DPP cross-lane moves inside a 16-lane row (no LDS traffic, ~VALU latency)
template <int CTRL> DMC_DEV int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }
template <int CTRL> DMC_DEV float dpp_f(float v) { return __int_as_float(dpp_i<CTRL>(__float_as_int(v))); }
template <int CTRL> DMC_DEV double dpp_f(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = dpp_i<CTRL>((int)(b & 0xffffffffll)), hi = dpp_i<CTRL>((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
#endif
// Exchanges across the 16-lane rows / the 32-lane halves of a wave with the gfx950 row / half swaps
// (v_permlane16_swap / v_permlane32_swap: VALU moves) instead of a trip through the LDS crossbar (ds_bpermute, what
// __shfl_xor compiles to): swapping a value with itself leaves {even row's copy, odd row's copy} of each row pair in
// the two results, whose sum / max is the same in both rows.  Reductions sit on the critical path of every solver
// iteration (their results feed the next branch), ~25 per Newton iteration.
#ifndef DMC_HOST_EMU
struct Pair32 { unsigned a, b; };
DMC_DEV Pair32 swap16(unsigned x) { const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false); Pair32 p = {r[0], r[1]}; return p; }
DMC_DEV Pair32 swap32(unsigned x) { const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false); Pair32 p = {r[0], r[1]}; return p; }
template <int W> DMC_DEV Pair32 swapW(unsigned x) { return W == 16 ? swap16(x) : swap32(x); }
template <int W> DMC_DEV float xsum(float v) { const Pair32 p = swapW<W>(__float_as_uint(v)); return __uint_as_float(p.a) + __uint_as_float(p.b); }
template <int W> DMC_DEV int xsum(int v) { const Pair32 p = swapW<W>((unsigned)v); return (int)p.a + (int)p.b; }
template <int W> DMC_DEV double xsum(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const Pair32 lo = swapW<W>((unsigned)u), hi = swapW<W>((unsigned)(u >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi.a << 32) | lo.a) + __builtin_bit_cast(double, ((unsigned long long)hi.b << 32) | lo.b);
}
template <int W> DMC_DEV int xmax(int v) { const Pair32 p = swapW<W>((unsigned)v); return (int)p.a > (int)p.b ? (int)p.a : (int)p.b; }
#endif
// Sum over the LPE lanes of a group; every lane receives the total.  Same
// pairing tree as an xor butterfly (1, 2, 4, 8 inside a row via DPP quad_perm /
// row_half_mirror / row_mirror, then 16 and 32 via the row / half swaps).
template <int LPE, typename V> DMC_DEV V group_sum(V v) {
#ifndef DMC_HOST_EMU
  if (LPE >= 2) v += dpp_f<0xB1>(v);    // quad_perm [1,0,3,2]
  if (LPE >= 4) v += dpp_f<0x4E>(v);    // quad_perm [2,3,0,1]
  if (LPE >= 8) v += dpp_f<0x141>(v);   // row_half_mirror
  if (LPE >= 16) v += dpp_f<0x140>(v);  // row_mirror
  if (LPE >= 32) v = xsum<16>(v);
  if (LPE >= 64) v = xsum<32>(v);
#endif
  return v;
}
// N independent group sums, step by step side by side: each is group_sum's pairing tree (the same bits), and a step of
// one chain fills the wait of the others' DPP moves (a dependent chain pays the full latency at every step).
// Each step's result passes through an empty asm: left alone, the SLP vectoriser pairs the chains' adds into v_pk_add_f32,
// and a packed add cannot take the DPP move as its operand -- a step of a pair was then two zeroing moves, two
// v_mov_b32_dpp and the packed add, five instructions where two v_add_f32_dpp do it.
template <int LPE, int N, typename V> DMC_DEV void group_sum_n(V (&v)[N]) {
#ifndef DMC_HOST_EMU
#define DMC_EACH(expr) _Pragma("unroll") for (int k = 0; k < N; k++) { expr; asm("" : "+v"(v[k])); }
  if (LPE >= 2) DMC_EACH(v[k] += dpp_f<0xB1>(v[k]))
  if (LPE >= 4) DMC_EACH(v[k] += dpp_f<0x4E>(v[k]))
  if (LPE >= 8) DMC_EACH(v[k] += dpp_f<0x141>(v[k]))
  if (LPE >= 16) DMC_EACH(v[k] += dpp_f<0x140>(v[k]))
  if (LPE >= 32) DMC_EACH(v[k] = xsum<16>(v[k]))
  if (LPE >= 64) DMC_EACH(v[k] = xsum<32>(v[k]))
#undef DMC_EACH
#endif
}
// value held by lane `k` of each group when k is WAVE-uniform (a loop counter): v_readlane
// into an SGPR (one per group of the wave) instead of a trip through the LDS crossbar
#ifndef DMC_HOST_EMU
DMC_DEV float readlane_t(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
DMC_DEV int readlane_t(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
DMC_DEV double readlane_t(double v, int l) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
#endif
template <int LPE, typename V> DMC_DEV V wave_bcast(V v, int k) {
#ifndef DMC_HOST_EMU
  if (LPE == 64) return readlane_t(v, k);
  const int g = (int)(__lane_id()) / LPE;   // which group of the wave this lane belongs to
  V r = readlane_t(v, k);
#pragma unroll
  for (int q = 1; q < 64 / LPE; q++) { const V w = readlane_t(v, q*LPE + k); r = g == q ? w : r; }
  return r;
#else
  (void)k; return v;
#endif
}
// The same when every lane that holds something sits in the FIRST 16-lane row of its group (one lane per matrix row of a
// model with nv <= 16): the gfx90a+ DPP control row_newbcast:k hands lane k of each 16-lane row to all lanes of that row
// in ONE VALU move (folded into the consuming multiply where the encoding allows) -- against two v_readlane, a trip
// through two SGPRs and a v_cndmask per value for two environments per wave.  The 9 x 9 factorisations of the cheetah
// were ~200 instructions of which 135 were these broadcasts; the lanes of the group's other rows receive the value of
// THEIR row's lane k, which nothing reads (they own no matrix row).  k must be a constant after unrolling.
#ifndef DMC_HOST_EMU
template <int CTRL> DMC_DEV float dpp_all(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true)); }
template <int CTRL> DMC_DEV double dpp_all(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xF, 0xF, true), hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// (every lane of a row_newbcast has a source lane: bound_ctrl spares the move that would initialise the "old" value)
template <typename V> DMC_DEV V row_bcast16(V v, int k) {
  switch (k & 15) {
    case 0: return dpp_all<0x150>(v); case 1: return dpp_all<0x151>(v); case 2: return dpp_all<0x152>(v); case 3: return dpp_all<0x153>(v);
    case 4: return dpp_all<0x154>(v); case 5: return dpp_all<0x155>(v); case 6: return dpp_all<0x156>(v); case 7: return dpp_all<0x157>(v);
    case 8: return dpp_all<0x158>(v); case 9: return dpp_all<0x159>(v); case 10: return dpp_all<0x15A>(v); case 11: return dpp_all<0x15B>(v);
    case 12: return dpp_all<0x15C>(v); case 13: return dpp_all<0x15D>(v); case 14: return dpp_all<0x15E>(v); default: return dpp_all<0x15F>(v);
  }
}
#endif
// broadcast of matrix row k's value among the N <= LPE row-holding lanes of a group
template <int LPE, int N, typename V> DMC_DEV V bcast_rows(V v, int k) {
#if !defined(DMC_HOST_EMU) && !defined(DMC_NO_ROW_NEWBCAST)
  if constexpr (N <= 16 && LPE >= 16) return row_bcast16(v, k);
#endif
  return wave_bcast<LPE>(v, k);
}
template <int LPE> DMC_DEV int group_max(int v) {
#ifndef DMC_HOST_EMU
  int w;
  if (LPE >= 2) { w = dpp_i<0xB1>(v); v = w > v ? w : v; }
  if (LPE >= 4) { w = dpp_i<0x4E>(v); v = w > v ? w : v; }
  if (LPE >= 8) { w = dpp_i<0x141>(v); v = w > v ? w : v; }
  if (LPE >= 16) { w = dpp_i<0x140>(v); v = w > v ? w : v; }
  if (LPE >= 32) v = xmax<16>(v);
  if (LPE >= 64) v = xmax<32>(v);
#endif
  return v;
}
// exclusive prefix sum over the group; *total receives the group sum.  Hillis-Steele inside a 16-lane row with DPP
// row shifts (zeros shifted in), then the row totals travel with row_bcast:15 / row_bcast:31 -- no LDS crossbar trips
// (__shfl_up is a ds_bpermute: six dependent ones per scan).
template <int LPE> DMC_DEV int group_scan(int v, int lane, int* total) {
#ifndef DMC_HOST_EMU
  int inc = v;
  (void)lane;
  if (LPE >= 2) inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xF, 0xF, true);    // row_shr:1
  if (LPE >= 4) inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xF, 0xF, true);    // row_shr:2
  if (LPE >= 8) inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xF, 0xF, true);    // row_shr:4
  if (LPE >= 16) inc += __builtin_amdgcn_update_dpp(0, inc, 0x118, 0xF, 0xF, true);   // row_shr:8
  if (LPE >= 32) inc += __builtin_amdgcn_update_dpp(0, inc, 0x142, 0xA, 0xF, false);  // row_bcast:15 into rows 1, 3
  if (LPE >= 64) inc += __builtin_amdgcn_update_dpp(0, inc, 0x143, 0xC, 0xF, false);  // row_bcast:31 into rows 2, 3
  *total = wave_bcast<LPE>(inc, LPE - 1);
  return inc - v;
#else
  (void)lane; *total = v; return 0;
#endif
}
}  // namespace dmc
