// TEST INFRASTRUCTURE (tests/test_coop_open_cpu.py): the host build of the kernel core (emu.cpp) plus the opening stage of
// a step on stashed kinematics, run three ways from one state of the environment's scratch: the stage as one wave runs it
// (stage_posvel), and its two cooperative sides (StepCore::coop_side_a / coop_side_b) in both orders.
#include "emu.cpp"

// out_r: 3 x n_sr reals, out_i: 3 x n_si ints -- the whole scratch after {stage_posvel, A then B, B then A}
template <typename T>
static void coop_open_t(Emu* e, const T* mr, const double* qpos, const double* qvel, double* out_r, int* out_i) {
  const StepLayout& L = e->tb.L;
  StepOpts<T> o = step_opts_cast<T>(e->tb.opts);
  if (!e->xfrc64.empty()) { o.xfrc = sizeof(T) == 8 ? (const void*)e->xfrc64.data() : (const void*)e->xfrc32.data(); o.xfrc_B = 1; }
  if (L.d.nmocap) {
    o.mocap_pos = sizeof(T) == 8 ? (const void*)e->mpos64.data() : (const void*)e->mpos32.data();
    o.mocap_quat = sizeof(T) == 8 ? (const void*)e->mquat64.data() : (const void*)e->mquat32.data(); o.mocap_B = 1;
  }
  o.g_mr = mr;
  e->gs.resize(L.n_gs + 2); o.gscr = e->gs.data();
  if (L.d.nslip) { e->nsA.resize((size_t)L.d.nslip * L.d.nslip + 2); o.ns_A = e->nsA.data(); }
  std::vector<T> q(qpos, qpos + L.d.nq), v(qvel, qvel + L.d.nv), zero(L.d.nv + L.d.nu + L.d.na + 1, (T)0);
  double time = 0;
  int epoch = 1;
  StepIO<T> io;
  memset(&io, 0, sizeof(io));
  io.B = 1; io.qpos = q.data(); io.qvel = v.data(); io.qacc_warmstart = zero.data(); io.ctrl = zero.data(); io.act = zero.data();
  io.time = &time; io.epoch = &epoch;
  DynLayoutSrc ls; ls.p = &L;
  typedef StepCore<T, 1> Core;
  typename Core::Entry en = {0, 0, 0, epoch};
  // what the launch's entry and the kinematic stash leave in the scratch: the state, poses, the COM frame, velocities
  std::vector<T> s0(L.n_sr, (T)0); std::vector<int> si0(L.n_si, 0);
  {
    Core c(ls, o, e->tb.mi.data(), mr, e->tb.mc.data(), s0.data(), si0.data(), 0);
    c.load_state(io, 0, false, en);
    c.kinematics(); c.com_pos(); c.com_vel();
  }
  for (int variant = 0; variant < 3; variant++) {
    std::vector<T> s(s0); std::vector<int> si(si0);
    Core c(ls, o, e->tb.mi.data(), mr, e->tb.mc.data(), s.data(), si.data(), 0);
    if (variant == 0) c.stage_posvel(false, OUT_ALL, true, true);
    else if (variant == 1) { c.coop_side_a(); c.coop_side_b(); }
    else { c.coop_side_b(); c.coop_side_a(); }
    for (int i = 0; i < L.n_sr; i++) out_r[(size_t)variant * L.n_sr + i] = (double)s[i];
    for (int i = 0; i < L.n_si; i++) out_i[(size_t)variant * L.n_si + i] = si[i];
  }
}

extern "C" int emu_coop_open(void* h, int prec, const double* qpos, const double* qvel, double* out_r, int* out_i) {
  Emu* e = (Emu*)h;
  if (e->tb.L.d.nmocap && e->mpos64.empty()) return -1;      // (emu_set_mocap first)
  if (e->tb.L.n_gs) return -2;      // (a model with global scratch: not what this view copies)
  if (prec == 64) coop_open_t<double>(e, e->tb.mr.data(), qpos, qvel, out_r, out_i);
  else coop_open_t<float>(e, e->mr32.data(), qpos, qvel, out_r, out_i);
  return 0;
}
