// TEST INFRASTRUCTURE (tests/test_ls_fused_cpu.py, scripts/ls_evals_probe.py): the host build of the kernel core (emu.cpp)
// plus the line search's pass counters.  Built twice by the test: as it is, and with -DDMC_NO_LS_FUSED (the bracket
// phase of primal_search one evaluation after the other).
#include "emu.cpp"

extern "C" void emu_set_ls_iterations(void* h, int v) { ((Emu*)h)->tb.opts.ls_iterations = v; }      // StepOpts::ls_iterations (the cap)

// out[0..2]: passes (a fused pass counts once), searches that entered the bracket phase, fused passes; returns whether
// this build fuses
extern "C" int emu_ls_passes_get(long long* out) {
  for (int k = 0; k < 3; k++) out[k] = dmc::emu_ls_passes()[k];
#ifdef DMC_NO_LS_FUSED
  return 0;
#else
  return 1;
#endif
}
