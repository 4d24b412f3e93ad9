// TEST INFRASTRUCTURE (tests/test_content_dims_cpu.py): the host build of the kernel core (emu.cpp) plus a view of the
// content facts step_tables_build put into StepDims.  Built twice by the test: as it is, and with -DDMC_NO_CONTENT_DIMS
// (the kernel core assumes every joint and sensor type present).
#include "emu.cpp"

extern "C" int emu_content_dims(void* h, int* out) {
  const StepDims& d = ((Emu*)h)->tb.L.d;
  const int v[] = {d.jtypes, d.nsens_pos, d.nsens_vel, d.nsens_acc, d.nsens_rne, d.nsens_touch};
  for (int k = 0; k < 6; k++) out[k] = v[k];
#ifdef DMC_NO_CONTENT_DIMS
  return 0;
#else
  return 1;
#endif
}
