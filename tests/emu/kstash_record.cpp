// TEST INFRASTRUCTURE (tests/test_kstash_record_cpu.py): the layout step_tables_build gives a model and the record of its
// kinematic stash (kstash_record, step_layout.h) as the kernels and the allocation see them.  Host only.
#include <string>

#include "../../dm_control_amd/csrc/step_tables.h"

// out: nq, nv, s_xpos, s_qM, n_mi, n_mr_lds, n_mc, n_sr, n_si, then (kin, stride) for 4-byte and for 8-byte reals
extern "C" int kstash_facts(const int* ints, int n_ints, const double* reals, int n_reals, int nconmax, int* out) {
  dmc::HostModel hm; std::string err;
  if (!dmc::host_model_parse(&hm, ints, n_ints, reals, n_reals, &err)) return 1;
  dmc::StepTables tb;
  if (!dmc::step_tables_build(&tb, hm, nconmax, 0, &err, 0)) return 2;
  const StepLayout& L = tb.L;
  const int v[] = {L.d.nq, L.d.nv, L.s_xpos, L.s_qM, L.n_mi, L.n_mr_lds, L.n_mc, L.n_sr, L.n_si};
  for (int k = 0; k < 9; k++) out[k] = v[k];
  for (int p = 0; p < 2; p++) {
    const KStashRecord r = kstash_record(L.d.nq, L.d.nv, L.s_qM - L.s_xpos, L.s_xpos, p ? 8 : 4);
    out[9 + 2*p] = r.kin; out[10 + 2*p] = r.stride;
  }
  return 0;
}
