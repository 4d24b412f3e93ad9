// step_defs.h -- what every header of the step core needs: the function / address-space qualifiers and the wave-level
// fence, in their device form and in the form of the host build (DMC_HOST_EMU: tests/emu), and the model constants.
#pragma once
#include <math.h>
#include <stdint.h>
#ifdef DMC_HOST_EMU
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#endif

#include "../../include/dmc_model_layout.h"

#ifdef DMC_HOST_EMU
#define DMC_DEV inline
#define DMC_FN inline
#define DMC_LDS
#define DMC_GLB
// (host build: a counter -- how many wave-level fences one step executes is what a match on several waves would have to
// turn into workgroup barriers: scripts/multiwave_probe.py)
#define DMC_WSYNC() ((void)++dmc_emu_wsync_count)
static long long dmc_emu_wsync_count = 0;
#else
#define DMC_DEV __device__ __forceinline__
// out-of-line device functions (one copy of the code for all call sites) taking
// explicitly LDS-qualified pointers so that they still compile to ds_* ops
#define DMC_FN __device__ __attribute__((noinline, not_tail_called))
#define DMC_LDS __attribute__((address_space(3)))
#define DMC_GLB __attribute__((address_space(1)))   // the per-env global scratch: global_load / global_store, not flat
#define DMC_WSYNC()                                             \
  do {                                                          \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      \
    __builtin_amdgcn_wave_barrier();                            \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");      \
  } while (0)
#endif
