// Internal: the launch plan of an NT GEMM.  vc_gemm_plan (gemm_plan.cpp, host only) is the one place that chooses a launch form: it runs
// every argument check that needs no pointer VALUE and names the launch -- kernel family, that family's template arguments, the values
// patched into GemmArgs, grid and dynamic LDS -- and launches nothing.  vitcap_gemm_ex (gemm.hip) switches from the plan onto the template
// launchers; vitcap_gemm_plan, vitcap_gemm_large_form and vitcap_gemm_tile_plan answer from the same functions.
#pragma once
#include "../../include/vitcap_hip.h"

typedef vitcap_gemm_plan_info GemmPlan;      // include/vitcap_hip.h: the VITCAP_GEMM_FAMILY_* / VITCAP_GEMM_4W_* values live there too

// which optional operands a launch carries, and what vitcap_gemm_ex found about the pointers it was handed (the queries pass 0)
struct GemmOperands {
  bool bias, res, aux, zout;
  int ldaux, ldz;
  unsigned misaligned;      // bit 0: A / W / C, bit 1: residual, bit 2: bias -- not 16-byte aligned
};

// VITCAP_OK and the plan, or VITCAP_EINVAL and the error text of the first failed check (in vitcap_gemm_ex's documented order)
int vc_gemm_plan(const vitcap_gemm_desc* d, const GemmOperands& o, GemmPlan* pl);
