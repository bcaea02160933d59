// Host program of tests/test_ar_plan_tail.py: the two tail fields of the decode step's plan (ar_plan.h,
// ar_plan_step: ArStepPlan::x_folded and ArStepPlan::lm_fused) next to the field they ride on (la_fused), for
// every weight dtype, KV dtype, B = 1..64, table presence and sample flag under each option set given as an
// argument ("-" = defaults, else name=value[,name=value]). One line per combination:
//   set wdtype kvdtype B q0 sample path l0_fused la_fused x_folded lm_fused
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ar_plan.h"

using namespace lvx;

static bool set_opt(Opts& o, const char* name, int v) {
  int* f = !strcmp(name, "l0a") ? &o.l0a : !strcmp(name, "laf") ? &o.laf : !strcmp(name, "xfold") ? &o.xfold
         : !strcmp(name, "lmf") ? &o.lmf : nullptr;
  if (f) *f = v;
  return f != nullptr;
}

int main(int argc, char** argv) {
  static_assert(PATH_F32B == 4, "names below");
  const char* pn[] = {"gemv", "mfma_ln", "mfma_rows", "v3", "f32b"};
  for (int i = 1; i < argc; ++i) {
    Opts o;
    char spec[256];
    snprintf(spec, sizeof spec, "%s", argv[i]);
    if (strcmp(spec, "-"))
      for (char* t = strtok(spec, ","); t; t = strtok(nullptr, ",")) {
        char* eq = strchr(t, '=');
        if (!eq) return 2;
        *eq = 0;
        if (!set_opt(o, t, atoi(eq + 1))) return 2;
      }
    const int wds[] = {LVX_DTYPE_F32, LVX_DTYPE_BF16}, kvs[] = {LVX_DTYPE_F32, LVX_DTYPE_BF16, LVX_DTYPE_FP8};
    const char* wn[] = {"fp32", "bf16"};
    const char* kn[] = {"fp32", "bf16", "fp8"};
    for (int w = 0; w < 2; ++w)
      for (int k = 0; k < 3; ++k)
        for (int B = 1; B <= 64; ++B)
          for (int q0 = 0; q0 < 2; ++q0)
            for (int sample = 0; sample < 2; ++sample) {
              const ArStepPlan p = ar_plan_step(o, wds[w], kvs[k], B, false, q0 != 0, sample != 0);
              printf("%s %s %s %d %d %d %s %d %d %d %d\n", argv[i], wn[w], kn[k], B, q0, sample, pn[p.path], p.l0_fused,
                     p.la_fused, p.x_folded, p.lm_fused);
            }
  }
  return 0;
}
