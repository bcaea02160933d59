// Host program of tests/test_ar_plan_la.py: the fused layers field of the decode step's plan (ar_plan.h,
// ar_plan_step: ArStepPlan::la_fused) with every other field of the plan, for every weight dtype, KV dtype,
// B = 1..66, row mode (B = 1), table presence and sample flag under each option set given as an argument
// ("-" = defaults, else name=value[,name=value]). One line per combination:
//   set wdtype kvdtype B row q0 sample path sel end nsplit attn_direct attn8 selcopy l0_fused fused_mlp q0_gran
//   xpk ksplit qsplit la_fused
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ar_plan.h"

using namespace lvx;

static bool set_opt(Opts& o, const char* name, int v) {
  int* f = !strcmp(name, "defer_select") ? &o.defer_select : !strcmp(name, "bt") ? &o.bt
         : !strcmp(name, "f32b") ? &o.f32b : !strcmp(name, "ln_max") ? &o.ln_max : !strcmp(name, "l0q") ? &o.l0q
         : !strcmp(name, "l0a") ? &o.l0a : !strcmp(name, "laf") ? &o.laf : nullptr;
  if (f) *f = v;
  return f != nullptr;
}

int main(int argc, char** argv) {
  static_assert(SEL_Q0_ROWS == 4 && SEL_SAMPLE == 5 && PATH_F32B == 4, "names below");
  const char* pn[] = {"gemv", "mfma_ln", "mfma_rows", "v3", "f32b"};
  const char* sn[] = {"argmax", "gran", "embed", "ln_gran", "q0_rows", "sample"};
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
        for (int B = 1; B <= 66; ++B)
          for (int row = 0; row <= (B == 1); ++row)
            for (int q0 = 0; q0 < 2; ++q0)
              for (int sample = 0; sample < 2; ++sample) {
                const ArStepPlan p = ar_plan_step(o, wds[w], kvs[k], B, row != 0, q0 != 0, sample != 0);
                printf("%s %s %s %d %d %d %d %s %s %d %d %d %d %d %d %d %d %d %d %d %d\n", argv[i], wn[w], kn[k], B, row,
                       q0, sample, pn[p.path], sn[p.sel], (int)p.end, p.nsplit, p.attn_direct, p.attn8, p.selcopy,
                       p.l0_fused, p.fused_mlp, p.q0_gran, p.xpk, p.ksplit, p.qsplit, p.la_fused);
              }
  }
  return 0;
}
