// Host program of tests/test_ar_plan.py: prints the decode step's plan (ar_plan.h, ar_plan_step) for
// every weight dtype, KV dtype, B = 1..66, row mode (B = 1) and table presence under each option set
// given as an argument ("-" = defaults, else name=value[,name=value]). One line per combination:
//   set wdtype kvdtype B row q0 path sel end fused_mlp q0_gran nsplit attn_direct attn8 selcopy xpk ksplit qsplit
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ar_plan.h"

using namespace lvx;

static bool set_opt(Opts& o, const char* name, int v) {
  int* f = !strcmp(name, "defer_select") ? &o.defer_select : !strcmp(name, "fuse_mlp") ? &o.fuse_mlp
         : !strcmp(name, "bt") ? &o.bt : !strcmp(name, "exp") ? &o.exp : !strcmp(name, "f32b") ? &o.f32b
         : !strcmp(name, "ln_max") ? &o.ln_max : !strcmp(name, "l0q") ? &o.l0q : nullptr;
  if (f) *f = v;
  return f != nullptr;
}

int main(int argc, char** argv) {
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
    // the select forms are GemvArgs::defer_sel, which device code reads: fixed values
    static_assert(SEL_ARGMAX == 0 && SEL_GRAN == 1 && SEL_EMBED == 2 && SEL_LN_GRAN == 3 && SEL_Q0_ROWS == 4, "ArSelect");
    static_assert(PATH_GEMV == 0 && PATH_MFMA_LN == 1 && PATH_MFMA_ROWS == 2 && PATH_BT == 3 && PATH_F32B == 4, "pn");
    static_assert(END_NONE == 0 && END_SELECT_FINAL == 1 && END_ARGMAX == 2, "en");
    const char* pn[] = {"gemv", "mfma_ln", "mfma_rows", "v3", "f32b"};
    const char* sn[] = {"argmax", "gran", "embed", "ln_gran", "q0_rows"};
    const char* en[] = {"none", "select_final", "argmax"};
    for (int w = 0; w < 2; ++w)
      for (int k = 0; k < 3; ++k)
        for (int B = 1; B <= 66; ++B)
          for (int row = 0; row <= (B == 1); ++row)
            for (int q0 = 0; q0 < 2; ++q0) {
              const ArStepPlan p = ar_plan_step(o, wds[w], kvs[k], B, row != 0, q0 != 0);
              if (p.B != B || p.kv_dtype != kvs[k] || p.bf16 != (w == 1) || p.row != (row != 0)) return 3;
              printf("%s %s %s %d %d %d %s %s %s %d %d %d %d %d %d %d %d %d\n", argv[i], wn[w], kn[k], B, row, q0,
                     pn[p.path], sn[p.sel], en[p.end], p.fused_mlp, p.q0_gran, p.nsplit, p.attn_direct, p.attn8,
                     p.selcopy, p.xpk, p.ksplit, p.qsplit);
            }
  }
  return 0;
}
