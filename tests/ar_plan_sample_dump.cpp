// Host program of tests/test_ar_plan_sample.py: the decode step's plan (ar_plan.h, ar_plan_step) with and
// without the trailing `sample` argument, for every weight dtype, KV dtype, B = 1..66, row mode (B = 1)
// and table presence under each option set given as an argument ("-" = defaults, else
// name=value[,name=value]). Three lines per combination, tagged
//   six     the six-argument call            false   sample = false            true   sample = true
// and, per option set and non-row combination, a fourth, `nodefer`: the six-argument call with option
// defer_select forced to 0. Fields after the tag:
//   set wdtype kvdtype B row q0 path sel end fused_mlp q0_gran nsplit attn_direct attn8 selcopy xpk ksplit qsplit
// With no argument: the known answers of the host form of philox4x32_10 (lvx_common.h), one line
// `philox c0 c1 c2 c3 k0 k1 -> x0 x1 x2 x3` per vector.
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

static void line(const char* tag, const char* set, const char* wn, const char* kn, int B, int row, int q0,
                 const ArStepPlan& p) {
  static_assert(SEL_SAMPLE == 5, "ArSelect");
  const char* pn[] = {"gemv", "mfma_ln", "mfma_rows", "v3", "f32b"};
  const char* sn[] = {"argmax", "gran", "embed", "ln_gran", "q0_rows", "sample"};
  const char* en[] = {"none", "select_final", "argmax"};
  printf("%s %s %s %s %d %d %d %s %s %s %d %d %d %d %d %d %d %d %d\n", tag, set, wn, kn, B, row, q0, pn[p.path],
         sn[p.sel], en[p.end], p.fused_mlp, p.q0_gran, p.nsplit, p.attn_direct, p.attn8, p.selcopy, p.xpk, p.ksplit,
         p.qsplit);
}

int main(int argc, char** argv) {
  if (argc == 1) {
    const uint32_t v[3][6] = {{0u, 0u, 0u, 0u, 0u, 0u},
                              {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                              {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
    for (int i = 0; i < 3; ++i) {
      uint32_t c[4] = {v[i][0], v[i][1], v[i][2], v[i][3]};
      philox4x32_10(c, v[i][4], v[i][5]);
      printf("philox %08x %08x %08x %08x %08x %08x -> %08x %08x %08x %08x\n", v[i][0], v[i][1], v[i][2], v[i][3],
             v[i][4], v[i][5], c[0], c[1], c[2], c[3]);
    }
    return 0;
  }
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
    Opts nd = o;
    nd.defer_select = 0;
    const int wds[] = {LVX_DTYPE_F32, LVX_DTYPE_BF16}, kvs[] = {LVX_DTYPE_F32, LVX_DTYPE_BF16, LVX_DTYPE_FP8};
    const char* wn[] = {"fp32", "bf16"};
    const char* kn[] = {"fp32", "bf16", "fp8"};
    for (int w = 0; w < 2; ++w)
      for (int k = 0; k < 3; ++k)
        for (int B = 1; B <= 66; ++B)
          for (int row = 0; row <= (B == 1); ++row)
            for (int q0 = 0; q0 < 2; ++q0) {
              line("six", argv[i], wn[w], kn[k], B, row, q0, ar_plan_step(o, wds[w], kvs[k], B, row != 0, q0 != 0));
              line("false", argv[i], wn[w], kn[k], B, row, q0,
                   ar_plan_step(o, wds[w], kvs[k], B, row != 0, q0 != 0, false));
              line("true", argv[i], wn[w], kn[k], B, row, q0,
                   ar_plan_step(o, wds[w], kvs[k], B, row != 0, q0 != 0, true));
              if (!row) line("nodefer", argv[i], wn[w], kn[k], B, row, q0, ar_plan_step(nd, wds[w], kvs[k], B, false, q0 != 0));
            }
  }
  return 0;
}
