// Host-side plan of one AR decode step: which kernels a step runs, decided once per call from the
// bound options, the dtypes, B and the call's mode (ar_plan_step), and the names of the integer mode
// codes the AR kernel families take as template arguments. No kernels here: this header compiles and
// runs without a GPU (tests/test_ar_plan.py).
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include "lvx_internal.h"

namespace lvx {

// ---------------------------------------------------------------------------------
// Mode codes of the kernel families (template parameters stay int). The epilogue (OUT) has one numbering
// for every family: ArOut. The prologue codes (IN / MODE / XM) keep one enum and one prefix per family,
// because there the same number does mean different things (4: GIN_LN_Y, RMODE_LN_Y, FIN_ATTN_ROWS).
// The step's op (launch_op, ar_probe's `which`): c_attn (layer 0: + embedding), attention, c_proj
// (+ split merge), c_fc, mlp c_proj, lm_head.
enum { OP_QKV = 0, OP_ATTN = 1, OP_CPROJ = 2, OP_FC = 3, OP_MPROJ = 4, OP_LM_HEAD = 5 };
// OUT, the epilogue of every GEMM family (step_store): q + KV append | x += out | h = gelu(out) (fp32) |
// logits | hb (bf16) = gelu(out) | split-K partial into a pending copy | x += out with the bf16 copy
// x * ln_2.weight and the row statistics (c_fc's operand) | logits + per-block top-1 / top-2 granules.
// What each family is instantiated with:
//   ar_gemv_kernel     QKV RESID GELU LOGITS LOGITS_GRAN (its own epilogue: prefetched operands)
//   ar_mfma2_kernel    QKV RESID LOGITS GELU_BF16 SPLITK RESID_STATS
//   ar_mfma_ln_kernel  QKV LOGITS GELU_BF16
//   ar_bt_kernel       QKV RESID LOGITS GELU_BF16
//   ar_f32b_kernel     QKV RESID GELU LOGITS SPLITK
enum ArOut {
  OUT_QKV = 0, OUT_RESID = 1, OUT_GELU = 2, OUT_LOGITS = 3, OUT_GELU_BF16 = 5, OUT_SPLITK = 6, OUT_RESID_STATS = 7,
  OUT_LOGITS_GRAN = 9
};
// ar_gemv_kernel IN (operand prologue): LayerNorm(x) | h (fp32, K = 3072) | merge of the split-KV
// partials | layer-0 embedding (stores x) then LayerNorm | LayerNorm(x + the fused MLP's pending
// copies) | EMBED after committing the previous step's select from lm_head's granules (B <= 2)
enum { GIN_LN = 0, GIN_H = 1, GIN_MERGE = 2, GIN_EMBED = 3, GIN_LN_Y = 4, GIN_EMBED_SELECT = 5 };
// ar_rows_kernel MODE (-> bf16 operand rows xn): LayerNorm(x) | embedding (stores x) then LayerNorm |
// LayerNorm(x + pending copies), x made final | as LN_Y / EMBED with fp32 output rows in st.h | LN_Y that
// also copies the fused layer-0 attention's shadow control records back (layer 1 of an l0_fused step)
enum { RMODE_LN = 0, RMODE_EMBED = 3, RMODE_LN_Y = 4, RMODE_LN_Y_F32 = 5, RMODE_EMBED_F32 = 6, RMODE_LN_Y_COPY = 7 };
// ar_mfma2_kernel XM: LayerNorm applied after the GEMM from OUT_RESID_STATS's statistics (c_fc) | OUT_RESID_STATS
// with the residual from ArState::x2(), where the fused attention left x + the pending copies (x_folded steps)
enum { M2X_NONE = 0, M2X_LN_AFTER = 1, M2X_X2 = 2 };
// ar_mfma_ln_kernel MODE (the prologue every block runs for all B rows): as RMODE, plus EMBED after
// committing the previous step's select from lm_head's granules (SEL_LN_GRAN)
enum { MLMODE_LN = 0, MLMODE_EMBED = 3, MLMODE_LN_Y = 4, MLMODE_EMBED_SELECT = 7 };
// ar_bt_kernel IN: LayerNorm(x) | bf16 operand rows as they are (xn / hb) | embedding then LayerNorm
enum { BIN_LN = 0, BIN_ROWS = 1, BIN_EMBED = 3 };
// ar_f32b_kernel IN: LayerNorm(x) | h (fp32) | split-KV merge | embedding then LayerNorm | the
// one-split attention's normalised rows (ATTN_F32_ROWS) | ar_rows_kernel's fp32 rows in st.h
enum { FIN_LN = 0, FIN_H = 1, FIN_MERGE = 2, FIN_EMBED = 3, FIN_ATTN_ROWS = 4, FIN_LN_ROWS = 6 };
// launch_attn's `direct` (where a one-split attention writes the head output; 0: split partials for
// a merge): bf16 operand row xn | xn fragment-packed (xfrag) | fp32 rows in split 0 of part_o
enum { ATTN_PARTIALS = 0, ATTN_XN = 1, ATTN_XN_PACKED = 2, ATTN_F32_ROWS = 3 };
// ---------------------------------------------------------------------------------

// Path: the kernel family of the step's GEMMs.
//   PATH_GEMV       ar_gemv_kernel family (B <= 2, B > 64, the row forward, fp32 with option f32b 0)
//   PATH_MFMA_LN    batched bf16, LayerNorm in the GEMM prologue (ar_mfma_ln_kernel; B <= ln_max)
//   PATH_MFMA_ROWS  batched bf16, rows kernel + pure MFMA GEMMs (ar_mfma2_kernel)
//   PATH_BT         batched bf16 v3, one kernel per op (ar_bt_kernel; option bt)
//   PATH_F32B       batched fp32 on exact-fp32 MFMA (ar_f32b_kernel; option f32b)
enum ArPath { PATH_GEMV, PATH_MFMA_LN, PATH_MFMA_ROWS, PATH_BT, PATH_F32B };
// Select form: who commits a step's greedy token. Device code reads it as GemvArgs::defer_sel: fixed values.
//   SEL_ARGMAX   ar_argmax_kernel after lm_head
//   SEL_GRAN     B <= 2 GEMV: lm_head publishes per-block granules, the next step's c_attn layer 0 reduces them
//   SEL_EMBED    batched: the next step's ar_embed_select_kernel reduces the logits, then c_attn
//   SEL_LN_GRAN  4 <= B <= 8: granules reduced in the prologue of c_attn layer 0 (MLMODE_EMBED_SELECT)
//   SEL_Q0_ROWS  bf16, 4 <= B <= 32: select + layer 0's c_attn from the q0 tables (ar_q0_rows_kernel; where the
//                plan sets l0_fused, inside attention layer 0 instead: ar_attn_l0_kernel)
//   SEL_SAMPLE   ar_sample_kernel after lm_head: the seeded temperature / top-k draw of the slots that
//                sample, the greedy select for the others (not deferred: the step's other kernels run
//                as under SEL_ARGMAX, and GemvArgs::defer_sel carries SEL_ARGMAX)
enum ArSelect { SEL_ARGMAX = 0, SEL_GRAN = 1, SEL_EMBED = 2, SEL_LN_GRAN = 3, SEL_Q0_ROWS = 4, SEL_SAMPLE = 5 };
enum ArEndCommit { END_NONE, END_SELECT_FINAL, END_ARGMAX };  // kernel that commits a call's last step

struct ArStepPlan {
  int B, kv_dtype;
  bool bf16, row;  // weight dtype; the drop-in row forward (B = 1, the caller's embedding row)
  ArPath path;
  ArSelect sel;
  ArEndCommit end;
  // attention: KV splits, where one split writes its output (ATTN_*), 8-wave blocks (128-key tiles),
  // layer 0 copies the select's shadow records back
  int nsplit, attn_direct;
  bool attn8, selcopy;
  // SEL_Q0_ROWS with a one-split 4-wave attention (option l0a): no ar_q0_rows_kernel launch, attention layer 0
  // runs the select and the q0 tables for its own (row, head) (ar_attn_l0_kernel), and the shadow records are
  // copied back by layer 1's ar_rows_kernel instead of attention layer 0
  bool l0_fused;
  bool fused_mlp; // c_fc + gelu + mlp c_proj in ar_mlp_fused_kernel (mlp c_proj has no kernel of its own)
  bool q0_gran;    // SEL_GRAN with layer 0's c_attn from the q0 tables (ar_q0_gran_kernel)
  int xpk;         // bf16 operand rows kept fragment-packed (GemvArgs::xpk)
  bool ksplit, qsplit;  // PATH_F32B: mlp c_proj / c_attn as K slices
  // l0_fused steps with option laf: layers >= 1 have no ar_rows_kernel / c_attn launch either; their attention
  // block (row, head) runs the row's LayerNorm and its head's c_attn rows itself (ar_attn_la_kernel), layer 1's
  // copies the shadow records back, and c_proj folds the pending copies into x
  bool la_fused;
  // la_fused steps at B >= 16 with option xfold: that attention block publishes its 96-column stripe of x + the pending copies
  // (the sum it formed for the LayerNorm) into ArState::x2(), and c_proj of layers 1-3 takes its residual from
  // there instead of loading x and the four copies and adding them again (ar_mfma2_kernel XM = M2X_X2)
  bool x_folded;
  // la_fused steps with option lmf: no ar_rows_kernel launch ahead of lm_head; ln_f of a row group and a vocab
  // slice of lm_head in one launch (ar_lm_rows_kernel)
  bool lm_fused;
};

constexpr int MFMA_BATCH_MIN = 3;  // smallest B on the batched MFMA path (measured B = 3: 117 vs 154 us, B = 2: 119 vs 114)
constexpr int LM8_ROWS = 8;        // most rows of the SEL_LN_GRAN granule layout
// Attention launch shape, measured (tools/step_sweep.py, us/step): 4 waves per block (8 waves,
// 128-key tiles: B = 32 t = 256+ 153.7 vs 149.4; B = 64 211.1 vs 209.0), 2 KV tiles in flight per
// wave (4: B = 32 157.9 vs 152.0, B = 64 234.2 vs 216.3), splits until ns x 8 heads x B <= 256
// blocks (B = 32 at t = 256-511: 1024 blocks 164, 512 169, 256 = one split that writes xn
// itself 155.5; B = 16: 138 / 136 / 131; B = 8: 144 / 133 / 130).
constexpr int ATTN_BLOCKS = 256;
inline int attn_ns_max(int B) {  // enough splits to fill the chip, no more (early-exit blocks cost)
  int ns = NSPLIT;
  while (ns > 1 && ns * N_HEAD * B > ATTN_BLOCKS) ns >>= 1;
  return ns;
}

[[noreturn]] inline void ar_plan_bug(const ArStepPlan& p, const char* where) {  // a select form its path cannot run
  fprintf(stderr, "llmvox: %s: no kernel for select form %d on path %d at B = %d\n", where, (int)p.sel, (int)p.path, p.B);
  abort();
}

// The select form, chosen after the path and from that path's legal set. Deferred against the argmax
// kernel, us/step (tools/step_sweep.py, t = 256+) argmax kernel / deferred: B = 3: 112.9 / 114.7 (B = 3
// keeps the argmax kernel), B = 4: 106.0 / 104.9, 8: 120.7 / 118.3, 12: 123.0 / 120.5,
// 16: 128.4 / 125.5, 32: 150.3 / 147.3, 64: 213.4 / 206.8
inline ArSelect ar_plan_select(const Opts& o, const ArStepPlan& p, bool q0) {
  if (!o.defer_select) return SEL_ARGMAX;
  // GEMV: every row of the step is prefetched by its own wave of c_attn layer 0 (B <= 2, one batch group)
  if (p.path == PATH_GEMV) return p.B <= 2 ? SEL_GRAN : SEL_ARGMAX;
  if (p.B < 4) return SEL_ARGMAX;
  if (p.path == PATH_BT) return SEL_EMBED;
  // fp32 parity mode (round 3): with the K-split c_attn (its layer-0 rows kernel becomes
  // ar_embed_select_kernel<true>); B = 32 t = 384-639: 213.9 -> 210.8 us/step
  if (p.path == PATH_F32B) return p.qsplit ? SEL_EMBED : SEL_ARGMAX;
  // bf16 with option l0q, 4 <= B <= 32: the previous step's select and layer 0's c_attn from the q0
  // tables in one launch, ar_q0_rows_kernel (9 column slices per row): at B > 8 the c_attn
  // GEMM launch goes, at 4 <= B <= 8 the c_attn-with-select launch reads table rows instead of weight
  // slices (round 6, us per step at t = 384-639, each A/B on one box: the tables in one block per row
  // took B = 32 -2.9, B = 8 -1.8 / -2.5 (fp8 / bf16 KV), B = 4 -1.4 (l0q_ab.txt, b8_l0q_ab.txt); the 9
  // slices per row a further -1.1 / -1.7 / -1.7 (q0rows_ab.txt); the reference-agreement measures
  // unchanged). B <= 2 keep their granule select with the tables in ar_q0_gran_kernel.
  if (o.l0q && q0 && p.B <= 32) return SEL_Q0_ROWS;
  // 4 <= B <= 8 on the LayerNorm-prologue GEMMs: the select folded into c_attn layer 0's prologue from
  // lm_head's granules instead of ar_embed_select_kernel + the c_attn launch (option defer_select 2:
  // the embedding + select kernel at these B too, the cross-check)
  if (o.defer_select == 1 && p.path == PATH_MFMA_LN && p.B <= LM8_ROWS) return SEL_LN_GRAN;
  return SEL_EMBED;
}

// row: the drop-in row forward (no select); q0: ArWeights::q0_text exists (bf16, lvx_finalize);
// sample: some slot of the context samples (lvx_stream_sampling): the plan of option defer_select 0 with
// ar_sample_kernel in the argmax kernel's place (a deferred form cannot host the draw: its select runs
// inside the next step's first kernel). The row forward has no select and ignores it.
inline ArStepPlan ar_plan_step(const Opts& o_, int wdtype, int kvdtype, int B, bool row, bool q0, bool sample = false) {
  sample = sample && !row;
  Opts o = o_;
  if (sample) o.defer_select = 0;
  ArStepPlan p{};
  p.B = B; p.kv_dtype = kvdtype; p.bf16 = wdtype == LVX_DTYPE_BF16; p.row = row;
  const bool batched = !row && B >= MFMA_BATCH_MIN && B <= 64;
  // v3 only where v2 has no kernels (32 < B <= 64) unless option bt 2 (the measurements before launch_bt)
  if (!batched || (!p.bf16 && !o.f32b)) p.path = PATH_GEMV;
  else if (!p.bf16) p.path = PATH_F32B;
  else if (o.bt && (B > 32 || o.bt == 2)) p.path = PATH_BT;
  // LayerNorm / embedding fused into the MFMA GEMM prologue for B <= option ln_max, default 8 (measured:
  // B = 8 147 vs 156 us/step; B = 32 slower, every block re-normalising 32 rows; a runtime value for A/B
  // of the two batched structures at small B)
  else p.path = B <= o.ln_max ? PATH_MFMA_LN : PATH_MFMA_ROWS;
  const bool mf = p.path == PATH_MFMA_LN || p.path == PATH_MFMA_ROWS;
  p.ksplit = p.path == PATH_F32B && !(o.exp & 512);
  p.qsplit = p.ksplit && B <= 32 && !(o.exp & 1024);

  p.sel = row ? SEL_ARGMAX : sample ? SEL_SAMPLE : ar_plan_select(o, p, q0);
  p.end = p.sel == SEL_ARGMAX || p.sel == SEL_SAMPLE ? END_NONE : p.sel == SEL_GRAN ? END_SELECT_FINAL : END_ARGMAX;
  p.selcopy = p.sel == SEL_GRAN || p.sel == SEL_LN_GRAN || p.sel == SEL_Q0_ROWS;
  p.q0_gran = p.sel == SEL_GRAN && o.l0q && q0;
  // fused MLP, measured at B = 1 (round 1): 16 h rows per block (192 blocks) 76.7 us/step; 32 rows (96
  // blocks) +6.8 us; 12 rows (256 blocks, one per CU) 77.4 us; 8 accumulator copies slower than 4
  p.fused_mlp = p.path == PATH_GEMV && p.bf16 && o.fuse_mlp && B <= 2;

  // Attention. Batched steps at B >= 9: one attention split per (row, head), the head output written straight
  // into the bf16 operand row (no merge kernel). Round 3, tools/step_sweep.py (graph replay, us per
  // step at t = 128 / 640): bf16 KV B = 12 104.3 / 113.0 -> 95.4 / 107.7, B = 16 107.1 / 126.7 ->
  // 97.4 / 119.0; fp8 KV B = 12 103.2 / 110.3 -> 95.4 / 108.4, B = 16 104.2 / 111.5 -> 96.1 / 109.2.
  // At B = 8 (64 blocks) one split loses at long histories (fp8 KV 102.4 -> 105.7 at t = 640 while
  // 98.1 -> 92.5 at t = 128): B <= 8 keeps the split-KV attention + merge.
  // 5 <= B <= 8: one split too, in 8-wave blocks (128-key tiles: twice the KV bytes in flight per
  // block, 40-64 blocks); tools/step_sweep.py, fp8 KV, B = 8, t = 128 / 640 / 896: 98.0 / 102.3 / 104.2
  // -> 92.6 / 102.8 / 106.5 us (bf16 KV 98.7 / 105.9 / 108.5 -> 95.1 / 105.3 / 108.8): ~1 % over a
  // 1,024-token utterance; at B = 4 it loses (91.9 / 94.5 / 95.5 -> 87.6 / 96.3 / 100.8). fp8 KV (half the bytes per
  // key) keeps the 8-wave blocks up to B = 16: B = 12 / 16, t = 128 / 640 / 896: 95.8 / 108.3 / 114.8 ->
  // 97.0 / 105.5 / 109.6 and 95.8 / 109.6 / 115.5 -> 97.0 / 106.8 / 110.2 us; bf16 KV there loses
  // (B = 16: 97.0 / 109.9 / 128.1 -> 100.8 / 112.5 / 130.5). (The switches restoring the older forms,
  // option exp bits 32 / 64 / 128, were removed in round 6.)
  p.attn8 = mf && B >= 5 && (B <= 8 || (kvdtype == LVX_DTYPE_FP8 && B <= 16));
  p.nsplit = p.path == PATH_GEMV ? NSPLIT : (mf && (B > 8 || p.attn8)) ? 1 : attn_ns_max(B);
  // The fused layer-0 form where the step has ar_q0_rows_kernel and its attention is one split per (row, head) in
  // 4-wave blocks: bf16 KV at 9 <= B <= 32, fp8 KV at 17 <= B <= 32 (the 8-wave cells keep the two launches).
  // Every block then has the select chain ahead of its tile loop, with the history's first tiles in flight under it.
  // (fp32 KV under bf16 weights keeps the two launches: the fused form has the per-key-slot kernels only)
  p.l0_fused = o.l0a && p.sel == SEL_Q0_ROWS && p.nsplit == 1 && !p.attn8 && B >= 9 && kvdtype != LVX_DTYPE_F32;
  // The fused layers form on the same cells (each attention block of layers 1-3 is then its own c_attn: no
  // hand-off between workgroups, the head's weight slice shared through the XCD's L2)
  p.la_fused = o.laf && p.l0_fused;
  // The two tail forms ride on the fused layers form (ar_probe / ar_ops plan without the tables and so keep the
  // separate kernels they model; sampling plans are never la_fused)
  // Measured per part (tools/step_sweep.py, t = 384-639, option sets in one process, us per step off -> on, against
  // the parent library's max - min over its runs in that cell):
  //   xfold  bf16 KV B = 32: 116.3 -> 114.0 (spread 1.9), B = 16: 95.9 -> 94.5 (1.0), B = 9: 90.9 -> 91.0 (0.2);
  //          fp8 KV B = 32: 100.0 -> 98.0 (0.5), B = 17: 95.2 -> 94.7 (0.4)
  //   lmf    bf16 KV B = 32: 116.3 -> 115.7 (1.9), B = 16: 95.9 -> 95.1 (1.0), B = 9: 90.9 -> 89.9 (0.2);
  //          fp8 KV B = 32: 100.0 -> 99.2 (0.5), B = 17: 95.2 -> 94.2 (0.4)
  // xfold does nothing for few rows (c_proj's loads are not what such a step waits for): off below B = 16. At fp8 KV
  // B = 17 its 0.4-0.5 only equals the spread; it stays on there, since the gain repeats to 0.1 in process and the cell
  // sits between two that clear it. lmf at bf16 KV B = 16 / 32 is inside the parent's process-to-process spread but
  // repeats to 0.1 in process (twice each) and is never a loss: it stays on in every la_fused cell.
  p.x_folded = o.xfold && p.la_fused && B >= 16;
  p.lm_fused = o.lmf && p.la_fused;
  // fragment-packed operand rows on the v2 steps with the rows kernel at B <= 32
  p.xpk = (p.path == PATH_MFMA_ROWS && B <= 32) ? 1 : 0;
  p.attn_direct = p.nsplit > 1 || !(mf || p.path == PATH_F32B) ? ATTN_PARTIALS
                  : p.path == PATH_F32B ? ATTN_F32_ROWS : p.xpk ? ATTN_XN_PACKED : ATTN_XN;
  return p;
}

}  // namespace lvx
