/*
 * llmvox.h — C ABI of the MI355X-native LLMVoX streaming-TTS hot path
 * (libllmvox_hip.so, built for gfx950).
 *
 * The reference has no native boundary: its hot path is reached through the
 * duck-typed ModelHandler members that streaming_server.audio_generator_sync
 * calls (reference: streaming_server.py:250-426, inference/model_handler.py:45-166).
 * Each entry point below replaces one of those calls; the Python shim
 * (llmvox_amd/handler.py) binds them with ctypes and keeps the reference
 * signatures.
 *
 * Conventions
 *   - Every function returns 0 on success, a negative LVX_E* code on error;
 *     lvx_last_error() gives the message of the calling thread's last error.
 *   - Pointers named *_dev are device pointers on the context's device
 *     (e.g. torch tensor .data_ptr()); *_host are host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = legacy default stream).
 *     All compute calls are asynchronous on that stream.
 *   - Layouts are row-major, dtypes are fixed per argument (float32 / int32 /
 *     int64) as named.
 */
#ifndef LLMVOX_H
#define LLMVOX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LVX_OK 0
#define LVX_E_ARG (-1)      /* bad argument / shape (reference: ValueError) */
#define LVX_E_STATE (-2)    /* weights missing / not finalized */
#define LVX_E_HIP (-3)      /* HIP runtime error */
#define LVX_E_CAPACITY (-4) /* position >= block_size or KV capacity (reference: AssertionError,
                               src/model.py:205) */
#define LVX_E_NAME (-5)     /* unknown weight name */
#define LVX_E_INDEX (-6)    /* an embedding id out of range, reported by lvx_check_errors (reference:
                               IndexError from nn.Embedding / the codebook gather) */

#define LVX_DTYPE_F32 0
#define LVX_DTYPE_BF16 1
#define LVX_DTYPE_FP8 2 /* kv_dtype: OCP e4m3fn (the gfx950 format), saturating at +-448, unscaled;
                           codec_dtype: e4m3fn codec GEMM weights with one fp32 scale per output row */

typedef struct lvx_ctx lvx_ctx;

typedef struct {
  int device;           /* HIP device ordinal */
  int weight_dtype;     /* LVX_DTYPE_F32 (parity mode; the reference runs fp32) or LVX_DTYPE_BF16 */
  int kv_dtype;         /* LVX_DTYPE_F32, LVX_DTYPE_BF16 or LVX_DTYPE_FP8 */
  int max_streams;      /* KV slots (concurrent utterance streams) */
  int max_positions;    /* per-slot KV capacity, <= 8192 (GPTConfig.block_size) */
  int max_codec_frames; /* max sum over streams of frames per codec call */
  int codec_dtype;      /* codec conv / linear weight storage: 0 = weight_dtype, or LVX_DTYPE_FP8 (needs
                           weight_dtype BF16: fp8 weights, bf16 operands, fp32 accumulation) */
} lvx_config;

/* ---- lifetime ----------------------------------------------------------- */
int lvx_create(const lvx_config* cfg, lvx_ctx** out);
/* replaces ModelHandler.__init__'s device placement (model_handler.py:48-63) */
void lvx_destroy(lvx_ctx* ctx);
const char* lvx_last_error(void);
int lvx_version(void);

/* ---- weights (by reference state_dict key, fp32 host data) -------------
 * replaces initialize_gpt_model / initialize_wavtokenizer / initialize_llm_model
 * (model_handler.py:66-78,80-106,140-166). Keys: "transformer.*", "lm_head.weight",
 * "backbone.*", "head.out.*", the codebook
 * "feature_extractor.encodec.quantizer.vq.layers.0._codebook.embed", and
 * "encoder.embed_tokens.weight" (the [386,256] text table). */
int lvx_set_weight(lvx_ctx* ctx, const char* name, const float* data_host, int64_t numel);
int lvx_finalize(lvx_ctx* ctx);
/* number of required weights not yet set; fills *first_missing (may be NULL) */
int lvx_missing_weights(lvx_ctx* ctx, const char** first_missing);

/* ---- text / code embeddings -------------------------------------------- */
/* ModelHandler.llm_model(ids): T5 encoder.embed_tokens gather
 * (streaming_server.py:315,319). ids int64 [n] -> out float32 [n,256]. An id outside [0, 386) is
 * clamped and flagged: the next lvx_check_errors returns LVX_E_INDEX (the same for codes outside
 * [0, 4096) in lvx_codes_to_features). */
int lvx_text_embed(lvx_ctx* ctx, const int64_t* ids_dev, int n, float* out_dev, void* stream);
/* WavTokenizer.codes_to_features (decoder/pretrained.py:209-239), n_q = 1:
 * codes int64 [B,L] -> features float32 [B,512,L] */
int lvx_codes_to_features(lvx_ctx* ctx, const int64_t* codes_dev, int B, int L, float* feats_dev,
                          void* stream);

/* ---- speech-token GPT ------------------------------------------------------ */
/* Forget a stream's KV (the reference sets kvcache = None, streaming_server.py:412). */
int lvx_stream_reset(lvx_ctx* ctx, int slot, void* stream);
/* GPT.forward(emb, kvcache) for one stream (src/model.py:201-237): emb_row_dev is the LAST
 * row of the caller's history (already normalised input, float32 [768]); pos is its index
 * t-1. Appends K/V at pos in slot `slot`, attends over [0, pos], writes logits float32
 * [4096]. */
int lvx_ar_forward_row(lvx_ctx* ctx, int slot, int pos, const float* emb_row_dev, float* logits_dev,
                       void* stream);
/* One fused decode step for B batch rows (a2..a11 of the hot path). Row b drives slot
 * slots[b] (-1 = idle row: computes nothing that is stored). With j = rowstep[b] and p the
 * slot's device-side position: input = normalize(cat(text_table[text_plan[b][j]],
 * p == 0 ? 0 : codebook[prev_token[slot]])) + wpe[p]  (streaming_server.py:325-338,
 * src/model.py:206-217); runs the 4 blocks, ln_f, lm_head and the greedy argmax (first
 * maximal index = argmax(softmax), streaming_server.py:342-346); writes tok_plan[b][j]
 * (and margin_plan[b][j] = top1 - top2 logit, optional), stores the token as the slot's
 * prev_token, advances the slot's position and rowstep[b]. text_plan / tok_plan /
 * margin_plan are [B][plan_stride] device arrays, so a whole chunk of steps can be enqueued
 * back to back (replayed as a HIP graph) and read back once. Inside a call the select of step i
 * is committed by the first kernel of step i + 1 (option "defer_select"); the last one by a
 * closing kernel of the call, so every output is in place when the call's work on `stream` is. */
int lvx_ar_step(lvx_ctx* ctx, int B, const int32_t* slots_dev, const int32_t* text_plan_dev,
                int plan_stride, int32_t* rowstep_dev, int32_t* tok_plan_dev, float* margin_plan_dev,
                void* stream);
/* n_steps consecutive lvx_ar_step calls with the same arguments. */
int lvx_ar_steps(lvx_ctx* ctx, int n_steps, int B, const int32_t* slots_dev, const int32_t* text_plan_dev,
                 int plan_stride, int32_t* rowstep_dev, int32_t* tok_plan_dev, float* margin_plan_dev,
                 void* stream);
/* Copy the logits [B][4096] of the last lvx_ar_step(s) call (diagnostics / tests). */
int lvx_ar_logits(lvx_ctx* ctx, int B, float* dst_dev, void* stream);
/* Synchronises the stream and reports (then clears) device-side errors of both error words: an embedding id or codec
 * code out of range (LVX_E_INDEX), the ISTFT window envelope <= 1e-11 (LVX_E_STATE; reference:
 * the assertion of decoder/spectral_ops.py:72 -- the fixed periodic Hann envelope is >= 0.72 on the
 * trimmed span, so this is a self-check), a slot past max_positions (LVX_E_CAPACITY; reference:
 * the block_size AssertionError, src/model.py:205) or a row past the end of its plan
 * (LVX_E_CAPACITY), or a non-finite / out-of-range (|v| >= 2^25) partial in the B <= 2 fused MLP's
 * fixed-point accumulation (LVX_E_STATE; the reference would carry the value into its logits). */
int lvx_check_errors(lvx_ctx* ctx, void* stream);
/* The device error bits live in two words: the AR word (decode steps, lvx_text_embed,
 * lvx_codes_to_features) and the codec word (lvx_codec_decode_*), so a codec running on a second stream
 * beside the decode keeps its flags apart. lvx_check_errors takes both; every condition that is set is
 * named in lvx_last_error (the code is the most specific one: LVX_E_INDEX > LVX_E_STATE >
 * LVX_E_CAPACITY). A take reads and clears the words atomically, in stream order: bits set later by
 * work in flight on another stream stay for the next take. */
#define LVX_ERRW_AR 1
#define LVX_ERRW_CODEC 2
/* Asynchronous take (no synchronisation): the bits of the chosen words (`which` = LVX_ERRW_AR and/or
 * LVX_ERRW_CODEC) into bits_dev[0] (device int32: AR bits | codec bits << 16), enqueued on `stream`
 * after the work already there; pass them to lvx_error_status once they are on the host. Lets a
 * scheduler read a chunk's errors with its tokens, without a stream synchronisation. */
int lvx_error_take(lvx_ctx* ctx, int which, int32_t* bits_dev, void* stream);
/* The status (and lvx_last_error message) of taken bits, as lvx_check_errors would return it; 0 if none. */
int lvx_error_status(int bits);
/* Set a slot's position and previous token (rewind after a speculative run-ahead, or jump). */
int lvx_stream_set(lvx_ctx* ctx, int slot, int pos, int prev_token, void* stream);
/* Sampling of a slot's decode steps (reference: GPT.generate, src/model.py:384-410). temperature 0
 * (the default of every slot): greedy. top_k 0 or >= 4096: no crop. Stream-ordered like
 * lvx_stream_set: call it on the stream of the slot's decode steps. lvx_stream_reset keeps it.
 * LVX_E_ARG for a slot out of range, temperature < 0 or not finite, top_k < 0.
 *
 * The rule of a sampled step (temperature T > 0, p the position of the step being decided, the value
 * lvx_stream_position would give before it; all arithmetic fp32):
 *   z[i] = logits[i] / T                          IEEE division, as the reference divides;
 *   thr  = the top_k-th largest z (exact), i is kept iff z[i] >= thr: the ties at the threshold are
 *          all kept, as in logits[logits < v[:, [-1]]] = -inf; with no crop every i is kept;
 *   w[i] = exp(z[i] - max z) for kept i, else 0;  S = sum of w;
 *   u    = (x0 >> 8) * 2^-24, x0 the first output word of Philox4x32-10 with the counter
 *          (p, 0, 0, 0) and the key (seed & 0xffffffff, seed >> 32) (multipliers 0xD2511F53 /
 *          0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, 10 rounds);
 *   token = the first kept index, in vocabulary order, whose inclusive running sum of w exceeds u * S;
 *          the last kept index if rounding leaves none.
 * The running sums are formed as 16-term sums of consecutive indices and a tree over the 256 partial
 * sums, so a token can differ from an exact-arithmetic evaluation only where u lies within ~2^-16 of a
 * boundary of the cumulative distribution (tests/sampling_ref.py). Neither the slot nor the batch row
 * enters the generator: the same (seed, position, logits) give the same token in any row of any
 * batch, and a rewind (lvx_stream_set) reproduces the draws of the positions decoded again.
 * margin_plan of a sampled row keeps its meaning, top-1 minus top-2 of the raw logits: it says how
 * peaked the distribution was, not how close the drawn token was to another.
 * While any slot of the context has temperature > 0, every lvx_ar_step(s) call of the context runs
 * the plan of option "defer_select" 0 with the sampled select (ar_sample_kernel) after lm_head; rows
 * of greedy slots run the argmax kernel's code inside it. In fp32 parity mode their ids are those of
 * the default plan. In bf16 with option "l0q" 1 they are the "defer_select" 0 ids: layer 0's c_attn
 * then comes from the GEMM instead of the table rows, and the logits differ in the last bits. With no
 * slot sampling, plans, kernels and ids are exactly those of a context that never sampled. */
int lvx_stream_sampling(lvx_ctx* ctx, int slot, float temperature, int top_k, uint64_t seed, void* stream);
/* lvx_stream_sampling with a nucleus (top_p), a min-p crop and a repetition penalty over the slot's recent
 * tokens. lvx_stream_sampling is this call with the neutral values top_p 1, min_p 0, repetition_penalty 1,
 * repetition_window 64: with those the kernel skips every phase below and draws today's tokens, bit for bit.
 * LVX_E_ARG: a null p, a value that is not finite or outside: temperature >= 0, top_k >= 0, top_p in (0, 1],
 * min_p in [0, 1), repetition_penalty > 0, repetition_window in [1, 256]. A slot with temperature 0 decodes
 * greedily and ignores every other field, as it ignores top_k: penalised or cropped greedy decoding is not
 * offered.
 *
 * The rule of a sampled step (T > 0, p the position of the step being decided; fp32 unless it says integer):
 *   1. penalty. R = repetition_penalty (1: off), W = repetition_window. The window set is the tokens decided
 *      by the steps at positions max(hist_from, p - W) .. p - 1 (empty at p = 0 or when hist_from >= p; see
 *      "history" below); a token that occurs several times is penalised once. For i in the set
 *        l'[i] = logits[i] > 0 ? logits[i] / R : logits[i] * R    (IEEE division / product; +-0 take the product),
 *      otherwise l'[i] = logits[i]. Exact.
 *   2. temperature. z[i] = l'[i] / T, zmax = max z: taken after the penalty, which can move the maximum.
 *   3. top_k on z as above, ties at the threshold kept.
 *   4. top_p (1: off, the step is skipped), over integers, so that no summation order enters:
 *        w[i] = exp(z[i] - zmax) for the i kept so far, else 0;   q[i] = floor(w[i] * 2^24) (integer);
 *        Sq = sum q;   Aq(v) = sum of q[i] over z[i] > v;   P = round(top_p * 2^24) clamped to [1, 2^24]
 *        (P = 2^24 counts as off);
 *        i stays kept iff Aq(z[i]) * 2^24 < P * Sq   (64-bit integers; the largest product is below 2^61).
 *      The mass strictly above a token decides it: equal z are kept or dropped together, the maximum always stays.
 *   5. min_p (0: off). lnminp = (float)log((double)min_p), computed once by this call;
 *        i stays kept iff fl(z[i] - zmax) >= lnminp. Exact.
 *   6. the draw, as above, over the final kept set: the same w, running sums, u, first crossing and fallback.
 *   7. margin_plan keeps its meaning: top-1 minus top-2 of the raw logits.
 * Every crop is a threshold on z: the kept set is {i : z[i] >= v} for one v, which lvx_sample_kept reports.
 * The result is a function of (logits, parameters, seed, position, history) alone, the same in any row of any
 * batch and in any run.
 *
 * History. While any slot of the context samples, the select of every step stores the token it decides at
 * position p into a per-slot record hist[slot][p] (uint16, max_streams * max_positions * 2 bytes), for the rows
 * of greedy slots beside sampling ones too; a context with no sampling slot runs today's kernels and records
 * nothing. Entries are written by absolute position, so a speculative run-ahead followed by a rewind only
 * rewrites entries at and above the rewind point. hist_from[slot], the first position whose entry is known,
 * is kept on the device in stream order: lvx_stream_reset sets it to 0; lvx_stream_set(slot, pos, prev) stores
 * prev at hist[slot][pos - 1] (pos > 0) and then, for pos <= the slot's old position, hist_from =
 * min(hist_from, max(pos - 1, 0)), otherwise (a jump over positions never decoded) hist_from = max(pos - 1, 0);
 * a call of this function that takes the slot's temperature from 0 to > 0 sets hist_from to the slot's
 * current position (plans that do not record may have decided its earlier tokens).
 * lvx_ar_forward_row (the drop-in row mode) moves a slot's position without recording a token or touching
 * hist_from: call lvx_stream_set or lvx_stream_reset on the slot before sampled steps with a penalty follow
 * row-mode calls, or the window reaches entries that were never recorded. */
typedef struct {
  float temperature;
  int top_k;
  float top_p;
  float min_p;
  float repetition_penalty;
  int repetition_window;
  uint64_t seed;
} lvx_sampling;
int lvx_stream_sampling_ex(lvx_ctx* ctx, int slot, const lvx_sampling* p, void* stream);
/* Test hook: read (write = 0) or write (write != 0) the history entries hist[slot][pos0 .. pos0 + n) from / to
 * tokens_dev int32 [n] (written values are clamped to [0, 4096)); a write also lowers hist_from to pos0.
 * LVX_E_ARG for a slot out of range or null tokens_dev, LVX_E_CAPACITY for pos0 < 0, n < 1 or
 * pos0 + n > max_positions. */
int lvx_stream_history(lvx_ctx* ctx, int slot, int pos0, int n, int32_t* tokens_dev, int write, void* stream);
/* Test hook: per batch row b of the last sampled select (a row of a slot with temperature > 0), dst_dev int32
 * [B][4] = {number of kept tokens, the fp32 bits of the lowest kept z, number of distinct penalised tokens, 0}.
 * The kernel leaves them with one 16-byte store beside its commit. */
int lvx_sample_kept(lvx_ctx* ctx, int B, int32_t* dst_dev, void* stream);
/* Measurement hook (bench.py): launch one kernel class of the decode step `iters` times for the
 * batch rows `slots` at their current positions (0 c_attn, 1 attention, 2 c_proj+merge,
 * 3 c_fc (with the bf16 fused MLP at B <= 2: c_fc + gelu + mlp c_proj), 4 mlp c_proj, 5 lm_head).
 * Writes only scratch and the K/V row at the current position (which the next real step
 * overwrites). LVX_E_STATE when the op has no kernel of its own at this B (fused). */
int lvx_probe_kernel(lvx_ctx* ctx, int which, int B, const int32_t* slots_dev, int iters, void* stream);
/* Test hook: the greedy select (argmax(softmax(logits)) with the reference's tie semantics,
 * streaming_server.py:342-346) of one production kernel path over caller-given logits float32
 * [B][4096], committed exactly as a decode step commits it (tok_plan[b][rowstep[b]], margin,
 * slot prev / position, rowstep advance). path 0: ar_argmax_kernel; 1: the lm_head-granule
 * reduction of the B <= 2 deferred select (B <= 4 here); 2: the batched deferred select
 * (ar_embed_select_kernel); 3: the 4 <= B <= 8 prologue-granule reduction (B <= 8); 4: the sampled
 * select, ar_sample_kernel, with the slots' current lvx_stream_sampling parameters and positions
 * (the commit advances the positions, so consecutive calls draw with consecutive counters).
 * plan_stride >= 2. */
int lvx_select_probe(lvx_ctx* ctx, int path, int B, const int32_t* slots_dev, const float* logits_dev,
                     const int32_t* text_plan_dev, int plan_stride, int32_t* rowstep_dev, int32_t* tok_plan_dev,
                     float* margin_plan_dev, void* stream);
/* Test hooks (tests/test_gpu_attn_probe.py, tests/test_gpu_kv_append.py): direct access to the KV cache
 * rows of one (slot, layer) and to the decode attention. They add no kernel to a decode step and are
 * never captured into a graph.
 * lvx_kv_write: k_dev / v_dev float32 [n][768] (head-major, as c_attn produces k and v; either may be
 *   null) are stored as positions pos0 .. pos0 + n - 1 with the conversion of the step's own appends
 *   (fp32 copy, bf16 round-to-nearest-even, or saturated e4m3fn). Rows up to the end of the slot's last
 *   allocated 64-position chunk may be written (LVX_E_CAPACITY beyond).
 * lvx_kv_write_raw: the same with caller-given bit patterns: the low 32 / 16 / 8 bits of each uint32
 *   become the stored element (NaN encodings, for instance).
 * lvx_kv_read: the inverse: the stored elements widened exactly to float32. */
int lvx_kv_write(lvx_ctx* ctx, int slot, int layer, int pos0, int n, const float* k_dev, const float* v_dev,
                 void* stream);
int lvx_kv_write_raw(lvx_ctx* ctx, int slot, int layer, int pos0, int n, const uint32_t* k_dev, const uint32_t* v_dev,
                     void* stream);
int lvx_kv_read(lvx_ctx* ctx, int slot, int layer, int pos0, int n, float* k_dev, float* v_dev, void* stream);
/* Test hook: the production decode attention of the step plan at this B under the context's options
 * (its split count, output form and block shape; the non-K-split kernel, no layer-0 record copy), plus
 * the plan's merge kernel where it has one, at `layer`, over q_dev float32 [B][768] and the KV rows of
 * slots_dev (-1: idle row). Row b attends over keys [0, P_b], P_b the slot's current position
 * (lvx_stream_set): what a step at that position sees after its append.
 * form_out is int[4]: {form, nsplit, attn_direct, attn8} of the plan that ran.
 *   form 0: the plan leaves normalised rows (the attention's own bf16 / fp32 rows or the merge kernel's);
 *           they are widened exactly into out_dev float32 [B][768] (an idle row: whatever the kernels
 *           left in the scratch row).
 *   form 1: the plan merges the splits inside c_proj's prologue (the GEMV family, fp32 FIN_MERGE): the
 *           partials are copied out as the attention left them, part_o_dev float32 [B][8][16][96] and
 *           part_ml_dev float32 [B][8][16][2] (running max, sum); row b has min(nsplit, ceil((P_b + 1)
 *           / 64)) valid splits, the others are not written. The prologue merges themselves are not
 *           run by this hook: lvx_ar_ops runs them (a window from this attention through c_proj).
 * LVX_E_STATE where the plan's attention takes no q rows (the fp32 K-split c_attn; option "exp" 1024
 * selects the one-launch form). form_out is written before the call returns; the device buffers are
 * written in stream order. */
int lvx_attn_probe(lvx_ctx* ctx, int B, const int32_t* slots_dev, int layer, const float* q_dev, float* out_dev,
                   float* part_o_dev, float* part_ml_dev, int* form_out, void* stream);
/* Test hook (tests/test_gpu_ar_ops.py): ops [first, last] of ONE decode step on caller-supplied input, each
 * launched as the step plan at this B under the context's options launches it (the form with the argmax
 * kernel: no deferred select, no layer-0 record copy), kernel by kernel, never captured into a graph; the
 * counterpart of lvx_codec_stages for the AR step. It adds nothing to a step.
 * Ops are numbered 5 * layer + {0 c_attn (layer 0: + embedding), 1 attention, 2 c_proj (+ split merge),
 * 3 c_fc, 4 mlp c_proj}; op 20 (LVX_AR_OPS - 1) is lm_head. A window starts
 *   at a layer boundary, first = 5 l: for l >= 1 (and for 20) x_in_dev float32 [B][768] is the final residual
 *     entering the layer, and the pending mlp c_proj copies are zeroed; for l = 0 the embedding builds x from
 *     the slots' positions and previous tokens (lvx_stream_set) and text_ids_dev int32 [B], and with
 *     poison != 0 the pending copies are first filled with the byte 0x7f, which layer 0 must ignore;
 *   or at an attention, first = 5 l + 1: x_in_dev and q_in_dev float32 [B][768], over the KV rows of the slots
 *     up to their positions, as lvx_attn_probe (LVX_E_STATE where the plan's attention takes no q rows).
 * It ends at any op >= first and hands out what that op left, widened exactly to float32:
 *   LVX_AR_OUT_Q           c_attn: q in out_dev [B][768] (k, v: lvx_kv_read at the slots' positions)
 *   LVX_AR_OUT_QKV_PARTS   c_attn of the fp32 K split: its four partials, out_dev [4][B][2304]
 *   LVX_AR_OUT_ATTN_ROWS / LVX_AR_OUT_ATTN_PARTS   attention: forms 0 / 1 of lvx_attn_probe
 *   LVX_AR_OUT_X           c_proj, mlp c_proj: x in out_dev [B][768]; after mlp c_proj also the info[11]
 *                          copies the plan holds pending, raw: copies_dev float32 [B][n][768], or, for the
 *                          fused MLP (info[10]), copies_fx_dev int64 [B][n][768] in 2^-32 fixed point
 *   LVX_AR_OUT_H           c_fc: gelu(c_fc) in out_dev [B][3072] (LVX_E_STATE inside the fused MLP, which
 *                          has no c_fc kernel: end at mlp c_proj)
 *   LVX_AR_OUT_LOGITS      lm_head: out_dev [B][4096]
 * out_dev holds 4 * B * 2304 floats, copies_dev B * 4 * 768 floats, copies_fx_dev as many int64.
 * info is int[LVX_AR_INFO], written before the call returns: {output form, path (0 GEMV, 1 LayerNorm-
 * prologue MFMA, 2 rows kernel + MFMA, 3 v3, 4 fp32 MFMA), fused_mlp, nsplit, attn_direct, attn8, xpk, ksplit,
 * qsplit, pending copies of the plan, 1 if they are fixed point, copies pending at the exit}. */
#define LVX_AR_OPS 21
#define LVX_AR_INFO 12
#define LVX_AR_OUT_Q 0
#define LVX_AR_OUT_QKV_PARTS 1
#define LVX_AR_OUT_ATTN_ROWS 2
#define LVX_AR_OUT_ATTN_PARTS 3
#define LVX_AR_OUT_X 4
#define LVX_AR_OUT_H 5
#define LVX_AR_OUT_LOGITS 6
int lvx_ar_ops(lvx_ctx* ctx, int B, const int32_t* slots_dev, int first, int last, const float* x_in_dev,
               const float* q_in_dev, const int32_t* text_ids_dev, int poison, float* out_dev, float* copies_dev,
               int64_t* copies_fx_dev, float* part_o_dev, float* part_ml_dev, int* info, void* stream);
/* Test hook: stages [first, last] of the codec decode on caller-supplied input, through the decode's own
 * launch helpers and scratch (so kernel routing, split-K choice and the split-image decisions are exactly
 * those of lvx_codec_decode_codes at this B, L and these options). Never part of a step or a graph.
 * Stages, in decode order (LVX_CODEC_STAGES of them):
 *    0      code gather + embed conv (k7)       in: codes int32 [B][L]      out: x float32 [B*L][768]
 *    1, 2   pos_net ResnetBlocks 0, 1           x -> x
 *    3      AttnBlock                           x -> x
 *    4, 5   pos_net ResnetBlocks 2, 3           x -> x
 *    6      pos_net GroupNorm + backbone AdaLN  x -> x
 *    7..18  ConvNeXt blocks 0..11               x -> x
 *   19      final LayerNorm + head Linear       x -> spec float32 [B*L][1282]
 *   20      iSTFT frames + overlap-add          spec -> pcm float32 [B][320*L]
 * in_dev holds the input of stage `first`, out_dev receives the output of stage `last` (device buffers,
 * copied / written in stream order). routes_out (host, may be null with route_cap 0) receives one record
 * per GEMM launched in the window, in launch order; *n_routes_out their number (which may exceed
 * route_cap: only route_cap are written). Arguments are checked as lvx_codec_decode_codes checks them
 * (LVX_E_CAPACITY, LVX_E_ARG), plus 0 <= first <= last < LVX_CODEC_STAGES. */
#define LVX_CODEC_STAGES 21
#define LVX_ROUTE_MFMA64 0   /* gemm_mfma_kernel, 64 x 64 tile: v = {bf16 operands, batch, K % 32 == 0} */
#define LVX_ROUTE_BF16_128 1 /* gemm_bf16_kernel, 128 x 128 tile: v = {bytes of A, bytes of W (1: fp8), 0} */
#define LVX_ROUTE_GLDS 2     /* gemm_glds_kernel, 128 x 192 tile: v = {NS stages, SPLIT form, bytes of A} */
#define LVX_ROUTE_SKINNY 3   /* gemm_skinny_kernel: v = {MI, NJ, NWV} */
typedef struct lvx_codec_route {
  int32_t family;   /* LVX_ROUTE_* */
  int32_t ksplit;   /* K splits of the launch (1: none) */
  int32_t inlaunch; /* 1: the split-K partials are combined inside the GEMM launch, 0: by a reduce kernel */
  int32_t v[3];     /* per family, above */
  int32_t N, K;     /* the GEMM's N and K */
} lvx_codec_route;
int lvx_codec_stages(lvx_ctx* ctx, int first, int last, const void* in_dev, int B, int L, int bandwidth_id,
                     float* out_dev, lvx_codec_route* routes_out, int route_cap, int* n_routes_out, void* stream);
/* Host-side view of a slot's position (synchronises the stream). */
int lvx_stream_position(lvx_ctx* ctx, int slot, int* pos_out, void* stream);
/* Cross-check switches between two correct implementations of the same step, per context (round 4:
 * an option set on one context never changes another context's kernels; each call binds a snapshot
 * of its context's options, and the context drops its captured graphs on its next call after a
 * change). Defaults are the measured-faster variants:
 *   "defer_select" 1: the greedy select is committed by the next step's first kernel (bf16 with "l0q"
 *                     1: ar_embed_select at every B; otherwise B <= 2 and 4 <= B <= 8: c_attn layer 0
 *                     reduces lm_head's granules, larger B: ar_embed_select); 2: 4 <= B <= 8 through
 *                     ar_embed_select with "l0q" 0 too; 0: ar_argmax_kernel after every lm_head
 *                     (bit-identical results with "l0q" 0: tests/test_gpu_select.py);
 *   "fuse_mlp"     1: bf16, B <= 2: c_fc + gelu + mlp c_proj in one kernel (2^-32 fixed-point int64
 *                     atomics: exact sums, reproducible run to run); 0: the two GEMV kernels;
 *   "bt"           1: batched path v3 for 32 < B <= 64; 2: v3 for every batched B; 0: never;
 *   "codec_g2"     1: large-M bf16 codec GEMMs on the 128 x 128 MFMA tile kernel; 0: the general one;
 *   "codec_skinny" 1: bf16 codec weight GEMMs with M <= 384 frames on the K-split-over-waves kernel
 *                     (no split-K combine); 0: the tile kernels;
 *   "codec_g3f"    fp32 (parity mode) codec GEMMs with >= 192 tiles of 128 x 192: 2 (default): the
 *                     LDS-DMA kernel with fp32 operands split into bf16 hi + lo, hi.hi + lo.hi + hi.lo
 *                     on v_mfma_f32_16x16x32_bf16 (fp32 accumulation); 1: the same kernel with exact-fp32
 *                     v_mfma_f32_16x16x4_f32 (slower; the tests' exact-fp32 oracle for the split form);
 *   "codec_exp"    codec development bits, 0 = production kernels; bit 0: the general GroupNorm
 *                     kernel at every L (same bits); bits 1-2: dwconv+AdaLN frames per block at
 *                     >= 2,048 frames (0: 4, 1: 16, 2: 32, 3: 8; same bits); bit 3: library
 *                     exp / sin / cos in the bf16 iSTFT; bit 4: fp32 bf16x3 GEMMs split their
 *                     operands in registers, no split-image producers (same bits);
 *   "exp"          cross-check bits, 0 = production kernels (fp32 parity mode, each bit-identical or
 *                     within fp32 summation noise: tests/test_gpu_f32b.py); bit 8: fp32 batched GEMMs
 *                     in 32-row instead of 16-row batch tiles (bit-identical); bit 512: fp32 mlp c_proj
 *                     unsplit, bit 1024: fp32 c_attn in one launch (another summation order);
 *   "f32b"         1: fp32 weights, 3 <= B <= 64: batched steps on exact-fp32 MFMA (ar_f32b_kernel);
 *                     0: the fp32 GEMV family (same ids against the reference: tests/test_gpu_f32b.py);
 *   "ln_max"       (2..8, default 8) largest B whose batched GEMMs normalise in their own prologue;
 *                  larger B run the rows kernel + batched GEMM structure;
 *   "l0q"          1: bf16 weights, B <= 32 (not 3) with the deferred select: layer 0's c_attn from
 *                     table rows precomputed at lvx_finalize (text / codebook / position x ln_1 x W),
 *                     inside the embedding + select kernel (B > 8: one launch less per step; B <= 8:
 *                     the step's first launch reads three table rows instead of weight slices; the
 *                     operand is not rounded to bf16, so the sums differ from the GEMM's in the last
 *                     bits: tests/test_gpu_batched.py, test_gpu_select.py); 0: the c_attn GEMM / GEMV
 *                     (B > 8 after the embedding + select kernel; B <= 8 with the granule select);
 *   "l0a"          1: "l0q" steps whose attention is one split per (row, head) in 4-wave blocks (bf16 KV
 *                     9 <= B <= 32, fp8 KV 17 <= B <= 32): the select and layer 0's q / k / v from the
 *                     tables run inside attention layer 0, one launch less per step; 0: the select +
 *                     table launch, then the attention (bit-identical: tests/test_gpu_l0_fused.py);
 *   "laf"          1: on the same steps ("l0a" 1), layers 1-3 have no LayerNorm-rows and no c_attn launch:
 *                     every attention block (row, head) normalises its row and computes its head's 288
 *                     c_attn rows itself while its first KV tiles are in flight, and c_proj folds the
 *                     pending mlp copies into x (three launches and their gaps less per layer);
 *                     0: the three launches (bit-identical: tests/test_gpu_la_fused.py). The per-op entry
 *                     points (lvx_probe_kernel, lvx_attn_probe, lvx_ar_ops) plan without the tables, so
 *                     they go on running and timing the separate kernels whatever this option says;
 *   "fmt_group"    0: lvx_pcm_formant and lvx_pcm_mark choose, per launch, how many output hop blocks a workgroup
 *                     writes (few in a small launch, up to 32 in a large one); 1 .. 32: that many (bit-identical at
 *                     every value: tests/test_gpu_pcm_formant.py, tests/test_gpu_pcm_mark.py). */
int lvx_set_option(lvx_ctx* ctx, const char* name, int value);
/* The stream the decode graphs are captured on (then replayed on the caller's stream). NULL (default):
 * the caller's stream. Name another one when something may query, from another thread, an event
 * recorded on the caller's stream while lvx_ar_step* runs (a process group's watchdog after a
 * synchronous collective on that stream): HIP refuses such a query during a capture. The stream
 * named must not be the caller's and must outlive the context's use of it. */
int lvx_set_capture_stream(lvx_ctx* ctx, void* stream);
/* Enable/disable HIP-graph replay of lvx_ar_step for a given B (default on). */
int lvx_set_graphs(lvx_ctx* ctx, int enable);

/* ---- codec decoder ------------------------------------------------------- */
/* WavTokenizer.decode(features, bandwidth_id) (decoder/pretrained.py:192-207):
 * features float32 [B,512,L] (the reference layout) -> pcm float32 [B, 320*L]. Streams are
 * decoded independently (each one exactly as a separate reference call with its own L). */
int lvx_codec_decode_features(lvx_ctx* ctx, const float* feats_dev, int B, int L, int bandwidth_id,
                              float* pcm_dev, void* stream);
/* codes_to_features + decode fused: codes int32 [B,L] -> pcm float32 [B,320*L]. A code outside
 * [0, 4096) is clamped for the gather and flagged (the next lvx_check_errors: LVX_E_INDEX). */
int lvx_codec_decode_codes(lvx_ctx* ctx, const int32_t* codes_dev, int B, int L, int bandwidth_id,
                           float* pcm_dev, void* stream);

/* ---- PCM output stage ---------------------------------------------------------
 * The codec writes float32 PCM at 24 kHz (what the reference streams). This stage turns rows of it, on
 * the device, into what a client asked for: another sample rate and / or 16-bit integers. A stream that
 * asks for nothing never comes here: 24000 Hz f32le is the codec's own output, and lvx_pcm_convert
 * launches nothing for it.
 *
 * Output sample rates: 24000 (no resampling), 16000, 8000, 48000. Encodings: f32le, s16le, and the 8-bit
 * G.711 mu-law and A-law of "PCM G.711" below.
 *
 * Resampling is a rational polyphase FIR with fixed L / M (output rate = 24000 L / M):
 *   16000: L / M = 2 / 3, N = 72 (145 prototype taps, <= 73 per output);
 *    8000: L / M = 1 / 3, N = 72 (145 prototype taps, 145 per output);
 *   48000: L / M = 2 / 1, N = 48 (97 prototype taps, <= 49 per output).
 * The prototype is a Kaiser-windowed sinc built on the host in double precision, stored as fp32:
 *   lo = min(1, L / M);  fc = 0.5 lo 0.85 / L;  N = round(24 L / lo);
 *   h[n] = L 2 fc sinc(2 fc n) kaiser(2 N + 1, beta = 9.0)[n + N],  n = -N .. N,
 *   sinc(x) = sin(pi x) / (pi x), kaiser(K, beta)[k] = I0(beta sqrt(1 - (2 k / (K - 1) - 1)^2)) / I0(beta).
 * Its 0.1 dB passband edge is 0.765 of the lower of the two Nyquist frequencies, its stopband
 * <= -91 dB from that frequency on (float64 design); the DC gain of every phase is 1 within 1e-5.
 *
 * One segment is one sentence of one stream. Its input is x[0 .. T), zero outside; its output is
 *   y[m] = sum over the i with |m M - i L| <= N of x[i] h[m M - i L],   m = 0 .. ceil(T L / M) - 1,
 * evaluated in fp32 in ONE fixed order: acc = 0, then for i ascending (every i of the range, the ones
 * outside [0, T) as x[i] = 0) acc = fl(acc + fl(x[i] h[m M - i L])): a rounded product and a rounded sum,
 * no fused multiply-add. Each output is an independent dot product, so THE CONCATENATED OUTPUTS OF ANY
 * CHUNKING OF A SEGMENT ARE BIT-IDENTICAL TO ITS ONE-SHOT OUTPUT, and a host evaluation of the same
 * order in fp32 (llmvox_amd/audio.py: resample_ref) gives the same bits.
 *
 * Streaming. After a non-final call that brings the segment's input count to T, the outputs emitted so
 * far are the m < E(T) = min(floor(((T - 1) L - N) / M) + 1, ceil(T L / M)), E(T) = 0 if (T - 1) L < N;
 * a final call emits up to ceil(T L / M). The first output of a call reaches back at most 2 N / L =
 * 144 / 72 / 48 inputs (8 / 16 / 48 kHz) before the call's first input, so the library keeps, per KV
 * slot, the last 160 inputs of the previous call (two buffers per slot: a launch reads one and writes
 * the other) and, on the host, the slot's input count and rate (a mirror, as lvx_stream_sampling keeps
 * one): a slot's calls are issued in order on one stream. A segment is resampled at one rate: another
 * rate before its final call is LVX_E_ARG.
 *
 * s16le: q = rint(clamp(v 32768, -32768, 32767)), round half to even, v the fp32 sample (resampled or
 * not); NaN -> 0. Exact in fp32. 24000 Hz s16le is the same kernel without a filter: elementwise, stateless. */
#define LVX_PCM_F32LE 0
#define LVX_PCM_S16LE 1
#define LVX_PCM_ALAW 6 /* G.711 A-law and mu-law ("PCM G.711" below): the WAVE format tags; 2 .. 5 are no encodings */
#define LVX_PCM_ULAW 7
/* host only: L, M, N and the 2 N + 1 fp32 taps h[-N .. N] of a rate (24000: 1, 1, 0 and the tap 1).
 * taps_host may be NULL (only L, M, N). LVX_E_ARG for an unsupported rate or cap < 2 N + 1. */
int lvx_pcm_filter(int sample_rate, int* L, int* M, int* N, float* taps_host, int cap);
/* host only: samples a call emits for a slot that has consumed t0 inputs of its segment
 * (negative: LVX_E_ARG for an unsupported rate, t0 < 0 or n_in < 0) */
int lvx_pcm_emitted(int sample_rate, long long t0, int n_in, int final);
/* forget a slot's history and position (a new segment) in every PCM stage below; stream-ordered */
int lvx_pcm_reset(lvx_ctx* ctx, int slot, void* stream);
/* rows b of pcm_dev [B][n_in] f32 continue the segments of slots_host[b]; final_host[b] != 0 flushes and
 * resets the slot. n_in may be 0 with final (flush only). out row b starts at out_dev + b * out_stride_bytes
 * (float32, int16 or, G.711, uint8 samples); n_out_host[b] = samples written. Host arrays are consumed
 * before the call returns. 24000 Hz f32le: nothing is launched and nothing written, the rows of pcm_dev are
 * the output (n_out_host[b] = n_in; out_dev may be NULL). 24000 Hz in another encoding: the kernel without a
 * filter. LVX_E_ARG (and no slot's state changed): a bad rate or encoding, B < 1, n_in < 0, a slot out of
 * range or named twice, out_dev or out_stride_bytes not a multiple of 4 (G.711's byte rows too),
 * out_stride_bytes smaller than a row's output. */
int lvx_pcm_convert(lvx_ctx* ctx, const float* pcm_dev, int B, int n_in, const int32_t* slots_host,
                    const uint8_t* final_host, int sample_rate, int encoding, void* out_dev,
                    long long out_stride_bytes, int32_t* n_out_host, void* stream);

/* ---- PCM time stretch ---------------------------------------------------------
 * The speaking-rate control. LLMVoX has no model-side handle for speed (one speech token per decode
 * step, the length decided by end-of-audio), so a stream that asks for another speed has the codec's
 * f32 rows time-stretched on the device, pitch preserved, BEFORE the resampling and quantisation above:
 * waveform-similarity overlap-add (WSOLA) at 24 kHz. A stream at speed 100 never comes here. Everything
 * is integer or fp32 arithmetic in ONE fixed order, so the device output is bit-identical to a host
 * evaluation of the same order (llmvox_amd/audio.py: stretch_ref) and INDEPENDENT OF CHUNKING.
 *
 * Constants: H = 240 (the output hop, 10 ms), D = 240 (the search radius), C = 480 (the correlation
 * length); speed_pct an integer in [50, 200], 100 = no stretch. The nominal analysis position of hop j
 * is a_j = (j H speed_pct) / 100 in integer (floor) arithmetic.
 *
 * Windows, built on the host in double and stored as fp32 (lvx_pcm_stretch_window):
 *   wr[n] = 0.5 - 0.5 cos(pi (n + 0.5) / H), n = 0 .. H - 1;  wf[n] = 1 - wr[n] (subtracted in double;
 *   each table rounded once).
 *
 * One segment is one sentence of one stream: x[0 .. T), zero outside. p_{-1} = -H. Hop j writes
 * y[j H .. j H + H); e_j = p_{j-1} + H is where the previous frame would naturally continue.
 *   j = 0: d_0 = 0, p_0 = 0.
 *   j >= 1: for every d in [-D, D], c = a_j + d:
 *     corr_d = sum for k = 0 .. C - 1, ascending, of fl(x[c + k] x[e_j + k]),
 *     en_d   = the same sequential sum of fl(x[c + k] x[c + k])
 *     (acc = 0, then acc = fl(acc + fl(product)): every product and every sum rounded to fp32, no fused
 *     multiply-add),
 *     score_d = fl(fl(corr_d |corr_d|) / fl(en_d + 1e-9f)), IEEE division; a NaN score counts as -inf.
 *     d_j = the d with the largest score; among equal scores (+0 and -0 are equal) the smallest |d|, of
 *     +-d the negative one; all scores equal (silence) gives d_j = 0. p_j = a_j + d_j.
 *   y[j H + n] = fl(fl(x[e_j + n] wf[n]) + fl(x[p_j + n] wr[n])), n = 0 .. H - 1.
 * Every output hop is complete when written: there is no overlap-add tail to carry.
 *
 * Counts. The segment delivers ceil(T 100 / speed_pct) samples; the last hop is cut there. With
 *   need_0 = 2 H,  need_j = max(a_j + D + 2 H, a_{j-1} + D + 3 H)  (j >= 1),
 * hop j reads no input at or after need_j. After a non-final call that brings the consumed input to T
 * the emitted hops are exactly the j with need_j <= T, each as H whole samples; a final call emits the
 * rest, up to the total. A hop reaches back at most 1199 inputs before need_j - 1, so the library keeps,
 * per KV slot, the last 1280 inputs of the previous call (two buffers per slot: a launch reads one and
 * writes the other) and d_{j-1}, one int that stays on the device; on the host, a mirror of the slot's
 * consumed input, emitted hops and speed_pct: a slot's calls are issued in order on one stream. A
 * segment has one speed: another speed_pct before its final call is LVX_E_ARG. */
/* host only: the fp32 window tables wr[0 .. 240) and wf[0 .. 240). LVX_E_ARG: a null table, cap < 240. */
int lvx_pcm_stretch_window(float* wr_host, float* wf_host, int cap);
/* host only: samples a stretch call emits for a slot that has consumed t0 inputs of its segment
 * (speed_pct 100: n_in; negative: LVX_E_ARG for speed_pct outside [50, 200], t0 < 0 or n_in < 0) */
int lvx_pcm_stretch_emitted(int speed_pct, long long t0, int n_in, int final);
/* lvx_pcm_convert's conventions: rows b of pcm_dev [B][n_in] f32 continue the stretch segments of
 * slots_host[b]; final_host[b] != 0 emits the rest and resets the slot; n_in may be 0 with final (flush
 * only). out row b (f32) starts at out_dev + b * out_stride_bytes; n_out_host[b] = samples written.
 * d_out_dev (optional, may be NULL): row b's chosen d_j of the hops this call emits, int32 at
 * d_out_dev + b * d_stride. speed_pct 100: nothing is launched and nothing written, the rows of pcm_dev
 * are the output (n_out_host[b] = n_in; out_dev may be NULL). LVX_E_ARG (and no slot's state changed):
 * speed_pct outside [50, 200] or another than the slot's open segment has, B < 1, n_in < 0, a slot out
 * of range or named twice, out_dev or out_stride_bytes not a multiple of 4, out_stride_bytes smaller than
 * a row's output, d_stride smaller than a row's hops. lvx_pcm_reset also forgets a slot's stretch state. */
int lvx_pcm_stretch(lvx_ctx* ctx, const float* pcm_dev, int B, int n_in, const int32_t* slots_host,
                    const uint8_t* final_host, int speed_pct, float* out_dev, long long out_stride_bytes,
                    int32_t* n_out_host, int32_t* d_out_dev, int d_stride, void* stream);

/* ---- PCM pitch shift ----------------------------------------------------------
 * The pitch control. LLMVoX has one voice and no conditioning input, so pitch, like speed, is made on the
 * PCM: a pitch shift is a time stretch by one factor followed by a resampling by the inverse factor. The
 * stretch is lvx_pcm_stretch above, unchanged; what this section adds is the resampler for an arbitrary
 * ratio, lvx_pcm_ratio, and the integer plan that ties the two to a stream's speed and pitch. A stream
 * that names no pitch (or 100) never comes here. The order of the stages is stretch, ratio, then
 * lvx_pcm_convert for the rate and the encoding; each keeps its own bit-exact rule.
 *
 * Plan (lvx_pcm_pitch_plan; all integers). speed_pct and pitch_pct each in [50, 200], 100 neutral.
 *   stretch_pct = (200 speed_pct + pitch_pct) div (2 pitch_pct)     (speed 100 / pitch, rounded half up)
 * The combination is valid iff 50 <= stretch_pct <= 200 (else LVX_E_ARG).
 *   g = gcd(stretch_pct, speed_pct),  L = stretch_pct / g,  M = speed_pct / g.
 * The stream is stretched at stretch_pct (100: nothing is launched), the stretched signal resampled by
 * L / M (output count over input count), still nominally at 24 kHz (L == M, which every pitch_pct 100
 * gives: nothing is launched). The duration is that of speed_pct; the pitch is multiplied by the realised
 * ratio M / L = speed_pct / stretch_pct, which approximates pitch_pct / 100 to within the rounding of
 * stretch_pct. A sentence of T samples delivers n1 = ceil(T 100 / stretch_pct), then n2 = ceil(n1 L / M)
 * samples, then the rate conversion's count of n2.
 *
 * Ratio resampler: the rule of the "PCM output stage" with a general (L, M), L and M coprime.
 *   lo = min(1, L / M);  fc = 0.5 lo 0.85 / L;  N = round(24 L / lo) = 24 max(L, M) <= 4800;
 *   h[n] = L 2 fc sinc(2 fc n) kaiser(2 N + 1, beta = 9.0)[n + N],  n = -N .. N,
 * built on the host in double, stored as fp32, by the very function that designs the three fixed rates:
 * (L, M) = (2, 3), (1, 3), (2, 1) give N = 72, 72, 48 and the taps of 16000 / 8000 / 48000 Hz bit for bit.
 *   y[m] = sum over the i with |m M - i L| <= N of x[i] h[m M - i L],   m = 0 .. ceil(T L / M) - 1,
 * in fp32 in the same ONE fixed order: acc = 0, then for i ascending (x[i] = 0 outside [0, T))
 * acc = fl(acc + fl(x[i] h[m M - i L])), no fused multiply-add. Every output is an independent dot
 * product: THE CONCATENATED OUTPUTS OF ANY CHUNKING OF A SEGMENT ARE BIT-IDENTICAL TO ITS ONE-SHOT OUTPUT,
 * and llmvox_amd/audio.py: ratio_ref gives the same bits on the host. An output takes at most
 * floor(2 N / L) + 1 taps.
 * Over the 9,155 reduced (L, M) != (1, 1) the plan can produce (float64 response of the fp32 taps): the
 * passband is within 0.1 dB up to 0.765 lo, the stopband <= -91 dB from lo on (lo in units of the input's
 * Nyquist frequency), the DC gain of every phase is 1 within 5e-5, and an output reaches back <= 96 inputs.
 *
 * Streaming counts: the same formula. After a non-final call that brings the input count to T the emitted
 * outputs are the m < E(T) = min(floor(((T - 1) L - N) / M) + 1, ceil(T L / M)), 0 if (T - 1) L < N; a
 * final call emits the rest. lvx_pcm_ratio accepts any coprime 1 <= L, M <= 200 with M <= 4 L and
 * L <= 4 M (wider than the plan produces; (1, 1) is the identity: N = 0, the tap 1, nothing launched).
 * With M <= 4 L an output reaches back at most ceil(2 N / L) <= 192 inputs: the library keeps, per KV slot,
 * the last 256 inputs of the previous call (two buffers per slot) and, on the host, the slot's input count
 * and ratio. The taps are designed once per (L, M) and cached on the host; on the device every slot has a
 * table region of its own, written by a stream-ordered copy on the call's stream when the slot's call
 * finds another ratio in it: a slot's calls are issued in order on one stream, so no launch reads a table
 * that a later segment overwrites. A segment has one ratio: another before its final call is LVX_E_ARG. */
/* host only: the plan of a (speed_pct, pitch_pct). LVX_E_ARG: either outside [50, 200], or a combination
 * whose stretch_pct falls outside [50, 200]. Any of the three outputs may be NULL. */
int lvx_pcm_pitch_plan(int speed_pct, int pitch_pct, int* stretch_pct, int* L, int* M);
/* host only: N and the 2 N + 1 fp32 taps h[-N .. N] of a ratio ((1, 1): 0 and the tap 1). taps_host may be
 * NULL (only N). LVX_E_ARG: L, M not coprime, outside 1 .. 200, M > 4 L or L > 4 M, or cap < 2 N + 1. */
int lvx_pcm_ratio_filter(int L, int M, int* N, float* taps_host, int cap);
/* host only: samples a call emits for a slot that has consumed t0 inputs of its segment (negative:
 * LVX_E_ARG for a bad ratio, t0 < 0 or n_in < 0) */
int lvx_pcm_ratio_emitted(int L, int M, long long t0, int n_in, int final);
/* lvx_pcm_stretch's conventions: rows b of pcm_dev [B][n_in] f32 continue the ratio segments of
 * slots_host[b]; final_host[b] != 0 emits the rest and resets the slot; n_in may be 0 with final (flush
 * only). out row b (f32) starts at out_dev + b * out_stride_bytes; n_out_host[b] = samples written.
 * L == M == 1: nothing is launched and nothing written, the rows of pcm_dev are the output (n_out_host[b]
 * = n_in; out_dev may be NULL). LVX_E_ARG (and no slot's state changed): a bad ratio or another than the
 * slot's open segment has, B < 1, n_in < 0, a slot out of range or named twice, out_dev or
 * out_stride_bytes not a multiple of 4, out_stride_bytes smaller than a row's output. lvx_pcm_reset also
 * forgets a slot's ratio state. */
int lvx_pcm_ratio(lvx_ctx* ctx, const float* pcm_dev, int B, int n_in, const int32_t* slots_host,
                  const uint8_t* final_host, int L, int M, float* out_dev, long long out_stride_bytes,
                  int32_t* n_out_host, void* stream);

/* ---- PCM dump join ------------------------------------------------------------
 * The click-free join of a sentence's dumps. A sentence reaches the listener as a series of dumps, each
 * decoded by the codec on its own; the codec is not causal (k7 depthwise and k3 convolutions, attention
 * over the call), so the last frames of a dump are rendered against zero padding and the first frames of
 * the next one without left context: plain concatenation has a seam at every dump boundary. A stream that
 * asks for the join has every dump after a sentence's first decoded with up to LVX_JOIN_CONTEXT frames of
 * context in front (the tokens dumped just before it), and this stage, IN FRONT of the stretch, the ratio
 * and the rate conversion, holds back the last frame of every non-final rendering and crossfades it with
 * the next call's rendering of the same frame. A stream that does not ask never comes here.
 *
 * UNLIKE THE OTHER THREE STAGES THE RESULT DEPENDS ON WHERE THE DUMPS WERE CUT: that is its nature (the
 * renderings it joins differ with the cuts). Given the cuts and the context counts, the device output is
 * bit-identical to a host evaluation of the same order (llmvox_amd/audio.py: join_ref).
 *
 * Constants: LVX_JOIN_HOLD = 320 samples, one codec frame: the hold-back and the crossfade length.
 * LVX_JOIN_CONTEXT = 16 frames: the most context a call may carry.
 * Windows, built on the host in double, each rounded once to fp32 (lvx_pcm_join_window):
 *   wr[n] = 0.5 - 0.5 cos(pi (n + 0.5) / 320), n = 0 .. 319;  wf[n] = 1 - wr[n] (subtracted in double).
 *
 * One segment is one sentence of one stream. A slot's segment is OPEN after a non-final call and closed
 * after a final call or lvx_pcm_reset. An open slot holds tail[0 .. 320): the last 320 samples of its
 * previous call's rendering, which were not emitted.
 *
 * A call's row is r[0 .. n_in), n_in = 320 (c + Lb): c = ctx_frames in [0, 16] frames that re-render what
 * the segment has already delivered, then Lb >= 1 new frames; s = 320 c. In this order:
 *   1. Head. Open slot, c >= 1: emit x[n] = fl(fl(tail[n] wf[n]) + fl(r[s - 320 + n] wr[n])), n = 0 .. 319
 *      (two rounded products and a rounded sum, no fused multiply-add). Open slot, c = 0: emit tail
 *      unchanged (plain concatenation at this seam). Closed slot: emit nothing, and c must be 0.
 *   2. Body. Not final: emit r[s .. n_in - 320). Final: emit r[s .. n_in).
 *   3. State. Not final: tail = r[n_in - 320 .. n_in), the slot is open. Final: the slot is closed.
 *   4. Flush (n_in = 0, final, c = 0): an open slot emits tail, a closed one nothing.
 * Samples emitted: closed, non-final 320 Lb - 320 (0 for a one-frame dump); open, non-final 320 Lb; open,
 * final 320 Lb + 320; closed, final 320 Lb. A SENTENCE OF T FRAMES DELIVERS EXACTLY 320 T SAMPLES, as
 * without the join, and a sentence that is one dump delivers the codec's row bit for bit.
 *
 * The library keeps, per KV slot, the tail in two device buffers (a launch reads one and writes the other)
 * and, on the host, a mirror of "open" and of which buffer is current: a slot's calls are issued in order
 * on one stream. The window table is uploaded once. */
#define LVX_JOIN_HOLD 320
#define LVX_JOIN_CONTEXT 16
/* host only: the fp32 window tables wr[0 .. 320) and wf[0 .. 320). LVX_E_ARG: a null table, cap < 320. */
int lvx_pcm_join_window(float* wr_host, float* wf_host, int cap);
/* host only: samples a join call emits for a slot whose segment is open (open != 0) or closed (negative:
 * LVX_E_ARG for n_in negative or no multiple of 320, ctx_frames outside [0, 16], n_in > 0 with
 * 320 ctx_frames >= n_in, ctx_frames > 0 on a closed slot, n_in = 0 without final or with ctx_frames != 0) */
int lvx_pcm_join_emitted(int open, int ctx_frames, int n_in, int final);
/* lvx_pcm_stretch's conventions: rows b of pcm_dev [B][n_in] f32 (n_in common to the call) continue the
 * join segments of slots_host[b] with ctx_frames_host[b] frames of context in front; final_host[b] != 0
 * emits the row to its end and closes the slot; n_in may be 0 with final (flush only). out row b (f32)
 * starts at out_dev + b * out_stride_bytes; n_out_host[b] = samples written. LVX_E_ARG (and no slot's state
 * changed): the cases of lvx_pcm_join_emitted for any row, B < 1, a slot out of range or named twice,
 * out_dev null or out_dev / out_stride_bytes not a multiple of 4, out_stride_bytes smaller than a row's
 * output. lvx_pcm_reset also closes a slot's join segment. */
int lvx_pcm_join(lvx_ctx* ctx, const float* pcm_dev, int B, int n_in, const int32_t* slots_host,
                 const int32_t* ctx_frames_host, const uint8_t* final_host, float* out_dev,
                 long long out_stride_bytes, int32_t* n_out_host, void* stream);

/* ---- PCM G.711 ----------------------------------------------------------------
 * Telephony's encodings: 8-bit mu-law (PCMU, LVX_PCM_ULAW) and A-law (PCMA, LVX_PCM_ALAW), two further
 * encodings of lvx_pcm_convert at every rate. Integer arithmetic only, so THE DEVICE'S BYTES ARE THOSE OF A HOST
 * EVALUATION (llmvox_amd/audio.py: g711_encode) and, like every stage but the join, do not depend on how a
 * sentence was cut into dumps. A per-sample epilogue of the kernel: slot state, history, counts and
 * lvx_pcm_emitted are those of the other encodings.
 *
 * Quantisation first: q is the s16le rule above applied to the fp32 sample (resampled or not), NaN -> 0, the
 * same clamp. So a G.711 stream's bytes are the G.711 codes of the s16le stream's samples.
 *
 * Companding: the ITU-T G.191 STL form. A negative q is taken in one's complement (~q); every shift is
 * arithmetic on a 32-bit int.
 *   mu-law:  a = min(((q < 0 ? ~q : q) >> 2) + 33, 0x1FFF);  seg = 1 + the bit length of (a >> 6), so 1 .. 8;
 *            code = ((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF)), with 0x80 or-ed in when q >= 0.
 *   A-law:   x = (q < 0 ? ~q : q) >> 4;  if x > 15: e = 1; while x > 31: x >>= 1, e += 1; then
 *            x = x - 16 + (e << 4);  0x80 or-ed in when q >= 0;  code = x ^ 0x55.
 * (The loop's e is the bit length of the first x >> 4: the library and the kernel count leading zeros.)
 * Decoders (host only, for clients and tests):
 *   mu-law:  m = ~c & 0xFF;  e = (m >> 4) & 7;  step = 4 << (e + 1);
 *            lin = sgn ((0x80 << e) + step (m & 0xF) + step / 2 - 132),  sgn = -1 for c < 0x80.
 *   A-law:   i = c ^ 0x55;  e = (i & 0x7F) >> 4;  m = i & 0xF;  if e > 0: m += 16;  m = (m << 4) + 8;
 *            if e > 1: m <<= e - 1;  negative when (i & 0x80) == 0.
 * Silence (q = 0) is 0xFF in mu-law and 0xD5 in A-law, not 0. All 256 codes occur; enc(~q) = enc(q) ^ 0x80;
 * dec(enc(q)) does not decrease with q; enc(dec(c)) = c but for mu-law's 0x7F (negative zero, which decodes
 * to 0); |dec(enc(q)) - q| <= 512 for A-law and, for mu-law, on |q| <= 32124 (644 at its clip). */
/* host only: the codes of n s16 samples, and back. encoding: LVX_PCM_ULAW or LVX_PCM_ALAW. LVX_E_ARG: another
 * encoding, n < 0, a null pointer with n > 0. */
int lvx_pcm_g711_encode(int encoding, const int16_t* in, long long n, uint8_t* out);
int lvx_pcm_g711_decode(int encoding, const uint8_t* in, long long n, int16_t* out);

/* ---- PCM level ----------------------------------------------------------------
 * The volume control: a gain followed by a peak limiter, because louder speech clips. It runs AFTER the join,
 * the stretch and the ratio resampler and BEFORE lvx_pcm_convert (rate and encoding), always at the nominal
 * 24 kHz, so its constants are fixed sample counts. A stream at volume_pct 100 never comes here.
 *
 * The limiter has no recursion (no attack / release state carried from sample to sample): every output is a
 * fixed function of a bounded window of inputs, a sliding minimum (exact in any evaluation order) and ONE
 * fixed-order fp32 sum. So the device output is bit-identical to a host evaluation of the same order
 * (llmvox_amd/audio.py: level_ref) and INDEPENDENT OF CHUNKING, like the resamplers and the stretch.
 *
 * Constants: A = LVX_LEVEL_A = 120 samples (5 ms), the attack half-window; R = LVX_LEVEL_R = 1200 samples
 * (50 ms), the hold; c = LVX_LEVEL_CEIL = the fp32 value 0.8912509f (-1 dBFS), the ceiling, which is fixed.
 * volume_pct is an integer in [0, 400], 100 neutral; G = (float)((double)volume_pct / 100.0), once, on the host.
 * Window, built on the host in double, each tap rounded once to fp32 (lvx_pcm_level_window):
 *   w[k] = (0.5 + 0.5 cos(pi k / (A + 1))) / (A + 1),  k = -A .. A  (241 taps; their sum is 1).
 *
 * One segment is one sentence of one stream: x[0 .. T), x = 0 outside. All arithmetic is fp32; every product,
 * sum and quotient is rounded, no fused multiply-add, IEEE division.
 *   1. v[i] = fl(G x[i]).
 *   2. r[i] = fl(c / |v[i]|) if |v[i]| > c, else 1. (A NaN compares false: r = 1 and the NaN passes through;
 *      an infinity gives r = 0.)
 *   3. m[i] = min of r[k] over k in [i - R, i + A]: exact, however it is evaluated.
 *   4. d[i] = fl(1 - m[i]);  S[n]: acc = 0, then for k = -A .. A ascending acc = fl(acc + fl(d[n + k] w[k]));
 *      s[n] = fl(1 - S[n]).
 *   5. g[n] = max(0, min(s[n], r[n])). (Every m[n + k] with |k| <= A covers n, because R >= A, so s is at most
 *      r[n] up to rounding; the clamp makes that exact.)
 *   6. y[n] = fl(v[n] g[n]),  n = 0 .. T - 1: one output per input.
 * Ceiling: |y[n]| <= c (1 + 2^-22) for finite input. Transparency: if no |v| exceeds c in
 * [n - 2 A - R, n + 2 A], every d of the sum is exactly 0, so g[n] = 1 exactly and y[n] = v[n] bit for bit.
 * Dependence: output n depends on x[n - 2 A - R .. n + 2 A] only. THE CONCATENATED OUTPUTS OF ANY CHUNKING OF A
 * SEGMENT ARE BIT-IDENTICAL TO ITS ONE-SHOT OUTPUT, and bit-identical to audio.level_ref.
 * The rate conversion that follows can overshoot the ceiling slightly; the s16le quantiser still clamps.
 *
 * Streaming. After a non-final call that brings the consumed input to T the emitted outputs are the
 * n < max(0, T - 2 A); a final call emits up to T: a stream holds back 240 samples (10 ms) until its
 * sentence's final call. The first output of a call reaches back 3 A + R = 1560 inputs before the call's first
 * input, so the library keeps, per KV slot, the last 1600 raw inputs x of the previous call (two buffers per
 * slot: a launch reads one and writes the other) and, on the host, a mirror of the slot's consumed count and
 * volume_pct: a slot's calls are issued in order on one stream. A segment has one volume: another before its
 * final call is LVX_E_ARG. */
#define LVX_LEVEL_A 120
#define LVX_LEVEL_R 1200
#define LVX_LEVEL_CEIL 0.8912509f
/* host only: the 241 fp32 taps w[-120 .. 120]. LVX_E_ARG: a null table, cap < 241. */
int lvx_pcm_level_window(float* w_host, int cap);
/* host only: samples a level call emits for a slot that has consumed t0 inputs of its segment (volume_pct
 * 100: n_in; negative: LVX_E_ARG for volume_pct outside [0, 400], t0 < 0 or n_in < 0) */
int lvx_pcm_level_emitted(int volume_pct, long long t0, int n_in, int final);
/* lvx_pcm_ratio's conventions: rows b of pcm_dev [B][n_in] f32 continue the level segments of slots_host[b];
 * final_host[b] != 0 emits the rest and resets the slot; n_in may be 0 with final (flush only). out row b (f32)
 * starts at out_dev + b * out_stride_bytes; n_out_host[b] = samples written. g_out_dev (optional test hook, may
 * be NULL): row b's g[n] of the samples this call emits, f32 at g_out_dev + b * g_stride_bytes. volume_pct 100:
 * nothing is launched and nothing written, the rows of pcm_dev are the output (n_out_host[b] = n_in; out_dev
 * may be NULL). LVX_E_ARG (and no slot's state changed): volume_pct outside [0, 400] or another than the slot's
 * open segment has, B < 1, n_in < 0, a slot out of range or named twice, out_dev / out_stride_bytes (and
 * g_out_dev / g_stride_bytes when given) not a multiple of 4 or a stride smaller than a row's output.
 * lvx_pcm_reset also forgets a slot's level state. */
int lvx_pcm_level(lvx_ctx* ctx, const float* pcm_dev, int B, int n_in, const int32_t* slots_host,
                  const uint8_t* final_host, int volume_pct, float* out_dev, long long out_stride_bytes,
                  int32_t* n_out_host, float* g_out_dev, long long g_stride_bytes, void* stream);

/* ---- PCM formant --------------------------------------------------------------
 * The formant control: a correction of the spectral envelope, because the pitch control is a resampling and moves
 * the vocal-tract resonances with f0. It runs AFTER the ratio resampler and BEFORE the level stage, always at the
 * nominal 24 kHz: a seventh stage. A stream that names no formant never comes here.
 *
 * The plan (integers, lvx_pcm_formant_plan). After the ratio stage the envelope sits at r = M / L times the model's,
 * (L, M) lvx_pcm_pitch_plan's. To leave it at formant_pct / 100 the stage corrects by
 *   rho = (100 M) / (formant_pct L), in lowest terms Fn / Fd, valid iff Fd <= 2 Fn and Fn <= 2 Fd.
 * Fn == Fd is the identity: nothing is launched. The envelope of the output at bin k is that of the input at k rho.
 *
 * The rule is a short-time Fourier transform with a fixed fp32 order, so the device output is bit-identical to a host
 * evaluation of the same order (llmvox_amd/audio.py: formant_ref) and INDEPENDENT OF CHUNKING.
 * Constants: N = 1024 the frame, H = 256 the hop, K = 12 the smoothing half-width in bins, e = the fp32 nearest to
 * 1e-10, the clamp [1/256, 256] on the squared gain (+-24 dB), s = the fp32 nearest to 2/3.
 * Tables, built on the host in double, each entry rounded once to fp32 (lvx_pcm_formant_tables):
 *   w[n] = 0.5 - 0.5 cos(2 pi (n + 0.5) / N),  n = 0 .. N - 1;
 *   c[d] = (0.5 + 0.5 cos(pi d / (K + 1))) / (K + 1),  d = -K .. K  (25 taps; their sum is 1);
 *   the twiddles exp(-2 pi i k / N): tr[k] = cos(2 pi k / N), ti[k] = -sin(2 pi k / N),  k = 0 .. N / 2 - 1.
 *
 * One segment is one sentence of one stream: x[0 .. T), x = 0 outside. Frame j (j >= 0) covers the inputs
 * [(j - 3) H, (j + 1) H). Only + - * / and the square root occur, each correctly rounded to fp32, no fused multiply-add.
 * A complex product (a + b i)(wr + wi i) is (fl(fl(a wr) - fl(b wi)), fl(fl(a wi) + fl(b wr))).
 *   DFT_N: radix 2, decimation in time. The input goes to bit-reversed places: a[rev10(n)] = in[n]. Then ten stages,
 *     h = 1, 2, .. 512: for every i whose bit h is clear, with p = i mod h: t = a[i + h] (tr + ti i)[p N / (2 h)] (the
 *     product above), then a[i] = u + t and a[i + h] = u - t componentwise, u the old a[i]. EVERY stage runs the full
 *     product, the first (whose twiddle is 1 - 0 i) included. The inverse transform is the same with ti negated,
 *     followed by the product with 2^-10.
 *   1. X = DFT_N(fl(w[n] frame[n]) + 0 i).
 *   2. P[k] = fl(fl(re re) + fl(im im)),  k = 0 .. N / 2.
 *   3. P[-k] = P[k] and P[N / 2 + k] = P[N / 2 - k].
 *   4. E[k]: acc = 0, then for d = -K .. K ascending acc = fl(acc + fl(c[d] P[k + d])).
 *   5. i = (k Fn) div Fd;  f = fl(float((k Fn) mod Fd) / float(Fd));  Es = E[N / 2] where i >= N / 2, otherwise
 *      Es = fl(E[i] + fl(f fl(E[i + 1] - E[i]))).
 *   6. G2 = min(max(fl(fl(Es + e) / fl(E[k] + e)), 1/256), 256);  G = sqrt(G2). (Silence: e / e = 1, no 0 / 0.)
 *   7. Y[k] = (fl(G re), fl(G im)),  k = 0 .. N / 2;  Y[N - k] = conj(Y[k]),  k = 1 .. N / 2 - 1.
 *   8. y_j[n] = fl(w[n] fl(2^-10 re(a[n]))), a the inverse transform of Y (its imaginary part is not used).
 * Output sample n, in hop block b = n div H: fl(s (((y_b + y_{b+1}) + y_{b+2}) + y_{b+3})[n]), each frame read at
 * its own index of n, the frames added in ascending j, every sum rounded. (The four shifted w^2 sum to 1.5.)
 * Dependence: output n depends on x[(b - 3) H .. (b + 4) H) only. THE CONCATENATED OUTPUTS OF ANY CHUNKING OF A
 * SEGMENT ARE BIT-IDENTICAL TO ITS ONE-SHOT OUTPUT, and, for finite input, bit-identical to audio.formant_ref. (A NaN
 * or an infinity reaches every bin of the frames that cover it, and a power that overflows gives inf / inf: in those
 * frames the device and numpy may differ, because which NaN an operation returns, and what min and max make of one
 * (the device's drop it, numpy's keep it), is each processor's own. Codec PCM is finite.)
 *
 * Streaming. After a non-final call that brings the consumed input to T the emitted outputs are the
 * n < max(0, (T div H - 3) H); a final call emits up to T: a stream holds back 768 .. 1023 samples (32 .. 43 ms)
 * until more arrives or its sentence's final call. The first output of a call reaches back at most 7 H - 1 = 1791
 * inputs before the call's first input, so the library keeps, per KV slot, the last 1792 inputs of the previous call
 * (two buffers per slot: a launch reads one and writes the other) and, on the host, a mirror of the slot's consumed
 * count and ratio: a slot's calls are issued in order on one stream. A segment has one ratio: another before its
 * final call is LVX_E_ARG. */
#define LVX_FORMANT_N 1024
#define LVX_FORMANT_H 256
#define LVX_FORMANT_K 12
/* host only: Fn / Fd of a speed, a pitch and a formant, each in percent (the outputs may be NULL). LVX_E_ARG: one of
 * them outside [50, 200], a pair of speed and pitch lvx_pcm_pitch_plan rejects, or a ratio outside 1/2 .. 2. */
int lvx_pcm_formant_plan(int speed_pct, int pitch_pct, int formant_pct, int* Fn, int* Fd);
/* host only: the fp32 tables: w [1024], c [25] (c[-12 .. 12]), tw [1024] (tr[0 .. 512) then ti[0 .. 512)). A NULL
 * table is left out; cap_w, cap_c, cap_tw are the floats each holds. LVX_E_ARG: a table given with a smaller cap. */
int lvx_pcm_formant_tables(float* w_host, int cap_w, float* c_host, int cap_c, float* tw_host, int cap_tw);
/* host only: samples a formant call emits for a slot that has consumed t0 inputs of its segment (negative:
 * LVX_E_ARG for t0 < 0 or n_in < 0) */
int lvx_pcm_formant_emitted(long long t0, int n_in, int final);
/* lvx_pcm_level's conventions: rows b of pcm_dev [B][n_in] f32 continue the formant segments of slots_host[b];
 * final_host[b] != 0 emits the rest and resets the slot; n_in may be 0 with final (flush only). out row b (f32)
 * starts at out_dev + b * out_stride_bytes; n_out_host[b] = samples written. Fn == Fd (1 / 1): nothing is launched
 * and nothing written, the rows of pcm_dev are the output (n_out_host[b] = n_in; out_dev may be NULL). LVX_E_ARG (and
 * no slot's state changed): Fn / Fd not coprime, outside 1 .. 40000 or 1/2 .. 2, or another than the slot's open
 * segment has, B < 1, n_in < 0, a slot out of range or named twice, out_dev / out_stride_bytes not a multiple of 4
 * or a stride smaller than a row's output. lvx_pcm_reset also forgets a slot's formant state. */
int lvx_pcm_formant(lvx_ctx* ctx, const float* pcm_dev, int B, int n_in, const int32_t* slots_host,
                    const uint8_t* final_host, int Fn, int Fd, float* out_dev, long long out_stride_bytes,
                    int32_t* n_out_host, void* stream);

/* ---- PCM mark -----------------------------------------------------------------
 * The synthetic-speech watermark: a keyed, blind, multiplicative mark in 562 .. 3,375 Hz, so that a detector that
 * holds the key (llmvox_amd/audio.py: mark_detect) can say of delivered audio, the 8 kHz G.711 path included, that
 * this service made it, and read one payload byte. It runs AFTER the formant stage and BEFORE the level stage,
 * always at the nominal 24 kHz, so the limiter's ceiling still holds behind it. A stream without a mark never comes
 * here and makes exactly the calls it made before.
 *
 * The frames, the window w, the twiddles, DFT_N, the inverse transform, the overlap-add and the scale s are those of
 * "PCM formant": N = 1024, H = 256, lvx_pcm_formant_tables' tables, the same fp32 order, no fused multiply-add.
 * Frame j (j >= 0) covers the inputs [(j - 3) H, (j + 1) H). The formant rule's steps 2 to 6 are replaced by a table
 * lookup, so the device output is bit-identical to audio.mark_ref and INDEPENDENT OF CHUNKING.
 * Constants: K0 = 24 the first marked bin, BW = 5 the bins of a sub-band, U = 24 the sub-bands (sub-band u is the
 * bins K0 + 5 u .. K0 + 5 u + 4); pair m = 0 .. 11 is the sub-bands (2 m, 2 m + 1); Q = 4 frames make a block,
 * P = 64 blocks a period (2.73 s); strength is 1, 2 or 3 and a = 2^-(7 - strength) (1/64, 1/32, 1/16);
 * g+ = 1 + a and g- = 1 - a, both exact in fp32.
 * The sign table (host, integers only; lvx_pcm_mark_table): 64 words of 16 bits. Bit m of word p is
 *   c(p, m) XOR bit ((12 p + m) mod 8) of the payload id (0 .. 255, bit 0 the lowest),
 * c from SplitMix64 over the 64-bit key: state = key; for i = 12 p + m ascending: state += 0x9E3779B97F4A7C15,
 * z = state, z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9, z = (z ^ (z >> 27)) * 0x94D049BB133111EB, z = z ^ (z >> 31),
 * all modulo 2^64; c is the top bit of z. Bits 12 .. 15 of a word are clear. A set bit: the pair's even sub-band
 * gets g- and its odd one g+; a clear bit: the opposite. (The antipodal pair lets the detector cancel the speech's
 * own envelope.)
 *   Gain of frame j at bin k: 1 outside [K0, K0 + U BW); inside, the pair's gain from word (j div Q) mod P.
 *   Y[k] = (fl(G re), fl(G im)), k = 0 .. N / 2, X the formant rule's step 1; then that rule's steps 7 (the Hermitian
 *   extension) and 8 and its output sum. (G = 1 leaves a bin's bits; silence stays exactly silent.)
 * THE CONCATENATED OUTPUTS OF ANY CHUNKING OF A SEGMENT ARE BIT-IDENTICAL TO ITS ONE-SHOT OUTPUT, and, for finite
 * input, bit-identical to audio.mark_ref. Zero input gives zero output.
 *
 * Streaming: exactly the formant stage's counts (lvx_pcm_mark_emitted is lvx_pcm_formant_emitted's rule): a stream
 * holds back 768 .. 1023 samples until more arrives or its sentence's final call, on top of the formant stage's own
 * where both run; the library keeps 1792 inputs of history per slot in two buffers of the stage's own. Every segment
 * (sentence) starts the pattern again at frame 0. A segment has one (table, strength): another before its final call
 * is LVX_E_ARG. The 128-byte table travels with every launch as a kernel argument: nothing is uploaded or kept on
 * the device. No error text names the key. */
#define LVX_MARK_K0 24
#define LVX_MARK_BW 5
#define LVX_MARK_U 24
#define LVX_MARK_Q 4
#define LVX_MARK_P 64
/* host only: the 64 words of the sign table of (key, id). LVX_E_ARG: id outside 0 .. 255, cap < 64, words_host NULL */
int lvx_pcm_mark_table(unsigned long long key, int id, uint16_t* words_host, int cap);
/* host only: samples a mark call emits for a slot that has consumed t0 inputs of its segment (negative:
 * LVX_E_ARG for t0 < 0 or n_in < 0) */
int lvx_pcm_mark_emitted(long long t0, int n_in, int final);
/* lvx_pcm_formant's conventions: rows b of pcm_dev [B][n_in] f32 continue the mark segments of slots_host[b];
 * final_host[b] != 0 emits the rest and resets the slot; n_in may be 0 with final (flush only). out row b (f32)
 * starts at out_dev + b * out_stride_bytes; n_out_host[b] = samples written. LVX_E_ARG (and no slot's state
 * changed): id outside 0 .. 255, strength outside 1 .. 3, another mark than the slot's open segment has, B < 1,
 * n_in < 0, a slot out of range or named twice, out_dev / out_stride_bytes not a multiple of 4 or a stride smaller
 * than a row's output. lvx_pcm_reset also forgets a slot's mark state. */
int lvx_pcm_mark(lvx_ctx* ctx, const float* pcm_dev, int B, int n_in, const int32_t* slots_host,
                 const uint8_t* final_host, unsigned long long key, int id, int strength, float* out_dev,
                 long long out_stride_bytes, int32_t* n_out_host, void* stream);

/* ---- PCM FLAC ------------------------------------------------------------------
 * A lossless compressed output: a sixth stage BEHIND lvx_pcm_convert. Its input is the s16le samples of the
 * format's rate, exactly what lvx_pcm_convert writes with LVX_PCM_S16LE (int16 rows on the device); a decoder
 * gives those samples back. Integer arithmetic only, so THE DEVICE'S BYTES ARE THOSE OF A HOST EVALUATION
 * (llmvox_amd/audio.py: flac_subframe; here: lvx_flac_subframe) and THE CONCATENATED OUTPUT OF ANY CHUNKING OF A
 * SEGMENT IS BIT-IDENTICAL TO ITS ONE-SHOT OUTPUT. One segment is one sentence of one stream. The rule is
 * self-consistent (a separately written decoder round-trips it); it has not been held to libFLAC.
 *
 * Frames. BS = sample_rate / 25 (40 ms): 320, 640, 960, 1920 samples. A sentence of T > 0 samples is
 * k = max(0, floor((T - 16) / BS)) frames of BS samples, then one frame of the remaining T - k BS: every frame has
 * 16 .. BS + 15 samples, but for a sentence shorter than 16 samples, which is one frame. The stream is of FLAC's
 * variable-blocksize kind. STREAMINFO: min blocksize 16, max blocksize BS + 15, mono, 16 bits; the frame sizes, the
 * total sample count and the MD5 are 0 (unknown).
 *
 * Streaming. After a non-final call that brings the segment's input to T the frames emitted so far are
 * max(0, floor((T - 16) / BS)); a final call emits the rest. The library keeps, per KV slot, the <= BS + 15 samples
 * no frame has taken yet (two buffers per slot: a launch reads one and writes the other) and, on the host, a
 * mirror of the slot's count and rate. A segment has one rate: another before its final call is LVX_E_ARG.
 *
 * The subframe of a frame x[0 .. n), made on the device:
 *   CONSTANT, if all samples are equal: the byte 0x00, then x[0] in 16 bits.
 *   Predictor order: r_p = the p-th difference of x; E_p = sum of |r_p[i]| over i = 4 .. n - 1; p = the smallest
 *     of 0 .. 4 with the least E_p (so p = 0 for n <= 4).
 *   Folding: u = 2 r for r >= 0, else -2 r - 1 (u < 2^21 for int16 input).
 *   Partition order: P = min(3, trailing zero bits of n), lowered while P > 0 and (n >> P) < 16; partition j has
 *     n >> P samples, less p in partition 0.
 *   Rice parameter of a partition: the k of 0 .. 14 with the least sum((u >> k) + 1 + k), the smallest at a tie;
 *     the escape code is never used.
 *   FIXED: the byte (8 | p) << 1; p warm-up samples of 16 bits; 00 (the coding method); P in 4 bits; per
 *     partition k in 4 bits, then per sample u >> k zeros, a one, and the low k bits of u.
 *   VERBATIM, if that bit count is not smaller than 8 + 16 n: the byte 0x02, then the samples in 16 bits.
 *   Bits are packed MSB first and zero-padded to a byte: at most 1 + 2 n bytes.
 * The rest of a frame depends on where the sentence sits in the request (a request's sentences alternate between
 * two streams, so no device call knows a frame's sample number) and is made on the host, lvx_flac_finish:
 *   sync 0xFFF9; block size code 0111; sample-rate code 0100 / 0101 / 0111 / 1010 (8 / 16 / 24 / 48 kHz); the byte
 *   0x08 (mono, 16 bits); the first sample's number in FLAC's UTF-8-like coding (1 .. 7 bytes); n - 1 in 16 bits;
 *   the CRC-8 of these bytes (polynomial 0x07, initial value 0); the subframe; the CRC-16 of everything before it
 *   (polynomial 0x8005, initial value 0, not reflected), high byte first. At most 2 n + 17 bytes.
 *   (Over "123456789" the two CRCs are 0xF4 and 0xFEE8.)
 *
 * Device output. Row b holds the frames a call emits in fixed slots of LVX_FLAC_SLOT(rate) bytes: an 8-byte record
 * {uint16 n, uint16 body_bytes, uint32 0} (little endian), the subframe, zeros to the slot's end. How many frames
 * a call emits is a closed form of the counts (lvx_pcm_flac_emitted): n_frames_host is filled on the host. */
#define LVX_FLAC_SLOT(rate) ((8 + 1 + 2 * ((rate) / 25 + 15) + 15) / 16 * 16)
/* host only: BS of a rate (negative: LVX_E_ARG for an unsupported rate) */
int lvx_pcm_flac_block(int sample_rate);
/* host only: frames a call emits for a slot that has consumed t0 inputs of its segment (negative: LVX_E_ARG for
 * an unsupported rate, t0 < 0 or n_in < 0) */
int lvx_pcm_flac_emitted(int sample_rate, long long t0, int n_in, int final);
/* host only: "fLaC" and the STREAMINFO block, 42 bytes. LVX_E_ARG: an unsupported rate, a null pointer, cap < 42. */
int lvx_flac_stream_header(int sample_rate, uint8_t* out, int cap);
/* host only: the subframe of x[0 .. n) by the rule above. Returns its bytes (<= 1 + 2 n). LVX_E_ARG: n outside
 * 1 .. 65535, a null pointer; LVX_E_CAPACITY: cap is smaller than the subframe (nothing is written). */
int lvx_flac_subframe(const int16_t* x, int n, uint8_t* out, int cap);
/* host only: the n_frames slots of one row of lvx_pcm_flac made frames (header, subframe, CRC-16), the first at
 * sample number *sample_no, which advances by the frames' samples. Returns the bytes written. LVX_E_ARG: an
 * unsupported rate, a null pointer, n_frames < 0, a record that is none of this stage's, a sample number past 2^36,
 * frames of 2^31 bytes or more in one call;
 * LVX_E_CAPACITY: cap is smaller than the frames (2 n + 17 bytes each always suffice). In both cases nothing is
 * written and *sample_no stays. */
int lvx_flac_finish(int sample_rate, const uint8_t* slots, int n_frames, unsigned long long* sample_no, uint8_t* out,
                    int cap);
/* lvx_pcm_convert's conventions: rows b of s16_dev (int16, row b at s16_dev + b * in_stride_bytes, n_in samples)
 * continue the FLAC segments of slots_host[b]; final_host[b] != 0 emits the last frame and resets the slot; n_in
 * may be 0 with final. out row b starts at out_dev + b * out_stride_bytes; n_frames_host[b] = slots written.
 * LVX_E_ARG (and no slot's state changed): an unsupported rate or another than the slot's open segment has, B < 1,
 * n_in < 0, a slot out of range or named twice, s16_dev or in_stride_bytes odd, in_stride_bytes smaller than a row,
 * out_dev or out_stride_bytes not a multiple of 4, out_stride_bytes smaller than a row's slots. lvx_pcm_reset also
 * forgets a slot's FLAC state. lvx_pcm_convert itself takes no such encoding. */
int lvx_pcm_flac(lvx_ctx* ctx, const int16_t* s16_dev, long long in_stride_bytes, int B, int n_in,
                 const int32_t* slots_host, const uint8_t* final_host, int sample_rate, void* out_dev,
                 long long out_stride_bytes, int32_t* n_frames_host, void* stream);

/* ---- PCM pause -------------------------------------------------------------------
 * The pacing between sentences: the LAST stage, behind lvx_pcm_convert (or behind whichever stage produced the rows
 * of a 24 kHz f32le format, whose conversion does not run). It drops nothing on the device: it cuts the rows, in the
 * format's own encoding (LVX_PCM_F32LE, _S16LE, _ULAW, _ALAW) at any of the four rates, into blocks of 10 ms, marks
 * each silent or not and says where the sentence ends; the host then trims, caps and spaces by whole blocks
 * (llmvox_amd/audio.py: PauseMux, the rule stated there as pause_ref). Bytes are copied and integers compared, so THE
 * DEVICE'S SLOTS ARE THOSE OF A HOST EVALUATION (lvx_pause_slots; audio.py: pause_slots_ref) AND DO NOT DEPEND ON HOW
 * A SEGMENT IS CUT INTO CALLS. One segment is one sentence of one stream.
 *
 * Blocks. bl = sample_rate / 100: 80, 160, 240, 480 samples. A sentence of T > 0 samples is ceil(T / bl) blocks;
 * block j holds samples j bl .. min((j + 1) bl, T) - 1, so every block has bl samples but the last, which has
 * 1 .. bl. A sentence of no samples has no block.
 *
 * Slots. One per block, LVX_PAUSE_SLOT(rate, bytes per sample) = 8 + bl * bytes bytes, a multiple of 8:
 *   the record {uint16 n (samples of the block, 1 .. bl, little endian), uint8 active, uint8 last (1 on the
 *   sentence's last block), uint32 0};
 *   the payload: the block's n samples, byte for byte as the stage before wrote them, then the encoding's silence up
 *   to bl samples (the G.711 code of 0: 0xFF mu-law, 0xD5 A-law; zero bytes otherwise).
 *
 * The mark. active = 1 iff some sample of the block is louder than LVX_PAUSE_THRESH = 103 on the 16-bit scale
 * (about -50 dBFS): s16le |q| > 103, the magnitude taken in 32 bits (q = -32768 is active); f32le |v| > 103 / 32768
 * (= 0.003143310546875, exact in fp32), a NaN counting as active; mu-law / A-law the s16le test on the decoded sample
 * (lvx_pcm_g711_decode: the decoded magnitudes nearest the threshold are 96 and 104 for mu-law, 88 and 104 for A-law;
 * A-law's silence 0xD5 decodes to 8 and is silent). THE MARK IS A PROPERTY OF THE ENCODED SAMPLES: the same audio can
 * mark differently as f32le and as s16le at the edge (103.4 / 32768 is loud as f32le and rounds to 103, silent, as
 * s16le).
 *
 * Streaming. After a non-final call that brings the segment's input to T > 0 the blocks emitted so far are
 * floor((T - 1) / bl): the complete ones that at least one more sample follows; a final call emits the rest,
 * ceil(T / bl) in all. So the sentence's last block always leaves with the final call and always carries last = 1,
 * and the stage HOLDS BACK 1 .. bl SAMPLES (UP TO 10 ms) UNTIL THE SENTENCE ENDS. The library keeps them per KV slot
 * (two buffers of 480 * 4 bytes per slot: a launch reads one and writes the other) and, on the host, a mirror of the
 * slot's count, rate and encoding. A segment has one rate and one encoding: another before its final call is
 * LVX_E_ARG.
 *
 * The host's rule (audio.py), per request, P = pause_ms / 10 blocks and C = max_pause_ms / 10 blocks or none, with
 * LVX_PAUSE_LEAD = 2 and LVX_PAUSE_TRAIL = 5 blocks: a sentence without an active block delivers nothing; any other
 * delivers its blocks from max(first active - 2, 0) through min(last active + 5, its last block), the sentence's last
 * block with its n samples only; with C, a run of more than C silent blocks between two active ones keeps its first
 * C - 2 and its last 2; between two delivering sentences come exactly P blocks of the encoding's silence. With only
 * max_pause_ms named no edge is trimmed and no gap inserted. There is no crossfade at a cut: both sides of every cut
 * are blocks whose peak is at most the threshold, -50 dBFS; nothing more is claimed. */
#define LVX_PAUSE_THRESH 103
#define LVX_PAUSE_LEAD 2
#define LVX_PAUSE_TRAIL 5
#define LVX_PAUSE_SLOT(rate, sample_bytes) (8 + (rate) / 100 * (sample_bytes))
/* host only: blocks a call emits for a slot that has consumed t0 inputs of its segment (negative: LVX_E_ARG for an
 * unsupported rate, t0 < 0 or n_in < 0) */
int lvx_pcm_pause_emitted(int sample_rate, long long t0, int n_in, int final);
/* host only: bytes of one slot (negative: LVX_E_ARG for an unsupported rate or encoding) */
int lvx_pcm_pause_slot(int sample_rate, int encoding);
/* host only: the slots of blocks j0 .. j1 - 1 of the finished sentence y (T samples of the encoding) by the rule
 * above, serially. Returns their bytes. LVX_E_ARG: an unsupported rate or encoding, a null pointer, T < 0, blocks
 * outside 0 <= j0 <= j1 <= ceil(T / bl), slots of 2^31 bytes or more in one call; LVX_E_CAPACITY: cap is smaller
 * than the slots (nothing is written). */
int lvx_pause_slots(int sample_rate, int encoding, const void* y, long long T, long long j0, long long j1, uint8_t* out,
                    long long cap);
/* lvx_pcm_flac's conventions: rows b of in_dev (samples of the encoding, row b at in_dev + b * in_stride_bytes, n_in
 * samples) continue the pause segments of slots_host[b]; final_host[b] != 0 emits the sentence's last block and
 * resets the slot; n_in may be 0 with final. out row b starts at out_dev + b * out_stride_bytes; n_blocks_host[b] =
 * slots written. LVX_E_ARG (and no slot's state changed): an unsupported rate or encoding, or another pair than the
 * slot's open segment has, B < 1, n_in < 0, a slot out of range or named twice, in_dev or in_stride_bytes no multiple
 * of the sample's bytes, in_stride_bytes smaller than a row, out_dev or out_stride_bytes no multiple of 8.
 * LVX_E_CAPACITY (and no slot's state changed): out_stride_bytes smaller than a row's slots. lvx_pcm_reset also
 * forgets a slot's pause state. */
int lvx_pcm_pause(lvx_ctx* ctx, const void* in_dev, long long in_stride_bytes, int B, int n_in,
                  const int32_t* slots_host, const uint8_t* final_host, int sample_rate, int encoding, void* out_dev,
                  long long out_stride_bytes, int32_t* n_blocks_host, void* stream);

/* ---- WavTokenizer encoder, a context of its own (its weights are not needed for TTS).
 * Replaces WavTokenizer.encode_infer (WavTokenizer/decoder/pretrained.py:185-190 ->
 * decoder/feature_extractors.py:122-133): SEANet encoder (encoder/modules/seanet.py:94-143) + the
 * 1-codebook quantiser (encoder/quantization/vq.py:115-140, core_vq.py:175-183), fp32.
 * Weights by reference state_dict name: "feature_extractor.encodec.encoder.model.<i>.conv.conv.weight"
 * with weight_norm already resolved (w = g v / |v|, torch._weight_norm(v, g, 0)) [cout][cin][k], ".bias",
 * the LSTM's "<...>.13.lstm.{weight,bias}_{ih,hh}_l{0,1}", and the codebook
 * "feature_extractor.encodec.quantizer.vq.layers.0._codebook.embed" [4096][512]. */
typedef struct lvx_enc lvx_enc;
int lvx_enc_create(int device, long long max_samples, lvx_enc** out);  /* max_samples >= B * N of any call */
int lvx_enc_set_weight(lvx_enc* enc, const char* name, const float* data, int64_t numel);
int lvx_enc_finalize(lvx_enc* enc);
void lvx_enc_destroy(lvx_enc* enc);
/* frames T of an N-sample input (ceil(N / 320): the SConv1d padding chain) */
int lvx_enc_frames(int n_samples);
/* audio_dev [B][N] f32 -> features_dev [B][512][T] (codebook rows of the codes, the reference's
 * features layout), codes_dev [B][T] int32 (the reference returns them as [1][B][T]). Async on stream. */
int lvx_encode(lvx_enc* enc, const float* audio_dev, int B, int N, float* features_dev, int32_t* codes_dev,
               void* stream);
/* test hook: the pre-quantisation embedding [B][T][512] of the last lvx_encode */
int lvx_enc_embedding(lvx_enc* enc, float* dst_dev, int B, int T, void* stream);
/* Test hook (tests/test_gpu_encoder_stages.py): stages [first, last] of lvx_encode on caller-supplied input,
 * through lvx_encode's own stage list, launch helpers, SConv1d geometry, scratch and capacity checks (lvx_encode
 * is the window [0, LVX_ENC_STAGES - 1] of the same walk); the counterpart of lvx_codec_stages for the encoder.
 * It adds no kernel and no launch to lvx_encode. Activations are time-major float32, as the kernels use them.
 * Stages (LVX_ENC_STAGES of them), d = 32, 64, 128, 256 for the ratios r = 2, 4, 5, 8:
 *    0           conv "0" (k7, 1 -> 32)                        in: audio [B][L]     out: [B][L][32]
 *    1, 3, 5, 7  residual block of ratio 2, 4, 5, 8: block.1,
 *                shortcut, block.3 + shortcut                  [B][L][d]         -> [B][L][d]
 *    2, 4, 6, 8  ELU + strided down conv of that ratio         [B][L][d]         -> [B][ceil(L / r)][2 d]
 *    9           SLSTM: both layers and the skip               [B][T][512]       -> [B][T][512]
 *   10           ELU + conv "15" (k7)                          [B][T][512]       -> [B][T][512]
 *   11           quantiser: scores + select                    [B][T][512]       -> codes_dev int32 [B][T],
 *                                                                                   features_dev [B][512][T]
 * L is the length per stream of the input of stage `first`; any L >= 1 is legal at any stage. in_dev holds that
 * input; out_dev receives the output of stage `last` when last < 11 (it may be null otherwise); a window that
 * ends at 11 writes codes_dev and features_dev and, where scores_dev is not null, the scores x . e it selected
 * from, [B][T][4096]. Buffers are device buffers, copied / written in stream order. Arguments are checked as
 * lvx_encode checks them (LVX_E_CAPACITY: an intermediate of the window beyond the scratch sized by max_samples,
 * B beyond 1,024, and B * L beyond max_samples where first = 0; LVX_E_ARG), plus
 * 0 <= first <= last < LVX_ENC_STAGES. */
#define LVX_ENC_STAGES 12
int lvx_enc_stages(lvx_enc* enc, int first, int last, const float* in_dev, int B, int L, float* out_dev,
                   int32_t* codes_dev, float* features_dev, float* scores_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMVOX_H */
