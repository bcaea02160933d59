// C-ABI front end of libllmvox_hip.so (see include/llmvox.h).
//
// Owns: the device copies of all hot-path weights (converted / repacked for the kernels),
// the KV pool (max_streams slots x max_positions), the per-step scratch, the codec scratch,
// and the HIP graphs of the fused decode step.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "llmvox.h"
#include "ar_plan.h"

using namespace lvx;

namespace lvx {
static const Opts kDefaultOpts{};
static thread_local const Opts* t_opts = nullptr;
const Opts& opts() { return t_opts ? *t_opts : kDefaultOpts; }
OptScope::OptScope(const Opts* o) : prev(t_opts) { t_opts = o; }
OptScope::~OptScope() { t_opts = prev; }
}  // namespace lvx

static constexpr int kMaxCodecL = 4096;
#ifndef LVX_GRAPH_STEPS
#define LVX_GRAPH_STEPS 16  // A/B builds (tools/build_variant.sh NAME -DLVX_GRAPH_STEPS=n)
#endif
static constexpr int kGraphSteps = LVX_GRAPH_STEPS;  // decode steps per captured graph

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// Status of taken error bits (AR word | codec word << 16, as err_take_kernel reports them): the message
// names EVERY set condition; the code is the most specific one (index > state > capacity).
int bits_status(int32_t bits) {
  if (!bits) return LVX_OK;
  const int32_t ar = bits & 0xffff, cd = (bits >> 16) & 0xffff;
  std::string m;
  int code = 0;
  auto add = [&](int c, const char* what) {
    if (!m.empty()) m += "; ";
    m += what;
    if (code == 0 || (c == LVX_E_INDEX) || (c == LVX_E_STATE && code == LVX_E_CAPACITY)) code = c;
  };
  if (ar & 4) add(LVX_E_INDEX, "index out of range in self (a text id outside [0, 386) given to lvx_text_embed or a code "
                               "outside [0, 4096) given to lvx_codes_to_features)");
  if (cd & 4) add(LVX_E_INDEX, "index out of range in self (codec: a code outside [0, 4096) given to lvx_codec_decode_codes)");
  if (ar & 32) add(LVX_E_STATE, "a non-finite or out-of-range (|v| >= 2^25) partial in the fused MLP's fixed-point "
                                "accumulation (B <= 2): the logits of that step's rows are invalid");
  if (cd & 8) add(LVX_E_STATE, "ISTFT window envelope <= 1e-11 (spectral_ops.py:72 assertion)");
  if (ar & 1) add(LVX_E_CAPACITY, "a stream exceeded its KV capacity (max_positions)");
  if (ar & 2) add(LVX_E_CAPACITY, "a batch row ran past the end of its text plan (plan_stride)");
  if (!code) add(LVX_E_STATE, "unknown device error bits");
  char hex[32];
  snprintf(hex, sizeof hex, " [error bits 0x%x]", (unsigned)bits);
  return fail(code, m + hex);
}

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      return fail(LVX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));         \
  } while (0)

struct WeightSpec {
  std::vector<int64_t> shape;
};

std::map<std::string, WeightSpec> make_specs() {
  std::map<std::string, WeightSpec> s;
  s["transformer.wpe.weight"] = {{BLOCK_SIZE, D}};
  for (int i = 0; i < N_LAYER; ++i) {
    std::string p = "transformer.h." + std::to_string(i) + ".";
    s[p + "ln_1.weight"] = {{D}};
    s[p + "attn.c_attn.weight"] = {{3 * D, D}};
    s[p + "attn.c_proj.weight"] = {{D, D}};
    s[p + "ln_2.weight"] = {{D}};
    s[p + "mlp.c_fc.weight"] = {{DFF, D}};
    s[p + "mlp.c_proj.weight"] = {{D, DFF}};
  }
  s["transformer.ln_f.weight"] = {{D}};
  s["lm_head.weight"] = {{VOCAB, D}};
  s["encoder.embed_tokens.weight"] = {{TEXT_VOCAB, TEXT_DIM}};
  s["feature_extractor.encodec.quantizer.vq.layers.0._codebook.embed"] = {{4096, SPEECH_DIM}};
  const int CD = 768, CFF = 2304;
  s["backbone.embed.weight"] = {{CD, 512, 7}};
  s["backbone.embed.bias"] = {{CD}};
  s["backbone.norm.scale.weight"] = {{4, CD}};
  s["backbone.norm.shift.weight"] = {{4, CD}};
  for (int i : {0, 1, 3, 4}) {
    std::string p = "backbone.pos_net." + std::to_string(i) + ".";
    for (const char* n : {"norm1", "norm2"}) {
      s[p + n + ".weight"] = {{CD}};
      s[p + n + ".bias"] = {{CD}};
    }
    for (const char* n : {"conv1", "conv2"}) {
      s[p + n + ".weight"] = {{CD, CD, 3}};
      s[p + n + ".bias"] = {{CD}};
    }
  }
  s["backbone.pos_net.2.norm.weight"] = {{CD}};
  s["backbone.pos_net.2.norm.bias"] = {{CD}};
  for (const char* n : {"q", "k", "v", "proj_out"}) {
    s[std::string("backbone.pos_net.2.") + n + ".weight"] = {{CD, CD, 1}};
    s[std::string("backbone.pos_net.2.") + n + ".bias"] = {{CD}};
  }
  s["backbone.pos_net.5.weight"] = {{CD}};
  s["backbone.pos_net.5.bias"] = {{CD}};
  for (int i = 0; i < 12; ++i) {
    std::string p = "backbone.convnext." + std::to_string(i) + ".";
    s[p + "dwconv.weight"] = {{CD, 1, 7}};
    s[p + "dwconv.bias"] = {{CD}};
    s[p + "norm.scale.weight"] = {{4, CD}};
    s[p + "norm.shift.weight"] = {{4, CD}};
    s[p + "pwconv1.weight"] = {{CFF, CD}};
    s[p + "pwconv1.bias"] = {{CFF}};
    s[p + "pwconv2.weight"] = {{CD, CFF}};
    s[p + "pwconv2.bias"] = {{CD}};
    s[p + "gamma"] = {{CD}};
  }
  s["backbone.final_layer_norm.weight"] = {{CD}};
  s["backbone.final_layer_norm.bias"] = {{CD}};
  s["head.out.weight"] = {{1282, CD}};
  s["head.out.bias"] = {{1282}};
  return s;
}

const std::map<std::string, WeightSpec>& specs() {
  static const std::map<std::string, WeightSpec> s = make_specs();
  return s;
}

int64_t numel_of(const WeightSpec& w) {
  int64_t n = 1;
  for (auto d : w.shape) n *= d;
  return n;
}

}  // namespace

struct GraphKey {
  int B, stride, nsteps;
  const void *slots, *text, *rowstep, *tok, *margin;
  void* stream;
  bool sample = false;  // captured with the sampled select (greedy and sampling graphs sit side by side)
  bool operator<(const GraphKey& o) const {
    return std::tie(B, stride, nsteps, slots, text, rowstep, tok, margin, stream, sample) <
           std::tie(o.B, o.stride, o.nsteps, o.slots, o.text, o.rowstep, o.tok, o.margin, o.stream, o.sample);
  }
};

// host f32 -> OCP e4m3fn (gfx950 fp8), round to nearest even, saturated to +-448, NaN -> 0x7f
static uint8_t f32_to_e4m3_host(float x) {
  if (std::isnan(x)) return 0x7f;
  const uint8_t sign = std::signbit(x) ? 0x80 : 0x00;
  double a = std::fabs((double)x);
  if (a >= 448.0) return sign | 0x7e;
  if (a < std::ldexp(1.0, -6)) {  // subnormal: value = mant * 2^-9 (mant 8 is the smallest normal)
    const int q = (int)std::nearbyint(a * 512.0);
    return sign | (uint8_t)q;
  }
  int e;
  const double m = std::frexp(a, &e);  // a = m * 2^e, m in [0.5, 1)
  int mant = (int)std::nearbyint((m * 2.0 - 1.0) * 8.0);
  int ex = e - 1;
  if (mant == 8) { mant = 0; ++ex; }
  int code = ((ex + 7) << 3) | mant;
  if (code > 0x7e) code = 0x7e;
  return sign | (uint8_t)code;
}

// the second record of ArState::smp for a slot that asks for none of the extended controls: top_p 1, min_p 0 (lnminp -inf),
// repetition_penalty 1.0f, repetition_window 64
static const uint4 kSamplingNeutral{1u << 24, 0xff800000u, 0x3f800000u, 64u};

struct lvx_ctx {
  lvx_config cfg{};
  std::map<std::string, std::vector<float>> host;  // staged fp32 weights (released at finalize)
  std::vector<void*> allocs;
  bool finalized = false;
  ArWeights arw;
  ArState st;
  CodecWeights cw;
  CodecScratch cs;
  float* window_override = nullptr;
  std::map<GraphKey, hipGraphExec_t> graphs;
  std::vector<hipGraph_t> graph_defs;
  bool use_graphs = true;
  Opts opts;                 // this context's kernel options (lvx_set_option, under mu)
  unsigned opt_epoch = 0;    // bumped by every lvx_set_option on this context (under mu)
  unsigned graph_epoch = 0;  // opt_epoch when the cached graphs were captured
  hipStream_t capture_stream = nullptr;  // lvx_set_capture_stream (not owned); null: capture on the caller's
  hipStream_t own_capture_stream = nullptr;  // created for null-stream callers only (cached_graph)
  std::vector<float> smp_temp;  // host mirror of the slots' temperatures (lvx_stream_sampling, under mu)
  int n_sampling = 0;           // slots with temperature > 0: while any, the steps plan with sample = true
  // The PCM stages (pcm_host.h: the skeleton of their calls). Each has its device tables, a pool of two buffers per
  // slot [2][max_streams][*_HIST] and, in seg (under mu), the host mirror of every slot's segment.
  enum { SEG_CONVERT, SEG_STRETCH, SEG_RATIO, SEG_JOIN, SEG_LEVEL, SEG_FLAC, SEG_FORMANT, SEG_PAUSE, SEG_MARK, SEG_STAGES };
  std::vector<PcmSeg> seg[SEG_STAGES];
  float* pcm_taps = nullptr;  // rate and encoding: the taps of the three resampling rates
  float* pcm_hist = nullptr;
  float* str_win = nullptr;  // time stretch: the window tables (wr then wf)
  float* str_hist = nullptr;
  int* str_d = nullptr;      // the slots' d_{j-1} (one int per slot, device only)
  // pitch shift: every slot's table region [max_streams][RAT_TAPS_STRIDE] and the ratio it holds (it outlives the
  // segment and lvx_pcm_reset), and the host cache of the designed tables (never evicted: a stream-ordered copy may
  // still read an entry)
  float* rat_taps = nullptr;
  float* rat_hist = nullptr;
  std::map<std::pair<int, int>, std::vector<float>> rat_cache;
  std::vector<std::pair<int, int>> rat_tab;  // (L, M) of the table in the slot's region, (0, 0): none
  float* join_win = nullptr;  // dump join: the window tables (wr then wf)
  float* join_tail = nullptr;  // an open segment's current buffer holds the 320 samples not emitted yet
  float* lvl_win = nullptr;  // level: the window table w[-A .. A]
  float* lvl_hist = nullptr;  // (raw inputs)
  int16_t* flac_hist = nullptr;  // FLAC: the s16 samples no frame has taken yet
  float* fmt_tab = nullptr;   // formant: the tables [FMT_TABLES]: w, c, the twiddles
  float* fmt_hist = nullptr;
  unsigned char* pause_hist = nullptr;  // pause: the 1 .. bl encoded samples no block has taken yet (bytes)
  float* mrk_hist = nullptr;  // mark: its own [FMT_HIST] buffers (the tables are the formant stage's, the signs an argument)
  std::mutex mu;

  bool sampling_snapshot() {
    std::lock_guard<std::mutex> lk(mu);
    return n_sampling > 0;
  }
  // a snapshot of the options, taken under mu: the caller binds it (OptScope) for its launches
  Opts opts_snapshot() {
    std::lock_guard<std::mutex> lk(mu);
    return opts;
  }

  template <typename T>
  int dalloc(T** p, size_t n) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, n * sizeof(T) + 256);
    if (e != hipSuccess) return fail(LVX_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    allocs.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return 0;
  }
  int upload_f32(const std::vector<float>& v, const float** out) {
    float* d;
    if (int r = dalloc(&d, v.size())) return r;
    HIP_TRY(hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    *out = d;
    return 0;
  }
  // matrices in the weight dtype
  int upload_w(const std::vector<float>& v, const void** out) {
    if (cfg.weight_dtype == LVX_DTYPE_F32) return upload_f32(v, reinterpret_cast<const float**>(out));
    std::vector<bf16_t> h(v.size());
    for (size_t i = 0; i < v.size(); ++i) h[i] = f32_to_bf16(v[i]);
    bf16_t* d;
    if (int r = dalloc(&d, h.size())) return r;
    HIP_TRY(hipMemcpy(d, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    *out = d;
    return 0;
  }
  // codec GEMM weights: the weight dtype, or e4m3fn with one scale per output row (codec_dtype FP8:
  // s = max|w_row| / 448, q = RNE(w / s) saturated; dequantised exactly to bf16 in the GEMM loader)
  //
  // fp32 (parity mode) with K % 32 == 0: the matrix [rows][K] is followed in the same allocation by its
  // bf16x3 split image (same size, read by gemm_glds_kernel<float, SPLIT> in place of the fp32 rows):
  // per row and 32-k block kb, 16-B segment g (g < 4) holds bf16_rn(w) of k = kb + 4 g + e and
  // kb + 16 + 4 g + e (e = 0..3), segment 4 + g the lo parts bf16_rn(w - hi) of the same k (the k
  // order the kernel's A fragments are read in)
  int upload_cw(const std::vector<float>& v, int rows, const void** out, const float** scale_out) {
    const size_t K = v.size() / rows;
    if (cfg.codec_dtype != LVX_DTYPE_FP8 && cfg.weight_dtype == LVX_DTYPE_F32 && K % 32 == 0) {
      std::vector<float> both(2 * v.size());
      std::memcpy(both.data(), v.data(), v.size() * 4);
      bf16_t* sp = reinterpret_cast<bf16_t*>(both.data() + v.size());
      for (size_t n = 0; n < (size_t)rows; ++n)
        for (size_t kb = 0; kb < K; kb += 32) {
          bf16_t* o = sp + (n * K + kb) * 2;  // 128 B: 8 segments of 8 bf16
          for (int g = 0; g < 4; ++g)
            for (int h = 0; h < 2; ++h)
              for (int e = 0; e < 4; ++e) {
                const float x = v[n * K + kb + 16 * h + 4 * g + e];
                const bf16_t hi = f32_to_bf16(x);
                const uint32_t hb = (uint32_t)hi << 16;
                float hf;
                std::memcpy(&hf, &hb, 4);
                o[g * 8 + h * 4 + e] = hi;
                o[(4 + g) * 8 + h * 4 + e] = f32_to_bf16(x - hf);
              }
        }
      return upload_f32(both, reinterpret_cast<const float**>(out));
    }
    if (cfg.codec_dtype != LVX_DTYPE_FP8) return upload_w(v, out);
    std::vector<uint8_t> q(v.size());
    std::vector<float> sc(rows);
    for (int n = 0; n < rows; ++n) {
      float mx = 0.f;
      for (size_t k = 0; k < K; ++k) mx = std::max(mx, std::fabs(v[n * K + k]));
      const float s = mx > 0.f ? mx / 448.f : 1.f;
      sc[n] = s;
      for (size_t k = 0; k < K; ++k) q[n * K + k] = f32_to_e4m3_host(v[n * K + k] / s);
    }
    uint8_t* d;
    if (int r = dalloc(&d, q.size())) return r;
    HIP_TRY(hipMemcpy(d, q.data(), q.size(), hipMemcpyHostToDevice));
    *out = d;
    return upload_f32(sc, scale_out);
  }
  const std::vector<float>& H(const std::string& k) { return host.at(k); }
};

// conv weight [N][C][T] -> tap-major [N][T*C]
static std::vector<float> repack_conv(const std::vector<float>& w, int N, int C, int T) {
  std::vector<float> o((size_t)N * C * T);
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < C; ++c)
      for (int t = 0; t < T; ++t) o[(size_t)n * T * C + (size_t)t * C + c] = w[((size_t)n * C + c) * T + t];
  return o;
}

// mlp.c_proj [768][3072] -> [3072/16 blocks][256 threads][3][16]: block k's thread t holds
// W[t + 256 jj][16 k + j] as 96 contiguous bytes (bf16), the operand order of ar_mlp_fused_kernel
// mlp.c_proj [768][3072] for ar_mlp_fused_kernel: groups of 4 columns k4, then the output row's
// third jj (e = t + 256 jj), then thread t, 4 values: a wave's 8-byte load covers 512 contiguous bytes
static std::vector<float> pack_mproj(const std::vector<float>& w) {
  std::vector<float> o((size_t)D * DFF);
  size_t q = 0;
  for (int k4 = 0; k4 < DFF / 4; ++k4)
    for (int jj = 0; jj < 3; ++jj)
      for (int t = 0; t < 256; ++t)
        for (int j = 0; j < 4; ++j) o[q++] = w[(size_t)(t + 256 * jj) * DFF + 4 * k4 + j];
  return o;
}

// [N][K] -> [N / 16][K / 32][64 lanes][8]: lane l of fragment (T, j) holds W[16 T + l % 16][32 j + 8 (l / 16) ..+8],
// the A operand of v_mfma_f32_16x16x32_bf16 as the batched GEMMs load it (one contiguous KB per wave load)
static std::vector<float> pack_frag(const std::vector<float>& w, int N, int K) {
  std::vector<float> o((size_t)N * K);
  size_t q = 0;
  for (int t = 0; t < N / 16; ++t)
    for (int j = 0; j < K / 32; ++j)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 8; ++e) o[q++] = w[(size_t)(16 * t + l % 16) * K + 32 * j + 8 * (l / 16) + e];
  return o;
}

// fp32 [N][K] -> [N / 16][K / 16][64 lanes][4]: lane l of fragment (T, j) holds
// W[16 T + l % 16][16 j + 4 (l / 16) .. +4] (ar_f32b_kernel: v_mfma_f32_16x16x4_f32 k-step 4 j + e takes
// element e)
static std::vector<float> pack_frag32(const std::vector<float>& w, int N, int K) {
  std::vector<float> o((size_t)N * K);
  size_t q = 0;
  for (int t = 0; t < N / 16; ++t)
    for (int j = 0; j < K / 16; ++j)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 4; ++e) o[q++] = w[(size_t)(16 * t + l % 16) * K + 16 * j + 4 * (l / 16) + e];
  return o;
}

// ---- the PCM stages' entries (below) ----
// The arguments every stage's entry takes (arrays: the host arrays, null if one is missing); out_dev only where the
// call launches. Then the entry runs pcm_host.h's skeleton: pcm_plan under mu (the mirror only: released before the
// launches), pcm_launches behind it.
static int pcm_args(int B, int n_in, const void* pcm, const void* arrays, bool launch, const void* out, long long out_stride) {
  if (B < 1 || n_in < 0 || !arrays) return fail(LVX_E_ARG, "bad B / n_in / host arrays");
  if (n_in > 0 && !pcm) return fail(LVX_E_ARG, "null pcm_dev");
  if (launch && (!out || (reinterpret_cast<uintptr_t>(out) & 3) || out_stride < 0 || (out_stride & 3)))
    return fail(LVX_E_ARG, "out_dev and out_stride_bytes must be multiples of 4");
  return LVX_OK;
}

template <class Rows, class Row, class Launch>
static int pcm_launches(lvx_ctx* c, const std::vector<Row>& rows, Launch launch) {
  HIP_TRY(hipSetDevice(c->cfg.device));
  pcm_chunks<Rows>(rows, launch);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

extern "C" {

int lvx_version(void) { return 2; }

const char* lvx_last_error(void) { return g_err.c_str(); }

int lvx_create(const lvx_config* cfg, lvx_ctx** out) {
  if (!cfg || !out) return fail(LVX_E_ARG, "null argument");
  if (cfg->weight_dtype != LVX_DTYPE_F32 && cfg->weight_dtype != LVX_DTYPE_BF16)
    return fail(LVX_E_ARG, "weight_dtype must be LVX_DTYPE_F32 or LVX_DTYPE_BF16");
  if (cfg->kv_dtype != LVX_DTYPE_F32 && cfg->kv_dtype != LVX_DTYPE_BF16 && cfg->kv_dtype != LVX_DTYPE_FP8)
    return fail(LVX_E_ARG, "kv_dtype must be LVX_DTYPE_F32, LVX_DTYPE_BF16 or LVX_DTYPE_FP8");
  if (cfg->max_streams < 1 || cfg->max_streams > 1024) return fail(LVX_E_ARG, "max_streams out of range [1,1024]");
  if (cfg->max_positions < 1 || cfg->max_positions > BLOCK_SIZE)
    return fail(LVX_E_ARG, "max_positions out of range [1,8192] (GPTConfig.block_size)");
  if (cfg->max_codec_frames < 1) return fail(LVX_E_ARG, "max_codec_frames must be >= 1");
  if (cfg->codec_dtype != 0 && !(cfg->codec_dtype == LVX_DTYPE_FP8 && cfg->weight_dtype == LVX_DTYPE_BF16))
    return fail(LVX_E_ARG, "codec_dtype must be 0 or LVX_DTYPE_FP8 (with weight_dtype LVX_DTYPE_BF16)");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) return fail(LVX_E_HIP, "no HIP device available");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(LVX_E_ARG, "device ordinal out of range");
  auto* c = new lvx_ctx();
  c->cfg = *cfg;
  *out = c;
  return LVX_OK;
}

void lvx_destroy(lvx_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->cfg.device);
  for (auto& kv : c->graphs) (void)hipGraphExecDestroy(kv.second);
  for (auto g : c->graph_defs) (void)hipGraphDestroy(g);
  if (c->own_capture_stream) (void)hipStreamDestroy(c->own_capture_stream);
  for (void* p : c->allocs) (void)hipFree(p);
  delete c;
}

int lvx_set_weight(lvx_ctx* c, const char* name, const float* data, int64_t numel) {
  if (!c || !name || !data) return fail(LVX_E_ARG, "null argument");
  std::string k(name);
  if (c->finalized) return fail(LVX_E_STATE, "weights are frozen after lvx_finalize");
  if (k == "head.istft.window") {
    if (numel != 1280) return fail(LVX_E_ARG, "head.istft.window must have 1280 elements");
    c->host[k] = std::vector<float>(data, data + numel);
    return LVX_OK;
  }
  auto it = specs().find(k);
  if (it == specs().end()) return fail(LVX_E_NAME, "unknown weight name: " + k);
  if (numel != numel_of(it->second))
    return fail(LVX_E_ARG, "weight " + k + ": expected " + std::to_string(numel_of(it->second)) + " elements, got " +
                               std::to_string(numel));
  c->host[k] = std::vector<float>(data, data + numel);
  return LVX_OK;
}

int lvx_missing_weights(lvx_ctx* c, const char** first) {
  if (!c) return fail(LVX_E_ARG, "null ctx");
  if (c->finalized) return 0;
  int n = 0;
  static thread_local std::string name;
  for (auto& kv : specs())
    if (!c->host.count(kv.first)) {
      if (n == 0) name = kv.first;
      ++n;
    }
  if (first) *first = n ? name.c_str() : nullptr;
  return n;
}

int lvx_finalize(lvx_ctx* c) {
  if (!c) return fail(LVX_E_ARG, "null ctx");
  if (c->finalized) return LVX_OK;
  const char* miss = nullptr;
  if (lvx_missing_weights(c, &miss) > 0) return fail(LVX_E_STATE, std::string("missing weight: ") + miss);
  HIP_TRY(hipSetDevice(c->cfg.device));
  int r;
#define UP_F(key, dst) \
  if ((r = c->upload_f32(c->H(key), &(dst)))) return r;
#define UP_W(vec, dst) \
  if ((r = c->upload_w((vec), &(dst)))) return r;
  // ---- AR ----
  ArWeights& w = c->arw;
  UP_F("transformer.wpe.weight", w.wpe);
  UP_F("encoder.embed_tokens.weight", w.text_table);
  UP_F("feature_extractor.encodec.quantizer.vq.layers.0._codebook.embed", w.codebook);
  for (int i = 0; i < N_LAYER; ++i) {
    std::string p = "transformer.h." + std::to_string(i) + ".";
    UP_F(p + "ln_1.weight", w.ln1[i]);
    UP_F(p + "ln_2.weight", w.ln2[i]);
    UP_W(c->H(p + "attn.c_attn.weight"), w.w_attn[i]);
    UP_W(c->H(p + "attn.c_proj.weight"), w.w_aproj[i]);
    UP_W(c->H(p + "mlp.c_fc.weight"), w.w_fc[i]);
    UP_W(c->H(p + "mlp.c_proj.weight"), w.w_mproj[i]);
    if (c->cfg.weight_dtype == LVX_DTYPE_BF16) {  // thread-packed copy for the fused MLP (ar_mlp_fused_kernel)
      UP_W(pack_mproj(c->H(p + "mlp.c_proj.weight")), w.w_mproj_pk[i]);
      UP_W(pack_frag(c->H(p + "attn.c_attn.weight"), 3 * D, D), w.f_attn[i]);
      UP_W(pack_frag(c->H(p + "attn.c_proj.weight"), D, D), w.f_aproj[i]);
      UP_W(pack_frag(c->H(p + "mlp.c_fc.weight"), DFF, D), w.f_fc[i]);
      UP_W(pack_frag(c->H(p + "mlp.c_proj.weight"), D, DFF), w.f_mproj[i]);
      // batched c_fc: LN2(x) . W^T = rstd * ((x * g) . W^T - mean * G), G[n] = sum_k g[k] W[n][k]
      // over the bf16 weights the GEMM multiplies (double accumulation, rounded once)
      const std::vector<float>& wf = c->H(p + "mlp.c_fc.weight");
      const std::vector<float>& g2 = c->H(p + "ln_2.weight");
      std::vector<float> gs(DFF);
      for (int n = 0; n < DFF; ++n) {
        double acc = 0.0;
        for (int k = 0; k < D; ++k) {
          const uint32_t hb = (uint32_t)f32_to_bf16(wf[(size_t)n * D + k]) << 16;
          float wv;
          std::memcpy(&wv, &hb, 4);
          acc += (double)g2[k] * (double)wv;
        }
        gs[n] = (float)acc;
      }
      if ((r = c->upload_f32(gs, &w.fc_gsum[i]))) return r;
    } else {  // fp32 parity mode: packed copies for the batched exact-fp32 MFMA GEMMs (ar_f32b_kernel)
      UP_W(pack_frag32(c->H(p + "attn.c_attn.weight"), 3 * D, D), w.f_attn[i]);
      UP_W(pack_frag32(c->H(p + "attn.c_proj.weight"), D, D), w.f_aproj[i]);
      UP_W(pack_frag32(c->H(p + "mlp.c_fc.weight"), DFF, D), w.f_fc[i]);
      UP_W(pack_frag32(c->H(p + "mlp.c_proj.weight"), D, DFF), w.f_mproj[i]);
    }
  }
  UP_F("transformer.ln_f.weight", w.lnf);
  UP_W(c->H("lm_head.weight"), w.w_lm);
  if (c->cfg.weight_dtype == LVX_DTYPE_BF16) {
    UP_W(pack_frag(c->H("lm_head.weight"), VOCAB, D), w.f_lm);
    // layer 0's c_attn as table rows (ArWeights q0_*): G on the host over the bf16 weights (as fc_gsum),
    // the three tables by a device GEMM over the uploaded bf16 c_attn weight
    const std::vector<float>& wa = c->H("transformer.h.0.attn.c_attn.weight");
    const std::vector<float>& g1 = c->H("transformer.h.0.ln_1.weight");
    std::vector<float> gq(3 * D);
    for (int n = 0; n < 3 * D; ++n) {
      double acc = 0.0;
      for (int k = 0; k < D; ++k) {
        const uint32_t hb = (uint32_t)f32_to_bf16(wa[(size_t)n * D + k]) << 16;
        float wv;
        std::memcpy(&wv, &hb, 4);
        acc += (double)g1[k] * (double)wv;
      }
      gq[n] = (float)acc;
    }
    if ((r = c->upload_f32(gq, &w.q0_g))) return r;
    float *tt, *tc, *tp;
    const int P = c->cfg.max_positions;
    if ((r = c->dalloc(&tt, (size_t)TEXT_VOCAB * 3 * D)) || (r = c->dalloc(&tc, (size_t)VOCAB * 3 * D)) ||
        (r = c->dalloc(&tp, (size_t)P * 3 * D)))
      return r;
    ar_launch_q0_tables(w, P, tt, tc, tp, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    w.q0_text = tt;
    w.q0_code = tc;
    w.q0_pos = tp;
  } else {
    UP_W(pack_frag32(c->H("lm_head.weight"), VOCAB, D), w.f_lm);
  }
  // ---- codec ----
  CodecWeights& cw = c->cw;
  cw.codebook = w.codebook;
#define UP_CW(vec, rows, dst, sdst) \
  if ((r = c->upload_cw((vec), (rows), &(dst), &(sdst)))) return r;
  cw.wfp8 = c->cfg.codec_dtype == LVX_DTYPE_FP8;
  UP_CW(repack_conv(c->H("backbone.embed.weight"), 768, 512, 7), 768, cw.embed_w, cw.embed_s);
  UP_F("backbone.embed.bias", cw.embed_b);
  UP_F("backbone.norm.scale.weight", cw.ada_scale);
  UP_F("backbone.norm.shift.weight", cw.ada_shift);
  int ri = 0;
  for (int i : {0, 1, 3, 4}) {
    std::string p = "backbone.pos_net." + std::to_string(i) + ".";
    UP_F(p + "norm1.weight", cw.rn_n1w[ri]);
    UP_F(p + "norm1.bias", cw.rn_n1b[ri]);
    UP_F(p + "norm2.weight", cw.rn_n2w[ri]);
    UP_F(p + "norm2.bias", cw.rn_n2b[ri]);
    UP_CW(repack_conv(c->H(p + "conv1.weight"), 768, 768, 3), 768, cw.rn_c1w[ri], cw.rn_c1s[ri]);
    UP_F(p + "conv1.bias", cw.rn_c1b[ri]);
    UP_CW(repack_conv(c->H(p + "conv2.weight"), 768, 768, 3), 768, cw.rn_c2w[ri], cw.rn_c2s[ri]);
    UP_F(p + "conv2.bias", cw.rn_c2b[ri]);
    ++ri;
  }
  {
    const std::string p = "backbone.pos_net.2.";
    UP_F(p + "norm.weight", cw.at_nw);
    UP_F(p + "norm.bias", cw.at_nb);
    std::vector<float> qkv, qkvb;
    for (const char* n : {"q", "k", "v"}) {
      auto& m = c->H(p + n + ".weight");
      qkv.insert(qkv.end(), m.begin(), m.end());
      auto& b = c->H(p + n + ".bias");
      qkvb.insert(qkvb.end(), b.begin(), b.end());
    }
    UP_CW(qkv, 3 * 768, cw.at_qkv_w, cw.at_qkv_s);
    if ((r = c->upload_f32(qkvb, &cw.at_qkv_b))) return r;
    UP_CW(c->H(p + "proj_out.weight"), 768, cw.at_proj_w, cw.at_proj_s);
    UP_F(p + "proj_out.bias", cw.at_proj_b);
  }
  UP_F("backbone.pos_net.5.weight", cw.pn_w);
  UP_F("backbone.pos_net.5.bias", cw.pn_b);
  for (int i = 0; i < 12; ++i) {
    std::string p = "backbone.convnext." + std::to_string(i) + ".";
    {  // depthwise conv [768][1][7] -> tap-major [7][768] (16-byte weight loads in dwconv_adaln)
      const std::vector<float>& dwv = c->H(p + "dwconv.weight");
      std::vector<float> t(dwv.size());
      for (int ch = 0; ch < 768; ++ch)
        for (int k = 0; k < 7; ++k) t[(size_t)k * 768 + ch] = dwv[(size_t)ch * 7 + k];
      if ((r = c->upload_f32(t, &cw.dw_w[i]))) return r;
    }
    UP_F(p + "dwconv.bias", cw.dw_b[i]);
    UP_F(p + "norm.scale.weight", cw.cn_scale[i]);
    UP_F(p + "norm.shift.weight", cw.cn_shift[i]);
    UP_CW(c->H(p + "pwconv1.weight"), 2304, cw.pw1_w[i], cw.pw1_s[i]);
    UP_F(p + "pwconv1.bias", cw.pw1_b[i]);
    UP_CW(c->H(p + "pwconv2.weight"), 768, cw.pw2_w[i], cw.pw2_s[i]);
    UP_F(p + "pwconv2.bias", cw.pw2_b[i]);
    UP_F(p + "gamma", cw.gamma[i]);
  }
  UP_F("backbone.final_layer_norm.weight", cw.fln_w);
  UP_F("backbone.final_layer_norm.bias", cw.fln_b);
  UP_CW(c->H("head.out.weight"), 1282, cw.head_w, cw.head_s);
  UP_F("head.out.bias", cw.head_b);
  {
    std::vector<float> win(1280);
    if (c->host.count("head.istft.window")) win = c->H("head.istft.window");
    else
      for (int n = 0; n < 1280; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / 1280.0));
    if ((r = c->upload_f32(win, &cw.window))) return r;
    std::vector<float> tw(2 * 1280);
    for (int m = 0; m < 1280; ++m) {
      tw[2 * m] = (float)std::cos(2.0 * M_PI * m / 1280.0);
      tw[2 * m + 1] = (float)std::sin(2.0 * M_PI * m / 1280.0);
    }
    if ((r = c->upload_f32(tw, &cw.twiddle))) return r;
  }
#undef UP_F
#undef UP_W
#undef UP_CW
  // ---- AR state ----
  ArState& st = c->st;
  const int S = c->cfg.max_streams, P = c->cfg.max_positions;
  // the bf16 operand rows (xn, xb, hb) are stored and read in whole 16-row MFMA tiles when they are
  // fragment-packed (xfrag, 9 <= B <= 32): a partly filled tile spans 16 rows, so round up
  const int S16 = (S + 15) / 16 * 16;
  st.max_pos = P;
  st.max_streams = S;
  st.kv_chunks = (P + KV_CHUNK - 1) / KV_CHUNK;
  {  // the slots' sampling state: every slot greedy with the neutral extended record
    char* blk;
    if ((r = c->dalloc(&blk, ArState::smp_bytes(S)))) return r;
    st.smp = reinterpret_cast<uint4*>(blk);
    HIP_TRY(hipMemset(blk, 0, ArState::smp_bytes(S)));
    std::vector<uint4> rec((size_t)2 * S, uint4{0u, 0u, 0u, 0u});
    for (int s = 0; s < S; ++s) rec[2 * s + 1] = kSamplingNeutral;
    HIP_TRY(hipMemcpy(st.smp, rec.data(), rec.size() * sizeof(uint4), hipMemcpyHostToDevice));
  }
  c->smp_temp.assign(S, 0.f);
  c->n_sampling = 0;
  if ((r = c->dalloc(&st.slots, S)) || (r = c->dalloc(&st.pos, S)) || (r = c->dalloc(&st.prev, S)) ||
      (r = c->dalloc(&st.err, 4)) || (r = c->dalloc(&st.x, (size_t)2 * S * D)) || (r = c->dalloc(&st.q, (size_t)S * D)) ||
      (r = c->dalloc(&st.part_o, (size_t)S * N_HEAD * NSPLIT * HD)) ||
      (r = c->dalloc(&st.part_ml, (size_t)S * N_HEAD * NSPLIT * 2)) || (r = c->dalloc(&st.h, (size_t)S * DFF)) ||
      (r = c->dalloc(&st.logits, (size_t)S * VOCAB)) || (r = c->dalloc(&st.rowinfo, S)) ||
      (r = c->dalloc(&st.rowinfo_n, S)) || (r = c->dalloc(&st.rowx, S)) || (r = c->dalloc(&st.rowx_n, S)) ||
      (r = c->dalloc(&st.selp, 4)) || (r = c->dalloc(&st.selrow, S)) ||
      (r = c->dalloc(&st.xn, (size_t)S16 * D)) || (r = c->dalloc(&st.hb, (size_t)S16 * DFF)) ||
      (r = c->dalloc(&st.xb, (size_t)S16 * D)) || (r = c->dalloc(&st.xstat, (size_t)(D / 16) * S * 2)) ||
      (r = c->dalloc(&st.lmbest, (size_t)LM_MAX_BLOCKS * 4 * 2)) ||
      (r = c->dalloc(&st.yacc, (size_t)YCOPIES * S * D)) || (r = c->dalloc(&st.qkvp, (size_t)4 * S * 3 * D)) ||
      (r = c->dalloc(&st.yfx, (size_t)YCOPIES * S * D)))
    return r;
  HIP_TRY(hipMemset(st.yfx, 0, (size_t)YCOPIES * S * D * 8));
  HIP_TRY(hipMemset(st.yacc, 0, (size_t)YCOPIES * S * D * 4));
  HIP_TRY(hipMemset(st.x, 0, (size_t)2 * S * D * 4));  // (every row of x2 that c_proj reads was published by its attention blocks first: defined bytes, no more)
  HIP_TRY(hipMemset(st.selp, 0, 16));
  HIP_TRY(hipMemset(st.part_o, 0, (size_t)S * N_HEAD * NSPLIT * HD * 4));
  HIP_TRY(hipMemset(st.part_ml, 0, (size_t)S * N_HEAD * NSPLIT * 2 * 4));
  HIP_TRY(hipMemset(st.pos, 0, S * 4));
  HIP_TRY(hipMemset(st.prev, 0, S * 4));
  HIP_TRY(hipMemset(st.err, 0, 16));
  const size_t kvn = (size_t)N_LAYER * st.kv_chunks * S * N_HEAD * KV_CHUNK * HD;
  const size_t kvb = c->cfg.kv_dtype == LVX_DTYPE_BF16 ? 2 : c->cfg.kv_dtype == LVX_DTYPE_FP8 ? 1 : 4;
  {
    char* k;
    char* v;
    if ((r = c->dalloc(&k, kvn * kvb)) || (r = c->dalloc(&v, kvn * kvb))) return r;
    st.kc = k;
    st.vc = v;
  }
  // ---- codec scratch ----
  CodecScratch& cs = c->cs;
  const int M = c->cfg.max_codec_frames;
  cs.max_frames = M;
  cs.ws_floats = (size_t)std::max(M, 256) * 2304 * 4;
  if ((r = c->dalloc(&cs.x, (size_t)M * 768)) || (r = c->dalloc(&cs.t1, (size_t)M * 2304)) ||
      (r = c->dalloc(&cs.t2, (size_t)(M + 4 * 64) * 2304 + (size_t)768 * 4 * M)) ||
      (r = c->dalloc(&cs.feats, (size_t)M * 512)) || (r = c->dalloc(&cs.gn, (size_t)M * 768)) ||
      (r = c->dalloc(&cs.ws, (size_t)std::max(M, 256) * 2304 * 4)) ||
      (r = c->dalloc(&cs.att, (size_t)M * (std::min(M, kMaxCodecL) + 4))) ||
      (r = c->dalloc(&cs.stats, (size_t)M * 32 * 2)) || (r = c->dalloc(&cs.spec, (size_t)M * 1282)) ||
      (r = c->dalloc(&cs.frames, (size_t)M * 1280)) || (r = c->dalloc(&cs.rowscale, (size_t)M)) ||
      (r = c->dalloc(&cs.tick, 4096)))
    return r;
  HIP_TRY(hipMemset(cs.tick, 0, 4096 * 4));
  cs.err = st.err + 1;  // the codec's own word (it may run on a second stream beside the AR)
  // ---- PCM output stage (allocated last: every other buffer stays where it was) ----
  {
    std::vector<float> taps;
    for (const PcmRate& pr : kPcmRates) {
      const std::vector<float> h = pcm_design(pr);
      taps.insert(taps.end(), h.begin(), h.end());
    }
    if ((r = c->dalloc(&c->pcm_taps, taps.size())) || (r = c->dalloc(&c->pcm_hist, (size_t)2 * S * PCM_HIST))) return r;
    HIP_TRY(hipMemcpy(c->pcm_taps, taps.data(), taps.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(c->pcm_hist, 0, (size_t)2 * S * PCM_HIST * 4));
    float win[2 * STR_H];
    stretch_design(win, win + STR_H);
    if ((r = c->dalloc(&c->str_win, 2 * STR_H)) || (r = c->dalloc(&c->str_hist, (size_t)2 * S * STR_HIST)) ||
        (r = c->dalloc(&c->str_d, (size_t)S)))
      return r;
    HIP_TRY(hipMemcpy(c->str_win, win, sizeof(win), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(c->str_hist, 0, (size_t)2 * S * STR_HIST * 4));
    HIP_TRY(hipMemset(c->str_d, 0, (size_t)S * 4));
  }
  // ---- the slots' token history (S * P * 2 bytes; allocated last: every other buffer stays where it was) ----
  if ((r = c->dalloc(&st.hist, (size_t)S * P)) || (r = c->dalloc(&st.hist_from, S))) return r;
  HIP_TRY(hipMemset(st.hist, 0, (size_t)S * P * 2));
  HIP_TRY(hipMemset(st.hist_from, 0, (size_t)S * 4));
  // ---- PCM pitch shift (allocated last: every other buffer stays where it was) ----
  if ((r = c->dalloc(&c->rat_taps, (size_t)S * RAT_TAPS_STRIDE)) || (r = c->dalloc(&c->rat_hist, (size_t)2 * S * RAT_HIST)))
    return r;
  HIP_TRY(hipMemset(c->rat_taps, 0, (size_t)S * RAT_TAPS_STRIDE * 4));
  HIP_TRY(hipMemset(c->rat_hist, 0, (size_t)2 * S * RAT_HIST * 4));
  c->rat_tab.assign(S, {0, 0});
  // ---- PCM dump join (allocated last: every other buffer stays where it was) ----
  {
    float win[2 * JOIN_HOLD];
    join_design(win, win + JOIN_HOLD);
    if ((r = c->dalloc(&c->join_win, 2 * JOIN_HOLD)) || (r = c->dalloc(&c->join_tail, (size_t)2 * S * JOIN_HOLD))) return r;
    HIP_TRY(hipMemcpy(c->join_win, win, sizeof(win), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(c->join_tail, 0, (size_t)2 * S * JOIN_HOLD * 4));
  }
  // ---- PCM level (allocated last: every other buffer stays where it was) ----
  {
    float win[LVL_TAPS];
    level_design(win);
    if ((r = c->dalloc(&c->lvl_win, LVL_TAPS)) || (r = c->dalloc(&c->lvl_hist, (size_t)2 * S * LVL_HIST))) return r;
    HIP_TRY(hipMemcpy(c->lvl_win, win, sizeof(win), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(c->lvl_hist, 0, (size_t)2 * S * LVL_HIST * 4));
  }
  // ---- PCM FLAC (allocated last: every other buffer stays where it was) ----
  if ((r = c->dalloc(&c->flac_hist, (size_t)2 * S * FLAC_HIST))) return r;
  HIP_TRY(hipMemset(c->flac_hist, 0, (size_t)2 * S * FLAC_HIST * 2));
  // ---- PCM formant (allocated last: every other buffer stays where it was) ----
  {
    std::vector<float> tab(FMT_TABLES);
    formant_design(tab.data(), tab.data() + FMT_N, tab.data() + FMT_N + FMT_TAPS);
    if ((r = c->dalloc(&c->fmt_tab, FMT_TABLES)) || (r = c->dalloc(&c->fmt_hist, (size_t)2 * S * FMT_HIST))) return r;
    HIP_TRY(hipMemcpy(c->fmt_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(c->fmt_hist, 0, (size_t)2 * S * FMT_HIST * 4));
  }
  // ---- PCM pause (allocated last: every other buffer stays where it was) ----
  if ((r = c->dalloc(&c->pause_hist, (size_t)2 * S * PAUSE_HIST))) return r;
  HIP_TRY(hipMemset(c->pause_hist, 0, (size_t)2 * S * PAUSE_HIST));
  // ---- PCM mark (allocated last: every other buffer stays where it was) ----
  if ((r = c->dalloc(&c->mrk_hist, (size_t)2 * S * FMT_HIST))) return r;
  HIP_TRY(hipMemset(c->mrk_hist, 0, (size_t)2 * S * FMT_HIST * 4));
  for (auto& v : c->seg) v.assign(S, PcmSeg{});
  HIP_TRY(hipDeviceSynchronize());
  c->host.clear();
  c->finalized = true;
  return LVX_OK;
}

#define NEED_FINAL(c)                                                              \
  do {                                                                             \
    if (!(c)) return fail(LVX_E_ARG, "null ctx");                                  \
    if (!(c)->finalized) return fail(LVX_E_STATE, "call lvx_finalize first");      \
  } while (0)

int lvx_text_embed(lvx_ctx* c, const int64_t* ids, int n, float* out, void* stream) {
  NEED_FINAL(c);
  if (n < 0 || (n > 0 && (!ids || !out))) return fail(LVX_E_ARG, "bad ids/out");
  HIP_TRY(hipSetDevice(c->cfg.device));
  launch_text_embed(c->arw.text_table, ids, n, out, c->st.err, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

int lvx_codes_to_features(lvx_ctx* c, const int64_t* codes, int B, int L, float* feats, void* stream) {
  NEED_FINAL(c);
  if (B < 0 || L < 0 || ((B * L) > 0 && (!codes || !feats))) return fail(LVX_E_ARG, "bad codes/feats");
  HIP_TRY(hipSetDevice(c->cfg.device));
  launch_codes_to_features(c->arw.codebook, codes, B, L, feats, c->st.err, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

int lvx_stream_reset(lvx_ctx* c, int slot, void* stream) {
  NEED_FINAL(c);
  if (slot < 0 || slot >= c->cfg.max_streams) return fail(LVX_E_ARG, "slot out of range");
  HIP_TRY(hipSetDevice(c->cfg.device));
  launch_reset_slot(c->st, slot, (hipStream_t)stream);  // position 0, the history known from 0
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

int lvx_stream_set(lvx_ctx* c, int slot, int pos, int prev_token, void* stream) {
  NEED_FINAL(c);
  if (slot < 0 || slot >= c->cfg.max_streams) return fail(LVX_E_ARG, "slot out of range");
  if (pos < 0 || pos > c->cfg.max_positions) return fail(LVX_E_CAPACITY, "position out of range");
  if (prev_token < 0 || prev_token >= VOCAB) return fail(LVX_E_ARG, "prev_token out of range");
  HIP_TRY(hipSetDevice(c->cfg.device));
  launch_set_slot(c->st, slot, pos, prev_token, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

int lvx_stream_sampling_ex(lvx_ctx* c, int slot, const lvx_sampling* p, void* stream) {
  NEED_FINAL(c);
  if (slot < 0 || slot >= c->cfg.max_streams) return fail(LVX_E_ARG, "slot out of range");
  if (!p) return fail(LVX_E_ARG, "null sampling parameters");
  if (!std::isfinite(p->temperature) || p->temperature < 0.f) return fail(LVX_E_ARG, "temperature must be finite and >= 0");
  if (p->top_k < 0) return fail(LVX_E_ARG, "top_k must be >= 0");
  if (!(p->top_p > 0.f && p->top_p <= 1.f)) return fail(LVX_E_ARG, "top_p must be in (0, 1]");
  if (!(p->min_p >= 0.f && p->min_p < 1.f)) return fail(LVX_E_ARG, "min_p must be in [0, 1)");
  if (!std::isfinite(p->repetition_penalty) || !(p->repetition_penalty > 0.f))
    return fail(LVX_E_ARG, "repetition_penalty must be finite and > 0");
  if (p->repetition_window < 1 || p->repetition_window > 256) return fail(LVX_E_ARG, "repetition_window must be in [1, 256]");
  HIP_TRY(hipSetDevice(c->cfg.device));
  const long long P = std::min(std::max(std::llround((double)p->top_p * 16777216.0), 1LL), 1LL << 24);
  const float lnminp = (float)std::log((double)p->min_p);  // min_p 0: -inf, no crop
  uint4 ex;
  ex.x = (uint32_t)P;
  std::memcpy(&ex.y, &lnminp, 4);
  std::memcpy(&ex.z, &p->repetition_penalty, 4);
  ex.w = (uint32_t)p->repetition_window;
  bool fresh;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    fresh = p->temperature > 0.f && !(c->smp_temp[slot] > 0.f);
    c->n_sampling += (p->temperature > 0.f) - (c->smp_temp[slot] > 0.f);
    c->smp_temp[slot] = p->temperature;
  }
  launch_set_sampling(c->st, slot, p->temperature, p->top_k, p->seed, ex, fresh, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

int lvx_stream_sampling(lvx_ctx* c, int slot, float temperature, int top_k, uint64_t seed, void* stream) {
  const lvx_sampling p{temperature, top_k, 1.f, 0.f, 1.f, 64, seed};
  return lvx_stream_sampling_ex(c, slot, &p, stream);
}

int lvx_stream_history(lvx_ctx* c, int slot, int pos0, int n, int32_t* tokens, int write, void* stream) {
  NEED_FINAL(c);
  if (slot < 0 || slot >= c->cfg.max_streams) return fail(LVX_E_ARG, "slot out of range");
  if (!tokens) return fail(LVX_E_ARG, "null tokens");
  if (pos0 < 0 || n < 1 || (long long)pos0 + n > (long long)c->cfg.max_positions)
    return fail(LVX_E_CAPACITY, "entries outside the slot's history");
  HIP_TRY(hipSetDevice(c->cfg.device));
  launch_history(c->st, slot, pos0, n, tokens, write != 0, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

int lvx_sample_kept(lvx_ctx* c, int B, int32_t* dst, void* stream) {
  NEED_FINAL(c);
  if (B < 1 || B > c->cfg.max_streams || !dst) return fail(LVX_E_ARG, "bad B/dst");
  HIP_TRY(hipSetDevice(c->cfg.device));
  HIP_TRY(hipMemcpyAsync(dst, c->st.smp_kept(), (size_t)B * 16, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return LVX_OK;
}

int lvx_stream_position(lvx_ctx* c, int slot, int* pos_out, void* stream) {
  NEED_FINAL(c);
  if (slot < 0 || slot >= c->cfg.max_streams || !pos_out) return fail(LVX_E_ARG, "bad slot/pos_out");
  HIP_TRY(hipSetDevice(c->cfg.device));
  int32_t v[2];
  launch_err_take(c->st.err, 1, 0, c->st.err + 3, (hipStream_t)stream);  // the capacity bit only
  HIP_TRY(hipMemcpyAsync(&v[0], c->st.pos + slot, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipMemcpyAsync(&v[1], c->st.err + 3, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  *pos_out = v[0];
  return bits_status(v[1]);
}

int lvx_set_option(lvx_ctx* c, const char* name, int value) {
  if (!c || !name) return fail(LVX_E_ARG, "null argument");
  std::string n(name);
  std::lock_guard<std::mutex> lk(c->mu);
  Opts& o = c->opts;  // this context only (round 4: the switches were process-wide globals)
  if (n == "defer_select") o.defer_select = value;
  else if (n == "fuse_mlp") o.fuse_mlp = value != 0;
  else if (n == "bt") o.bt = std::min(std::max(value, 0), 2);
  else if (n == "codec_g2") o.codec_g2 = value != 0;
  else if (n == "codec_skinny") o.codec_skinny = value != 0;
  else if (n == "codec_g3") o.codec_g3 = value != 0;
  else if (n == "codec_g3f") o.codec_g3f = value == 1 ? 1 : 2;  // 1: the exact-fp32 kernel (a test oracle)
  else if (n == "codec_exp") o.codec_exp = value;
  else if (n == "exp") o.exp = value;
  else if (n == "f32b") o.f32b = value != 0;
  else if (n == "ln_max") o.ln_max = std::min(std::max(value, 2), 8);
  else if (n == "l0q") o.l0q = value != 0;
  else if (n == "l0a") o.l0a = value != 0;
  else if (n == "laf") o.laf = value != 0;
  else if (n == "xfold") o.xfold = value != 0;
  else if (n == "lmf") o.lmf = value != 0;
  else if (n == "fmt_group") o.fmt_group = std::min(std::max(value, 0), 32);
  else return fail(LVX_E_NAME, "unknown option " + n);
  ++c->opt_epoch;  // this context's captured kernels change (checked in cached_graph)
  return LVX_OK;
}

int lvx_set_capture_stream(lvx_ctx* c, void* stream) {
  if (!c) return fail(LVX_E_ARG, "null ctx");
  std::lock_guard<std::mutex> lk(c->mu);
  c->capture_stream = (hipStream_t)stream;
  return LVX_OK;
}

int lvx_set_graphs(lvx_ctx* c, int enable) {
  if (!c) return fail(LVX_E_ARG, "null ctx");
  c->use_graphs = enable != 0;
  return LVX_OK;
}

int lvx_ar_forward_row(lvx_ctx* c, int slot, int pos, const float* emb_row, float* logits, void* stream) {
  NEED_FINAL(c);
  if (slot < 0 || slot >= c->cfg.max_streams) return fail(LVX_E_ARG, "slot out of range");
  if (pos < 0 || pos >= BLOCK_SIZE)
    return fail(LVX_E_CAPACITY, "Cannot forward sequence of length " + std::to_string(pos + 1) +
                                    ", block size is only " + std::to_string(BLOCK_SIZE));
  if (pos >= c->cfg.max_positions)
    return fail(LVX_E_CAPACITY, "position " + std::to_string(pos) + " exceeds the KV capacity " +
                                    std::to_string(c->cfg.max_positions));
  if (!emb_row || !logits) return fail(LVX_E_ARG, "null emb_row/logits");
  HIP_TRY(hipSetDevice(c->cfg.device));
  const Opts o = c->opts_snapshot();
  OptScope os(&o);
  ar_launch_step(c->arw, c->st, ar_plan_step(o, c->cfg.weight_dtype, c->cfg.kv_dtype, 1, true, false), emb_row, slot,
                 pos, logits, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

// Capture `launch(stream)` into a graph cached under `key` (instantiated once), then replay it on the
// caller's stream. The capture runs on the caller's stream unless lvx_set_capture_stream named another:
// torch's synchronous collectives record their completion events on the current stream, a process
// group's watchdog thread queries them, and HIP refuses a query of an event last recorded in a stream
// that is capturing (round 6: a configs[4] line with the one-rank RCCL group aborted mid-capture). The
// Python engine therefore hands over a pooled stream once an RCCL group exists; without one it keeps
// the caller's, since one more stream per process cost the two-ranks-on-one-GPU configs[3] rehearsal
// 6.5x (22.4k -> 3.4k tokens/s, profiles/r06/capture_stream_ab.txt) while a single rank per GPU saw no
// difference. (The legacy null stream cannot be captured: lvx_ar_step* null-stream callers launch the
// steps one by one; lvx_probe_kernel's capture on a stream the context creates.)
// Caller holds c->mu.
static int cached_graph(lvx_ctx* c, const GraphKey& key, hipStream_t s,
                        const std::function<void(hipStream_t)>& launch, hipGraphExec_t* out) {
  const unsigned epoch = c->opt_epoch;  // (caller holds c->mu)
  if (c->graph_epoch != epoch) {  // an option changed since these graphs were captured
    for (auto& kv : c->graphs) (void)hipGraphExecDestroy(kv.second);
    c->graphs.clear();
    c->graph_epoch = epoch;
  }
  auto it = c->graphs.find(key);
  if (it == c->graphs.end()) {
    hipStream_t cs = c->capture_stream ? c->capture_stream : s;
    if (!cs) {  // the legacy null stream cannot be captured (lvx_probe_kernel's null-stream callers)
      if (!c->own_capture_stream) HIP_TRY(hipStreamCreateWithFlags(&c->own_capture_stream, hipStreamNonBlocking));
      cs = c->own_capture_stream;
    }
    hipGraph_t g;
    HIP_TRY(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    launch(cs);
    hipError_t le = hipGetLastError();
    HIP_TRY(hipStreamEndCapture(cs, &g));
    if (le != hipSuccess) return fail(LVX_E_HIP, std::string("capture: ") + hipGetErrorString(le));
    hipGraphExec_t ex;
    HIP_TRY(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    c->graph_defs.push_back(g);
    it = c->graphs.emplace(key, ex).first;
  }
  *out = it->second;
  return 0;
}

static int ar_step_impl(lvx_ctx* c, int n_steps, int B, const int32_t* slots, const int32_t* text_plan,
                        int plan_stride, int32_t* rowstep, int32_t* tok_plan, float* margin_plan, void* stream) {
  NEED_FINAL(c);
  if (B < 1 || B > c->cfg.max_streams) return fail(LVX_E_ARG, "B out of range [1, max_streams]");
  if (plan_stride < 1) return fail(LVX_E_ARG, "plan_stride must be >= 1");
  if (n_steps < 0) return fail(LVX_E_ARG, "n_steps must be >= 0");
  if (!slots || !text_plan || !rowstep || !tok_plan) return fail(LVX_E_ARG, "null slots/text_plan/rowstep/tok_plan");
  if (n_steps == 0) return LVX_OK;
  HIP_TRY(hipSetDevice(c->cfg.device));
  ArState st = c->st;
  st.slots = const_cast<int32_t*>(slots);
  st.text_plan = text_plan;
  st.plan_stride = plan_stride;
  st.rowstep = rowstep;
  st.tok_plan = tok_plan;
  st.margin_plan = margin_plan;
  hipStream_t s = (hipStream_t)stream;
  ar_launch_rowinfo_init(st, B, s);  // per-row control records, then advanced by every step
  // one plan per call: the steps and the commit of the last one cannot disagree
  // (while a slot of the context samples: the sampled select, whatever slots this call drives)
  auto plan = [&](const Opts& o, bool sample) {
    return ar_plan_step(o, c->cfg.weight_dtype, c->cfg.kv_dtype, B, false, c->arw.q0_text != nullptr, sample);
  };
  // null-stream callers (torch's default stream) launch the steps one by one: replaying the same
  // steps as graphs on a stream of their own measured no faster (round 1)
  if (!c->use_graphs || s == nullptr) {
    const Opts o = c->opts_snapshot();
    OptScope os(&o);
    const ArStepPlan p = plan(o, c->sampling_snapshot());
    for (int i = 0; i < n_steps; ++i) ar_launch_step(c->arw, st, p, nullptr, 0, 0, nullptr, s);
    ar_launch_steps_end(st, p, s);
    HIP_TRY(hipGetLastError());
    return LVX_OK;
  }
  std::lock_guard<std::mutex> lk(c->mu);
  const Opts o = c->opts;  // the options the cached graphs were captured under (epoch checked under mu)
  OptScope os(&o);
  const bool sample = c->n_sampling > 0;
  const ArStepPlan p = plan(o, sample);
  // graphs of kGraphSteps consecutive steps (one replay per kGraphSteps tokens) + 1-step graph
  auto get_graph = [&](int nst, hipGraphExec_t* out) -> int {
    GraphKey key{B, plan_stride, nst, slots, text_plan, rowstep, tok_plan, margin_plan, stream, sample};
    return cached_graph(c, key, s, [&](hipStream_t cs) {
      for (int i = 0; i < nst; ++i) ar_launch_step(c->arw, st, p, nullptr, 0, 0, nullptr, cs);
    }, out);
  };
  int left = n_steps;
  if (left >= kGraphSteps) {
    hipGraphExec_t gx;
    if (int r = get_graph(kGraphSteps, &gx)) return r;
    for (; left >= kGraphSteps; left -= kGraphSteps) HIP_TRY(hipGraphLaunch(gx, s));
  }
  if (left > 0) {
    hipGraphExec_t g1;
    if (int r = get_graph(1, &g1)) return r;
    for (; left > 0; --left) HIP_TRY(hipGraphLaunch(g1, s));
  }
  ar_launch_steps_end(st, p, s);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

int lvx_ar_step(lvx_ctx* c, int B, const int32_t* slots, const int32_t* text_plan, int plan_stride,
                int32_t* rowstep, int32_t* tok_plan, float* margin_plan, void* stream) {
  return ar_step_impl(c, 1, B, slots, text_plan, plan_stride, rowstep, tok_plan, margin_plan, stream);
}

int lvx_ar_steps(lvx_ctx* c, int n_steps, int B, const int32_t* slots, const int32_t* text_plan, int plan_stride,
                 int32_t* rowstep, int32_t* tok_plan, float* margin_plan, void* stream) {
  return ar_step_impl(c, n_steps, B, slots, text_plan, plan_stride, rowstep, tok_plan, margin_plan, stream);
}

int lvx_ar_logits(lvx_ctx* c, int B, float* dst, void* stream) {
  NEED_FINAL(c);
  if (B < 1 || B > c->cfg.max_streams || !dst) return fail(LVX_E_ARG, "bad B/dst");
  HIP_TRY(hipSetDevice(c->cfg.device));
  HIP_TRY(hipMemcpyAsync(dst, c->st.logits, (size_t)B * VOCAB * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return LVX_OK;
}

int lvx_check_errors(lvx_ctx* c, void* stream) {
  NEED_FINAL(c);
  HIP_TRY(hipSetDevice(c->cfg.device));
  int32_t v = 0;
  // both words taken atomically in stream order: a bit that a codec call in flight on another stream
  // sets afterwards stays in its word for the next check (round 4 cleared the word with a memset)
  launch_err_take(c->st.err, -1, -1, c->st.err + 2, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(&v, c->st.err + 2, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return bits_status(v);
}

int lvx_error_take(lvx_ctx* c, int which, int32_t* bits_dev, void* stream) {
  NEED_FINAL(c);
  if (!bits_dev || which < 1 || which > 3) return fail(LVX_E_ARG, "which must be LVX_ERRW_AR | LVX_ERRW_CODEC, bits_dev non-null");
  HIP_TRY(hipSetDevice(c->cfg.device));
  launch_err_take(c->st.err, (which & LVX_ERRW_AR) ? -1 : 0, (which & LVX_ERRW_CODEC) ? -1 : 0, bits_dev,
                  (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

int lvx_error_status(int bits) { return bits_status(bits); }

int lvx_probe_kernel(lvx_ctx* c, int which, int B, const int32_t* slots, int iters, void* stream) {
  NEED_FINAL(c);
  if (B < 1 || B > c->cfg.max_streams || !slots || iters < 1) return fail(LVX_E_ARG, "bad probe arguments");
  HIP_TRY(hipSetDevice(c->cfg.device));
  ArState st = c->st;  // no plan bound: text_plan / rowstep / tok_plan stay null
  st.slots = const_cast<int32_t*>(slots);
  hipStream_t s = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(c->mu);
  const Opts o = c->opts;
  OptScope os(&o);
  // a dry run (no launches) validates the op id / fused case before anything is captured
  const int pr = ar_probe(c->arw, st, c->cfg.weight_dtype, c->cfg.kv_dtype, B, which, 0, s);
  if (pr < 0) return fail(LVX_E_ARG, "unknown probe kernel id");
  if (pr > 0) return fail(LVX_E_STATE, "this op has no kernel of its own at this batch size (fused into the previous op)");
  if (!c->use_graphs) {
    ar_probe(c->arw, st, c->cfg.weight_dtype, c->cfg.kv_dtype, B, which, iters, s);
    HIP_TRY(hipGetLastError());
    return LVX_OK;
  }
  // the `iters` launches are replayed as one graph, as the decode step is: launched one by one
  // from the host, back-to-back kernels of 3-5 us measured the host's launch rate as much as
  // the kernel (the first call of a (op, B, slots, iters) captures; time the second)
  GraphKey key{B, -1 - which, iters, slots, nullptr, nullptr, nullptr, nullptr, stream};
  hipGraphExec_t gx;
  if (int r = cached_graph(c, key, s, [&](hipStream_t cs) {
        ar_probe(c->arw, st, c->cfg.weight_dtype, c->cfg.kv_dtype, B, which, iters, cs);
      }, &gx))
    return r;
  HIP_TRY(hipGraphLaunch(gx, s));
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

int lvx_select_probe(lvx_ctx* c, int path, int B, const int32_t* slots, const float* logits,
                     const int32_t* text_plan, int plan_stride, int32_t* rowstep, int32_t* tok_plan,
                     float* margin_plan, void* stream) {
  NEED_FINAL(c);
  if (B < 1 || B > c->cfg.max_streams || (path == 1 && B > 4) || (path == 3 && B > 8))
    return fail(LVX_E_ARG, "B out of range for this path");
  if (path < 0 || path > 4) return fail(LVX_E_ARG, "path must be 0, 1, 2, 3 or 4");
  if (!slots || !logits || !text_plan || !rowstep || !tok_plan || plan_stride < 2)
    return fail(LVX_E_ARG, "null argument or plan_stride < 2");
  HIP_TRY(hipSetDevice(c->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  ArState st = c->st;
  st.slots = const_cast<int32_t*>(slots);
  st.text_plan = text_plan;
  st.plan_stride = plan_stride;
  st.rowstep = rowstep;
  st.tok_plan = tok_plan;
  st.margin_plan = margin_plan;
  HIP_TRY(hipMemcpyAsync(st.logits, logits, (size_t)B * VOCAB * 4, hipMemcpyDeviceToDevice, s));
  const Opts o = c->opts_snapshot();
  OptScope os(&o);
  ar_select_probe(c->arw, st, B, path, s);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

static int kv_hook_check(lvx_ctx* c, int slot, int layer, int pos0, int n) {
  if (slot < 0 || slot >= c->cfg.max_streams) return fail(LVX_E_ARG, "slot out of range");
  if (layer < 0 || layer >= N_LAYER) return fail(LVX_E_ARG, "layer out of range");
  if (pos0 < 0 || n < 1 || (long long)pos0 + n > (long long)c->st.kv_chunks * KV_CHUNK)
    return fail(LVX_E_CAPACITY, "rows outside the slot's allocated KV rows");
  return 0;
}

static int kv_write(lvx_ctx* c, int slot, int layer, int pos0, int n, const void* k, const void* v, bool raw, void* stream) {
  NEED_FINAL(c);
  if (int r = kv_hook_check(c, slot, layer, pos0, n)) return r;
  if (!k && !v) return fail(LVX_E_ARG, "null k and v");
  HIP_TRY(hipSetDevice(c->cfg.device));
  ar_launch_kv_write(c->st, c->cfg.kv_dtype, slot, layer, pos0, n, (const float*)k, (const float*)v, raw, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

int lvx_kv_write(lvx_ctx* c, int slot, int layer, int pos0, int n, const float* k, const float* v, void* stream) {
  return kv_write(c, slot, layer, pos0, n, k, v, false, stream);
}

int lvx_kv_write_raw(lvx_ctx* c, int slot, int layer, int pos0, int n, const uint32_t* k, const uint32_t* v, void* stream) {
  return kv_write(c, slot, layer, pos0, n, k, v, true, stream);
}

int lvx_kv_read(lvx_ctx* c, int slot, int layer, int pos0, int n, float* k, float* v, void* stream) {
  NEED_FINAL(c);
  if (int r = kv_hook_check(c, slot, layer, pos0, n)) return r;
  if (!k && !v) return fail(LVX_E_ARG, "null k and v");
  HIP_TRY(hipSetDevice(c->cfg.device));
  ar_launch_kv_read(c->st, c->cfg.kv_dtype, slot, layer, pos0, n, k, v, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

int lvx_attn_probe(lvx_ctx* c, int B, const int32_t* slots, int layer, const float* q, float* out, float* part_o,
                   float* part_ml, int* form_out, void* stream) {
  NEED_FINAL(c);
  if (B < 1 || B > c->cfg.max_streams) return fail(LVX_E_ARG, "B out of range");
  if (layer < 0 || layer >= N_LAYER) return fail(LVX_E_ARG, "layer out of range");
  if (!slots || !q || !out || !part_o || !part_ml || !form_out) return fail(LVX_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(c->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  ArState st = c->st;  // no plan bound: text_plan / rowstep / tok_plan stay null
  st.slots = const_cast<int32_t*>(slots);
  const Opts o = c->opts_snapshot();
  OptScope os(&o);
  HIP_TRY(hipMemcpyAsync(st.q, q, (size_t)B * D * 4, hipMemcpyDeviceToDevice, s));
  // launched kernel by kernel, never captured into a graph
  if (ar_attn_probe(c->arw, st, c->cfg.weight_dtype, c->cfg.kv_dtype, B, layer, out, form_out, s))
    return fail(LVX_E_STATE, "the plan's attention at this B takes its q from the K-split c_attn (fp32: set option exp 1024)");
  HIP_TRY(hipGetLastError());
  if (form_out[0] == 1) {  // merged in c_proj's prologue: the partials as the kernel left them
    HIP_TRY(hipMemcpyAsync(part_o, st.part_o, (size_t)B * N_HEAD * NSPLIT * HD * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(part_ml, st.part_ml, (size_t)B * N_HEAD * NSPLIT * 2 * 4, hipMemcpyDeviceToDevice, s));
  }
  return LVX_OK;
}

int lvx_ar_ops(lvx_ctx* c, int B, const int32_t* slots, int first, int last, const float* x_in, const float* q_in,
               const int32_t* text_ids, int poison, float* out, float* copies, int64_t* copies_fx, float* part_o,
               float* part_ml, int* info, void* stream) {
  NEED_FINAL(c);
  if (B < 1 || B > c->cfg.max_streams) return fail(LVX_E_ARG, "B out of range");
  if (first < 0 || last < first || last >= LVX_AR_OPS) return fail(LVX_E_ARG, "need 0 <= first <= last < LVX_AR_OPS");
  const bool at_attn = first < 5 * N_LAYER && first % 5 == 1;
  if (first % 5 != 0 && !at_attn) return fail(LVX_E_ARG, "a window starts at a layer boundary (5 l) or at an attention (5 l + 1)");
  if (!slots || !out || !copies || !copies_fx || !part_o || !part_ml || !info) return fail(LVX_E_ARG, "null argument");
  if (first == 0 ? !text_ids : !x_in) return fail(LVX_E_ARG, "layer 0 takes text ids, every other entry x_in");
  if (at_attn && !q_in) return fail(LVX_E_ARG, "an entry at the attention takes q_in");
  HIP_TRY(hipSetDevice(c->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  ArState st = c->st;  // no plan bound but the rows' text ids: rowstep / tok_plan stay null
  st.slots = const_cast<int32_t*>(slots);
  st.text_plan = first == 0 ? text_ids : nullptr;
  st.plan_stride = 1;
  const Opts o = c->opts_snapshot();
  OptScope os(&o);
  // launched kernel by kernel, never captured into a graph
  const int r = ar_ops(c->arw, st, c->cfg.weight_dtype, c->cfg.kv_dtype, B, first, last, x_in, q_in, poison != 0, out,
                       copies, reinterpret_cast<long long*>(copies_fx), info, s);
  if (r == 1) return fail(LVX_E_STATE, "the plan's attention at this B takes its q from the K-split c_attn (fp32: set option exp 1024)");
  if (r == 2) return fail(LVX_E_STATE, "c_fc has no kernel of its own at this B (fused MLP): end the window at mlp c_proj");
  HIP_TRY(hipGetLastError());
  if (info[0] == LVX_AR_OUT_ATTN_PARTS) {  // merged in c_proj's prologue: the partials as the kernel left them
    HIP_TRY(hipMemcpyAsync(part_o, st.part_o, (size_t)B * N_HEAD * NSPLIT * HD * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(part_ml, st.part_ml, (size_t)B * N_HEAD * NSPLIT * 2 * 4, hipMemcpyDeviceToDevice, s));
  }
  return LVX_OK;
}

static int codec_check(lvx_ctx* c, int B, int L, int bw) {
  if (B < 1 || L < 1) return fail(LVX_E_ARG, "B and L must be >= 1");
  if ((long long)B * L > c->cfg.max_codec_frames)
    return fail(LVX_E_CAPACITY, "B*L = " + std::to_string((long long)B * L) + " exceeds max_codec_frames " +
                                    std::to_string(c->cfg.max_codec_frames));
  if (L > kMaxCodecL) return fail(LVX_E_CAPACITY, "L exceeds the codec's max frames per stream (4096)");
  if (bw < 0 || bw > 3) return fail(LVX_E_ARG, "bandwidth_id out of range [0,3]");
  return 0;
}

int lvx_codec_decode_features(lvx_ctx* c, const float* feats, int B, int L, int bw, float* pcm, void* stream) {
  NEED_FINAL(c);
  if (int r = codec_check(c, B, L, bw)) return r;
  if (!feats || !pcm) return fail(LVX_E_ARG, "null feats/pcm");
  HIP_TRY(hipSetDevice(c->cfg.device));
  const Opts o = c->opts_snapshot();
  OptScope os(&o);
  codec_launch_decode(c->cw, c->cs, c->cfg.weight_dtype, feats, nullptr, B, L, bw, pcm, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

int lvx_codec_decode_codes(lvx_ctx* c, const int32_t* codes, int B, int L, int bw, float* pcm, void* stream) {
  NEED_FINAL(c);
  if (int r = codec_check(c, B, L, bw)) return r;
  if (!codes || !pcm) return fail(LVX_E_ARG, "null codes/pcm");
  HIP_TRY(hipSetDevice(c->cfg.device));
  const Opts o = c->opts_snapshot();
  OptScope os(&o);
  codec_launch_decode(c->cw, c->cs, c->cfg.weight_dtype, nullptr, codes, B, L, bw, pcm, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

int lvx_codec_stages(lvx_ctx* c, int first, int last, const void* in, int B, int L, int bw, float* out,
                     lvx_codec_route* routes, int route_cap, int* n_routes, void* stream) {
  NEED_FINAL(c);
  if (int r = codec_check(c, B, L, bw)) return r;
  if (first < 0 || last >= LVX_CODEC_STAGES || first > last)
    return fail(LVX_E_ARG, "stage window must satisfy 0 <= first <= last < " + std::to_string(LVX_CODEC_STAGES));
  if (!in || !out) return fail(LVX_E_ARG, "null in/out");
  if (route_cap < 0 || (route_cap > 0 && !routes)) return fail(LVX_E_ARG, "route_cap without routes_out");
  HIP_TRY(hipSetDevice(c->cfg.device));
  const Opts o = c->opts_snapshot();
  OptScope os(&o);
  // launched kernel by kernel, never captured into a graph
  const int n = codec_launch_stages(c->cw, c->cs, c->cfg.weight_dtype, first, last, in, B, L, bw, out, routes,
                                    route_cap, (hipStream_t)stream);
  if (n_routes) *n_routes = n;
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

// ---- PCM output stage ----
int lvx_pcm_filter(int sample_rate, int* L, int* M, int* N, float* taps_host, int cap) {
  const PcmRate* pr = pcm_rate_of(sample_rate);
  if (!pr) return fail(LVX_E_ARG, "unsupported sample rate " + std::to_string(sample_rate) + " (24000, 16000, 8000, 48000)");
  if (L) *L = pr->L;
  if (M) *M = pr->M;
  if (N) *N = pr->N;
  if (taps_host) {
    if (cap < 2 * pr->N + 1) return fail(LVX_E_ARG, "taps_host holds fewer than 2 N + 1 floats");
    const std::vector<float> h = pcm_design(*pr);
    std::memcpy(taps_host, h.data(), h.size() * 4);
  }
  return LVX_OK;
}

int lvx_pcm_emitted(int sample_rate, long long t0, int n_in, int final) {
  const PcmRate* pr = pcm_rate_of(sample_rate);
  if (!pr) return fail(LVX_E_ARG, "unsupported sample rate " + std::to_string(sample_rate));
  if (t0 < 0 || n_in < 0) return fail(LVX_E_ARG, "t0 and n_in must be >= 0");
  return (int)(pcm_emitted_upto(*pr, t0 + n_in, final != 0) - pcm_emitted_upto(*pr, t0, false));
}

int lvx_pcm_reset(lvx_ctx* c, int slot, void* stream) {
  NEED_FINAL(c);
  if (slot < 0 || slot >= c->cfg.max_streams) return fail(LVX_E_ARG, "slot out of range");
  // the position travels to the kernel as an argument and inputs before it read as zero: forgetting it
  // here orders the reset behind every call already issued for the slot, on whatever stream
  (void)stream;
  std::lock_guard<std::mutex> lk(c->mu);
  for (auto& v : c->seg) v[slot].close();
  return LVX_OK;
}

int lvx_pcm_convert(lvx_ctx* c, const float* pcm, int B, int n_in, const int32_t* slots, const uint8_t* final_host,
                    int sample_rate, int encoding, void* out, long long out_stride, int32_t* n_out_host, void* stream) {
  NEED_FINAL(c);
  const PcmRate* pr = pcm_rate_of(sample_rate);
  if (!pr) return fail(LVX_E_ARG, "unsupported sample rate " + std::to_string(sample_rate) + " (24000, 16000, 8000, 48000)");
  const int bps = pcm_sample_bytes(encoding);
  if (!bps) return fail(LVX_E_ARG, "encoding must be LVX_PCM_F32LE, LVX_PCM_S16LE, LVX_PCM_ULAW or LVX_PCM_ALAW");
  const bool launch = !(pr->N == 0 && encoding == LVX_PCM_F32LE);  // 24000 Hz f32le: the rows are the output
  if (int r = pcm_args(B, n_in, pcm, slots && final_host && n_out_host ? slots : nullptr, launch, out, out_stride)) return r;
  std::vector<PcmRow> rows;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    // (the one stage whose identity call advances the segment: the mirror of a 24 kHz f32le stream counts too)
    const std::string e = pcm_plan(
        c->seg[lvx_ctx::SEG_CONVERT], PCM_HIST, B, n_in, slots, final_host, n_out_host, sample_rate, true,
        [](long long k) { return std::to_string(k) + " Hz"; }, rows,
        [&](const PcmCall& q, PcmRow& r) { return plan_convert(q, n_in, *pr, bps, launch, out_stride, r); });
    if (!e.empty()) return fail(LVX_E_ARG, e);
  }
  if (!launch) return LVX_OK;
  return pcm_launches<PcmRows>(c, rows, [&](const PcmRows& pk, int nr, int max_out) {
    pcm_launch_convert(sample_rate, encoding, pk, nr, max_out, pcm, n_in, c->pcm_taps + pr->tap_off, c->pcm_hist, out, out_stride,
                       (hipStream_t)stream);
  });
}

// ---- PCM G.711 (host only) ----
int lvx_pcm_g711_encode(int encoding, const int16_t* in, long long n, uint8_t* out) {
  if (g711_encode(encoding, in, n, out)) return fail(LVX_E_ARG, "encoding must be LVX_PCM_ULAW or LVX_PCM_ALAW, n >= 0, in / out not null");
  return LVX_OK;
}

int lvx_pcm_g711_decode(int encoding, const uint8_t* in, long long n, int16_t* out) {
  if (g711_decode(encoding, in, n, out)) return fail(LVX_E_ARG, "encoding must be LVX_PCM_ULAW or LVX_PCM_ALAW, n >= 0, in / out not null");
  return LVX_OK;
}

// ---- PCM time stretch ----
int lvx_pcm_stretch_window(float* wr_host, float* wf_host, int cap) {
  if (!wr_host || !wf_host) return fail(LVX_E_ARG, "null wr_host / wf_host");
  if (cap < STR_H) return fail(LVX_E_ARG, "wr_host / wf_host hold fewer than 240 floats");
  stretch_design(wr_host, wf_host);
  return LVX_OK;
}

int lvx_pcm_stretch_emitted(int speed_pct, long long t0, int n_in, int final) {
  if (speed_pct < 50 || speed_pct > 200) return fail(LVX_E_ARG, "speed_pct must be in [50, 200]");
  if (t0 < 0 || n_in < 0) return fail(LVX_E_ARG, "t0 and n_in must be >= 0");
  return (int)(stretch_emitted_upto(speed_pct, t0 + n_in, final != 0) - stretch_emitted_upto(speed_pct, t0, false));
}

int lvx_pcm_stretch(lvx_ctx* c, const float* pcm, int B, int n_in, const int32_t* slots, const uint8_t* final_host,
                    int speed_pct, float* out, long long out_stride, int32_t* n_out_host, int32_t* d_out, int d_stride,
                    void* stream) {
  NEED_FINAL(c);
  if (speed_pct < 50 || speed_pct > 200) return fail(LVX_E_ARG, "speed_pct must be in [50, 200], got " + std::to_string(speed_pct));
  const bool launch = speed_pct != 100;  // 100: the rows of pcm_dev are the output
  if (int r = pcm_args(B, n_in, pcm, slots && final_host && n_out_host ? slots : nullptr, launch, out, out_stride)) return r;
  if (launch && d_out && ((reinterpret_cast<uintptr_t>(d_out) & 3) || d_stride < 0))
    return fail(LVX_E_ARG, "d_out_dev must be a multiple of 4 and d_stride >= 0");
  std::vector<StretchRow> rows;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    const std::string e = pcm_plan(
        c->seg[lvx_ctx::SEG_STRETCH], STR_HIST, B, n_in, slots, final_host, n_out_host, speed_pct, launch,
        [](long long k) { return "speed_pct " + std::to_string(k); }, rows,
        [&](const PcmCall& q, StretchRow& r) { return plan_stretch(q, n_in, speed_pct, out_stride, d_out != nullptr, d_stride, r); });
    if (!e.empty()) return fail(LVX_E_ARG, e);
  }
  if (!launch) return LVX_OK;
  return pcm_launches<StretchRows>(c, rows, [&](const StretchRows& pk, int nr, int) {
    pcm_launch_stretch(pk, nr, speed_pct, pcm, n_in, c->str_win, c->str_hist, c->str_d, out, out_stride, d_out, d_stride,
                       (hipStream_t)stream);
  });
}

// ---- PCM pitch shift ----
int lvx_pcm_pitch_plan(int speed_pct, int pitch_pct, int* stretch_pct, int* L, int* M) {
  if (speed_pct < 50 || speed_pct > 200) return fail(LVX_E_ARG, "speed_pct must be in [50, 200], got " + std::to_string(speed_pct));
  if (pitch_pct < 50 || pitch_pct > 200) return fail(LVX_E_ARG, "pitch_pct must be in [50, 200], got " + std::to_string(pitch_pct));
  const int st = (200 * speed_pct + pitch_pct) / (2 * pitch_pct);  // speed 100 / pitch, rounded half up
  if (st < 50 || st > 200)
    return fail(LVX_E_ARG, "speed_pct " + std::to_string(speed_pct) + " with pitch_pct " + std::to_string(pitch_pct) +
                               " needs a time stretch of " + std::to_string(st) + " percent, outside [50, 200]");
  const int g = gcd_of(st, speed_pct);
  if (stretch_pct) *stretch_pct = st;
  if (L) *L = st / g;
  if (M) *M = speed_pct / g;
  return LVX_OK;
}

int lvx_pcm_ratio_filter(int L, int M, int* N, float* taps_host, int cap) {
  if (!ratio_ok(L, M)) return fail(LVX_E_ARG, ratio_msg(L, M));
  const int n = ratio_N(L, M);
  if (N) *N = n;
  if (taps_host) {
    if (cap < 2 * n + 1) return fail(LVX_E_ARG, "taps_host holds fewer than 2 N + 1 floats");
    const std::vector<float> h = pcm_design(L, M, n);
    std::memcpy(taps_host, h.data(), h.size() * 4);
  }
  return LVX_OK;
}

int lvx_pcm_ratio_emitted(int L, int M, long long t0, int n_in, int final) {
  if (!ratio_ok(L, M)) return fail(LVX_E_ARG, ratio_msg(L, M));
  if (t0 < 0 || n_in < 0) return fail(LVX_E_ARG, "t0 and n_in must be >= 0");
  const int N = ratio_N(L, M);
  return (int)(pcm_emitted_upto(L, M, N, t0 + n_in, final != 0) - pcm_emitted_upto(L, M, N, t0, false));
}

int lvx_pcm_ratio(lvx_ctx* c, const float* pcm, int B, int n_in, const int32_t* slots, const uint8_t* final_host,
                  int L, int M, float* out, long long out_stride, int32_t* n_out_host, void* stream) {
  NEED_FINAL(c);
  if (!ratio_ok(L, M)) return fail(LVX_E_ARG, ratio_msg(L, M));
  const int N = ratio_N(L, M);
  const bool launch = N != 0;  // 1 / 1: the rows of pcm_dev are the output
  if (int r = pcm_args(B, n_in, pcm, slots && final_host && n_out_host ? slots : nullptr, launch, out, out_stride)) return r;
  const std::pair<int, int> lm{L, M};
  std::vector<RatioRow> rows;
  std::vector<int> upload;  // slots whose table region gets this ratio's table
  const std::vector<float>* table = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->mu);  // (the host cache too)
    const std::string e = pcm_plan(
        c->seg[lvx_ctx::SEG_RATIO], RAT_HIST, B, n_in, slots, final_host, n_out_host, ratio_key(L, M), launch,
        [](long long k) { return "the ratio " + std::to_string(k >> 16) + " / " + std::to_string(k & 0xffff); }, rows,
        [&](const PcmCall& q, RatioRow& r) { return plan_ratio(q, n_in, L, M, out_stride, r); });
    if (!e.empty()) return fail(LVX_E_ARG, e);
    for (int b = 0; launch && b < B; ++b)
      if (rows[b].n_out > 0 && c->rat_tab[slots[b]] != lm) {
        c->rat_tab[slots[b]] = lm;
        upload.push_back(slots[b]);
      }
    if (!upload.empty()) {  // designed once per ratio; an entry stays (and stays where it is) for the context's life
      auto it = c->rat_cache.find(lm);
      if (it == c->rat_cache.end()) it = c->rat_cache.emplace(lm, pcm_design(L, M, N)).first;
      table = &it->second;
    }
  }
  if (!launch) return LVX_OK;
  HIP_TRY(hipSetDevice(c->cfg.device));
  // stream-ordered: behind the slot's earlier launches (which read the table of its last segment) and
  // before this call's
  for (int s : upload)
    HIP_TRY(hipMemcpyAsync(c->rat_taps + (size_t)s * RAT_TAPS_STRIDE, table->data(), table->size() * 4, hipMemcpyHostToDevice,
                           (hipStream_t)stream));
  return pcm_launches<RatioRows>(c, rows, [&](const RatioRows& pk, int nr, int max_out) {
    pcm_launch_ratio(pk, nr, max_out, L, M, N, pcm, n_in, c->rat_taps, c->rat_hist, out, out_stride, (hipStream_t)stream);
  });
}

// ---- PCM dump join ----
int lvx_pcm_join_window(float* wr_host, float* wf_host, int cap) {
  if (!wr_host || !wf_host) return fail(LVX_E_ARG, "null wr_host / wf_host");
  if (cap < JOIN_HOLD) return fail(LVX_E_ARG, "wr_host / wf_host hold fewer than 320 floats");
  join_design(wr_host, wf_host);
  return LVX_OK;
}

int lvx_pcm_join_emitted(int open, int ctx_frames, int n_in, int final) {
  const int n = join_emitted(open != 0, ctx_frames, n_in, final != 0);
  if (n < 0) return fail(LVX_E_ARG, join_msg(open != 0, ctx_frames, n_in, final != 0));
  return n;
}

int lvx_pcm_join(lvx_ctx* c, const float* pcm, int B, int n_in, const int32_t* slots, const int32_t* ctx_frames,
                 const uint8_t* final_host, float* out, long long out_stride, int32_t* n_out_host, void* stream) {
  NEED_FINAL(c);
  if (int r = pcm_args(B, n_in, pcm, slots && ctx_frames && final_host && n_out_host ? slots : nullptr, true, out, out_stride)) return r;
  std::vector<JoinRow> rows;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    // (no parameter: every call's key is 0, which marks the segment open, and no call is an identity)
    const std::string e = pcm_plan(
        c->seg[lvx_ctx::SEG_JOIN], JOIN_HOLD, B, n_in, slots, final_host, n_out_host, 0, true, [](long long) { return std::string(); },
        rows, [&](const PcmCall& q, JoinRow& r) { return plan_join(q, n_in, ctx_frames[q.row], out_stride, r); });
    if (!e.empty()) return fail(LVX_E_ARG, e);
  }
  return pcm_launches<JoinRows>(c, rows, [&](const JoinRows& pk, int nr, int max_out) {
    pcm_launch_join(pk, nr, max_out, pcm, n_in, c->join_win, c->join_tail, out, out_stride, (hipStream_t)stream);
  });
}

// ---- PCM level ----
int lvx_pcm_level_window(float* w_host, int cap) {
  if (!w_host) return fail(LVX_E_ARG, "null w_host");
  if (cap < LVL_TAPS) return fail(LVX_E_ARG, "w_host holds fewer than 241 floats");
  level_design(w_host);
  return LVX_OK;
}

int lvx_pcm_level_emitted(int volume_pct, long long t0, int n_in, int final) {
  if (volume_pct < 0 || volume_pct > 400) return fail(LVX_E_ARG, "volume_pct must be in [0, 400]");
  if (t0 < 0 || n_in < 0) return fail(LVX_E_ARG, "t0 and n_in must be >= 0");
  return (int)(level_emitted_upto(volume_pct, t0 + n_in, final != 0) - level_emitted_upto(volume_pct, t0, false));
}

int lvx_pcm_level(lvx_ctx* c, const float* pcm, int B, int n_in, const int32_t* slots, const uint8_t* final_host,
                  int volume_pct, float* out, long long out_stride, int32_t* n_out_host, float* g_out, long long g_stride,
                  void* stream) {
  NEED_FINAL(c);
  if (volume_pct < 0 || volume_pct > 400) return fail(LVX_E_ARG, "volume_pct must be in [0, 400], got " + std::to_string(volume_pct));
  const bool launch = volume_pct != 100;  // 100: the rows of pcm_dev are the output
  if (int r = pcm_args(B, n_in, pcm, slots && final_host && n_out_host ? slots : nullptr, launch, out, out_stride)) return r;
  if (launch && g_out && ((reinterpret_cast<uintptr_t>(g_out) & 3) || g_stride < 0 || (g_stride & 3)))
    return fail(LVX_E_ARG, "g_out_dev and g_stride_bytes must be multiples of 4");
  std::vector<PcmRow> rows;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    const std::string e = pcm_plan(
        c->seg[lvx_ctx::SEG_LEVEL], LVL_HIST, B, n_in, slots, final_host, n_out_host, volume_pct, launch,
        [](long long k) { return "volume_pct " + std::to_string(k); }, rows,
        [&](const PcmCall& q, PcmRow& r) { return plan_level(q, n_in, volume_pct, out_stride, g_out != nullptr, g_stride, r); });
    if (!e.empty()) return fail(LVX_E_ARG, e);
  }
  if (!launch) return LVX_OK;
  const float gain = (float)((double)volume_pct / 100.0);
  return pcm_launches<PcmRows>(c, rows, [&](const PcmRows& pk, int nr, int max_out) {
    pcm_launch_level(pk, nr, max_out, gain, pcm, n_in, c->lvl_win, c->lvl_hist, out, out_stride, g_out, g_stride,
                     (hipStream_t)stream);
  });
}

// ---- PCM formant ----
int lvx_pcm_formant_plan(int speed_pct, int pitch_pct, int formant_pct, int* Fn, int* Fd) {
  if (formant_pct < 50 || formant_pct > 200) return fail(LVX_E_ARG, "formant_pct must be in [50, 200], got " + std::to_string(formant_pct));
  if (int r = lvx_pcm_pitch_plan(speed_pct, pitch_pct, nullptr, nullptr, nullptr)) return r;
  int n = 0, d = 0;
  if (!formant_plan(speed_pct, pitch_pct, formant_pct, &n, &d))
    return fail(LVX_E_ARG, "speed_pct " + std::to_string(speed_pct) + ", pitch_pct " + std::to_string(pitch_pct) + " and formant_pct " +
                               std::to_string(formant_pct) + " need an envelope correction outside 1/2 .. 2");
  if (Fn) *Fn = n;
  if (Fd) *Fd = d;
  return LVX_OK;
}

int lvx_pcm_formant_tables(float* w_host, int cap_w, float* c_host, int cap_c, float* tw_host, int cap_tw) {
  if ((w_host && cap_w < FMT_N) || (c_host && cap_c < FMT_TAPS) || (tw_host && cap_tw < FMT_N))
    return fail(LVX_E_ARG, "w_host holds fewer than 1024 floats, c_host fewer than 25 or tw_host fewer than 1024");
  formant_design(w_host, c_host, tw_host);
  return LVX_OK;
}

int lvx_pcm_formant_emitted(long long t0, int n_in, int final) {
  if (t0 < 0 || n_in < 0) return fail(LVX_E_ARG, "t0 and n_in must be >= 0");
  return (int)(formant_emitted_upto(t0 + n_in, final != 0) - formant_emitted_upto(t0, false));
}

int lvx_pcm_formant(lvx_ctx* c, const float* pcm, int B, int n_in, const int32_t* slots, const uint8_t* final_host,
                    int Fn, int Fd, float* out, long long out_stride, int32_t* n_out_host, void* stream) {
  NEED_FINAL(c);
  if (!formant_ok(Fn, Fd)) return fail(LVX_E_ARG, formant_msg(Fn, Fd));
  const bool launch = Fn != Fd;  // 1 / 1: the rows of pcm_dev are the output
  if (int r = pcm_args(B, n_in, pcm, slots && final_host && n_out_host ? slots : nullptr, launch, out, out_stride)) return r;
  std::vector<PcmRow> rows;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    const std::string e = pcm_plan(
        c->seg[lvx_ctx::SEG_FORMANT], FMT_HIST, B, n_in, slots, final_host, n_out_host, ratio_key(Fn, Fd), launch,
        [](long long k) { return "the ratio " + std::to_string(k >> 16) + " / " + std::to_string(k & 0xffff); }, rows,
        [&](const PcmCall& q, PcmRow& r) { return plan_formant(q, n_in, Fn, Fd, out_stride, r); });
    if (!e.empty()) return fail(LVX_E_ARG, e);
  }
  if (!launch) return LVX_OK;
  const Opts o = c->opts_snapshot();
  OptScope os(&o);
  return pcm_launches<PcmRows>(c, rows, [&](const PcmRows& pk, int nr, int max_out) {
    pcm_launch_formant(pk, nr, max_out, Fn, Fd, pcm, n_in, c->fmt_tab, c->fmt_hist, out, out_stride, (hipStream_t)stream);
  });
}

// ---- PCM mark ----
int lvx_pcm_mark_table(unsigned long long key, int id, uint16_t* words_host, int cap) {
  if (id < 0 || id > 255) return fail(LVX_E_ARG, "id must be in 0 .. 255, got " + std::to_string(id));
  if (!words_host || cap < MRK_P) return fail(LVX_E_ARG, "words_host is null or holds fewer than 64 words");
  const MarkTab t = mark_table(key, id);
  std::memcpy(words_host, t.w, sizeof t.w);
  return LVX_OK;
}

int lvx_pcm_mark_emitted(long long t0, int n_in, int final) { return lvx_pcm_formant_emitted(t0, n_in, final); }

int lvx_pcm_mark(lvx_ctx* c, const float* pcm, int B, int n_in, const int32_t* slots, const uint8_t* final_host,
                 unsigned long long key, int id, int strength, float* out, long long out_stride, int32_t* n_out_host,
                 void* stream) {
  NEED_FINAL(c);
  if (!mark_ok(id, strength)) return fail(LVX_E_ARG, mark_msg(id, strength));
  if (int r = pcm_args(B, n_in, pcm, slots && final_host && n_out_host ? slots : nullptr, true, out, out_stride)) return r;
  const MarkTab mt = mark_table(key, id);
  std::vector<PcmRow> rows;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    const std::string e = pcm_plan(
        c->seg[lvx_ctx::SEG_MARK], FMT_HIST, B, n_in, slots, final_host, n_out_host, mark_digest(mt, strength), true,
        [](long long) { return std::string("another mark (key, id or strength)"); }, rows,
        [&](const PcmCall& q, PcmRow& r) { return plan_mark(q, n_in, out_stride, r); });
    if (!e.empty()) return fail(LVX_E_ARG, e);
  }
  const Opts o = c->opts_snapshot();
  OptScope os(&o);
  return pcm_launches<PcmRows>(c, rows, [&](const PcmRows& pk, int nr, int max_out) {
    pcm_launch_mark(pk, nr, max_out, mt, mark_a(strength), pcm, n_in, c->fmt_tab, c->mrk_hist, out, out_stride, (hipStream_t)stream);
  });
}

// ---- PCM FLAC ----
int lvx_pcm_flac_block(int sample_rate) {
  const int bs = flac_block(sample_rate);
  if (!bs) return fail(LVX_E_ARG, "unsupported sample rate " + std::to_string(sample_rate) + " (24000, 16000, 8000, 48000)");
  return bs;
}

int lvx_pcm_flac_emitted(int sample_rate, long long t0, int n_in, int final) {
  const int bs = flac_block(sample_rate);
  if (!bs) return fail(LVX_E_ARG, "unsupported sample rate " + std::to_string(sample_rate));
  if (t0 < 0 || n_in < 0) return fail(LVX_E_ARG, "t0 and n_in must be >= 0");
  return (int)(flac_frames_upto(bs, t0 + n_in, final != 0) - flac_frames_upto(bs, t0, false));
}

int lvx_flac_stream_header(int sample_rate, uint8_t* out, int cap) {
  if (cap < 42 || !flac_stream_header(sample_rate, out)) return fail(LVX_E_ARG, "an unsupported sample rate, a null pointer or cap < 42");
  return LVX_OK;
}

int lvx_flac_subframe(const int16_t* x, int n, uint8_t* out, int cap) {
  const int r = flac_subframe(x, n, out, cap);
  if (r == LVX_E_CAPACITY) return fail(r, "cap is smaller than the subframe");
  if (r < 0) return fail(r, "n must be in 1 .. 65535, x / out not null");
  return r;
}

int lvx_flac_finish(int sample_rate, const uint8_t* slots, int n_frames, unsigned long long* sample_no, uint8_t* out, int cap) {
  if (n_frames > 0x7FFFFFFF / (2 * (FLAC_MAX_BS + 15) + 17)) return fail(LVX_E_ARG, "too many frames for one call");
  const long long r = flac_finish(sample_rate, slots, n_frames, sample_no, out, cap);
  if (r == LVX_E_CAPACITY) return fail(LVX_E_CAPACITY, "cap is smaller than the frames");
  if (r < 0) return fail(LVX_E_ARG, "an unsupported sample rate, a null pointer, n_frames < 0, a record of no FLAC slot or a sample number past 2^36");
  return (int)r;
}

int lvx_pcm_flac(lvx_ctx* c, const int16_t* s16, long long in_stride, int B, int n_in, const int32_t* slots,
                 const uint8_t* final_host, int sample_rate, void* out, long long out_stride, int32_t* n_frames_host, void* stream) {
  NEED_FINAL(c);
  const int bs = flac_block(sample_rate);
  if (!bs) return fail(LVX_E_ARG, "unsupported sample rate " + std::to_string(sample_rate) + " (24000, 16000, 8000, 48000)");
  if (int r = pcm_args(B, n_in, s16, slots && final_host && n_frames_host ? slots : nullptr, true, out, out_stride)) return r;
  if ((reinterpret_cast<uintptr_t>(s16) & 1) || in_stride < 0 || (in_stride & 1))
    return fail(LVX_E_ARG, "s16_dev and in_stride_bytes must be multiples of 2");
  std::vector<FlacRow> rows;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    const std::string e = pcm_plan(
        c->seg[lvx_ctx::SEG_FLAC], FLAC_HIST, B, n_in, slots, final_host, n_frames_host, sample_rate, true,
        [](long long k) { return std::to_string(k) + " Hz"; }, rows,
        [&](const PcmCall& q, FlacRow& r) { return plan_flac(q, n_in, sample_rate, in_stride, out_stride, r); });
    if (!e.empty()) return fail(LVX_E_ARG, e);
  }
  return pcm_launches<FlacRows>(c, rows, [&](const FlacRows& pk, int nr, int max_out) {
    pcm_launch_flac(pk, nr, max_out, bs, s16, n_in, in_stride, c->flac_hist, out, out_stride, (hipStream_t)stream);
  });
}

// ---- PCM pause ----
int lvx_pcm_pause_emitted(int sample_rate, long long t0, int n_in, int final) {
  const int bl = pause_block(sample_rate);
  if (!bl) return fail(LVX_E_ARG, "unsupported sample rate " + std::to_string(sample_rate));
  if (t0 < 0 || n_in < 0) return fail(LVX_E_ARG, "t0 and n_in must be >= 0");
  return (int)(pause_blocks_upto(bl, t0 + n_in, final != 0) - pause_blocks_upto(bl, t0, false));
}

int lvx_pcm_pause_slot(int sample_rate, int encoding) {
  const int bl = pause_block(sample_rate), bps = pcm_sample_bytes(encoding);
  if (!bl || !bps) return fail(LVX_E_ARG, "an unsupported sample rate or encoding");
  return pause_slot_bytes(bl, bps);
}

int lvx_pause_slots(int sample_rate, int encoding, const void* y, long long T, long long j0, long long j1, uint8_t* out,
                    long long cap) {
  if (j1 - j0 > 0x7FFFFFFF / pause_slot_bytes(PAUSE_MAX_BL, 4)) return fail(LVX_E_ARG, "too many blocks for one call");
  const long long r = pause_slots(sample_rate, encoding, y, T, j0, j1, out, cap);
  if (r == LVX_E_CAPACITY) return fail(LVX_E_CAPACITY, "cap is smaller than the slots");
  if (r < 0) return fail(LVX_E_ARG, "an unsupported sample rate or encoding, a null pointer, T < 0 or blocks outside the sentence");
  return (int)r;
}

int lvx_pcm_pause(lvx_ctx* c, const void* in, long long in_stride, int B, int n_in, const int32_t* slots,
                  const uint8_t* final_host, int sample_rate, int encoding, void* out, long long out_stride,
                  int32_t* n_blocks_host, void* stream) {
  NEED_FINAL(c);
  const int bl = pause_block(sample_rate), bps = pcm_sample_bytes(encoding);
  if (!bl) return fail(LVX_E_ARG, "unsupported sample rate " + std::to_string(sample_rate) + " (24000, 16000, 8000, 48000)");
  if (!bps) return fail(LVX_E_ARG, "encoding must be LVX_PCM_F32LE, LVX_PCM_S16LE, LVX_PCM_ULAW or LVX_PCM_ALAW");
  if (int r = pcm_args(B, n_in, in, slots && final_host && n_blocks_host ? slots : nullptr, true, out, out_stride)) return r;
  if ((reinterpret_cast<uintptr_t>(out) & 7) || (out_stride & 7)) return fail(LVX_E_ARG, "out_dev and out_stride_bytes must be multiples of 8");
  if ((reinterpret_cast<uintptr_t>(in) % bps) || in_stride < 0 || (in_stride % bps))
    return fail(LVX_E_ARG, "in_dev and in_stride_bytes must be multiples of the sample's bytes");
  std::vector<PauseRow> rows;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    bool capacity = false;
    const std::string e = pcm_plan(
        c->seg[lvx_ctx::SEG_PAUSE], PAUSE_HIST, B, n_in, slots, final_host, n_blocks_host, pause_key(sample_rate, encoding), true,
        [](long long k) { return std::to_string(k >> 8) + " Hz, encoding " + std::to_string(k & 0xff); }, rows,
        [&](const PcmCall& q, PauseRow& r) { return plan_pause(q, n_in, sample_rate, encoding, in_stride, out_stride, &capacity, r); });
    if (!e.empty()) return fail(capacity ? LVX_E_CAPACITY : LVX_E_ARG, e);
  }
  return pcm_launches<PauseRows>(c, rows, [&](const PauseRows& pk, int nr, int max_out) {
    pcm_launch_pause(pk, nr, max_out, bl, encoding, in, n_in, in_stride, c->pause_hist, out, out_stride, (hipStream_t)stream);
  });
}

}  // extern "C"

// ---------------------------------------------------------------------------
// WavTokenizer encoder (encode_infer): its own context, since its weights are not needed for TTS.
// ---------------------------------------------------------------------------
namespace {
constexpr const char* kEncPrefix = "feature_extractor.encodec.encoder.model.";
constexpr const char* kCodebookKey = "feature_extractor.encodec.quantizer.vq.layers.0._codebook.embed";
struct EncConv {
  std::string name;
  int cin, cout, k, stride, dil;
  bool elu;
};
// seanet.py:94-140 with n_filters 32, ratios [8, 5, 4, 2] reversed, compress 2 (llmvox_amd.weights.encoder_convs)
std::vector<EncConv> enc_convs() {
  std::vector<EncConv> v{{"0", 1, 32, 7, 1, 1, false}};
  int dim = 32, idx = 1;
  for (int ratio : {2, 4, 5, 8}) {
    v.push_back({std::to_string(idx) + ".block.1", dim, dim / 2, 3, 1, 1, true});
    v.push_back({std::to_string(idx) + ".block.3", dim / 2, dim, 1, 1, 1, true});
    v.push_back({std::to_string(idx) + ".shortcut", dim, dim, 1, 1, 1, false});
    v.push_back({std::to_string(idx + 2), dim, 2 * dim, 2 * ratio, ratio, 1, true});
    dim *= 2;
    idx += 3;
  }
  v.push_back({"15", 512, 512, 7, 1, 1, true});
  return v;
}
// SConv1d geometry (conv.py:54-61,79-96,195-211): left pad, reflect domain, output length
struct ConvGeo {
  int pl, lext, T;
};
ConvGeo conv_geo(int L, int k, int stride, int dil) {
  const int keff = (k - 1) * dil + 1, pt = keff - stride;
  const int nf = (L + stride - 1) / stride;  // ceil(n_frames) of get_extra_padding_for_conv1d (L >= 1)
  const int extra = nf * stride - L;
  const int pr = pt / 2, pl = pt - pr, right = pr + extra;
  const int max_pad = std::max(pl, right);
  const int ex0 = L <= max_pad ? max_pad - L + 1 : 0;
  return {pl, L + ex0, (pl + L + right - keff) / stride + 1};
}
// channels of the output of stage st < 11 (stages: llmvox.h, lvx_enc_stages)
int enc_stage_channels(int st) { return st >= 9 ? 512 : 32 << (st / 2); }
int enc_frames_of(int n) {
  int L = n;
  for (const EncConv& cv : enc_convs()) L = conv_geo(L, cv.k, cv.stride, cv.dil).T;
  return L;
}
}  // namespace

struct lvx_enc {
  int device = 0;
  long long max_samples = 0;
  bool finalized = false;
  std::map<std::string, std::vector<float>> host;
  std::vector<void*> allocs;
  std::vector<EncConv> convs = enc_convs();
  std::vector<const float*> cw, cb;  // per conv: [cout][k][cin] weights, bias
  const float *wih[2] = {}, *bih[2] = {}, *whh[2] = {}, *bhh[2] = {};
  const float* codebook = nullptr;  // [4096][512]
  const float* esq = nullptr;       // [4096] |e|^2
  float* buf[4] = {};
  size_t buf_floats = 0;
  float *h = nullptr, *c = nullptr;  // [2][Bmax][512], [Bmax][512]
  int bmax = 0;
  int alloc(float** p, size_t n) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, n * 4 + 256);
    if (e != hipSuccess) return fail(LVX_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    allocs.push_back(q);
    *p = reinterpret_cast<float*>(q);
    return 0;
  }
  int upload(const std::vector<float>& v, const float** out) {
    float* d;
    if (int r = alloc(&d, v.size())) return r;
    HIP_TRY(hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    *out = d;
    return 0;
  }
  std::map<std::string, size_t> expected() const {
    std::map<std::string, size_t> m;
    for (const EncConv& cv : convs) {
      m[std::string(kEncPrefix) + cv.name + ".conv.conv.weight"] = (size_t)cv.cout * cv.cin * cv.k;
      m[std::string(kEncPrefix) + cv.name + ".conv.conv.bias"] = cv.cout;
    }
    for (int l = 0; l < 2; ++l) {
      const std::string p = std::string(kEncPrefix) + "13.lstm.", sfx = "_l" + std::to_string(l);
      m[p + "weight_ih" + sfx] = m[p + "weight_hh" + sfx] = (size_t)2048 * 512;
      m[p + "bias_ih" + sfx] = m[p + "bias_hh" + sfx] = 2048;
    }
    m[kCodebookKey] = (size_t)4096 * 512;
    return m;
  }
};

extern "C" {

int lvx_enc_frames(int n_samples) { return n_samples >= 1 ? enc_frames_of(n_samples) : 0; }

int lvx_enc_create(int device, long long max_samples, lvx_enc** out) {
  if (!out) return fail(LVX_E_ARG, "null argument");
  if (max_samples < 1) return fail(LVX_E_ARG, "max_samples must be >= 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(LVX_E_HIP, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(LVX_E_ARG, "device ordinal out of range");
  auto* e = new lvx_enc();
  e->device = device;
  e->max_samples = max_samples;
  *out = e;
  return LVX_OK;
}

void lvx_enc_destroy(lvx_enc* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  for (void* p : e->allocs) (void)hipFree(p);
  delete e;
}

int lvx_enc_set_weight(lvx_enc* e, const char* name, const float* data, int64_t numel) {
  if (!e || !name || !data) return fail(LVX_E_ARG, "null argument");
  if (e->finalized) return fail(LVX_E_STATE, "weights are frozen after lvx_enc_finalize");
  const auto exp = e->expected();
  auto it = exp.find(name);
  if (it == exp.end()) return fail(LVX_E_NAME, std::string("unknown encoder weight name: ") + name);
  if ((size_t)numel != it->second)
    return fail(LVX_E_ARG, std::string("weight ") + name + ": expected " + std::to_string(it->second) + " elements");
  e->host[name] = std::vector<float>(data, data + numel);
  return LVX_OK;
}

int lvx_enc_finalize(lvx_enc* e) {
  if (!e) return fail(LVX_E_ARG, "null argument");
  if (e->finalized) return LVX_OK;
  for (auto& kv : e->expected())
    if (!e->host.count(kv.first)) return fail(LVX_E_STATE, "missing encoder weight: " + kv.first);
  HIP_TRY(hipSetDevice(e->device));
  int r;
  for (const EncConv& cv : e->convs) {
    const std::string p = std::string(kEncPrefix) + cv.name + ".conv.conv.";
    const float *w, *b;
    if ((r = e->upload(repack_conv(e->host[p + "weight"], cv.cout, cv.cin, cv.k), &w)) || (r = e->upload(e->host[p + "bias"], &b)))
      return r;
    e->cw.push_back(w);
    e->cb.push_back(b);
  }
  for (int l = 0; l < 2; ++l) {
    const std::string p = std::string(kEncPrefix) + "13.lstm.", sfx = "_l" + std::to_string(l);
    if ((r = e->upload(e->host[p + "weight_ih" + sfx], &e->wih[l])) || (r = e->upload(e->host[p + "bias_ih" + sfx], &e->bih[l])) ||
        (r = e->upload(e->host[p + "weight_hh" + sfx], &e->whh[l])) || (r = e->upload(e->host[p + "bias_hh" + sfx], &e->bhh[l])))
      return r;
  }
  const std::vector<float>& cbk = e->host[kCodebookKey];
  if ((r = e->upload(cbk, &e->codebook))) return r;
  std::vector<float> esq(4096);
  for (int n = 0; n < 4096; ++n) {  // |e|^2 (core_vq.py:180: embed.pow(2).sum(0)), double accumulation
    double a = 0.0;
    for (int k = 0; k < 512; ++k) a += (double)cbk[(size_t)n * 512 + k] * cbk[(size_t)n * 512 + k];
    esq[n] = (float)a;
  }
  if ((r = e->upload(esq, &e->esq))) return r;
  // activations: at most 32 channels per input sample through the SEANet stack; the LSTM gates
  // (2,048 per frame) and the quantiser scores (4,096 per frame) of up to 64 one-frame streams
  e->buf_floats = (size_t)e->max_samples * 32 + (size_t)64 * 4096;
  for (auto& b : e->buf)
    if ((r = e->alloc(&b, e->buf_floats))) return r;
  e->bmax = 1024;
  if ((r = e->alloc(&e->h, (size_t)2 * e->bmax * 512)) || (r = e->alloc(&e->c, (size_t)e->bmax * 512))) return r;
  HIP_TRY(hipDeviceSynchronize());
  e->host.clear();
  e->finalized = true;
  return LVX_OK;
}

// Stages [first, last] of the encoder (the table at lvx_enc_stages in llmvox.h) on `in`, the input of stage
// `first` with L frames per stream: the one stage list of lvx_encode (the window [0, last stage]) and of the
// test hook. It is walked twice per call: launch = false holds every intermediate of the window against the
// scratch and launches nothing, launch = true launches. A stage reads the caller's pointer or the buffer its
// predecessor wrote; *out / *Lout name what the last stage left (stage 11: the embedding it read, with the
// scores in buf[1]).
static int enc_walk(lvx_enc* e, int first, int last, const float* in, int B, int L, float* features, int32_t* codes,
                    bool launch, hipStream_t s, const float** out, int* Lout) {
  float** buf = e->buf;
  bool fits = true;
  auto conv = [&](int i, const float* x, int L, float* y, const float* res) {
    const EncConv& cv = e->convs[i];
    const ConvGeo g = conv_geo(L, cv.k, cv.stride, cv.dil);
    if (!launch)
      fits = fits && (size_t)B * g.T * cv.cout <= e->buf_floats && (size_t)B * L * cv.cin <= e->buf_floats;
    else
      enc_launch_conv(x, e->cw[i], e->cb[i], res, y, B, L, g.T, cv.cin, cv.cout, cv.k, cv.stride, cv.dil, g.pl, g.lext, cv.elu, s);
    return g.T;
  };
  // the LSTM's input projections and the quantiser's scores: a 1-tap "conv" with the matrix as weights
  auto proj = [&](const float* x, const float* w, const float* bias, float* y, int n) {
    if (!launch)
      fits = fits && (size_t)B * L * n <= e->buf_floats;
    else
      enc_launch_conv(x, w, bias, nullptr, y, B, L, L, 512, n, 1, 1, 1, 0, L, false, s);
  };
  const float* x = in;
  for (int st = first; st <= last; ++st) {
    if (st == 0) {
      L = conv(0, x, L, buf[0], nullptr);
      x = buf[0];
    } else if (st <= 8) {
      const int i = 1 + 4 * ((st - 1) / 2);
      if (st & 1) {  // residual block: t1 = block.1(ELU x), sc = shortcut(x), x' = block.3(ELU t1) + sc
        conv(i, x, L, buf[1], nullptr);
        conv(i + 2, x, L, buf[2], nullptr);
        conv(i + 1, buf[1], L, buf[3], buf[2]);
        x = buf[3];
      } else {  // down(ELU x')
        L = conv(i + 3, x, L, buf[0], nullptr);
        x = buf[0];
      }
    } else if (st == 9) {  // SLSTM: layer 0 -> buf[2], layer 1 (+ skip from the LSTM input) -> buf[3]
      for (int l = 0; l < 2; ++l) {
        float* yout = l == 0 ? buf[2] : buf[3];
        proj(l == 0 ? x : buf[2], e->wih[l], e->bih[l], buf[1], 2048);
        if (!launch) continue;
        HIP_TRY(hipMemsetAsync(e->h, 0, (size_t)B * 512 * 4, s));
        HIP_TRY(hipMemsetAsync(e->c, 0, (size_t)B * 512 * 4, s));
        for (int t = 0; t < L; ++t)
          enc_launch_lstm_step(buf[1], e->whh[l], e->bhh[l], e->h + (size_t)(t & 1) * e->bmax * 512,
                               e->h + (size_t)((t + 1) & 1) * e->bmax * 512, e->c, yout, l == 1 ? x : nullptr, B, L, t, s);
      }
      x = buf[3];
    } else if (st == 10) {  // ELU -> final conv: embedding [B][T][512]
      conv(17, x, L, buf[0], nullptr);
      x = buf[0];
    } else {  // quantiser: scores x . e, then argmax + gather
      proj(x, e->codebook, nullptr, buf[1], 4096);
      if (launch) enc_launch_vq(x, buf[1], e->esq, e->codebook, codes, features, B, L, s);
    }
  }
  if (!fits) return fail(LVX_E_CAPACITY, "encoder activations exceed the scratch sized by max_samples");
  *out = x;
  *Lout = L;
  return LVX_OK;
}

// the checks of a call, the capacity walk, then the launches
static int enc_run(lvx_enc* e, int first, int last, const float* in, int B, int L, float* features, int32_t* codes,
                   hipStream_t s, const float** out, int* Lout) {
  if (!e) return fail(LVX_E_ARG, "null argument");
  if (!e->finalized) return fail(LVX_E_STATE, "call lvx_enc_finalize first");
  if (B < 1 || L < 1 || !in || (last == LVX_ENC_STAGES - 1 && (!features || !codes)))
    return fail(LVX_E_ARG, "bad audio / outputs");
  if ((first == 0 && (long long)B * L > e->max_samples) || B > e->bmax)
    return fail(LVX_E_CAPACITY, "B*N = " + std::to_string((long long)B * L) + " exceeds max_samples " + std::to_string(e->max_samples));
  HIP_TRY(hipSetDevice(e->device));
  if (int r = enc_walk(e, first, last, in, B, L, features, codes, false, s, out, Lout)) return r;
  if (int r = enc_walk(e, first, last, in, B, L, features, codes, true, s, out, Lout)) return r;
  HIP_TRY(hipGetLastError());
  return LVX_OK;
}

// audio [B][N] -> features [B][512][T], codes [B][T] (device pointers; T = lvx_enc_frames(N))
int lvx_encode(lvx_enc* e, const float* audio, int B, int N, float* features, int32_t* codes, void* stream) {
  const float* x;
  int T;
  return enc_run(e, 0, LVX_ENC_STAGES - 1, audio, B, N, features, codes, (hipStream_t)stream, &x, &T);
}

// test hook: a window of the stage list on the caller's input
int lvx_enc_stages(lvx_enc* e, int first, int last, const float* in, int B, int L, float* out, int32_t* codes,
                   float* features, float* scores, void* stream) {
  if (first < 0 || last >= LVX_ENC_STAGES || first > last)
    return fail(LVX_E_ARG, "stage window must satisfy 0 <= first <= last < " + std::to_string(LVX_ENC_STAGES));
  if (last < LVX_ENC_STAGES - 1 && !out) return fail(LVX_E_ARG, "null out");
  hipStream_t s = (hipStream_t)stream;
  const float* x;
  int T;
  if (int r = enc_run(e, first, last, in, B, L, features, codes, s, &x, &T)) return r;
  if (last < LVX_ENC_STAGES - 1)
    HIP_TRY(hipMemcpyAsync(out, x, (size_t)B * T * enc_stage_channels(last) * 4, hipMemcpyDeviceToDevice, s));
  else if (scores)
    HIP_TRY(hipMemcpyAsync(scores, e->buf[1], (size_t)B * T * 4096 * 4, hipMemcpyDeviceToDevice, s));
  return LVX_OK;
}

// test hook: the encoder's output before quantisation ([B][T][512], time-major) of the last lvx_encode
int lvx_enc_embedding(lvx_enc* e, float* dst, int B, int T, void* stream) {
  if (!e || !e->finalized || !dst) return fail(LVX_E_ARG, "bad arguments");
  HIP_TRY(hipMemcpyAsync(dst, e->buf[0], (size_t)B * T * 512 * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return LVX_OK;
}

}  // extern "C"
