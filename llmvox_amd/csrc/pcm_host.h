// Host side of the PCM stages (include/llmvox.h: "PCM output stage", "PCM time stretch", "PCM pitch shift", "PCM dump
// join", "PCM level", "PCM formant", "PCM mark", "PCM G.711", "PCM FLAC", "PCM pause"): the stages' constants and kernel row packets, the tables and streaming
// counts of llmvox.h's rules in double, the G.711 companding, the FLAC stage's selection arithmetic and the host side of
// its frames, and the one skeleton every stage's entry point runs (lvx_api.cpp). No HIP header and no device:
// tests/host/pcm_stage_check.cpp, g711_check.cpp, flac_check.cpp, formant_check.cpp, pause_check.cpp and mark_check.cpp drive all of it
// with the system compiler.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <string>
#include <vector>

#include "llmvox.h"

namespace lvx {

// ---------------- the row packets (kernel arguments of pcm_kernels.hip: their layouts are the device's) ----------------
constexpr int PCM_HIST = 160;  // inputs of history a slot keeps between calls (the filters reach back <= 144)
constexpr int PCM_ROWS = 32;   // rows of one launch (their descriptors travel as kernel arguments)
struct PcmRow {
  long long t0;  // inputs of the slot's segment consumed before this call
  long long m0;  // outputs of the segment emitted before this call = index of the call's first output
  int n_out;     // outputs of this call
  int hist_in;   // float offset of the slot's history [PCM_HIST] (inputs t0 - 160 .. t0 - 1) in the pool
  int hist_out;  // where the history after this call goes (the slot's other buffer); -1: none kept
  int row;       // row of pcm / out
};
struct PcmRows {
  PcmRow r[PCM_ROWS];
};

// PCM pitch shift: the ratio resampler
constexpr int RAT_HIST = 256;        // inputs of history a slot keeps between calls (an output reaches back <= 192)
constexpr int RAT_MAX = 200;         // L and M of a ratio: 1 .. 200
constexpr int RAT_TAPS = 2 * 24 * RAT_MAX + 1;  // the longest prototype: 2 N + 1 with N = 24 max(L, M)
constexpr int RAT_TAPS_STRIDE = (RAT_TAPS + 63) / 64 * 64;  // floats of a slot's table region
struct RatioRow {  // PcmRow and where the slot's table is
  long long t0;  // inputs of the slot's segment consumed before this call
  long long m0;  // outputs of the segment emitted before this call = index of the call's first output
  int n_out;     // outputs of this call
  int hist_in;   // float offset of the slot's history [RAT_HIST] (inputs t0 - 256 .. t0 - 1) in the pool
  int hist_out;  // where the history after this call goes (the slot's other buffer); -1: none kept
  int row;       // row of pcm / out
  int taps;      // float offset of the slot's table region (h[-N .. N]) in the table pool
};
struct RatioRows {
  RatioRow r[PCM_ROWS];
};

// PCM time stretch
constexpr int STR_H = 240;      // output hop
constexpr int STR_D = 240;      // search radius
constexpr int STR_C = 480;      // correlation length
constexpr int STR_HIST = 1280;  // inputs of history a slot keeps between calls (a hop reaches back <= 1199)
struct StretchRow {
  long long t0;  // inputs of the slot's segment consumed before this call
  long long j0;  // hops of the segment emitted before this call = index of the call's first hop
  int n_hops;    // hops of this call
  int n_out;     // samples of this call: n_hops * STR_H, less where a final call cuts the last hop
  int hist_in;   // float offset of the slot's history [STR_HIST] (inputs t0 - 1280 .. t0 - 1) in the pool
  int hist_out;  // where the history after this call goes (the slot's other buffer); -1: none kept
  int slot;      // the slot's word of the d_{j-1} state
  int row;       // row of pcm / out / d_out
};
struct StretchRows {
  StretchRow r[PCM_ROWS];
};

// PCM dump join
constexpr int JOIN_HOLD = 320;  // samples held back and crossfaded: one codec frame
constexpr int JOIN_CTX = 16;    // the most context frames of a call
enum { JOIN_HEAD_NONE = 0, JOIN_HEAD_TAIL = 1, JOIN_HEAD_FADE = 2 };
struct JoinRow {
  int s;         // samples of context in front of the row: 320 c
  int head;      // JOIN_HEAD_*: nothing, the slot's tail as it is, the tail crossfaded with r[s - 320 .. s)
  int n_out;     // samples of this call: the head's 320 (if any), then r[s .. s + n_out - head's)
  int tail_in;   // float offset of the slot's current tail [JOIN_HOLD] in the pool
  int tail_out;  // where r[n_in - 320 .. n_in) goes (the slot's other buffer); -1: none kept
  int row;       // row of pcm / out
};
struct JoinRows {
  JoinRow r[PCM_ROWS];
};

// PCM level. The rows travel as PcmRows: t0 the inputs consumed before the call, m0 the outputs emitted before it (the
// index of the call's first output: max(0, t0 - 2 A)), hist_in / hist_out float offsets of [LVL_HIST] buffers.
constexpr int LVL_A = LVX_LEVEL_A;   // attack half-window
constexpr int LVL_R = LVX_LEVEL_R;   // hold
constexpr int LVL_TAPS = 2 * LVL_A + 1;
constexpr int LVL_HIST = 1600;       // raw inputs of history a slot keeps between calls (an output reaches back <= 3 A + R = 1560)

// PCM FLAC: the s16 rows of lvx_pcm_convert cut into frames, one subframe a workgroup
constexpr int FLAC_MAX_BS = 1920;            // the block size at 48 kHz, the largest
constexpr int FLAC_HIST = FLAC_MAX_BS + 16;  // int16 a slot keeps between calls: the <= BS + 15 samples no frame has taken yet
constexpr int FLAC_MAX_N = 65535;            // samples of a frame lvx_flac_subframe takes (the device's are <= BS + 15)
struct FlacRow {
  long long t0;  // inputs of the slot's segment consumed before this call
  long long j0;  // frames of the segment emitted before this call = index of the call's first frame
  int n_out;     // frames of this call
  int last_n;    // samples of the call's last frame (every frame before it has BS)
  int hist_in;   // int16 offset of the slot's history [FLAC_HIST] (inputs t0 - FLAC_HIST .. t0 - 1) in the pool
  int hist_out;  // where the history after this call goes (the slot's other buffer); -1: none kept
  int row;       // row of s16 / out
};
struct FlacRows {
  FlacRow r[PCM_ROWS];
};

// PCM pause: the encoded rows cut into blocks of 10 ms, one slot (a record and the block's bytes) each
constexpr int PAUSE_MAX_BL = 480;            // the block at 48 kHz, the largest
constexpr int PAUSE_HIST = PAUSE_MAX_BL * 4;  // bytes a slot keeps between calls: the 1 .. bl samples no block has taken yet
struct PauseRow {
  long long t0;  // inputs of the slot's segment consumed before this call
  long long j0;  // blocks of the segment emitted before this call = index of the call's first block
  int n_out;     // blocks of this call
  int last_n;    // samples of the call's last block (every block before it has bl)
  int hist_in;   // byte offset of the slot's history [PAUSE_HIST] (inputs t0 - bl .. t0 - 1 at its front) in the pool
  int hist_out;  // where the history after this call goes (the slot's other buffer); -1: none kept
  int row;       // row of in / out
  int last;      // 1: the call is final, its last block is the sentence's last
};
struct PauseRows {
  PauseRow r[PCM_ROWS];
};

// PCM formant: the spectral-envelope correction. The rows travel as PcmRows: t0 the inputs consumed before the call,
// m0 the outputs emitted before it (a multiple of FMT_H), hist_in / hist_out float offsets of [FMT_HIST] buffers.
constexpr int FMT_N = LVX_FORMANT_N;      // frame length
constexpr int FMT_H = LVX_FORMANT_H;      // hop
constexpr int FMT_K = LVX_FORMANT_K;      // smoothing half-width in bins
constexpr int FMT_TAPS = 2 * FMT_K + 1;
constexpr int FMT_BINS = FMT_N / 2 + 1;   // bins 0 .. N / 2 of a real signal's spectrum
constexpr int FMT_HIST = 7 * FMT_H;       // inputs of history a slot keeps between calls (a call's first output reaches back <= 7 H - 1)
constexpr int FMT_MAX = 40000;            // Fn and Fd of a correction ratio: 1 .. 40000 (the plan's are <= 100 * 200 and 200 * 200)
constexpr int FMT_TABLES = FMT_N + FMT_TAPS + FMT_N;  // floats of the device tables: w, c, then the twiddles (re then im)

// PCM mark: the watermark. The formant stage's frames, tables, counts, history and rows (PcmRows); its own pool of
// [FMT_HIST] buffers. The sign table travels by value with every launch.
constexpr int MRK_K0 = LVX_MARK_K0;       // first marked bin
constexpr int MRK_BW = LVX_MARK_BW;       // bins of a sub-band
constexpr int MRK_U = LVX_MARK_U;         // sub-bands: pair m is the sub-bands (2 m, 2 m + 1)
constexpr int MRK_PAIRS = MRK_U / 2;
constexpr int MRK_Q = LVX_MARK_Q;         // frames of a block
constexpr int MRK_P = LVX_MARK_P;         // blocks of a period
constexpr int MRK_STRENGTH_MIN = 1, MRK_STRENGTH_MAX = 3;
struct MarkTab {
  uint16_t w[MRK_P];  // bit m of word p: pair m of block p has g- on its even sub-band and g+ on its odd one
};
static_assert(MRK_K0 + MRK_U * MRK_BW <= FMT_N / 2 && MRK_PAIRS <= 16 && MRK_U % 2 == 0, "the band lies below N / 2 and a word holds the pairs");

// ---------------- the rules' tables and counts ----------------
// ---- PCM dump join: the window tables and the counts (llmvox.h) ----
// wr[n] = 0.5 - 0.5 cos(pi (n + 0.5) / 320), wf = 1 - wr in double; each table rounded once
inline void join_design(float* wr, float* wf) {
  const double pi = 3.14159265358979323846;
  for (int n = 0; n < JOIN_HOLD; ++n) {
    const double r = 0.5 - 0.5 * std::cos(pi * (n + 0.5) / JOIN_HOLD);
    wr[n] = (float)r;
    wf[n] = (float)(1.0 - r);
  }
}

// samples a join call emits, -1 where the call is not one the rule admits (llmvox.h: the LVX_E_ARG cases)
inline int join_emitted(bool open, int c, int n_in, bool final) {
  if (n_in < 0 || n_in % JOIN_HOLD || c < 0 || c > JOIN_CTX) return -1;
  if (n_in == 0) return (final && c == 0) ? (open ? JOIN_HOLD : 0) : -1;
  if ((long long)JOIN_HOLD * c >= n_in || (c > 0 && !open)) return -1;
  return (open ? JOIN_HOLD : 0) + n_in - JOIN_HOLD * c - (final ? 0 : JOIN_HOLD);
}

inline std::string join_msg(bool open, int c, int n_in, bool final) {
  return "not a join call: n_in " + std::to_string(n_in) + ", ctx_frames " + std::to_string(c) + (final ? ", final" : ", not final") +
         (open ? ", open segment" : ", closed segment") +
         " (n_in a multiple of 320; ctx_frames in [0, 16], 320 ctx_frames < n_in, 0 on a closed segment; n_in 0 only as a final "
         "flush without context)";
}

// ---- PCM output stage: the rates, their prototype filters and the streaming counts (llmvox.h) ----
struct PcmRate {
  int rate, L, M, N;
  int tap_off;  // float offset of the rate's taps in lvx_ctx::pcm_taps
};
inline constexpr PcmRate kPcmRates[] = {{16000, 2, 3, 72, 0}, {8000, 1, 3, 72, 145}, {48000, 2, 1, 48, 290}};
inline constexpr PcmRate kPcmNoFilter = {24000, 1, 1, 0, 0};

inline const PcmRate* pcm_rate_of(int sample_rate) {
  if (sample_rate == 24000) return &kPcmNoFilter;
  for (const PcmRate& pr : kPcmRates)
    if (pr.rate == sample_rate) return &pr;
  return nullptr;
}

inline double bessel_i0(double x) {  // the power series: sum ((x / 2)^k / k!)^2
  double sum = 1.0, term = 1.0;
  const double q = x * x / 4.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * k);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

// h[n] = L 2 fc sinc(2 fc n) kaiser(2 N + 1, 9.0)[n + N], n = -N .. N, designed in double, stored as fp32:
// the three fixed rates and every ratio of the pitch control (llmvox.h, "PCM pitch shift")
inline std::vector<float> pcm_design(int L, int M, int N) {
  if (N == 0) return {1.f};
  const double lo = std::min(1.0, (double)L / M), fc = 0.5 * lo * 0.85 / L, beta = 9.0, pi = 3.14159265358979323846;
  std::vector<float> h(2 * N + 1);
  for (int n = -N; n <= N; ++n) {
    const double a = 2.0 * fc * n, sinc = n == 0 ? 1.0 : std::sin(pi * a) / (pi * a);
    const double u = (double)n / N;
    const double w = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - u * u))) / bessel_i0(beta);
    h[n + N] = (float)(L * 2.0 * fc * sinc * w);
  }
  return h;
}
inline std::vector<float> pcm_design(const PcmRate& pr) { return pcm_design(pr.L, pr.M, pr.N); }

// outputs of a segment emitted once T inputs are consumed
inline long long pcm_emitted_upto(int L, int M, int N, long long T, bool final) {
  const long long all = (T * L + M - 1) / M;  // ceil(T L / M)
  if (final || N == 0) return all;
  const long long a = (T - 1) * L - N;
  return a < 0 ? 0 : std::min(a / M + 1, all);
}
inline long long pcm_emitted_upto(const PcmRate& pr, long long T, bool final) {
  return pcm_emitted_upto(pr.L, pr.M, pr.N, T, final);
}

// ---- PCM pitch shift: the plan and the ratios the resampler takes (llmvox.h) ----
inline int gcd_of(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}
// coprime 1 <= L, M <= 200 with M <= 4 L and L <= 4 M
inline bool ratio_ok(int L, int M) {
  return L >= 1 && M >= 1 && L <= RAT_MAX && M <= RAT_MAX && M <= 4 * L && L <= 4 * M && gcd_of(L, M) == 1;
}
inline int ratio_N(int L, int M) { return L == M ? 0 : 24 * std::max(L, M); }  // (coprime: L == M is 1 / 1, the identity)
inline std::string ratio_msg(int L, int M) {
  return "L / M must be coprime, each in 1 .. 200, with M <= 4 L and L <= 4 M, got " + std::to_string(L) + " / " + std::to_string(M);
}

// ---- PCM time stretch: the window tables and the streaming counts (llmvox.h) ----
// wr[n] = 0.5 - 0.5 cos(pi (n + 0.5) / H), wf[n] = 1 - wr[n] (in double), each rounded to fp32 once
inline void stretch_design(float* wr, float* wf) {
  const double pi = 3.14159265358979323846;
  for (int n = 0; n < STR_H; ++n) {
    const double r = 0.5 - 0.5 * std::cos(pi * (n + 0.5) / STR_H);
    wr[n] = (float)r;
    wf[n] = (float)(1.0 - r);
  }
}

inline long long stretch_a(long long j, int pct) { return (j * STR_H * pct) / 100; }

// inputs of the segment hop j reads: the exclusive upper end of its search and its output
inline long long stretch_need(long long j, int pct) {
  if (j == 0) return 2 * STR_H;
  return std::max(stretch_a(j, pct) + STR_D + 2 * STR_H, stretch_a(j - 1, pct) + STR_D + 3 * STR_H);
}

// how many hops j have need_j <= T (need_j does not decrease with j)
inline long long stretch_hops(int pct, long long T) {
  long long n = std::max(0ll, (T - 3 * STR_H) * 100 / ((long long)STR_H * pct)) + 2;
  while (n > 0 && stretch_need(n - 1, pct) > T) --n;
  while (stretch_need(n, pct) <= T) ++n;
  return n;
}

// samples of a segment emitted once T inputs are consumed
inline long long stretch_emitted_upto(int pct, long long T, bool final) {
  if (pct == 100) return T;
  if (final) return (T * 100 + pct - 1) / pct;
  return STR_H * stretch_hops(pct, T);
}

// ---- PCM level: the window table and the streaming counts (llmvox.h) ----
// w[k] = (0.5 + 0.5 cos(pi k / (A + 1))) / (A + 1), k = -A .. A, in double, each tap rounded to fp32 once
inline void level_design(float* w) {
  const double pi = 3.14159265358979323846;
  for (int k = -LVL_A; k <= LVL_A; ++k) w[k + LVL_A] = (float)((0.5 + 0.5 * std::cos(pi * k / (LVL_A + 1))) / (LVL_A + 1));
}

// samples of a segment emitted once T inputs are consumed: the last 2 A wait for their right-hand inputs
inline long long level_emitted_upto(int pct, long long T, bool final) {
  if (pct == 100 || final) return T;
  return std::max(0ll, T - 2 * LVL_A);
}

// ---- PCM formant: the plan, the tables and the streaming counts (llmvox.h) ----
// coprime 1 <= Fn, Fd <= 40000 with Fd <= 2 Fn and Fn <= 2 Fd
inline bool formant_ok(int Fn, int Fd) {
  return Fn >= 1 && Fd >= 1 && Fn <= FMT_MAX && Fd <= FMT_MAX && Fd <= 2 * Fn && Fn <= 2 * Fd && gcd_of(Fn, Fd) == 1;
}
inline std::string formant_msg(int Fn, int Fd) {
  return "Fn / Fd must be coprime, each in 1 .. 40000, with Fd <= 2 Fn and Fn <= 2 Fd, got " + std::to_string(Fn) + " / " + std::to_string(Fd);
}
// rho = (100 M) / (formant_pct L) in lowest terms, (L, M) the resampling of speed_pct and pitch_pct (lvx_pcm_pitch_plan's:
// L / M = stretch_pct / speed_pct). false: a percentage outside [50, 200], a stretch outside, or rho outside 1/2 .. 2
inline bool formant_plan(int speed_pct, int pitch_pct, int formant_pct, int* Fn, int* Fd) {
  if (speed_pct < 50 || speed_pct > 200 || pitch_pct < 50 || pitch_pct > 200 || formant_pct < 50 || formant_pct > 200) return false;
  const int st = (200 * speed_pct + pitch_pct) / (2 * pitch_pct);  // speed 100 / pitch, rounded half up
  if (st < 50 || st > 200) return false;
  const int g = gcd_of(st, speed_pct), L = st / g, M = speed_pct / g;
  const int n = 100 * M, d = formant_pct * L, h = gcd_of(n, d);
  if (!formant_ok(n / h, d / h)) return false;
  *Fn = n / h;
  *Fd = d / h;
  return true;
}

// w[n] = 0.5 - 0.5 cos(2 pi (n + 0.5) / N) [N]; c[d] = (0.5 + 0.5 cos(pi d / (K + 1))) / (K + 1), d = -K .. K [2 K + 1];
// the twiddles exp(-2 pi i k / N), k < N / 2: tw[k] = cos(2 pi k / N), tw[N / 2 + k] = -sin(2 pi k / N) [N]. In double,
// each entry rounded to fp32 once; a null table is left out
inline void formant_design(float* w, float* c, float* tw) {
  const double pi = 3.14159265358979323846;
  for (int n = 0; w && n < FMT_N; ++n) w[n] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (n + 0.5) / FMT_N));
  for (int d = -FMT_K; c && d <= FMT_K; ++d) c[d + FMT_K] = (float)((0.5 + 0.5 * std::cos(pi * d / (FMT_K + 1))) / (FMT_K + 1));
  for (int k = 0; tw && k < FMT_N / 2; ++k) {
    tw[k] = (float)std::cos(2.0 * pi * k / FMT_N);
    tw[FMT_N / 2 + k] = (float)(-std::sin(2.0 * pi * k / FMT_N));
  }
}

// samples of a segment emitted once T inputs are consumed: a hop block waits for the four frames that cover it
inline long long formant_emitted_upto(long long T, bool final) {
  if (final) return T;
  return std::max(0ll, (T / FMT_H - 3) * FMT_H);
}

// ---- PCM mark: the sign table, its digest and the gain step (llmvox.h); the counts are the formant stage's ----
inline bool mark_ok(int id, int strength) { return id >= 0 && id <= 255 && strength >= MRK_STRENGTH_MIN && strength <= MRK_STRENGTH_MAX; }
inline std::string mark_msg(int id, int strength) {
  return "id must be in 0 .. 255 and strength in 1 .. 3, got id " + std::to_string(id) + ", strength " + std::to_string(strength);
}
// bit m of word p: c(p, m) XOR bit ((12 p + m) mod 8) of id, c the top bit of SplitMix64's output number 12 p + m
inline MarkTab mark_table(uint64_t key, int id) {
  MarkTab t{};
  uint64_t state = key;
  for (int p = 0; p < MRK_P; ++p)
    for (int m = 0; m < MRK_PAIRS; ++m) {
      state += 0x9E3779B97F4A7C15ull;
      uint64_t z = state;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      const unsigned bit = (unsigned)(z >> 63) ^ (((unsigned)id >> ((MRK_PAIRS * p + m) % 8)) & 1u);
      t.w[p] = (uint16_t)(t.w[p] | (bit << m));
    }
  return t;
}
// a = 2^-(7 - strength): 1/64, 1/32, 1/16
inline float mark_a(int strength) { return 1.0f / (float)(1 << (7 - strength)); }
// what a segment is open at (PcmSeg::key): FNV-1a over the table's words and the strength, the sign bit cleared
inline long long mark_digest(const MarkTab& t, int strength) {
  uint64_t h = 0xCBF29CE484222325ull;
  auto eat = [&](unsigned byte) { h = (h ^ (byte & 0xffu)) * 0x100000001B3ull; };
  for (int p = 0; p < MRK_P; ++p) {
    eat(t.w[p]);
    eat(t.w[p] >> 8u);
  }
  eat((unsigned)strength);
  return (long long)(h & 0x7FFFFFFFFFFFFFFFull);
}

// ---- PCM G.711: the companding of an s16 sample and its inverse (llmvox.h), integers only ----
// constexpr and nothing else: one statement for the host entries below and for pcm_convert_kernel's epilogue (a
// constexpr function is callable from device code as it stands). The segment comes from the bit length, by a count of
// leading zeros (one instruction on the device), not from llmvox.h's loops.
constexpr int g711_bit_length(int t) { return 31 - __builtin_clz(2u * (unsigned)t + 1u); }  // of t >= 0 (0: 0)

constexpr int g711_ulaw(int q) {  // q in [-32768, 32767] -> the code, 0 .. 255
  const int b = ((q < 0 ? ~q : q) >> 2) + 33, a = b < 0x1FFF ? b : 0x1FFF;
  const int seg = 1 + g711_bit_length(a >> 6);  // 1 .. 8
  return ((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF)) | (q >= 0 ? 0x80 : 0);
}

constexpr int g711_alaw(int q) {
  int x = (q < 0 ? ~q : q) >> 4;
  const int e = g711_bit_length(x >> 4);  // 0: x <= 15, the linear segment; else the e of llmvox.h's loop, 1 .. 7
  if (e > 0) x = (x >> (e - 1)) - 16 + (e << 4);
  return (x | (q >= 0 ? 0x80 : 0)) ^ 0x55;
}

constexpr int g711_ulaw_linear(int c) {  // c in [0, 255] -> the s16 sample
  const int m = ~c & 0xFF, e = (m >> 4) & 7, step = 4 << (e + 1);
  const int lin = (0x80 << e) + step * (m & 0xF) + step / 2 - 132;
  return c < 0x80 ? -lin : lin;
}

constexpr int g711_alaw_linear(int c) {
  const int i = c ^ 0x55, e = (i & 0x7F) >> 4;
  int m = i & 0xF;
  if (e > 0) m += 16;
  m = (m << 4) + 8;
  if (e > 1) m <<= e - 1;
  return (i & 0x80) ? m : -m;
}

template <int ENC> constexpr int g711_code(int q) { return ENC == LVX_PCM_ULAW ? g711_ulaw(q) : g711_alaw(q); }
constexpr bool is_g711(int encoding) { return encoding == LVX_PCM_ULAW || encoding == LVX_PCM_ALAW; }

// lvx_pcm_g711_encode / lvx_pcm_g711_decode: LVX_OK, or LVX_E_ARG for another encoding, n < 0, a null pointer with n > 0
inline int g711_encode(int encoding, const int16_t* in, long long n, uint8_t* out) {
  if (!is_g711(encoding) || n < 0 || (n > 0 && (!in || !out))) return LVX_E_ARG;
  if (encoding == LVX_PCM_ULAW)
    for (long long i = 0; i < n; ++i) out[i] = (uint8_t)g711_ulaw(in[i]);
  else
    for (long long i = 0; i < n; ++i) out[i] = (uint8_t)g711_alaw(in[i]);
  return LVX_OK;
}

inline int g711_decode(int encoding, const uint8_t* in, long long n, int16_t* out) {
  if (!is_g711(encoding) || n < 0 || (n > 0 && (!in || !out))) return LVX_E_ARG;
  if (encoding == LVX_PCM_ULAW)
    for (long long i = 0; i < n; ++i) out[i] = (int16_t)g711_ulaw_linear(in[i]);
  else
    for (long long i = 0; i < n; ++i) out[i] = (int16_t)g711_alaw_linear(in[i]);
  return LVX_OK;
}

// bytes of one output sample of an encoding lvx_pcm_convert takes; 0: not one
constexpr int pcm_sample_bytes(int encoding) {
  return encoding == LVX_PCM_F32LE ? 4 : encoding == LVX_PCM_S16LE ? 2 : is_g711(encoding) ? 1 : 0;
}

// ---- PCM pause: the blocks, the mark and the slots (llmvox.h) ----
// The constexpr functions are the one statement of the mark that pcm_pause_kernel and lvx_pause_slots both call.
constexpr int pause_block(int rate) {  // bl = rate / 100 (10 ms); 0: not a rate of the stage
  return rate == 8000 || rate == 16000 || rate == 24000 || rate == 48000 ? rate / 100 : 0;
}
constexpr int pause_slot_bytes(int bl, int bps) { return 8 + bl * bps; }
static_assert(pause_slot_bytes(pause_block(8000), 1) == LVX_PAUSE_SLOT(8000, 1) && pause_slot_bytes(PAUSE_MAX_BL, 4) % 8 == 0, "");
// blocks of a segment emitted once T inputs are consumed: after a non-final call the complete ones that at least one
// more sample follows; a final call adds the rest, so the sentence's last block always leaves with the final call
constexpr long long pause_blocks_upto(int bl, long long T, bool final) {
  return T <= 0 ? 0 : final ? (T + bl - 1) / bl : (T - 1) / bl;
}
constexpr bool pause_loud_s16(int q) { return (q < 0 ? -q : q) > LVX_PAUSE_THRESH; }  // (in 32 bits: -32768 is loud)
// 103 / 32768 = 0.003143310546875 is exact in fp32, the bits 0x3B4E0000; of two fp32 that are no NaN the one of the
// larger magnitude has the larger bits below the sign, and a NaN's are above every number's
constexpr uint32_t PAUSE_THRESH_F32_BITS = 0x3B4E0000u;
// the sample whose little-endian bits are `bits` (the low 8 * bps of them) is louder than the threshold
template <int ENC> constexpr bool pause_loud(uint32_t bits) {
  if (ENC == LVX_PCM_F32LE) return (bits & 0x7FFFFFFFu) > PAUSE_THRESH_F32_BITS;  // |v| > 103 / 32768, or a NaN
  if (ENC == LVX_PCM_S16LE) return pause_loud_s16((int16_t)(uint16_t)bits);
  return pause_loud_s16(ENC == LVX_PCM_ULAW ? g711_ulaw_linear((int)(bits & 0xFFu)) : g711_alaw_linear((int)(bits & 0xFFu)));
}
constexpr int pause_silence(int encoding) { return encoding == LVX_PCM_ULAW ? 0xFF : encoding == LVX_PCM_ALAW ? 0xD5 : 0; }
inline bool pause_loud_of(int encoding, uint32_t bits) {
  return encoding == LVX_PCM_F32LE   ? pause_loud<LVX_PCM_F32LE>(bits)
         : encoding == LVX_PCM_S16LE ? pause_loud<LVX_PCM_S16LE>(bits)
         : encoding == LVX_PCM_ULAW  ? pause_loud<LVX_PCM_ULAW>(bits)
                                     : pause_loud<LVX_PCM_ALAW>(bits);
}

// lvx_pause_slots: the slots of blocks j0 .. j1 - 1 of the finished sentence y (T encoded samples), serially. Their
// bytes, or LVX_E_ARG (a bad rate or encoding, a null pointer, T < 0, blocks outside 0 <= j0 <= j1 <= ceil(T / bl)) or
// LVX_E_CAPACITY (cap smaller than the slots; nothing is written)
inline long long pause_slots(int rate, int encoding, const void* y, long long T, long long j0, long long j1, uint8_t* out,
                             long long cap) {
  const int bl = pause_block(rate), bps = pcm_sample_bytes(encoding);
  if (!bl || !bps || T < 0 || cap < 0 || j0 < 0 || j1 < j0 || j1 > pause_blocks_upto(bl, T, true)) return LVX_E_ARG;
  if (j1 > j0 && (!y || !out)) return LVX_E_ARG;
  const long long slot = pause_slot_bytes(bl, bps);
  if ((j1 - j0) * slot > cap) return LVX_E_CAPACITY;
  const uint8_t* src = static_cast<const uint8_t*>(y);
  const long long blocks = pause_blocks_upto(bl, T, true);
  for (long long j = j0; j < j1; ++j) {
    uint8_t* s = out + (j - j0) * slot;
    const int n = (int)std::min<long long>(bl, T - j * bl);
    bool active = false;
    for (int i = 0; i < n; ++i) {
      uint32_t bits = 0;
      for (int k = 0; k < bps; ++k) bits |= (uint32_t)src[((size_t)j * bl + i) * bps + k] << (8 * k);
      active = active || pause_loud_of(encoding, bits);
    }
    const uint8_t rec[8] = {(uint8_t)n, (uint8_t)(n >> 8), (uint8_t)active, (uint8_t)(j == blocks - 1), 0, 0, 0, 0};
    std::copy(rec, rec + 8, s);
    std::copy(src + (size_t)j * bl * bps, src + ((size_t)j * bl + n) * bps, s + 8);
    std::fill(s + 8 + (size_t)n * bps, s + slot, (uint8_t)pause_silence(encoding));
  }
  return (j1 - j0) * slot;
}

// ---- PCM FLAC: the frame cuts, the subframe's selection arithmetic and the host side of a frame (llmvox.h) ----
// The constexpr functions are the one statement of the cuts, the folding, the partition order, a difference and the
// cost of a Rice parameter that pcm_flac_kernel and the host entries below both call, as g711_ulaw is shared.
constexpr int flac_block(int rate) {  // BS = rate / 25 (40 ms); 0: not a rate of the stage
  return rate == 8000 || rate == 16000 || rate == 24000 || rate == 48000 ? rate / 25 : 0;
}
constexpr int flac_rate_code(int rate) { return rate == 8000 ? 4 : rate == 16000 ? 5 : rate == 24000 ? 7 : 10; }
constexpr int flac_slot_bytes(int bs) { return (8 + 1 + 2 * (bs + 15) + 15) / 16 * 16; }
static_assert(flac_slot_bytes(flac_block(8000)) == LVX_FLAC_SLOT(8000) && flac_slot_bytes(FLAC_MAX_BS) == LVX_FLAC_SLOT(48000), "");
// whole frames of BS a segment of T samples has in front of its last frame
constexpr long long flac_full_frames(int bs, long long T) { return T >= 16 ? (T - 16) / bs : 0; }
// frames of a segment emitted once T inputs are consumed: after a non-final call the whole ones; a final call adds
// the frame of the remaining T - k BS samples
constexpr long long flac_frames_upto(int bs, long long T, bool final) {
  return flac_full_frames(bs, T) + (final && T > 0 ? 1 : 0);
}
constexpr unsigned flac_fold(int r) { return r >= 0 ? 2u * (unsigned)r : 2u * (unsigned)(-r) - 1u; }
constexpr int flac_partition_order(int n) {  // n >= 1
  int P = __builtin_ctz((unsigned)n) < 3 ? __builtin_ctz((unsigned)n) : 3;
  while (P > 0 && (n >> P) < 16) --P;
  return P;
}
// the p-th difference at a sample: x[i], x[i - 1], .. x[i - 4] (those beyond p are not read)
constexpr int flac_diff(int p, int a, int b, int c, int d, int e) {
  return p == 0 ? a : p == 1 ? a - b : p == 2 ? a - 2 * b + c : p == 3 ? a - 3 * b + 3 * c - d : a - 4 * b + 6 * c - 4 * d + e;
}
constexpr unsigned flac_rice_bits(unsigned u, int k) { return (u >> k) + 1u + (unsigned)k; }  // of one folded residual
constexpr int FLAC_MAX_K = 14;

// CRC-8 (polynomial 0x07) and CRC-16 (0x8005), initial value 0, not reflected: the tables
struct FlacCrc {
  uint8_t t8[256];
  uint16_t t16[256];
  constexpr FlacCrc() : t8{}, t16{} {
    for (int i = 0; i < 256; ++i) {
      unsigned a = (unsigned)i, b = (unsigned)i << 8;
      for (int k = 0; k < 8; ++k) {
        a = (a & 0x80u) ? ((a << 1) ^ 0x07u) & 0xFFu : (a << 1) & 0xFFu;
        b = (b & 0x8000u) ? ((b << 1) ^ 0x8005u) & 0xFFFFu : (b << 1) & 0xFFFFu;
      }
      t8[i] = (uint8_t)a;
      t16[i] = (uint16_t)b;
    }
  }
};
inline constexpr FlacCrc kFlacCrc{};
inline unsigned flac_crc8(const uint8_t* p, size_t n) {
  unsigned c = 0;
  for (size_t i = 0; i < n; ++i) c = kFlacCrc.t8[c ^ p[i]];
  return c;
}
inline unsigned flac_crc16(const uint8_t* p, size_t n) {
  unsigned c = 0;
  for (size_t i = 0; i < n; ++i) c = ((c << 8) & 0xFFFFu) ^ kFlacCrc.t16[(c >> 8) ^ p[i]];
  return c;
}

// bits MSB first into a byte vector, zero-padded to a byte
struct FlacBits {
  std::vector<uint8_t> bytes;
  int free_bits = 0;  // unused low bits of the last byte
  void put(unsigned v, int len) {  // the low len bits of v, len <= 32
    for (int i = len - 1; i >= 0; --i) {
      if (free_bits == 0) {
        bytes.push_back(0);
        free_bits = 8;
      }
      --free_bits;
      bytes.back() |= (uint8_t)(((v >> i) & 1u) << free_bits);
    }
  }
  void zeros(unsigned n) {
    for (; n > 0; --n) put(0, 1);
  }
};

// lvx_flac_subframe: the subframe of x[0 .. n) by llmvox.h's rule, serially. Its bytes, or LVX_E_ARG (n outside
// 1 .. 65535, a null pointer) or LVX_E_CAPACITY (cap smaller than the subframe; nothing is written)
inline int flac_subframe(const int16_t* x, int n, uint8_t* out, int cap) {
  if (n < 1 || n > FLAC_MAX_N || !x || !out || cap < 0) return LVX_E_ARG;
  FlacBits w;
  bool same = true;
  for (int i = 1; i < n; ++i) same = same && x[i] == x[0];
  if (same) {
    w.put(0x00, 8);
    w.put((uint16_t)x[0], 16);
  } else {
    auto diff = [&](int p, int i) {
      return flac_diff(p, x[i], i >= 1 ? x[i - 1] : 0, i >= 2 ? x[i - 2] : 0, i >= 3 ? x[i - 3] : 0, i >= 4 ? x[i - 4] : 0);
    };
    int p = 0;
    unsigned long long best = ~0ull;
    for (int q = 0; q <= 4; ++q) {
      unsigned long long e = 0;
      for (int i = 4; i < n; ++i) e += (unsigned long long)std::abs(diff(q, i));
      if (e < best) {
        best = e;
        p = q;
      }
    }
    const int P = flac_partition_order(n), psize = n >> P;
    std::vector<unsigned> u(n, 0);
    for (int i = p; i < n; ++i) u[i] = flac_fold(diff(p, i));
    int ks[8];
    unsigned long long bits = 8 + 16ull * p + 2 + 4;
    for (int j = 0; j < (1 << P); ++j) {
      const int lo = std::max(p, j * psize), hi = (j + 1) * psize;
      unsigned long long least = ~0ull;
      for (int k = 0; k <= FLAC_MAX_K; ++k) {
        unsigned long long c = 0;
        for (int i = lo; i < hi; ++i) c += flac_rice_bits(u[i], k);
        if (c < least) {
          least = c;
          ks[j] = k;
        }
      }
      bits += 4 + least;
    }
    if (bits >= 8 + 16ull * n) {
      w.put(0x02, 8);
      for (int i = 0; i < n; ++i) w.put((uint16_t)x[i], 16);
    } else {
      w.put((8u | (unsigned)p) << 1, 8);
      for (int i = 0; i < p; ++i) w.put((uint16_t)x[i], 16);
      w.put(0, 2);
      w.put((unsigned)P, 4);
      for (int j = 0; j < (1 << P); ++j) {
        const int k = ks[j];
        w.put((unsigned)k, 4);
        for (int i = std::max(p, j * psize); i < (j + 1) * psize; ++i) {
          w.zeros(u[i] >> k);
          w.put(1, 1);
          w.put(u[i] & ((1u << k) - 1u), k);
        }
      }
    }
  }
  if ((size_t)cap < w.bytes.size()) return LVX_E_CAPACITY;
  std::copy(w.bytes.begin(), w.bytes.end(), out);
  return (int)w.bytes.size();
}

// lvx_flac_stream_header: "fLaC" and the one STREAMINFO block, 42 bytes; false: not a rate of the stage
inline bool flac_stream_header(int rate, uint8_t* out) {
  const int bs = flac_block(rate);
  if (!bs || !out) return false;
  const uint8_t head[8] = {'f', 'L', 'a', 'C', 0x80, 0, 0, 34};
  std::fill(out, out + 42, (uint8_t)0);
  std::copy(head, head + 8, out);
  out[8] = 0;
  out[9] = 16;  // min blocksize
  out[10] = (uint8_t)((bs + 15) >> 8);
  out[11] = (uint8_t)(bs + 15);  // max blocksize; the frame sizes stay 0 (unknown)
  // sample rate (20 bits), channels - 1 (3), bits per sample - 1 (5), total samples (36, 0: unknown)
  const unsigned long long v = ((unsigned long long)rate << 44) | (15ull << 36);
  for (int i = 0; i < 8; ++i) out[18 + i] = (uint8_t)(v >> (56 - 8 * i));
  return true;  // the MD5 stays 0 (unknown)
}

// the sample number in FLAC's UTF-8-like coding (1 .. 7 bytes for a number below 2^36); its length
inline int flac_utf8(unsigned long long v, uint8_t* out) {
  if (v < 0x80) {
    out[0] = (uint8_t)v;
    return 1;
  }
  int len = 2;  // bytes: the first carries 7 - len bits (none at len 7), the others 6 each
  while (len < 7 && v >= (1ull << (5 * len + 1))) ++len;
  out[0] = (uint8_t)((0xFF00u >> len) & 0xFFu) | (uint8_t)(len < 7 ? v >> (6 * (len - 1)) : 0);
  for (int i = 1; i < len; ++i) out[i] = (uint8_t)(0x80u | ((v >> (6 * (len - 1 - i))) & 0x3Fu));
  return len;
}

// lvx_flac_finish: the n_frames slots the device wrote (records and subframes) made frames, the first at sample
// number *sample_no. Bytes written, or LVX_E_ARG (a bad rate, a null pointer, n_frames < 0, a sample number past 2^36,
// a record that is none of the stage's) or LVX_E_CAPACITY (cap too small): then nothing is written and *sample_no stays.
inline long long flac_finish(int rate, const uint8_t* slots, int n_frames, unsigned long long* sample_no, uint8_t* out,
                             long long cap) {
  const int bs = flac_block(rate);
  if (!bs || n_frames < 0 || !sample_no || cap < 0 || (n_frames > 0 && (!slots || !out))) return LVX_E_ARG;
  const int slot = flac_slot_bytes(bs);
  unsigned long long no = *sample_no;
  long long need = 0;
  for (int f = 0; f < n_frames; ++f) {
    const uint8_t* s = slots + (size_t)f * slot;
    const int n = s[0] | (s[1] << 8), body = s[2] | (s[3] << 8);
    if (n < 1 || n > bs + 15 || body < 3 || body > 1 + 2 * n || (s[4] | s[5] | s[6] | s[7]) || no + n > (1ull << 36)) return LVX_E_ARG;
    uint8_t num[7];
    need += 4 + flac_utf8(no, num) + 3 + body + 2;
    no += n;
  }
  if (need > cap) return LVX_E_CAPACITY;
  no = *sample_no;
  uint8_t* o = out;
  for (int f = 0; f < n_frames; ++f) {
    const uint8_t* s = slots + (size_t)f * slot;
    const int n = s[0] | (s[1] << 8), body = s[2] | (s[3] << 8);
    uint8_t* h = o;
    *o++ = 0xFF;
    *o++ = 0xF9;
    *o++ = (uint8_t)(0x70 | flac_rate_code(rate));
    *o++ = 0x08;
    o += flac_utf8(no, o);
    *o++ = (uint8_t)((n - 1) >> 8);
    *o++ = (uint8_t)(n - 1);
    *o = (uint8_t)flac_crc8(h, (size_t)(o - h));
    ++o;
    o = std::copy(s + 8, s + 8 + body, o);
    const unsigned c = flac_crc16(h, (size_t)(o - h));
    *o++ = (uint8_t)(c >> 8);
    *o++ = (uint8_t)c;
    no += n;
  }
  *sample_no = no;
  return need;
}

// ---------------- the skeleton of a stage's call ----------------
// A stage keeps one record per slot, the host mirror of the slot's open segment, and two history buffers per slot in a
// device pool [2][slots][hist]: a call reads the current one and writes the other, so no launch reads what it writes.
struct PcmSeg {
  static constexpr long long NONE = -1;  // no segment open (not 0: 0 is a volume)
  long long t0 = 0;      // inputs of the segment consumed so far
  long long aux = 0;     // the work of its calls so far in the stage's unit (row_work; the stretch's hops emitted)
  long long key = NONE;  // the parameter the segment is open at: rate, speed, ratio_key, volume; the join has none (0)
  uint8_t par = 0;       // which of the slot's two buffers is current: outlives the segment and lvx_pcm_reset
  void close() {
    t0 = aux = 0;
    key = NONE;
  }
};
inline long long ratio_key(int L, int M) { return ((long long)L << 16) | M; }

// what a stage's planning function is given for one row of a call
struct PcmCall {
  const PcmSeg& seg;
  bool final;
  int cur, other;  // float offsets of the slot's current and other buffer in the stage's pool
  int slot, row;
};

// a row's work in its stage's unit, and where it keeps a history (-1: nowhere)
template <class Row> int row_work(const Row& r) { return r.n_out; }
inline int row_work(const StretchRow& r) { return r.n_hops; }
template <class Row> int row_kept(const Row& r) { return r.hist_out; }
inline int row_kept(const JoinRow& r) { return r.tail_out; }

// The part of a call under the context's lock; returns the error's text, empty when the call went through. Per row, in
// this order: the slot's range, a slot named twice, a segment open at another key (key_text(key) names it), then
// plan(PcmCall, Row&), the stage's own checks and its kernel row. Only when every row has passed do the records move
// and n_out_host fill: a final row closes its segment; any other, where the call advances (an identity call of the
// stretch, the ratio or the level does not), consumes n_in, takes the key and turns to the other buffer if the row
// keeps a history there.
template <class Row, class KeyText, class Plan>
std::string pcm_plan(std::vector<PcmSeg>& segs, int hist, int B, int n_in, const int32_t* slots, const uint8_t* final_host,
                     int32_t* n_out_host, long long key, bool advance, KeyText key_text, std::vector<Row>& rows, Plan plan) {
  const int S = (int)segs.size();
  rows.assign(B, Row{});
  std::vector<uint8_t> seen(S, 0);
  for (int b = 0; b < B; ++b) {
    const int s = slots[b];
    if (s < 0 || s >= S) return "slot out of range";
    if (seen[s]) return "slot " + std::to_string(s) + " named twice in one call";
    seen[s] = 1;
    const PcmSeg& g = segs[s];
    if (g.key != PcmSeg::NONE && g.key != key) return "slot " + std::to_string(s) + ": its segment is open at " + key_text(g.key);
    const std::string e = plan(PcmCall{g, final_host[b] != 0, (g.par * S + s) * hist, ((1 - g.par) * S + s) * hist, s, b}, rows[b]);
    if (!e.empty()) return e;
  }
  for (int b = 0; b < B; ++b) {
    PcmSeg& g = segs[slots[b]];
    n_out_host[b] = rows[b].n_out;
    if (final_host[b]) {
      g.close();
    } else if (advance) {
      g.t0 += n_in;
      g.aux += row_work(rows[b]);
      g.key = key;
      if (row_kept(rows[b]) >= 0) g.par ^= 1;
    }
  }
  return {};
}

// The part after the lock is dropped: the rows in packets of PCM_ROWS, launch(packet, rows, the most outputs of one);
// a packet none of whose rows has work or keeps a history (a flush with nothing left) is not launched.
template <class Rows, class Row, class Launch>
void pcm_chunks(const std::vector<Row>& rows, Launch launch) {
  const int B = (int)rows.size();
  for (int b0 = 0; b0 < B; b0 += PCM_ROWS) {
    const int nr = std::min(PCM_ROWS, B - b0);
    Rows pk{};
    int max_out = 0;
    bool any = false;
    for (int k = 0; k < nr; ++k) {
      pk.r[k] = rows[b0 + k];
      max_out = std::max(max_out, pk.r[k].n_out);
      any = any || row_work(pk.r[k]) > 0 || row_kept(pk.r[k]) >= 0;
    }
    if (any) launch(pk, nr, max_out);
  }
}

// ---------------- the stages' planning functions ----------------
inline std::string stride_msg(const char* what, long long stride, long long bytes) {
  return std::string(what) + " " + std::to_string(stride) + " is smaller than a row's output (" + std::to_string(bytes) + " bytes)";
}

// the row of a stage whose outputs are a closed form upto(T, final) of the inputs consumed (rate, ratio, level);
// filtered: the stage has a history to keep for the segment's next call
template <class Row, class Upto>
std::string plan_counted(const PcmCall& c, int n_in, Upto upto, bool filtered, bool check_stride, int bps, long long out_stride,
                         Row& r) {
  const long long t0 = c.seg.t0, m0 = upto(t0, false), m1 = upto(t0 + n_in, c.final);
  if (m1 - m0 > (1ll << 30)) return "n_in too large";
  if (check_stride && (m1 - m0) * bps > out_stride) return stride_msg("out_stride_bytes", out_stride, (m1 - m0) * bps);
  r.t0 = t0;
  r.m0 = m0;
  r.n_out = (int)(m1 - m0);
  r.hist_in = c.cur;
  r.hist_out = filtered && n_in > 0 && !c.final ? c.other : -1;
  r.row = c.row;
  return {};
}

// launch false (24 kHz f32le): the rows are the output and no stride is asked for, but the segment advances all the same
inline std::string plan_convert(const PcmCall& c, int n_in, const PcmRate& pr, int bps, bool launch, long long out_stride, PcmRow& r) {
  return plan_counted(c, n_in, [&](long long T, bool f) { return pcm_emitted_upto(pr, T, f); }, pr.N > 0, launch, bps, out_stride, r);
}

inline std::string plan_ratio(const PcmCall& c, int n_in, int L, int M, long long out_stride, RatioRow& r) {
  const int N = ratio_N(L, M);
  r = RatioRow{0, 0, n_in, 0, -1, c.row, 0};
  if (N == 0) return {};  // 1 / 1: the rows of pcm_dev are the output
  r.taps = c.slot * RAT_TAPS_STRIDE;
  return plan_counted(c, n_in, [&](long long T, bool f) { return pcm_emitted_upto(L, M, N, T, f); }, true, true, 4, out_stride, r);
}

inline std::string plan_level(const PcmCall& c, int n_in, int pct, long long out_stride, bool want_g, long long g_stride, PcmRow& r) {
  r = PcmRow{0, 0, n_in, 0, -1, c.row};
  if (pct == 100) return {};  // the rows of pcm_dev are the output
  std::string e = plan_counted(c, n_in, [&](long long T, bool f) { return level_emitted_upto(pct, T, f); }, true, true, 4, out_stride, r);
  if (e.empty() && want_g && r.n_out * 4ll > g_stride) e = stride_msg("g_stride_bytes", g_stride, r.n_out * 4ll);
  return e;
}

inline std::string plan_formant(const PcmCall& c, int n_in, int Fn, int Fd, long long out_stride, PcmRow& r) {
  r = PcmRow{0, 0, n_in, 0, -1, c.row};
  if (Fn == Fd) return {};  // 1 / 1: the rows of pcm_dev are the output
  return plan_counted(c, n_in, [&](long long T, bool f) { return formant_emitted_upto(T, f); }, true, true, 4, out_stride, r);
}

// the formant stage's counts and history; every call launches (there is no identity mark)
inline std::string plan_mark(const PcmCall& c, int n_in, long long out_stride, PcmRow& r) {
  return plan_counted(c, n_in, [&](long long T, bool f) { return formant_emitted_upto(T, f); }, true, true, 4, out_stride, r);
}

inline std::string plan_stretch(const PcmCall& c, int n_in, int pct, long long out_stride, bool want_d, int d_stride, StretchRow& r) {
  r = StretchRow{0, 0, 0, n_in, 0, -1, c.slot, c.row};
  if (pct == 100) return {};  // the rows of pcm_dev are the output
  const long long t0 = c.seg.t0, j0 = c.seg.aux;
  const long long m1 = stretch_emitted_upto(pct, t0 + n_in, c.final);
  const long long n_out = std::max(0ll, m1 - j0 * STR_H), hops = (n_out + STR_H - 1) / STR_H;
  if (n_out > (1ll << 30)) return "n_in too large";
  if (n_out * 4 > out_stride) return stride_msg("out_stride_bytes", out_stride, n_out * 4);
  if (want_d && hops > d_stride)
    return "d_stride " + std::to_string(d_stride) + " is smaller than a row's hops (" + std::to_string(hops) + ")";
  r = StretchRow{t0, j0, (int)hops, (int)n_out, c.cur, n_in > 0 && !c.final ? c.other : -1, c.slot, c.row};
  return {};
}

// no key, and every call that is not final keeps a tail (so it always advances and always turns the buffers)
inline std::string plan_join(const PcmCall& c, int n_in, int ctx_frames, long long out_stride, JoinRow& r) {
  const bool open = c.seg.key != PcmSeg::NONE;
  const int n_out = join_emitted(open, ctx_frames, n_in, c.final);
  if (n_out < 0) return "slot " + std::to_string(c.slot) + ": " + join_msg(open, ctx_frames, n_in, c.final);
  if (n_out * 4ll > out_stride) return stride_msg("out_stride_bytes", out_stride, n_out * 4ll);
  r = JoinRow{JOIN_HOLD * ctx_frames, !open ? JOIN_HEAD_NONE : ctx_frames > 0 ? JOIN_HEAD_FADE : JOIN_HEAD_TAIL, n_out, c.cur,
              c.final ? -1 : c.other, c.row};
  return {};
}

// the key is the rate; every call that brings samples keeps the ones no frame has taken (so it turns the buffers)
inline std::string plan_flac(const PcmCall& c, int n_in, int rate, long long in_stride, long long out_stride, FlacRow& r) {
  const int bs = flac_block(rate);
  if (n_in * 2ll > in_stride) return stride_msg("in_stride_bytes", in_stride, n_in * 2ll);
  const long long t0 = c.seg.t0, j0 = flac_frames_upto(bs, t0, false), j1 = flac_frames_upto(bs, t0 + n_in, c.final);
  if ((j1 - j0) * flac_slot_bytes(bs) > out_stride) return stride_msg("out_stride_bytes", out_stride, (j1 - j0) * flac_slot_bytes(bs));
  const long long last = c.final ? t0 + n_in - flac_full_frames(bs, t0 + n_in) * bs : bs;
  r = FlacRow{t0, j0, (int)(j1 - j0), (int)last, c.cur, n_in > 0 && !c.final ? c.other : -1, c.row};
  return {};
}

// the key is (rate, encoding); every call that brings samples keeps the ones no block has taken (so it turns the
// buffers). *capacity: the error is out_stride's (LVX_E_CAPACITY, not LVX_E_ARG)
constexpr long long pause_key(int rate, int encoding) { return ((long long)rate << 8) | encoding; }
inline std::string plan_pause(const PcmCall& c, int n_in, int rate, int encoding, long long in_stride, long long out_stride,
                              bool* capacity, PauseRow& r) {
  const int bl = pause_block(rate), bps = pcm_sample_bytes(encoding);
  if ((long long)n_in * bps > in_stride) return stride_msg("in_stride_bytes", in_stride, (long long)n_in * bps);
  const long long t0 = c.seg.t0, j0 = pause_blocks_upto(bl, t0, false), j1 = pause_blocks_upto(bl, t0 + n_in, c.final);
  if ((j1 - j0) * pause_slot_bytes(bl, bps) > out_stride) {
    *capacity = true;
    return stride_msg("out_stride_bytes", out_stride, (j1 - j0) * pause_slot_bytes(bl, bps));
  }
  const long long last = c.final && j1 > 0 ? t0 + n_in - (j1 - 1) * bl : bl;
  r = PauseRow{t0, j0, (int)(j1 - j0), (int)last, c.cur, n_in > 0 && !c.final ? c.other : -1, c.row, c.final ? 1 : 0};
  return {};
}

}  // namespace lvx
