// PCM output stage (include/llmvox.h, "PCM output stage"): rational polyphase resampling of the codec's
// 24 kHz fp32 rows to 16 / 8 / 48 kHz and the s16le quantisation or, behind it, the G.711 companding
// ("PCM G.711": 8-bit mu-law / A-law), one kernel family templated on (L, M, N, encoding). Launched only
// for a stream that asked for another format than f32le at 24 kHz.
// And the speaking-rate control in front of it ("PCM time stretch"): WSOLA on the 24 kHz rows, one block
// per row, launched only for a stream that asked for another speed. And the pitch control between the two
// ("PCM pitch shift"): the same polyphase rule with a run-time L / M, launched only for a pitched stream.
// And, in front of all three, the join of a sentence's dumps ("PCM dump join"): a copy that holds back one
// frame and crossfades it with the next dump's rendering of it, launched only for a stream that asked.
// And the volume control between the pitch control and the rate conversion ("PCM level"): a gain and a
// feed-forward peak limiter (a sliding minimum and one fixed-order sum), launched only for a stream at
// another volume than 100. And, behind the rate conversion's s16le rows, the lossless compressed output
// ("PCM FLAC"): one FLAC subframe a workgroup, launched only for a stream that asked for "flac". And the
// formant control between the pitch control and the volume control ("PCM formant"): a short-time Fourier
// correction of the spectral envelope in LDS, launched only for a stream that named a formant. And, last of all, the
// marks of the pause control ("PCM pause"): the encoded rows cut into slots of 10 ms, each marked silent or not,
// launched only for a stream that named a pause. And the watermark between the formant and the volume control ("PCM
// mark"): the formant stage's transform and frame loop under a keyed table of signs, launched only for a marked stream.
#include <algorithm>
#include <type_traits>

#include "lvx_internal.h"

namespace lvx {

namespace {

constexpr int PCM_THREADS = 256;
constexpr int PCM_PER_THREAD = 4;                        // consecutive outputs of a thread: one 4 / 8 / 16 byte store
constexpr int PCM_OB = PCM_THREADS * PCM_PER_THREAD;     // outputs of a block

// q = rint(clamp(v * 32768, -32768, 32767)), half to even (v_rndne_f32), NaN -> 0. v * 32768 is exact
// (or +-inf, which the clamp takes).
__device__ __forceinline__ int pcm_q16(float v) {
  if (v != v) return 0;
  const float s = fminf(fmaxf(__fmul_rn(v, 32768.f), -32768.f), 32767.f);
  return (int)__builtin_rintf(s);
}

__device__ __forceinline__ long long ceil_div(long long a, int d) { return a >= 0 ? (a + d - 1) / d : -((-a) / d); }
__device__ __forceinline__ long long floor_div(long long a, int d) { return a >= 0 ? a / d : -((-a + d - 1) / d); }

// Segment input g (t0 - HIST <= g < t1) of a row: from the call's row x (inputs t0 .. t1 - 1) or the slot's history
// [HIST] (inputs t0 - HIST .. t0 - 1); zero outside the segment
template <int HIST>
struct SegInput {
  const float* __restrict__ x;
  const float* hist;  // the pool; the slot's current buffer at hist_in (the launch writes the other one)
  long long t0, t1;
  int hist_in;
  __device__ __forceinline__ float operator()(long long g) const {
    if (g < 0 || g >= t1) return 0.f;
    if (g >= t0) return x[g - t0];
    const long long back = t0 - g;
    return back <= HIST ? hist[hist_in + HIST - back] : 0.f;
  }
};

// a thread's PCM_PER_THREAD consecutive floats, outputs ml .. of a block's nb: those below nb are stored, as one
// 16-byte store where all are and the address allows
__device__ __forceinline__ void store4(float* o, const float (&v)[PCM_PER_THREAD], int ml, int nb) {
  if (ml + PCM_PER_THREAD <= nb && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < PCM_PER_THREAD; ++e)
      if (ml + e < nb) o[e] = v[e];
  }
}

// The polyphase rule of llmvox.h for output m of the ratio L / M: the prototype h[-N .. N] in s_h; the output's first
// input, ilo = ceil((m M - N) / L), at s_x[k]; its first tap index t = m M - ilo L, in (N - L, N]. Inputs in ascending
// order, each product and each sum rounded to fp32 (no fused multiply-add: the compiler would contract the pair,
// __fmul_rn / __fadd_rn included, without the pragma): the rule's fixed order, which a host evaluation in fp32
// reproduces bit for bit.
__device__ __forceinline__ float polyphase(const float* s_x, const float* s_h, int k, int t, int L, int N) {
  float acc = 0.f;
  for (; t >= -N; t -= L, ++k) {
#pragma clang fp contract(off)
    const float prod = s_x[k] * s_h[t + N];
    acc = acc + prod;
  }
  return acc;
}

// blocks of PCM_OB outputs by the rows of the launch
dim3 pcm_grid(int max_out, int n_rows) {
  return dim3((unsigned)std::max(1, (max_out + PCM_OB - 1) / PCM_OB), (unsigned)n_rows);
}

// Grid (blocks of PCM_OB outputs, rows of the launch). Block (x, y) writes outputs
// [x * PCM_OB, min((x + 1) * PCM_OB, n_out)) of row y's call; block (0, y) also writes the slot's next
// history (into the buffer the launch does not read).
template <int L, int M, int N, int ENC>
__global__ __launch_bounds__(PCM_THREADS) void pcm_convert_kernel(PcmRows rows, const float* __restrict__ pcm, int n_in,
                                                                  const float* __restrict__ taps, float* hist,
                                                                  unsigned char* __restrict__ out, long long out_stride) {
  const PcmRow r = rows.r[blockIdx.y];
  const float* __restrict__ x = pcm + (size_t)r.row * (size_t)n_in;
  const int tid = threadIdx.x;
  const long long t1 = r.t0 + n_in;  // inputs of the segment once this call is consumed
  const SegInput<PCM_HIST> input{x, hist, r.t0, t1, r.hist_in};
  if (N > 0 && blockIdx.x == 0 && r.hist_out >= 0 && tid < PCM_HIST) hist[r.hist_out + tid] = input(t1 - PCM_HIST + tid);

  const int mb = blockIdx.x * PCM_OB;
  if (mb >= r.n_out) return;
  const int nb = min(PCM_OB, r.n_out - mb);
  const int ml = tid * PCM_PER_THREAD;  // the thread's first output within the block
  float v[PCM_PER_THREAD];

  if constexpr (N == 0) {  // no filter: elementwise
#pragma unroll
    for (int e = 0; e < PCM_PER_THREAD; ++e) v[e] = ml + e < nb ? x[mb + ml + e] : 0.f;
  } else {
    constexpr int SPAN = ((PCM_OB - 1) * M + 2 * N) / L + 3;
    __shared__ float s_h[2 * N + 1];
    __shared__ float s_x[SPAN];
    for (int k = tid; k < 2 * N + 1; k += PCM_THREADS) s_h[k] = taps[k];
    const long long m_first = r.m0 + mb;
    const long long i0 = ceil_div(m_first * M - N, L);
    const int span = (int)(floor_div((m_first + nb - 1) * M + N, L) - i0) + 1;  // <= SPAN
    for (int k = tid; k < span && k < SPAN; k += PCM_THREADS) s_x[k] = input(i0 + k);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < PCM_PER_THREAD; ++e) {
      float acc = 0.f;
      if (ml + e < nb) {
        // (the division by L stays here, where L is the template's constant: inside polyphase() the L = 2 kernels
        // came out eight instructions longer and 0.1 us slower)
        const long long mm = (m_first + ml + e) * M;
        const long long ilo = ceil_div(mm - N, L);  // the output's first input
        acc = polyphase(s_x, s_h, (int)(ilo - i0), (int)(mm - ilo * L), L, N);
      }
      v[e] = acc;
    }
  }

  unsigned char* orow = out + (size_t)r.row * (size_t)out_stride;
  if constexpr (ENC == LVX_PCM_S16LE) {
    int16_t* o = reinterpret_cast<int16_t*>(orow) + mb + ml;
    if (ml + PCM_PER_THREAD <= nb && (reinterpret_cast<uintptr_t>(o) & 7) == 0) {
      uint2 w;
      w.x = (uint32_t)(uint16_t)pcm_q16(v[0]) | ((uint32_t)(uint16_t)pcm_q16(v[1]) << 16);
      w.y = (uint32_t)(uint16_t)pcm_q16(v[2]) | ((uint32_t)(uint16_t)pcm_q16(v[3]) << 16);
      *reinterpret_cast<uint2*>(o) = w;
    } else {
#pragma unroll
      for (int e = 0; e < PCM_PER_THREAD; ++e)
        if (ml + e < nb) o[e] = (int16_t)pcm_q16(v[e]);
    }
  } else if constexpr (is_g711(ENC)) {
    // llmvox.h, "PCM G.711": the s16 quantisation, then the companding in integer ops (pcm_host.h's statement of it,
    // the one the host entries run). A thread's four codes are one dword: its address is 4-aligned by construction
    // (the row base and the stride are multiples of 4, and so is mb + ml).
    uint8_t* o = orow + mb + ml;
    if (ml + PCM_PER_THREAD <= nb) {
      *reinterpret_cast<uint32_t*>(o) = (uint32_t)g711_code<ENC>(pcm_q16(v[0])) | ((uint32_t)g711_code<ENC>(pcm_q16(v[1])) << 8) |
                                        ((uint32_t)g711_code<ENC>(pcm_q16(v[2])) << 16) | ((uint32_t)g711_code<ENC>(pcm_q16(v[3])) << 24);
    } else {
#pragma unroll
      for (int e = 0; e < PCM_PER_THREAD; ++e)
        if (ml + e < nb) o[e] = (uint8_t)g711_code<ENC>(pcm_q16(v[e]));
    }
  } else {
    store4(reinterpret_cast<float*>(orow) + mb + ml, v, ml, nb);
  }
}

template <int L, int M, int N>
void launch_enc(const PcmRows& rows, int n_rows, int max_out, int enc, const float* pcm, int n_in, const float* taps,
                float* hist, void* out, long long out_stride, hipStream_t s) {
  const dim3 grid = pcm_grid(max_out, n_rows);
  if (enc == LVX_PCM_S16LE)
    pcm_convert_kernel<L, M, N, LVX_PCM_S16LE><<<grid, PCM_THREADS, 0, s>>>(rows, pcm, n_in, taps, hist,
                                                                            (unsigned char*)out, out_stride);
  else if (enc == LVX_PCM_ULAW)
    pcm_convert_kernel<L, M, N, LVX_PCM_ULAW><<<grid, PCM_THREADS, 0, s>>>(rows, pcm, n_in, taps, hist,
                                                                           (unsigned char*)out, out_stride);
  else if (enc == LVX_PCM_ALAW)
    pcm_convert_kernel<L, M, N, LVX_PCM_ALAW><<<grid, PCM_THREADS, 0, s>>>(rows, pcm, n_in, taps, hist,
                                                                           (unsigned char*)out, out_stride);
  else
    pcm_convert_kernel<L, M, N, LVX_PCM_F32LE><<<grid, PCM_THREADS, 0, s>>>(rows, pcm, n_in, taps, hist,
                                                                            (unsigned char*)out, out_stride);
}

// ---- PCM pitch shift (llmvox.h, "PCM pitch shift"): the resampler of a run-time ratio L / M ----
// pcm_convert_kernel's rule, packet and grid with L, M, N as arguments, f32 in and out. The slot's table
// h[-N .. N] (its own region of the table pool) and the block's input span go to LDS: a block of PCM_OB
// outputs touches every phase of the table.
constexpr int RAT_SPAN = (PCM_OB - 1) * 4 + 2 * 24 * 4 + 3;  // inputs of a block at M = 4 L, the most the entry admits

__global__ __launch_bounds__(PCM_THREADS) void pcm_ratio_kernel(RatioRows rows, int L, int M, int N,
                                                                const float* __restrict__ pcm, int n_in,
                                                                const float* __restrict__ taps, float* hist,
                                                                unsigned char* __restrict__ out, long long out_stride) {
  const RatioRow r = rows.r[blockIdx.y];
  const float* __restrict__ x = pcm + (size_t)r.row * (size_t)n_in;
  const int tid = threadIdx.x;
  const long long t1 = r.t0 + n_in;  // inputs of the segment once this call is consumed
  const SegInput<RAT_HIST> input{x, hist, r.t0, t1, r.hist_in};
  if (blockIdx.x == 0 && r.hist_out >= 0 && tid < RAT_HIST) hist[r.hist_out + tid] = input(t1 - RAT_HIST + tid);

  const int mb = blockIdx.x * PCM_OB;
  if (mb >= r.n_out) return;
  const int nb = min(PCM_OB, r.n_out - mb);
  const int ml = tid * PCM_PER_THREAD;  // the thread's first output within the block

  __shared__ float s_h[RAT_TAPS];
  __shared__ float s_x[RAT_SPAN];
  const float* __restrict__ h = taps + r.taps;
  const int n_taps = min(2 * N + 1, RAT_TAPS);
  for (int k = tid; k < n_taps; k += PCM_THREADS) s_h[k] = h[k];
  const long long m_first = r.m0 + mb;
  const long long i0 = ceil_div(m_first * M - N, L);
  const int span = (int)(floor_div((m_first + nb - 1) * M + N, L) - i0) + 1;  // <= RAT_SPAN while M <= 4 L
  for (int k = tid; k < span && k < RAT_SPAN; k += PCM_THREADS) s_x[k] = input(i0 + k);
  __syncthreads();
  float v[PCM_PER_THREAD];
#pragma unroll
  for (int e = 0; e < PCM_PER_THREAD; ++e) {
    float acc = 0.f;
    if (ml + e < nb) {
      const long long mm = (m_first + ml + e) * M;
      const long long ilo = ceil_div(mm - N, L);  // the output's first input
      acc = polyphase(s_x, s_h, (int)(ilo - i0), (int)(mm - ilo * L), L, N);
    }
    v[e] = acc;
  }
  store4(reinterpret_cast<float*>(out + (size_t)r.row * (size_t)out_stride) + mb + ml, v, ml, nb);
}

// ---- PCM time stretch (llmvox.h, "PCM time stretch"): WSOLA on the 24 kHz rows ----
constexpr int STR_THREADS = 256;             // two adjacent candidates d per thread: 2 D + 1 = 481 of them
constexpr int STR_CAND = 2 * STR_D + 1;
constexpr int STR_SPAN = 2 * STR_D + STR_C;  // inputs the candidates of one hop cover
static_assert(STR_CAND <= 2 * STR_THREADS && STR_H <= STR_THREADS, "two candidates per thread");
typedef float str_f2 __attribute__((ext_vector_type(2)));

// fp32 -> unsigned with the same order (no NaN comes here; -0 has been made +0)
__device__ __forceinline__ unsigned str_ordered(float s) {
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One block per row walks the row's hops in order (hop j starts from p_{j-1}). Per hop: the candidate span
// x[a_j - D .. a_j + D + C) and the template x[e_j .. e_j + C) go to LDS; thread i runs the two
// sequential sums of the candidates d = 2 i - D and d + 1 side by side, as the two halves of packed fp32
// multiplies and adds (each half is the candidate's own rounded product and rounded sum, in the rule's
// order; the template word is a broadcast); a block arg-max on (score, -rank), rank = 2 |d| + (d > 0);
// then the H outputs.
__global__ __launch_bounds__(STR_THREADS) void pcm_stretch_kernel(StretchRows rows, int pct,
                                                                  const float* __restrict__ pcm, int n_in,
                                                                  const float* __restrict__ win, float* hist,
                                                                  int* dstate, unsigned char* __restrict__ out,
                                                                  long long out_stride, int* __restrict__ d_out,
                                                                  int d_stride) {
  const StretchRow r = rows.r[blockIdx.x];
  const float* __restrict__ x = pcm + (size_t)r.row * (size_t)n_in;
  const int tid = threadIdx.x;
  const long long t1 = r.t0 + n_in;  // inputs of the segment once this call is consumed
  // segment input g from the call's row or the slot's history; zero outside the segment. Its own form, not
  // SegInput: without a branch (an input outside loads a word of the window table and drops it), so that the
  // loads of a hop's staging are all in flight together: a hop waits for one memory latency, not for six in turn.
  auto input = [&](long long g) -> float {
    const long long back = r.t0 - g;
    const bool in_row = g >= r.t0 && g < t1, in_hist = g >= 0 && back >= 1 && back <= STR_HIST;
    const float* src = in_row ? x + (g - r.t0) : in_hist ? hist + (r.hist_in + STR_HIST - back) : win;
    const float v = *src;
    return (in_row || in_hist) ? v : 0.f;
  };
  if (r.hist_out >= 0)
    for (int i = tid; i < STR_HIST; i += STR_THREADS) hist[r.hist_out + i] = input(t1 - STR_HIST + i);
  if (r.n_hops <= 0) return;

  // both padded to whole rounds of the block's staging (the pad holds the inputs that follow; the 482nd,
  // unused, candidate's last step reads s_c[STR_SPAN])
  constexpr int SC = (STR_SPAN + STR_THREADS) / STR_THREADS * STR_THREADS, ST = (STR_C + STR_THREADS - 1) / STR_THREADS * STR_THREADS;
  __shared__ float s_c[SC];
  __shared__ float s_t[ST];
  __shared__ float s_wr[STR_H], s_wf[STR_H];
  __shared__ unsigned s_hi[STR_THREADS / 64], s_lo[STR_THREADS / 64];
  if (tid < STR_H) {
    s_wr[tid] = win[tid];
    s_wf[tid] = win[STR_H + tid];
  }
  // p_{j0 - 1} = a_{j0 - 1} + d_{j0 - 1}: the slot keeps the d (a new segment starts from p_{-1} = -H)
  long long p_prev = r.j0 == 0 ? -STR_H : ((r.j0 - 1) * STR_H * pct) / 100 + dstate[r.slot];
  float* __restrict__ orow = reinterpret_cast<float*>(out + (size_t)r.row * (size_t)out_stride);
  int d = 0;
  for (int h = 0; h < r.n_hops; ++h) {
    const long long j = r.j0 + h;
    const long long a = (j * STR_H * pct) / 100, e = p_prev + STR_H;
    float vc[SC / STR_THREADS], vt[ST / STR_THREADS];
#pragma unroll
    for (int u = 0; u < SC / STR_THREADS; ++u) vc[u] = input(a - STR_D + tid + u * STR_THREADS);
#pragma unroll
    for (int u = 0; u < ST / STR_THREADS; ++u) vt[u] = input(e + tid + u * STR_THREADS);
#pragma unroll
    for (int u = 0; u < SC / STR_THREADS; ++u) s_c[tid + u * STR_THREADS] = vc[u];
#pragma unroll
    for (int u = 0; u < ST / STR_THREADS; ++u) s_t[tid + u * STR_THREADS] = vt[u];
    __syncthreads();
    d = 0;
    if (j >= 1) {
      unsigned hi = 0, lo = 0;  // (below every candidate's key)
      if (2 * tid < STR_CAND) {
        str_f2 corr = {0.f, 0.f}, en = {0.f, 0.f};
        const float* c = s_c + 2 * tid;
        // k ascending, each product and each sum rounded to fp32 (no fused multiply-add): the rule's order
#pragma unroll 8
        for (int k = 0; k < STR_C; ++k) {
#pragma clang fp contract(off)
          const str_f2 xc = {c[k], c[k + 1]};
          const float t = s_t[k];
          const str_f2 tt = {t, t};
          const str_f2 pc = xc * tt;
          corr = corr + pc;
          const str_f2 pe = xc * xc;
          en = en + pe;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int dd = 2 * tid + q - STR_D;
          if (dd > STR_D) break;  // (the last thread has one candidate)
          float score;
          {
#pragma clang fp contract(off)
            const float num = corr[q] * fabsf(corr[q]);
            const float den = en[q] + 1e-9f;
            score = __fdiv_rn(num, den);
          }
          if (score != score) score = -INFINITY;
          if (score == 0.f) score = 0.f;  // (-0 and +0 are equal scores)
          const unsigned qhi = str_ordered(score), qlo = 0xFFFFFFFFu - (unsigned)(2 * abs(dd) + (dd > 0 ? 1 : 0));
          if (qhi > hi || (qhi == hi && qlo > lo)) {
            hi = qhi;
            lo = qlo;
          }
        }
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const unsigned ohi = __shfl_xor(hi, m), olo = __shfl_xor(lo, m);
        if (ohi > hi || (ohi == hi && olo > lo)) {
          hi = ohi;
          lo = olo;
        }
      }
      if ((tid & 63) == 0) {
        s_hi[tid >> 6] = hi;
        s_lo[tid >> 6] = lo;
      }
      __syncthreads();
      hi = s_hi[0];
      lo = s_lo[0];
#pragma unroll
      for (int w = 1; w < STR_THREADS / 64; ++w) {
        const unsigned ohi = s_hi[w], olo = s_lo[w];
        if (ohi > hi || (ohi == hi && olo > lo)) {
          hi = ohi;
          lo = olo;
        }
      }
      const int rank = (int)(0xFFFFFFFFu - lo);
      d = (rank & 1) ? (rank >> 1) : -(rank >> 1);
    }
    const int m = h * STR_H + tid;
    if (tid < STR_H && m < r.n_out) {
#pragma clang fp contract(off)
      const float fall = s_t[tid] * s_wf[tid];
      const float rise = s_c[d + STR_D + tid] * s_wr[tid];
      orow[m] = fall + rise;
    }
    if (d_out && tid == 0) d_out[(size_t)r.row * (size_t)d_stride + h] = d;
    p_prev = a + d;
    __syncthreads();  // (the next hop overwrites the span, the template and the wave maxima)
  }
  if (tid == 0) dstate[r.slot] = d;
}

// ---- PCM dump join (llmvox.h, "PCM dump join"): the crossfaded concatenation of a sentence's dumps ----
// pcm_convert_kernel's row packet and grid. Output m of row y's call is the head's sample m (the slot's
// tail, as it is or crossfaded with the row's rendering of the same frame) while m < the head's 320, then
// r[s + m - head's]: a streaming copy. The head's length, s and n_out are multiples of 4 samples, so a
// thread's PCM_PER_THREAD outputs lie wholly in the head or wholly in the body and move as one 16-byte
// load and store where the row's and the output's addresses allow (the tail pool and the window table are
// 16-byte aligned by construction). Block (0, y) also writes the slot's next tail.
__device__ __forceinline__ float4 join_fade(float4 t, float4 wf, float4 x, float4 wr) {
#pragma clang fp contract(off)
  float4 o;
  {
    const float a = t.x * wf.x, b = x.x * wr.x;
    o.x = a + b;
  }
  {
    const float a = t.y * wf.y, b = x.y * wr.y;
    o.y = a + b;
  }
  {
    const float a = t.z * wf.z, b = x.z * wr.z;
    o.z = a + b;
  }
  {
    const float a = t.w * wf.w, b = x.w * wr.w;
    o.w = a + b;
  }
  return o;
}

__global__ __launch_bounds__(PCM_THREADS) void pcm_join_kernel(JoinRows rows, const float* __restrict__ pcm, int n_in,
                                                               const float* __restrict__ win, float* tails,
                                                               unsigned char* __restrict__ out, long long out_stride) {
  const JoinRow r = rows.r[blockIdx.y];
  const float* __restrict__ x = pcm + (size_t)r.row * (size_t)n_in;  // (never read when n_in == 0: no body, no fade)
  const int tid = threadIdx.x;
  const bool xvec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  if (blockIdx.x == 0 && r.tail_out >= 0) {  // the next tail r[n_in - 320 .. n_in), into the buffer no block reads
    const float* __restrict__ src = x + (n_in - JOIN_HOLD);
    float* dst = tails + r.tail_out;
    if (xvec) {
      if (tid < JOIN_HOLD / 4) reinterpret_cast<float4*>(dst)[tid] = reinterpret_cast<const float4*>(src)[tid];
    } else {
      for (int i = tid; i < JOIN_HOLD; i += PCM_THREADS) dst[i] = src[i];
    }
  }

  const int mb = blockIdx.x * PCM_OB;
  if (mb >= r.n_out) return;
  const int m = mb + tid * PCM_PER_THREAD;  // the thread's first output
  if (m >= r.n_out) return;                 // (n_out is a multiple of PCM_PER_THREAD: a thread has all or none)
  const int hl = r.head != JOIN_HEAD_NONE ? JOIN_HOLD : 0;
  float* o = reinterpret_cast<float*>(out + (size_t)r.row * (size_t)out_stride) + m;
  const bool ovec = (reinterpret_cast<uintptr_t>(o) & 15) == 0;
  float4 v;
  if (m < hl) {
    const float* __restrict__ t = tails + r.tail_in + m;
    v = *reinterpret_cast<const float4*>(t);
    if (r.head == JOIN_HEAD_FADE) {
      const float* __restrict__ xs = x + (r.s - JOIN_HOLD + m);
      const float4 xv = xvec ? *reinterpret_cast<const float4*>(xs) : make_float4(xs[0], xs[1], xs[2], xs[3]);
      v = join_fade(v, *reinterpret_cast<const float4*>(win + JOIN_HOLD + m), xv,
                    *reinterpret_cast<const float4*>(win + m));
    }
  } else {
    const float* __restrict__ xs = x + (r.s + m - hl);
    v = xvec ? *reinterpret_cast<const float4*>(xs) : make_float4(xs[0], xs[1], xs[2], xs[3]);
  }
  if (ovec) {
    *reinterpret_cast<float4*>(o) = v;
  } else {
    o[0] = v.x;
    o[1] = v.y;
    o[2] = v.z;
    o[3] = v.w;
  }
}

// ---- PCM level (llmvox.h, "PCM level"): a gain and a feed-forward peak limiter ----
// pcm_convert_kernel's row packet and grid. A block of PCM_OB outputs n0 .. n0 + PCM_OB - 1 stages
// r[n0 - A - R .. n0 + PCM_OB + 2 A) into LDS (LVL_SPAN values, from the slot's history of raw inputs and the
// call's row, zeros outside the segment), forms the LVL_D sliding minima m[n0 - A .. n0 + PCM_OB + A) of window
// R + A + 1 by doubling (min over 2 k from two minima over k, ten passes between two LDS buffers, then two
// overlapping windows of 1024: a minimum is exact in any order) and keeps d = 1 - m. Each thread then runs the
// 241-term sum for its four consecutive outputs: d comes as aligned 16-byte LDS reads that slide through
// registers (a thread's four-float stride would make every 4-byte read a 4-way bank conflict), the window
// word is a broadcast.
constexpr int LVL_SPAN = PCM_OB + 3 * LVL_A + LVL_R;  // 2584
constexpr int LVL_D = PCM_OB + 2 * LVL_A;             // 1264
constexpr int LVL_WIN = LVL_R + LVL_A + 1;            // 1321: inputs of one sliding minimum
constexpr int LVL_POW = 1024;                         // the largest power of two <= LVL_WIN
static_assert(LVL_POW <= LVL_WIN && 2 * LVL_POW >= LVL_WIN, "two windows of LVL_POW cover the sliding minimum's");
static_assert(LVL_D + LVL_WIN - 1 == LVL_SPAN, "the last minimum ends at the span's last value");
static_assert(LVL_A % PCM_PER_THREAD == 0 && LVL_D == PCM_PER_THREAD * (PCM_THREADS + 2 * LVL_A / PCM_PER_THREAD),
              "a thread's last 16-byte read of d ends at the array's end");
static_assert(3 * LVL_A + LVL_R <= LVL_HIST, "the history covers what a call's first output reaches back");

__device__ __forceinline__ float level_r(float v) {
  const float a = fabsf(v);
  return a > LVX_LEVEL_CEIL ? __fdiv_rn(LVX_LEVEL_CEIL, a) : 1.f;  // (a NaN compares false: 1)
}

__global__ __launch_bounds__(PCM_THREADS) void pcm_level_kernel(PcmRows rows, float gain, const float* __restrict__ pcm,
                                                                int n_in, const float* __restrict__ win, float* hist,
                                                                unsigned char* __restrict__ out, long long out_stride,
                                                                unsigned char* __restrict__ g_out, long long g_stride) {
  const PcmRow r = rows.r[blockIdx.y];
  const float* __restrict__ x = pcm + (size_t)r.row * (size_t)n_in;
  const int tid = threadIdx.x;
  const long long t1 = r.t0 + n_in;  // inputs of the segment once this call is consumed
  const SegInput<LVL_HIST> input{x, hist, r.t0, t1, r.hist_in};
  if (blockIdx.x == 0 && r.hist_out >= 0)
    for (int i = tid; i < LVL_HIST; i += PCM_THREADS) hist[r.hist_out + i] = input(t1 - LVL_HIST + i);

  const int mb = blockIdx.x * PCM_OB;
  if (mb >= r.n_out) return;
  const int nb = min(PCM_OB, r.n_out - mb);
  const int ml = tid * PCM_PER_THREAD;  // the thread's first output within the block
  const long long n_first = r.m0 + mb;  // the block's first output in the segment

  __shared__ __attribute__((aligned(16))) float s_a[LVL_SPAN];
  __shared__ __attribute__((aligned(16))) float s_b[LVL_SPAN];
  __shared__ __attribute__((aligned(16))) float s_w[LVL_TAPS + 3];
  if (tid < LVL_TAPS) s_w[tid] = win[tid];
  const long long i0 = n_first - LVL_A - LVL_R;  // the segment index of s_a[0]
  for (int k = tid; k < LVL_SPAN; k += PCM_THREADS) s_a[k] = level_r(__fmul_rn(gain, input(i0 + k)));
  __syncthreads();
  // dst[i] = min of src over [i, i + 2 k) from src's minima over [i, i + k), wherever that lies within the span
  // (the entries past it keep a shorter minimum and are not read below)
  auto twice = [&](const float* src, float* dst, int k) {
    for (int i = tid; i < LVL_SPAN; i += PCM_THREADS) {
      const float a = src[i];
      dst[i] = i + k < LVL_SPAN ? fminf(a, src[i + k]) : a;
    }
    __syncthreads();
  };
  for (int k = 1; k < LVL_POW; k <<= 2) {  // ten passes: s_a holds the minima over [i, i + 1024) at the end
    twice(s_a, s_b, k);
    twice(s_b, s_a, 2 * k);
  }
  // d[j] = 1 - min r over [j, j + LVL_WIN): the segment's d[n_first - A + j], j < LVL_D
  for (int j = tid; j < LVL_D; j += PCM_THREADS) s_b[j] = __fsub_rn(1.f, fminf(s_a[j], s_a[j + LVL_WIN - LVL_POW]));
  __syncthreads();

  float acc[PCM_PER_THREAD] = {0.f, 0.f, 0.f, 0.f};
  {
    // k ascending, each product and each sum rounded to fp32 (no fused multiply-add): the rule's order
#pragma clang fp contract(off)
    const float4* __restrict__ d4 = reinterpret_cast<const float4*>(s_b) + tid;  // d[ml + 4 j ..]
    float4 cur = d4[0];
    for (int j = 0; j < 2 * LVL_A / 4; ++j) {
      const float4 nxt = d4[j + 1];
      const float q[7] = {cur.x, cur.y, cur.z, cur.w, nxt.x, nxt.y, nxt.z};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const float w = s_w[4 * j + kk];
#pragma unroll
        for (int e = 0; e < PCM_PER_THREAD; ++e) {
          const float prod = q[kk + e] * w;
          acc[e] = acc[e] + prod;
        }
      }
      cur = nxt;
    }
    const float w = s_w[2 * LVL_A];  // the last tap, k = A
    const float q[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
    for (int e = 0; e < PCM_PER_THREAD; ++e) {
      const float prod = q[e] * w;
      acc[e] = acc[e] + prod;
    }
  }
  float y[PCM_PER_THREAD], gg[PCM_PER_THREAD];
#pragma unroll
  for (int e = 0; e < PCM_PER_THREAD; ++e) {
    const float v = __fmul_rn(gain, ml + e < nb ? input(n_first + ml + e) : 0.f);
    const float s = __fsub_rn(1.f, acc[e]);
    gg[e] = fmaxf(0.f, fminf(s, level_r(v)));
    y[e] = __fmul_rn(v, gg[e]);
  }

  store4(reinterpret_cast<float*>(out + (size_t)r.row * (size_t)out_stride) + mb + ml, y, ml, nb);
  if (g_out) store4(reinterpret_cast<float*>(g_out + (size_t)r.row * (size_t)g_stride) + mb + ml, gg, ml, nb);
}


// ---- PCM FLAC (llmvox.h, "PCM FLAC"): one subframe a workgroup ----
// Grid (the most frames of a row, rows of the launch). Block (f, y) makes frame j0 + f of row y's segment: its
// samples from the slot's kept ones and the call's int16 row into LDS; the five error sums and the all-equal test by
// a workgroup reduction; the partitions' Rice parameters from bit counts (sum(u >> k) = sum over b >= k of
// 2^(b - k) count_b, count_b the samples of the partition whose u has bit b: one wave ballot a bit, exactly the sum
// the rule states, in uint32); every sample's bit length; an exclusive scan of the lengths (a wave64 shuffle scan,
// then one pass over the wave totals); then every thread ORs its samples' stop bit and low bits, at most 15 bits in
// at most two words, into a zeroed LDS word buffer (the unary zeros are the buffer's), and the buffer goes out
// byte-swapped in 32-bit stores. Block (0, y) also writes the slot's next history. The selection arithmetic is
// pcm_host.h's (flac_diff, flac_fold, flac_partition_order, flac_rice_bits), the one lvx_flac_subframe runs.
constexpr int FLAC_THREADS = 256;
constexpr int FLAC_SPT = 8;                                  // consecutive samples of a thread
constexpr int FLAC_CAP = FLAC_THREADS * FLAC_SPT;            // 2048 >= BS + 15
constexpr int FLAC_WORDS = (flac_slot_bytes(FLAC_MAX_BS) - 8) / 4;  // words of the largest slot's subframe
constexpr int FLAC_UBITS = 21;                               // u < 2^21
static_assert(FLAC_MAX_BS + 15 <= FLAC_CAP && FLAC_MAX_BS + 15 <= FLAC_HIST, "a frame fits a block and the history");
static_assert(8 + 16 * (FLAC_MAX_BS + 15) <= 32 * (FLAC_WORDS - 1), "a word past the longest subframe's last stays inside the buffer");

// the low len bits of v (len 1 .. 16) at bit pos of the stream (MSB first) into the word buffer
__device__ __forceinline__ void flac_put(unsigned* words, unsigned pos, int len, unsigned v) {
  const unsigned long long t = (unsigned long long)v << (64 - (int)(pos & 31u) - len);
  const unsigned hi = (unsigned)(t >> 32), lo = (unsigned)t;
  atomicOr(&words[pos >> 5], hi);
  if (lo) atomicOr(&words[(pos >> 5) + 1], lo);
}

__global__ __launch_bounds__(FLAC_THREADS) void pcm_flac_kernel(FlacRows rows, int bs, const int16_t* __restrict__ s16,
                                                                 int n_in, long long in_stride, int16_t* hist,
                                                                 unsigned char* __restrict__ out, long long out_stride) {
  const FlacRow r = rows.r[blockIdx.y];
  const int16_t* __restrict__ x =
      reinterpret_cast<const int16_t*>(reinterpret_cast<const unsigned char*>(s16) + (size_t)r.row * (size_t)in_stride);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long t1 = r.t0 + n_in;  // inputs of the segment once this call is consumed
  auto input = [&](long long g) -> int {  // segment input g from the call's row or the slot's history; zero outside
    if (g < 0 || g >= t1) return 0;
    if (g >= r.t0) return x[g - r.t0];
    const long long back = r.t0 - g;
    return back <= FLAC_HIST ? hist[r.hist_in + FLAC_HIST - back] : 0;
  };
  if (blockIdx.x == 0 && r.hist_out >= 0)
    for (int i = tid; i < FLAC_HIST; i += FLAC_THREADS) hist[r.hist_out + i] = (int16_t)input(t1 - FLAC_HIST + i);
  const int f = blockIdx.x;
  if (f >= r.n_out) return;
  const int n = min(f == r.n_out - 1 ? r.last_n : bs, FLAC_CAP);  // (<= BS + 15 by the plan)
  const long long s0 = (r.j0 + f) * bs;                            // the frame's first sample in the segment
  const int slot_bytes = flac_slot_bytes(bs);

  __shared__ __attribute__((aligned(16))) int s_x[4 + FLAC_CAP];  // x[-4 .. FLAC_CAP): zeros in front and behind
  __shared__ unsigned s_u[FLAC_CAP];                              // the folded residuals (0: a warm-up, none)
  __shared__ unsigned s_w[FLAC_WORDS];
  __shared__ unsigned s_cnt[8][FLAC_UBITS];
  __shared__ unsigned s_red[FLAC_THREADS / 64][6];
  __shared__ unsigned s_tot[FLAC_THREADS / 64];
  __shared__ int s_k[8];
  if (tid < 4) s_x[tid] = 0;
  for (int i = tid; i < FLAC_CAP; i += FLAC_THREADS) s_x[4 + i] = i < n ? input(s0 + i) : 0;
  for (int i = tid; i < FLAC_WORDS; i += FLAC_THREADS) s_w[i] = 0;
  if (tid < 8 * FLAC_UBITS) (&s_cnt[0][0])[tid] = 0;
  __syncthreads();

  // the thread's samples i0 .. i0 + 7 and the four in front of them
  const int i0 = tid * FLAC_SPT;
  int w[4 + FLAC_SPT];
  {
    const int4* __restrict__ p4 = reinterpret_cast<const int4*>(s_x + i0);
#pragma unroll
    for (int q = 0; q < (4 + FLAC_SPT) / 4; ++q) {
      const int4 v = p4[q];
      w[4 * q] = v.x;
      w[4 * q + 1] = v.y;
      w[4 * q + 2] = v.z;
      w[4 * q + 3] = v.w;
    }
  }
  // E_p over i = 4 .. n - 1 (|r_4| <= 2^19 and n < 2^11: uint32) and whether any sample differs from x[0]
  unsigned acc[6] = {0, 0, 0, 0, 0, 0};
  const int x0 = s_x[4];
#pragma unroll
  for (int e = 0; e < FLAC_SPT; ++e) {
    const int i = i0 + e;
    if (i < n) {
      if (w[e + 4] != x0) acc[5] = 1;
      if (i >= 4) {
#pragma unroll
        for (int p = 0; p <= 4; ++p) acc[p] += (unsigned)abs(flac_diff(p, w[e + 4], w[e + 3], w[e + 2], w[e + 1], w[e]));
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc[q] += __shfl_xor(acc[q], m);
    if (lane == 0) s_red[wave][q] = acc[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    acc[q] = 0;
#pragma unroll
    for (int v = 0; v < FLAC_THREADS / 64; ++v) acc[q] += s_red[v][q];
  }
  unsigned char* slot = out + (size_t)r.row * (size_t)out_stride + (size_t)f * (size_t)slot_bytes;
  uint32_t* slot_w = reinterpret_cast<uint32_t*>(slot);
  unsigned total_bits;  // of the subframe
  if (acc[5] == 0) {    // CONSTANT
    total_bits = 24;
    if (tid == 0) flac_put(s_w, 8, 16, (unsigned)x0 & 0xFFFFu);  // (the header byte is 0)
  } else {
    int p = 0;
#pragma unroll
    for (int q = 1; q <= 4; ++q)
      if (acc[q] < acc[p]) p = q;
    unsigned u[FLAC_SPT];
#pragma unroll
    for (int e = 0; e < FLAC_SPT; ++e) {
      const int i = i0 + e;
      u[e] = i >= p && i < n ? flac_fold(flac_diff(p, w[e + 4], w[e + 3], w[e + 2], w[e + 1], w[e])) : 0u;
      s_u[i] = u[e];
    }
    __syncthreads();
    // the bit counts of every partition: the waves walk the samples in runs of 64 consecutive ones
    const int P = flac_partition_order(n), psize = n >> P;
    for (int e = 0; e < FLAC_SPT; ++e) {
      const int i = e * FLAC_THREADS + tid;
      const bool valid = i >= p && i < n;
      const int j = valid ? min(i / psize, 7) : -1;
      const unsigned ui = s_u[i];
      unsigned long long todo = __ballot(valid);
      while (todo) {
        const int jj = __shfl(j, __ffsll((long long)todo) - 1);
        const bool mine = j == jj;
        todo &= ~__ballot(mine);
        unsigned c = 0;
#pragma unroll
        for (int b = 0; b < FLAC_UBITS; ++b) {
          const unsigned long long has = __ballot(mine && ((ui >> b) & 1u));
          if (lane == b) c = (unsigned)__popcll(has);
        }
        if (lane < FLAC_UBITS && c) atomicAdd(&s_cnt[jj][lane], c);
      }
    }
    __syncthreads();
    if (tid < (1 << P)) {  // the partition's k: the least sum((u >> k) + 1 + k), the smallest k at a tie
      const unsigned cnt = (unsigned)(psize - (tid == 0 ? p : 0));
      unsigned least = 0xFFFFFFFFu;
      int best = 0;
      for (int k = 0; k <= FLAC_MAX_K; ++k) {
        unsigned c = cnt * (unsigned)(1 + k);
        for (int b = k; b < FLAC_UBITS; ++b) c += s_cnt[tid][b] << (b - k);
        if (c < least) {
          least = c;
          best = k;
        }
      }
      s_k[tid] = best;
    }
    __syncthreads();
    // the bits of the thread's samples: a warm-up's 16, a residual's (u >> k) + 1 + k; the method and P (6 bits) ride
    // in front of residual p, a partition's k (4 bits) in front of its first residual
    unsigned len = 0;
#pragma unroll
    for (int e = 0; e < FLAC_SPT; ++e) {
      const int i = i0 + e;
      if (i < p) {
        len += 16;
      } else if (i < n) {
        const int j = min(i / psize, 7);
        len += flac_rice_bits(u[e], s_k[j]) + (i == p ? 10u : i == j * psize ? 4u : 0u);
      }
    }
    unsigned scan = len;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const unsigned o = __shfl_up(scan, m);
      if (lane >= m) scan += o;
    }
    if (lane == 63) s_tot[wave] = scan;
    __syncthreads();
    unsigned pos = 8 + scan - len, all = 0;
#pragma unroll
    for (int v = 0; v < FLAC_THREADS / 64; ++v) {
      if (v < wave) pos += s_tot[v];
      all += s_tot[v];
    }
    total_bits = 8 + all;
    if (total_bits >= 8u + 16u * (unsigned)n) {  // VERBATIM
      total_bits = 8u + 16u * (unsigned)n;
      if (tid == 0) flac_put(s_w, 0, 8, 0x02u);
#pragma unroll
      for (int e = 0; e < FLAC_SPT; ++e)
        if (i0 + e < n) flac_put(s_w, 8u + 16u * (unsigned)(i0 + e), 16, (unsigned)w[e + 4] & 0xFFFFu);
    } else {  // FIXED: every position below lies under total_bits < 8 + 16 n, inside the buffer
      if (tid == 0) flac_put(s_w, 0, 8, (8u | (unsigned)p) << 1);
#pragma unroll
      for (int e = 0; e < FLAC_SPT; ++e) {
        const int i = i0 + e;
        if (i < p) {
          flac_put(s_w, pos, 16, (unsigned)w[e + 4] & 0xFFFFu);
          pos += 16;
        } else if (i < n) {
          const int j = min(i / psize, 7), k = s_k[j];
          if (i == p) {
            flac_put(s_w, pos, 6, (unsigned)P);
            pos += 6;
          }
          if (i == p || i == j * psize) {
            flac_put(s_w, pos, 4, (unsigned)k);
            pos += 4;
          }
          const unsigned q = u[e] >> k;
          flac_put(s_w, pos + q, k + 1, (1u << k) | (u[e] & ((1u << k) - 1u)));
          pos += q + 1u + (unsigned)k;
        }
      }
    }
  }
  __syncthreads();
  // the record {u16 n, u16 body_bytes, u32 0}, then the subframe's words, big-endian bytes; zeros to the slot's end
  if (tid == 0) {
    slot_w[0] = (uint32_t)n | (((total_bits + 7u) >> 3) << 16);
    slot_w[1] = 0;
  }
  for (int i = tid; i < (slot_bytes - 8) / 4; i += FLAC_THREADS) slot_w[2 + i] = __builtin_bswap32(s_w[i]);
}

// ---- PCM formant (llmvox.h, "PCM formant"): the envelope correction, a short-time Fourier transform in LDS ----
// Grid (groups of `group` output hop blocks, rows of the launch). Workgroup (x, y) writes the hop blocks
// [x group, (x + 1) group) of row y's call: it runs the group + 3 frames that cover them one after the
// other in ascending j, each through the rule's eight steps (the window into bit-reversed places, ten radix-2 stages of
// 512 butterflies, two a thread, the power, the 25-tap smoothing, the gain, the Hermitian spectrum through registers
// into bit-reversed places again, ten stages back), and adds the frame's four quarters to the four hop blocks they
// cover. A thread owns sample tid of every hop block, so the sums are its own words of a four-block ring: the block's
// first frame sets, the next three add, in ascending j as the rule states, and the block goes out after its fourth.
// No float atomics and no scratch: the frames a neighbouring group also needs (3 of group + 3) are computed twice.
// group 1 is "one workgroup per output hop block computes its four frames": the shortest chain of frames, which a
// launch too small to fill the device wants; a large launch wants the redundancy small. pcm_launch_formant chooses;
// the bits do not depend on the choice (a block's four frames are added in the same order in any group).
// Block (0, y) also writes the slot's next history.
constexpr int FMT_GROUP_MAX = 32;
constexpr int FMT_WGS = 1024;  // workgroups a launch aims at: four a CU
constexpr int FMT_PER = FMT_N / PCM_THREADS;  // samples of a frame a thread moves: tid + 256 q, one of each quarter
constexpr int FMT_HALF = FMT_N / 2;
static_assert(FMT_N == 1024 && FMT_H == PCM_THREADS && FMT_PER == 4, "a thread owns one sample of each of a frame's four hop blocks");
static_assert(FMT_HIST >= 7 * FMT_H - 1, "the history covers what a call's first output reaches back");

__device__ __forceinline__ int fmt_rev(int n) { return (int)(__builtin_bitreverse32((unsigned)n) >> 22); }  // of 10 bits

// The ten stages of the rule's DFT_N in place, the input already in bit-reversed places; inverse: ti negated. Each
// product and each sum rounded (no fused multiply-add), the full product in every stage. Ends behind a barrier.
__device__ __forceinline__ void fmt_stages(float* s_re, float* s_im, const float* s_tr, const float* s_ti, bool inverse, int tid) {
#pragma clang fp contract(off)
  for (int s = 0; s < 10; ++s) {
    const int h = 1 << s;
#pragma unroll
    for (int t = tid; t < FMT_HALF; t += PCM_THREADS) {
      const int p = t & (h - 1), i = ((t >> s) << (s + 1)) + p, j = i + h;
      const float wr = s_tr[p << (9 - s)], wi0 = s_ti[p << (9 - s)], wi = inverse ? -wi0 : wi0;
      const float ur = s_re[i], ui = s_im[i], vr = s_re[j], vi = s_im[j];
      const float a = vr * wr, b = vi * wi, c = vr * wi, d = vi * wr;
      const float pr = a - b, pi = c + d;
      s_re[i] = ur + pr;
      s_im[i] = ui + pi;
      s_re[j] = ur - pr;
      s_im[j] = ui - pi;
    }
    __syncthreads();
  }
}

// The tables both transforms need, from the stage's device tables to LDS: the window and the twiddles. Ends behind no
// barrier: the caller's own follows.
__device__ __forceinline__ void fmt_load_tables(const float* __restrict__ tab, float* s_w, float* s_tr, float* s_ti, int tid) {
  for (int i = tid; i < FMT_N; i += PCM_THREADS) s_w[i] = tab[i];
  for (int i = tid; i < FMT_HALF; i += PCM_THREADS) {
    s_tr[i] = tab[FMT_N + FMT_TAPS + i];
    s_ti[i] = tab[FMT_N + FMT_TAPS + FMT_HALF + i];
  }
}

// The slot's next history: the last FMT_HIST inputs of the segment once the call is consumed
__device__ __forceinline__ void fmt_keep_history(const SegInput<FMT_HIST>& input, float* hist, int hist_out, long long t1, int tid) {
  for (int i = tid; i < FMT_HIST; i += PCM_THREADS) hist[hist_out + i] = input(t1 - FMT_HIST + i);
}

// The frame loop of a workgroup, one template over the gain step: the frames lb0 .. lb1 + 2 of the call (frame
// j = b_first + lj), each windowed, transformed, multiplied by its gains, transformed back and added to the ring of
// hop blocks. Gain: prepare(s_re, s_im, j, tid), which sees the spectrum behind a barrier and ends behind one where it
// wrote LDS, then operator()(k), the gain of bin k <= N / 2.
template <class Gain>
__device__ __forceinline__ void fmt_frames(const PcmRow& r, const SegInput<FMT_HIST>& input, float* __restrict__ o, int lb0, int lb1,
                                           long long b_first, float* s_re, float* s_im, float* s_acc, const float* s_w,
                                           const float* s_tr, const float* s_ti, Gain& gain, int tid) {
#pragma clang fp contract(off)
  const float two_thirds = (float)(2.0 / 3.0);
  for (int lj = lb0; lj < lb1 + 3; ++lj) {  // frame j = b_first + lj covers the call's hop blocks lj - 3 .. lj
    const long long g0 = (b_first + lj - 3) * FMT_H;  // its first input
    // 1. the windowed frame, to bit-reversed places
#pragma unroll
    for (int q = 0; q < FMT_PER; ++q) {
      const int n = tid + q * PCM_THREADS, v = fmt_rev(n);
      s_re[v] = s_w[n] * input(g0 + n);
      s_im[v] = 0.f;
    }
    __syncthreads();
    fmt_stages(s_re, s_im, s_tr, s_ti, false, tid);
    // 2 .. 6. the gains of the frame's bins
    gain.prepare(s_re, s_im, b_first + lj, tid);
    // 7. Y = G X on 0 .. N / 2 and its Hermitian extension, through registers to bit-reversed places
    float yr[FMT_PER], yi[FMT_PER];
#pragma unroll
    for (int q = 0; q < FMT_PER; ++q) {
      const int k = tid + q * PCM_THREADS, kk = k <= FMT_HALF ? k : FMT_N - k;
      const float g = gain(kk);
      yr[q] = g * s_re[kk];
      const float im = g * s_im[kk];
      yi[q] = k <= FMT_HALF ? im : -im;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < FMT_PER; ++q) {
      const int v = fmt_rev(tid + q * PCM_THREADS);
      s_re[v] = yr[q];
      s_im[v] = yi[q];
    }
    __syncthreads();
    fmt_stages(s_re, s_im, s_tr, s_ti, true, tid);
    // 8. the windowed frame, quarter q onto hop block lj - 3 + q: the block's first frame (q = 3) sets, the others add
#pragma unroll
    for (int q = 0; q < FMT_PER; ++q) {
      const int n = tid + q * PCM_THREADS, lb = lj - 3 + q;
      if (lb < lb0 || lb >= lb1) continue;  // a block of another group
      const float sc = 0.0009765625f * s_re[n];
      const float v = s_w[n] * sc;
      float* a = s_acc + ((lb & 3) * FMT_H + tid);
      *a = q == 3 ? v : *a + v;
    }
    if (lj - 3 >= lb0) {  // block lj - 3 has its four frames
      const int nl = (lj - 3) * FMT_H + tid;
      if (nl < r.n_out) o[nl] = two_thirds * s_acc[((lj - 3) & 3) * FMT_H + tid];
    }
    __syncthreads();  // (the next frame overwrites s_re)
  }
}

// The formant rule's steps 2 to 6: the power, its smoothing, the envelope at k Fn / Fd over the envelope at k
struct FormantGain {
  float *s_P, *s_E, *s_G;
  const float* s_c;
  int Fn, Fd;
  __device__ __forceinline__ void prepare(const float* s_re, const float* s_im, long long, int tid) {
#pragma clang fp contract(off)
    const float eps = 1e-10f, g2_lo = 1.f / 256.f, g2_hi = 256.f;
    // 2. the power of bins 0 .. N / 2
    for (int k = tid; k < FMT_BINS; k += PCM_THREADS) {
      const float a = s_re[k] * s_re[k], b = s_im[k] * s_im[k];
      s_P[k] = a + b;
    }
    __syncthreads();
    // 3, 4. the envelope: 25 taps over the symmetric extension, d ascending
    for (int k = tid; k < FMT_BINS; k += PCM_THREADS) {
      float acc = 0.f;
#pragma unroll
      for (int d = -FMT_K; d <= FMT_K; ++d) {
        const int at = k + d, idx = at < 0 ? -at : at > FMT_HALF ? FMT_N - at : at;
        const float prod = s_c[d + FMT_K] * s_P[idx];
        acc = acc + prod;
      }
      s_E[k] = acc;
    }
    __syncthreads();
    // 5, 6. the envelope at k Fn / Fd over the envelope at k: the gain
    for (int k = tid; k < FMT_BINS; k += PCM_THREADS) {
      const int kn = k * Fn, i = kn / Fd;
      float es = s_E[FMT_HALF];
      if (i < FMT_HALF) {
        const float f = __fdiv_rn((float)(kn - i * Fd), (float)Fd);
        const float e0 = s_E[i], de = s_E[i + 1] - e0, fd = f * de;
        es = e0 + fd;
      }
      const float num = es + eps, den = s_E[k] + eps;
      const float g2 = fminf(fmaxf(__fdiv_rn(num, den), g2_lo), g2_hi);
      s_G[k] = sqrtf(g2);  // (the correctly rounded one: the Makefile compiles this file with IEEE fp32 / and sqrt)
    }
    __syncthreads();
  }
  __device__ __forceinline__ float operator()(int k) const { return s_G[k]; }
};

// The mark rule's gain (llmvox.h, "PCM mark"): the word of the frame's block, then a bit of it per pair of sub-bands.
// No LDS of its own beyond the table's 64 words, and no barrier.
struct MarkGain {
  const uint16_t* s_tab;  // the sign table [MRK_P]
  float gp, gm;           // 1 + a, 1 - a
  unsigned word;
  __device__ __forceinline__ void prepare(const float*, const float*, long long j, int) { word = s_tab[(int)((j / MRK_Q) % MRK_P)]; }
  __device__ __forceinline__ float operator()(int k) const {
    const unsigned rel = (unsigned)(k - MRK_K0);
    if (rel >= (unsigned)(MRK_U * MRK_BW)) return 1.f;
    const unsigned u = rel / MRK_BW, bit = (word >> (u >> 1)) & 1u;
    return bit == (u & 1u) ? gp : gm;  // a set bit: g- on the even sub-band, g+ on the odd one
  }
};

__global__ __launch_bounds__(PCM_THREADS) void pcm_formant_kernel(PcmRows rows, int Fn, int Fd, const float* __restrict__ pcm,
                                                                  int n_in, const float* __restrict__ tab, float* hist,
                                                                  unsigned char* __restrict__ out, long long out_stride,
                                                                  int group) {
  const PcmRow r = rows.r[blockIdx.y];
  const float* __restrict__ x = pcm + (size_t)r.row * (size_t)n_in;
  const int tid = threadIdx.x;
  const long long t1 = r.t0 + n_in;  // inputs of the segment once this call is consumed
  const SegInput<FMT_HIST> input{x, hist, r.t0, t1, r.hist_in};
  if (blockIdx.x == 0 && r.hist_out >= 0) fmt_keep_history(input, hist, r.hist_out, t1, tid);

  const int n_blocks = (r.n_out + FMT_H - 1) / FMT_H;  // hop blocks of this call (the last may be cut by a final call)
  const int lb0 = blockIdx.x * group;                  // the group's first, counted from the call's first
  if (lb0 >= n_blocks) return;
  const int lb1 = min(lb0 + group, n_blocks);
  const long long b_first = r.m0 / FMT_H;  // (m0 is a multiple of H: only a final call emits part of a block)

  __shared__ float s_re[FMT_N], s_im[FMT_N], s_acc[FMT_N], s_w[FMT_N];
  __shared__ float s_tr[FMT_HALF], s_ti[FMT_HALF], s_c[FMT_TAPS];
  __shared__ float s_P[FMT_BINS], s_E[FMT_BINS], s_G[FMT_BINS];
  fmt_load_tables(tab, s_w, s_tr, s_ti, tid);
  if (tid < FMT_TAPS) s_c[tid] = tab[FMT_N + tid];
  __syncthreads();

  FormantGain gain{s_P, s_E, s_G, s_c, Fn, Fd};
  fmt_frames(r, input, reinterpret_cast<float*>(out + (size_t)r.row * (size_t)out_stride), lb0, lb1, b_first, s_re, s_im, s_acc,
             s_w, s_tr, s_ti, gain, tid);
}

// ---- PCM mark (llmvox.h, "PCM mark"): the watermark, the formant stage's transform under a table of signs ----
// The formant kernel's grid, group, frame loop and ring (fmt_frames); the gain of a bin is a bit of the block's word,
// so the kernel needs no power, envelope or gain arrays. The table's 128 bytes arrive as an argument.
__global__ __launch_bounds__(PCM_THREADS) void pcm_mark_kernel(PcmRows rows, MarkTab mt, float a, const float* __restrict__ pcm,
                                                               int n_in, const float* __restrict__ tab, float* hist,
                                                               unsigned char* __restrict__ out, long long out_stride, int group) {
  const PcmRow r = rows.r[blockIdx.y];
  const float* __restrict__ x = pcm + (size_t)r.row * (size_t)n_in;
  const int tid = threadIdx.x;
  const long long t1 = r.t0 + n_in;
  const SegInput<FMT_HIST> input{x, hist, r.t0, t1, r.hist_in};
  if (blockIdx.x == 0 && r.hist_out >= 0) fmt_keep_history(input, hist, r.hist_out, t1, tid);

  const int n_blocks = (r.n_out + FMT_H - 1) / FMT_H;
  const int lb0 = blockIdx.x * group;
  if (lb0 >= n_blocks) return;
  const int lb1 = min(lb0 + group, n_blocks);
  const long long b_first = r.m0 / FMT_H;

  __shared__ float s_re[FMT_N], s_im[FMT_N], s_acc[FMT_N], s_w[FMT_N];
  __shared__ float s_tr[FMT_HALF], s_ti[FMT_HALF];
  __shared__ uint16_t s_mt[MRK_P];
  fmt_load_tables(tab, s_w, s_tr, s_ti, tid);
  if (tid < MRK_P) s_mt[tid] = mt.w[tid];
  __syncthreads();

  MarkGain gain{s_mt, 1.f + a, 1.f - a, 0u};
  fmt_frames(r, input, reinterpret_cast<float*>(out + (size_t)r.row * (size_t)out_stride), lb0, lb1, b_first, s_re, s_im, s_acc,
             s_w, s_tr, s_ti, gain, tid);
}

// ---- PCM pause (llmvox.h, "PCM pause"): one slot a block of 10 ms, a copy and one vote ----
// Grid (groups of `group` blocks, rows of the launch). Workgroup (x, y) writes the slots of blocks [x group,
// (x + 1) group) of row y's call, a wave a block at a time: a lane moves 16 bytes of the payload, the unit u of the
// block, from the call's row (or, the call's first block, sample by sample from the slot's kept ones) to the slot,
// tests its samples against the threshold (pcm_host.h's pause_loud, the one lvx_pause_slots runs), and the block's mark
// is one wave vote; lane 0 writes the record. No LDS and no atomics. A slot starts on an 8-byte boundary, so a payload
// unit is stored as 16 bytes where its address allows and as two 8-byte halves where not. A block's first sample sits
// wherever the segment's count puts it in the row: a unit whose address is a multiple of 16 is one 16-byte load; any
// other is the five aligned words around it, shifted into place (the fifth only where the shift needs it and the row
// still holds it); a unit that reaches into the kept samples, past the block's n samples or before the row's first
// word is assembled sample by sample, the encoding's silence behind the n. Block (0, y) also writes the slot's next
// history: the call's last bl samples.
constexpr int PAUSE_WAVES = PCM_THREADS / 64;
constexpr int PAUSE_WGS = 1024;  // workgroups a launch aims at: four a CU

template <int ENC>
__global__ __launch_bounds__(PCM_THREADS) void pcm_pause_kernel(PauseRows rows, int bl, const unsigned char* __restrict__ in,
                                                                int n_in, long long in_stride, unsigned char* hist,
                                                                unsigned char* __restrict__ out, long long out_stride,
                                                                int group) {
  constexpr int BPS = pcm_sample_bytes(ENC), SPU = 16 / BPS;  // bytes of a sample, samples of a 16-byte unit
  constexpr uint32_t MASK = BPS == 4 ? 0xFFFFFFFFu : (1u << (8 * (BPS & 3))) - 1u;
  constexpr uint32_t SIL = (uint32_t)pause_silence(ENC);
  using T = typename std::conditional<BPS == 4, uint32_t, typename std::conditional<BPS == 2, uint16_t, uint8_t>::type>::type;
  const PauseRow r = rows.r[blockIdx.y];
  const unsigned char* __restrict__ xb = in + (size_t)r.row * (size_t)in_stride;
  const T* __restrict__ x = reinterpret_cast<const T*>(xb);
  const T* kept = reinterpret_cast<const T*>(hist + r.hist_in);  // inputs t0 - bl .. t0 - 1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long t1 = r.t0 + n_in;  // inputs of the segment once this call is consumed
  auto sample = [&](long long g) -> uint32_t {  // segment input g, t0 - bl <= g < t1, from the row or the kept ones
    return g >= r.t0 ? x[g - r.t0] : kept[bl - (int)(r.t0 - g)];
  };
  if (blockIdx.x == 0 && r.hist_out >= 0) {
    T* next = reinterpret_cast<T*>(hist + r.hist_out);
    for (int i = tid; i < bl; i += PCM_THREADS) {
      const long long g = t1 - bl + i;
      next[i] = g >= 0 ? (T)sample(g) : (T)0;
    }
  }

  const int lb0 = blockIdx.x * group, lb1 = min(lb0 + group, r.n_out);
  const int slot_bytes = pause_slot_bytes(bl, BPS), units = bl * BPS / 16;
  unsigned char* orow = out + (size_t)r.row * (size_t)out_stride;
  for (int f = lb0 + wave; f < lb1; f += PAUSE_WAVES) {
    const int n = f == r.n_out - 1 ? r.last_n : bl;  // samples of the block
    const long long s0 = (r.j0 + f) * bl;            // its first sample in the segment
    unsigned char* slot = orow + (size_t)f * (size_t)slot_bytes;
    bool loud = false;
    for (int u = lane; u < units; u += 64) {
      const int i0 = u * SPU;  // the unit's first sample within the block
      const long long g0 = s0 + i0;
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      bool done = false;
      if (g0 >= r.t0 && i0 + SPU <= n) {  // the whole unit lies in the call's row
        const unsigned char* p = xb + (size_t)(g0 - r.t0) * BPS;
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        const int sh = (int)(a & 3);
        const uint32_t* pa = reinterpret_cast<const uint32_t*>(p - sh);
        if ((a & 15) == 0) {
          const uint4 v = *reinterpret_cast<const uint4*>(p);
          w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
          done = true;
        } else if (sh == 0) {
#pragma unroll
          for (int k = 0; k < 4; ++k) w[k] = pa[k];
          done = true;
        } else if (reinterpret_cast<const unsigned char*>(pa) >= xb &&
                   reinterpret_cast<const unsigned char*>(pa) + 20 <= xb + (size_t)n_in * BPS) {
          uint32_t d[5];
#pragma unroll
          for (int k = 0; k < 5; ++k) d[k] = pa[k];
#pragma unroll
          for (int k = 0; k < 4; ++k) w[k] = (uint32_t)((((unsigned long long)d[k + 1] << 32) | d[k]) >> (8 * sh));
          done = true;
        }
      }
      if (!done) {
#pragma unroll
        for (int e = 0; e < SPU; ++e) {
          const uint32_t bits = i0 + e < n ? sample(g0 + e) : SIL;
          w[e * BPS / 4] |= bits << (8 * ((e * BPS) & 3));
        }
      }
#pragma unroll
      for (int e = 0; e < SPU; ++e) loud = loud || pause_loud<ENC>((w[e * BPS / 4] >> (8 * ((e * BPS) & 3))) & MASK);
      unsigned char* o = slot + 8 + (size_t)u * 16;
      if ((reinterpret_cast<uintptr_t>(o) & 15) == 0) {
        *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
        *reinterpret_cast<uint2*>(o) = make_uint2(w[0], w[1]);
        *reinterpret_cast<uint2*>(o + 8) = make_uint2(w[2], w[3]);
      }
    }
    const bool active = __any(loud ? 1 : 0) != 0;  // the block's mark: one vote of the wave
    if (lane == 0) {
      const bool last = r.last != 0 && f == r.n_out - 1;
      *reinterpret_cast<uint2*>(slot) = make_uint2((uint32_t)n | (active ? 1u << 16 : 0u) | (last ? 1u << 24 : 0u), 0u);
    }
  }
}

template <int ENC>
void launch_pause(dim3 grid, const PauseRows& rows, int bl, const void* in, int n_in, long long in_stride, unsigned char* hist,
                  void* out, long long out_stride, int group, hipStream_t s) {
  pcm_pause_kernel<ENC><<<grid, PCM_THREADS, 0, s>>>(rows, bl, (const unsigned char*)in, n_in, in_stride, hist,
                                                     (unsigned char*)out, out_stride, group);
}

}  // namespace

void pcm_launch_pause(const PauseRows& rows, int n_rows, int max_blocks, int bl, int enc, const void* in, int n_in,
                      long long in_stride, unsigned char* hist, void* out, long long out_stride, hipStream_t s) {
  // the smallest group, a whole number of blocks a wave, at which the launch has at most PAUSE_WGS workgroups
  const int per_row = std::max(1, PAUSE_WGS / n_rows);
  const int group = (std::max(1, (max_blocks + per_row - 1) / per_row) + PAUSE_WAVES - 1) / PAUSE_WAVES * PAUSE_WAVES;
  const dim3 grid((unsigned)std::max(1, (max_blocks + group - 1) / group), (unsigned)n_rows);
  switch (enc) {
    case LVX_PCM_S16LE: launch_pause<LVX_PCM_S16LE>(grid, rows, bl, in, n_in, in_stride, hist, out, out_stride, group, s); break;
    case LVX_PCM_ULAW: launch_pause<LVX_PCM_ULAW>(grid, rows, bl, in, n_in, in_stride, hist, out, out_stride, group, s); break;
    case LVX_PCM_ALAW: launch_pause<LVX_PCM_ALAW>(grid, rows, bl, in, n_in, in_stride, hist, out, out_stride, group, s); break;
    default: launch_pause<LVX_PCM_F32LE>(grid, rows, bl, in, n_in, in_stride, hist, out, out_stride, group, s); break;
  }
}

// hop blocks a workgroup of the formant and mark kernels writes: the option's, or the smallest group at which the
// launch has at most FMT_WGS workgroups (measured: DESIGN 4, "The formant: a short-time Fourier correction of the
// spectral envelope", "Which group")
static int fmt_group_of(int blocks, int n_rows) {
  int group = opts().fmt_group;
  if (group == 0) {
    const int per_row = std::max(1, FMT_WGS / n_rows);
    group = std::min(std::max(1, (blocks + per_row - 1) / per_row), FMT_GROUP_MAX);
  }
  return group;
}

void pcm_launch_formant(const PcmRows& rows, int n_rows, int max_out, int Fn, int Fd, const float* pcm, int n_in,
                        const float* tab, float* hist, float* out, long long out_stride, hipStream_t s) {
  const int blocks = (max_out + FMT_H - 1) / FMT_H, group = fmt_group_of(blocks, n_rows);
  pcm_formant_kernel<<<dim3((unsigned)std::max(1, (blocks + group - 1) / group), (unsigned)n_rows), PCM_THREADS, 0, s>>>(
      rows, Fn, Fd, pcm, n_in, tab, hist, (unsigned char*)out, out_stride, group);
}

void pcm_launch_mark(const PcmRows& rows, int n_rows, int max_out, const MarkTab& mt, float a, const float* pcm, int n_in,
                     const float* tab, float* hist, float* out, long long out_stride, hipStream_t s) {
  const int blocks = (max_out + FMT_H - 1) / FMT_H, group = fmt_group_of(blocks, n_rows);
  pcm_mark_kernel<<<dim3((unsigned)std::max(1, (blocks + group - 1) / group), (unsigned)n_rows), PCM_THREADS, 0, s>>>(
      rows, mt, a, pcm, n_in, tab, hist, (unsigned char*)out, out_stride, group);
}

void pcm_launch_flac(const FlacRows& rows, int n_rows, int max_frames, int bs, const int16_t* s16, int n_in,
                     long long in_stride, int16_t* hist, void* out, long long out_stride, hipStream_t s) {
  pcm_flac_kernel<<<dim3((unsigned)std::max(1, max_frames), (unsigned)n_rows), FLAC_THREADS, 0, s>>>(
      rows, bs, s16, n_in, in_stride, hist, (unsigned char*)out, out_stride);
}

void pcm_launch_level(const PcmRows& rows, int n_rows, int max_out, float gain, const float* pcm, int n_in,
                      const float* win, float* hist, float* out, long long out_stride, float* g_out, long long g_stride,
                      hipStream_t s) {
  pcm_level_kernel<<<pcm_grid(max_out, n_rows), PCM_THREADS, 0, s>>>(rows, gain, pcm, n_in, win, hist, (unsigned char*)out,
                                                                     out_stride, (unsigned char*)g_out, g_stride);
}

void pcm_launch_join(const JoinRows& rows, int n_rows, int max_out, const float* pcm, int n_in, const float* win,
                     float* tails, float* out, long long out_stride, hipStream_t s) {
  pcm_join_kernel<<<pcm_grid(max_out, n_rows), PCM_THREADS, 0, s>>>(rows, pcm, n_in, win, tails, (unsigned char*)out,
                                                                    out_stride);
}

void pcm_launch_stretch(const StretchRows& rows, int n_rows, int speed_pct, const float* pcm, int n_in,
                        const float* win, float* hist, int* dstate, float* out, long long out_stride, int* d_out,
                        int d_stride, hipStream_t s) {
  pcm_stretch_kernel<<<dim3((unsigned)n_rows), STR_THREADS, 0, s>>>(rows, speed_pct, pcm, n_in, win, hist, dstate,
                                                                    (unsigned char*)out, out_stride, d_out, d_stride);
}

void pcm_launch_ratio(const RatioRows& rows, int n_rows, int max_out, int L, int M, int N, const float* pcm, int n_in,
                      const float* taps, float* hist, float* out, long long out_stride, hipStream_t s) {
  pcm_ratio_kernel<<<pcm_grid(max_out, n_rows), PCM_THREADS, 0, s>>>(rows, L, M, N, pcm, n_in, taps, hist,
                                                                     (unsigned char*)out, out_stride);
}

void pcm_launch_convert(int sample_rate, int enc, const PcmRows& rows, int n_rows, int max_out, const float* pcm,
                        int n_in, const float* taps, float* hist, void* out, long long out_stride, hipStream_t s) {
  switch (sample_rate) {
    case 16000: launch_enc<2, 3, 72>(rows, n_rows, max_out, enc, pcm, n_in, taps, hist, out, out_stride, s); break;
    case 8000: launch_enc<1, 3, 72>(rows, n_rows, max_out, enc, pcm, n_in, taps, hist, out, out_stride, s); break;
    case 48000: launch_enc<2, 1, 48>(rows, n_rows, max_out, enc, pcm, n_in, taps, hist, out, out_stride, s); break;
    default: launch_enc<1, 1, 0>(rows, n_rows, max_out, enc, pcm, n_in, taps, hist, out, out_stride, s); break;
  }
}

}  // namespace lvx
