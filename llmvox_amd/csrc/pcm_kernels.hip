// PCM output stage (include/llmvox.h, "PCM output stage"): rational polyphase resampling of the codec's
// 24 kHz fp32 rows to 16 / 8 / 48 kHz and the s16le quantisation, one kernel family templated on
// (L, M, N, encoding). Launched only for a stream that asked for another format than f32le at 24 kHz.
#include <algorithm>

#include "lvx_internal.h"

namespace lvx {

namespace {

constexpr int PCM_THREADS = 256;
constexpr int PCM_PER_THREAD = 4;                        // consecutive outputs of a thread: one 8 / 16 byte store
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
  // segment input g (t0 - PCM_HIST <= g < t1) from the call's row or the slot's history; zero outside the segment
  auto input = [&](long long g) -> float {
    if (g < 0 || g >= t1) return 0.f;
    if (g >= r.t0) return x[g - r.t0];
    const long long back = r.t0 - g;
    return back <= PCM_HIST ? hist[r.hist_in + PCM_HIST - back] : 0.f;
  };
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
        const long long mm = (m_first + ml + e) * M;
        const long long ilo = ceil_div(mm - N, L);
        int t = (int)(mm - ilo * L);  // the first tap index: in (N - L, N]
        int k = (int)(ilo - i0);
        // inputs in ascending order, each product and each sum rounded to fp32 (no fused multiply-add:
        // the compiler would contract the pair, __fmul_rn / __fadd_rn included, without the pragma): the
        // rule's fixed order, which a host evaluation in fp32 reproduces bit for bit
        for (; t >= -N; t -= L, ++k) {
#pragma clang fp contract(off)
          const float prod = s_x[k] * s_h[t + N];
          acc = acc + prod;
        }
      }
      v[e] = acc;
    }
  }

  unsigned char* orow = out + (size_t)r.row * (size_t)out_stride;
  const bool full = ml + PCM_PER_THREAD <= nb;
  if constexpr (ENC == LVX_PCM_S16LE) {
    int16_t* o = reinterpret_cast<int16_t*>(orow) + mb + ml;
    if (full && (reinterpret_cast<uintptr_t>(o) & 7) == 0) {
      uint2 w;
      w.x = (uint32_t)(uint16_t)pcm_q16(v[0]) | ((uint32_t)(uint16_t)pcm_q16(v[1]) << 16);
      w.y = (uint32_t)(uint16_t)pcm_q16(v[2]) | ((uint32_t)(uint16_t)pcm_q16(v[3]) << 16);
      *reinterpret_cast<uint2*>(o) = w;
    } else {
#pragma unroll
      for (int e = 0; e < PCM_PER_THREAD; ++e)
        if (ml + e < nb) o[e] = (int16_t)pcm_q16(v[e]);
    }
  } else {
    float* o = reinterpret_cast<float*>(orow) + mb + ml;
    if (full && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < PCM_PER_THREAD; ++e)
        if (ml + e < nb) o[e] = v[e];
    }
  }
}

template <int L, int M, int N>
void launch_enc(const PcmRows& rows, int n_rows, int max_out, int enc, const float* pcm, int n_in, const float* taps,
                float* hist, void* out, long long out_stride, hipStream_t s) {
  const dim3 grid((unsigned)std::max(1, (max_out + PCM_OB - 1) / PCM_OB), (unsigned)n_rows);
  if (enc == LVX_PCM_S16LE)
    pcm_convert_kernel<L, M, N, LVX_PCM_S16LE><<<grid, PCM_THREADS, 0, s>>>(rows, pcm, n_in, taps, hist,
                                                                            (unsigned char*)out, out_stride);
  else
    pcm_convert_kernel<L, M, N, LVX_PCM_F32LE><<<grid, PCM_THREADS, 0, s>>>(rows, pcm, n_in, taps, hist,
                                                                            (unsigned char*)out, out_stride);
}

}  // namespace

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
