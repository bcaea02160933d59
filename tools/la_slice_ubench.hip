// Development micro-benchmark: how fast can one attention block stream its head's slice of c_attn's
// weights -- 288 of the 2,304 rows of a fragment-packed [2304][768] bf16 matrix, 18 column tiles of 24 KB
// = 442,368 B -- into registers while the B - 1 other blocks of the same head (same XCD: head = block id
// mod 8) stream the same slice? B x 8 blocks of 256 threads; wave w owns k-steps [6w, 6w + 6) of every
// tile (6 KB contiguous per wave per tile, as ar_mfma2_kernel reads a.Wf); INFL uint4 loads in flight per
// lane through a register ring, every refill right behind its use. Timed in-kernel (s_memrealtime,
// 100 MHz) from block entry to the last byte landed. KV = 1: two KV tiles of the attention's shape (per
// lane 3 + 3 uint4 of K and V per tile, distinct lines per block) are issued ahead of the stream and
// waited for with it, as the fused block holds them while it forms q / k / v. A different matrix of 16
// each launch (56 MB cycled): the first block of a head to ask misses its XCD's L2, as in the step.
// hipcc -O3 --offload-arch=gfx950 tools/la_slice_ubench.hip -o tools/la_slice_ubench && tools/la_slice_ubench
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int TILES = 144, TILE_U4 = 24 * 64;      // 16-row tiles of the matrix, uint4 per tile (24 k-steps x 64 lanes)
constexpr size_t MAT_U4 = (size_t)TILES * TILE_U4;  // 3,538,944 B
constexpr int NMAT = 16;
constexpr int KV_U4 = 2 * 6 * 256;                  // uint4 per block of two KV tiles

template <int INFL, int KV>
__global__ __launch_bounds__(256) void stream(const uint4* __restrict__ w, const uint4* __restrict__ kv, uint64_t* ts,
                                              unsigned* sink) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, head = blockIdx.x & 7;
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  uint4 kvr[KV ? 12 : 1];
  if constexpr (KV) {
#pragma unroll
    for (int i = 0; i < 12; ++i) kvr[i] = kv[(size_t)blockIdx.x * KV_U4 + i * 256 + tid];
  }
  // load l of this lane: tile (l / 6) of the head's 18 (q, k, v: 6 each, 48 tiles apart), k-step 6 wave + l % 6
  auto src = [&](int l) {
    const int i = l / 6, tile = (i / 6) * 48 + head * 6 + i % 6;
    return w + ((size_t)tile * 24 + wave * 6 + l % 6) * 64 + lane;
  };
  uint4 r[INFL];
  unsigned x = 0;
#pragma unroll
  for (int l = 0; l < INFL; ++l) r[l] = *src(l);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int l = 0; l < 108; ++l) {
    x ^= (r[l % INFL].x ^ r[l % INFL].y) ^ (r[l % INFL].z ^ r[l % INFL].w);  // (every dword used: the loads stay dwordx4)
    if (l + INFL < 108) r[l % INFL] = *src(l + INFL);
    __builtin_amdgcn_sched_barrier(0);
  }
  if constexpr (KV) {
#pragma unroll
    for (int i = 0; i < 12; ++i) x ^= (kvr[i].x ^ kvr[i].y) ^ (kvr[i].z ^ kvr[i].w);
  }
  __syncthreads();
  const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
  if (x == 0x9e3779b9u) sink[blockIdx.x] = x;  // (keeps the loads live)
  if (tid == 0) {
    ts[blockIdx.x * 2 + 0] = t0;
    ts[blockIdx.x * 2 + 1] = t1;
  }
}

template <int INFL, int KV>
static void run(int B, const uint4* w, const uint4* kv, uint64_t* ts, unsigned* sink) {
  const int G = B * 8, iters = 37;
  std::vector<double> dts, spans;
  std::vector<uint64_t> h(G * 2);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL((stream<INFL, KV>), dim3(G), dim3(256), 0, 0, w + (size_t)(it % NMAT) * MAT_U4, kv, ts, sink);
    CK(hipDeviceSynchronize());
    if (it < 5) continue;  // warm-up
    CK(hipMemcpy(h.data(), ts, G * 2 * 8, hipMemcpyDeviceToHost));
    uint64_t mn = ~0ull, mx = 0;
    for (int b = 0; b < G; ++b) {
      dts.push_back((h[b * 2 + 1] - h[b * 2]) * 0.01);  // us
      mn = std::min(mn, h[b * 2]);
      mx = std::max(mx, h[b * 2 + 1]);
    }
    spans.push_back((mx - mn) * 0.01);
  }
  std::sort(dts.begin(), dts.end());
  std::sort(spans.begin(), spans.end());
  const double bytes = 16.0 * 108 * 256;
  const double med = dts[dts.size() / 2], p90 = dts[dts.size() * 9 / 10];
  printf("B %2d (%3d blocks) in flight %2d kv %d: entry->landed p50 %5.2f us p90 %5.2f max %5.2f => %5.1f GB/s per CU (p50), "
         "%5.1f (p90); launch span p50 %5.2f us\n",
         B, G, INFL, KV, med, p90, dts.back(), bytes / med * 1e-3, bytes / p90 * 1e-3, spans[spans.size() / 2]);
}

int main() {
  uint4 *w, *kv;
  uint64_t* ts;
  unsigned* sink;
  CK(hipMalloc(&w, NMAT * MAT_U4 * 16));
  CK(hipMemset(w, 1, NMAT * MAT_U4 * 16));
  CK(hipMalloc(&kv, (size_t)256 * KV_U4 * 16));
  CK(hipMemset(kv, 2, (size_t)256 * KV_U4 * 16));
  CK(hipMalloc(&ts, 256 * 2 * 8));
  CK(hipMalloc(&sink, 256 * 4));
  for (int B : {9, 16, 32}) {
    run<8, 0>(B, w, kv, ts, sink);
    run<16, 0>(B, w, kv, ts, sink);
    run<24, 0>(B, w, kv, ts, sink);
    run<8, 1>(B, w, kv, ts, sink);
    run<16, 1>(B, w, kv, ts, sink);
    run<24, 1>(B, w, kv, ts, sink);
  }
  return 0;
}
