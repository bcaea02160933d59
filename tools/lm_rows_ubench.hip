// Development micro-benchmark: the load phase of a fused ln_f + lm_head block (ar_lm_rows_kernel). A block is
// (vocab slice of NCOL columns) x (group of R batch rows): it loads gamma (3 KB), x and the four pending copies of
// its R rows (15 KB of fp32 per row, R / 4 rows per wave) and its NCOL / 16 column tiles of the fragment-packed
// [4096][768] bf16 matrix (24 KB per tile, wave w the k-steps [6w, 6w + 6) of every tile) through a ring of at most
// 24 uint4 per lane, every refill behind its use. R = 4 / 8 / 16 with 128 / 64 / 32 columns: 257 / 221 / 294 KB per
// block, B / R x 4096 / NCOL blocks, in ar_lm_rows_kernel's order (the groups of a slice on one XCD, each starting at
// another tile). Timed in-kernel (s_memrealtime, 100 MHz) from block entry to the last byte landed. A producer
// kernel rewrites the rows before every launch, so they miss L2 as in the step, and the matrix is one of 16 each
// launch (100 MB cycled): the first block of a slice to ask misses its XCD's L2.
// hipcc -O3 --offload-arch=gfx950 tools/lm_rows_ubench.hip -o tools/lm_rows_ubench && tools/lm_rows_ubench
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int TILES = 256, TILE_U4 = 24 * 64;       // 16-row tiles of the matrix, uint4 per tile (24 k-steps x 64 lanes)
constexpr size_t MAT_U4 = (size_t)TILES * TILE_U4;  // 6,291,456 B
constexpr int NMAT = 16;
constexpr int ROW_U4 = 5 * 192;                     // x and four copies of one row, uint4
constexpr int MAXB = 32;

__global__ void produce(uint4* rows, unsigned v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < MAXB * ROW_U4) rows[i] = make_uint4(v, v + 1, v + 2, v + 3);
}

template <int R, int NCOL>
__global__ __launch_bounds__(256) void loads(const uint4* __restrict__ w, const uint4* __restrict__ rows,
                                             const uint4* __restrict__ gamma, int B, uint64_t* ts, unsigned* sink) {
  constexpr int NT = NCOL / 16, RW = R / 4, NL = NT * 6, INFL = NL < 24 ? NL : 24;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int G = (B + R - 1) / R, id = blockIdx.x, g = (id >> 3) % G, sl = (id / (8 * G)) * 8 + (id & 7);
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  uint4 gm[3], xr[RW][15];
#pragma unroll
  for (int j = 0; j < 3; ++j) gm[j] = gamma[j * 64 + lane];
#pragma unroll
  for (int i = 0; i < RW; ++i) {
    const int b = min(g * R + wave * RW + i, B - 1);
#pragma unroll
    for (int c = 0; c < 5; ++c)  // x, then the copies, 3 KB each
#pragma unroll
      for (int j = 0; j < 3; ++j) xr[i][c * 3 + j] = rows[(size_t)b * ROW_U4 + c * 192 + j * 64 + lane];
  }
  const int rot = g % NT;
  auto src = [&](int l) {  // load l of this lane: the (l / 6)-th tile this block runs, k-step 6 wave + l % 6
    int t = l / 6 + rot;
    if (t >= NT) t -= NT;
    return w + ((size_t)(sl * NT + t) * 24 + wave * 6 + l % 6) * 64 + lane;
  };
  uint4 r[INFL];
  unsigned x = 0;
#pragma unroll
  for (int l = 0; l < INFL; ++l) r[l] = *src(l);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < 3; ++j) x ^= (gm[j].x ^ gm[j].y) ^ (gm[j].z ^ gm[j].w);
#pragma unroll
  for (int i = 0; i < RW; ++i)
#pragma unroll
    for (int j = 0; j < 15; ++j) x ^= (xr[i][j].x ^ xr[i][j].y) ^ (xr[i][j].z ^ xr[i][j].w);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    x ^= (r[l % INFL].x ^ r[l % INFL].y) ^ (r[l % INFL].z ^ r[l % INFL].w);  // (every dword used: the loads stay dwordx4)
    if (l + INFL < NL) r[l % INFL] = *src(l + INFL);
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();
  const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
  if (x == 0x9e3779b9u) sink[blockIdx.x] = x;  // (keeps the loads live)
  if (tid == 0) {
    ts[blockIdx.x * 2 + 0] = t0;
    ts[blockIdx.x * 2 + 1] = t1;
  }
}

template <int R, int NCOL>
static void run(int B, const uint4* w, uint4* rows, const uint4* gamma, uint64_t* ts, unsigned* sink) {
  const int G = (B + R - 1) / R * (4096 / NCOL), iters = 37;
  std::vector<double> dts, spans;
  std::vector<uint64_t> h(G * 2);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(produce, dim3((MAXB * ROW_U4 + 255) / 256), dim3(256), 0, 0, rows, (unsigned)it);
    hipLaunchKernelGGL((loads<R, NCOL>), dim3(G), dim3(256), 0, 0, w + (size_t)(it % NMAT) * MAT_U4, rows, gamma, B, ts, sink);
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
  const double bytes = 16.0 * 256 * (3 + R / 4 * 15 + NCOL / 16 * 6);
  const double med = dts[dts.size() / 2], p90 = dts[dts.size() * 9 / 10];
  printf("B %2d R %2d x %3d columns (%3d blocks, %3.0f KB each): entry->landed p50 %5.2f us p90 %5.2f max %5.2f => %5.1f GB/s "
         "per CU (p50); first entry->last landed p50 %5.2f us max %5.2f\n",
         B, R, NCOL, G, bytes / 1024, med, p90, dts.back(), bytes / med * 1e-3, spans[spans.size() / 2], spans.back());
}

int main() {
  uint4 *w, *rows, *gamma;
  uint64_t* ts;
  unsigned* sink;
  CK(hipMalloc(&w, NMAT * MAT_U4 * 16));
  CK(hipMemset(w, 1, NMAT * MAT_U4 * 16));
  CK(hipMalloc(&rows, (size_t)MAXB * ROW_U4 * 16));
  CK(hipMalloc(&gamma, 192 * 16));
  CK(hipMemset(gamma, 3, 192 * 16));
  CK(hipMalloc(&ts, 1024 * 2 * 8));
  CK(hipMalloc(&sink, 1024 * 4));
  for (int B : {9, 17, 32}) {
    run<4, 128>(B, w, rows, gamma, ts, sink);
    run<8, 64>(B, w, rows, gamma, ts, sink);
    run<16, 32>(B, w, rows, gamma, ts, sink);
  }
  return 0;
}
