// Stand-alone check of the watermark stage's host side (llmvox_amd/csrc/pcm_host.h): the sign table against its
// definition written a second time, its digest, the streaming counts, and plan_mark through the skeleton pcm_plan /
// pcm_chunks without a device, the launches only recorded. Built and run by tests/test_mark_host.py with the system
// compiler under AddressSanitizer and UBSan; exit status 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <set>

#include "pcm_host.h"

using namespace lvx;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

constexpr int S = 40, N_IN = 640;
constexpr long long WIDE = 1 << 20;  // a stride no row outgrows
typedef std::vector<int32_t> Slots;
typedef std::vector<uint8_t> Finals;

struct Launch {
  int rows, max_out, first_row;
};
struct Out {
  std::string err;
  std::vector<int32_t> n;
  std::vector<int> in, out;  // per row: the buffer read and the buffer written (-1: none)
  std::vector<Launch> launches;
};
struct Mark {
  uint64_t key;
  int id, strength;
};

// what lvx_pcm_mark does with the skeleton, the launch recorded instead of made
static Out call(std::vector<PcmSeg>& g, const Slots& slots, const Finals& finals, int n_in, Mark m, long long stride) {
  Out o;
  const int B = (int)slots.size();
  o.n.assign(B, -7);
  std::vector<PcmRow> rows;
  CHECK(mark_ok(m.id, m.strength));
  const MarkTab mt = mark_table(m.key, m.id);
  o.err = pcm_plan(
      g, FMT_HIST, B, n_in, slots.data(), finals.data(), o.n.data(), mark_digest(mt, m.strength), true,
      [](long long) { return std::string("another mark"); }, rows, [&](const PcmCall& c, PcmRow& r) { return plan_mark(c, n_in, stride, r); });
  if (!o.err.empty()) return o;
  for (const PcmRow& r : rows) {
    o.in.push_back(r.hist_in);
    o.out.push_back(r.hist_out);
    CHECK(r.m0 % FMT_H == 0 && r.m0 == formant_emitted_upto(r.t0, false));
    // the call's first output reaches back at most 7 H - 1 inputs in front of the call's first
    if (r.n_out > 0) CHECK(r.t0 - (r.m0 / FMT_H - 3) * FMT_H <= FMT_HIST - 1);
  }
  pcm_chunks<PcmRows>(rows, [&](const PcmRows& pk, int nr, int max_out) { o.launches.push_back(Launch{nr, max_out, pk.r[0].row}); });
  return o;
}

static bool same(const std::vector<PcmSeg>& a, const std::vector<PcmSeg>& b) {
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].t0 != b[i].t0 || a[i].aux != b[i].aux || a[i].key != b[i].key || a[i].par != b[i].par) return false;
  return a.size() == b.size();
}

static Slots iota(int n) {
  Slots v(n);
  for (int i = 0; i < n; ++i) v[i] = i;
  return v;
}

// SplitMix64 a second time: the generator as a function of the index, not a running state
static unsigned chip(uint64_t key, int i) {
  uint64_t z = key + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (unsigned)((z ^ (z >> 31)) >> 63);
}

static void check_table() {
  // SplitMix64's published first output for the state 0
  {
    uint64_t z = 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    CHECK((z ^ (z >> 31)) == 0xE220A8397B1DCDAFull);
  }
  std::set<long long> digests;
  long long ones = 0;
  for (uint64_t key : {0ull, 1ull, 0x5EEDC0DEF00DFACEull, 0xFFFFFFFFFFFFFFFFull, 0x8000000000000000ull})
    for (int id : {0, 1, 0x5A, 0xA5, 255}) {
      const MarkTab t = mark_table(key, id), t0 = mark_table(key, 0);
      for (int p = 0; p < MRK_P; ++p) {
        CHECK(t.w[p] >> MRK_PAIRS == 0);
        for (int m = 0; m < MRK_PAIRS; ++m) {
          const int i = MRK_PAIRS * p + m;
          const unsigned bit = (t.w[p] >> m) & 1u;
          CHECK(bit == (chip(key, i) ^ ((id >> (i % 8)) & 1)));
          CHECK((bit ^ ((t0.w[p] >> m) & 1u)) == (unsigned)((id >> (i % 8)) & 1));  // the payload is an XOR on the key's signs
          ones += bit;
        }
      }
      for (int st = MRK_STRENGTH_MIN; st <= MRK_STRENGTH_MAX; ++st) {
        const long long d = mark_digest(t, st);
        CHECK(d >= 0 && d != PcmSeg::NONE && digests.insert(d).second);  // (25 tables x 3 strengths: all different)
      }
    }
  CHECK(ones > 25 * 768 * 2 / 5 && ones < 25 * 768 * 3 / 5);  // about half the bits are set
  // every payload bit has 96 chips in a period
  int chips[8] = {0};
  for (int i = 0; i < MRK_P * MRK_PAIRS; ++i) ++chips[i % 8];
  for (int b = 0; b < 8; ++b) CHECK(chips[b] == 96);
  CHECK(mark_a(1) == 1.f / 64 && mark_a(2) == 1.f / 32 && mark_a(3) == 1.f / 16);
  CHECK(!mark_ok(-1, 2) && !mark_ok(256, 2) && !mark_ok(0, 0) && !mark_ok(0, 4) && mark_ok(0, 1) && mark_ok(255, 3));
  CHECK(MRK_K0 * 24000 / FMT_N == 562 && (MRK_K0 + MRK_U * MRK_BW) * 24000 / FMT_N == 3375);  // the band in Hz
}

// the formant stage's counts: what plan_mark emits over any cutting adds up
static void check_counts() {
  std::vector<PcmSeg> g(1);
  unsigned seed = 99;
  for (int T : {1, 255, 256, 257, 1025, 7 * 256 + 5, 20000}) {
    long long t0 = 0, sum = 0;
    while (t0 < T) {
      seed = seed * 1664525u + 1013904223u;
      const int n = (int)std::min<long long>(T - t0, 1 + (seed >> 8) % 1500);
      const bool fin = t0 + n == T;
      const Out o = call(g, {0}, {(uint8_t)fin}, n, Mark{7, 1, 2}, WIDE);
      CHECK(o.err.empty() && o.n[0] == formant_emitted_upto(t0 + n, fin) - formant_emitted_upto(t0, false));
      sum += o.n[0];
      t0 += n;
      // held back behind a call that is not final: everything below 3 H inputs, then 768 .. 1023
      if (!fin) CHECK(t0 < 3 * FMT_H ? sum == 0 : (t0 - sum >= 3 * FMT_H && t0 - sum <= 4 * FMT_H - 1));
    }
    CHECK(sum == T && g[0].key == PcmSeg::NONE);
  }
}

static void check_skeleton() {
  std::vector<PcmSeg> g(S);
  const Slots three{0, 1, 2};
  const Finals go(3, 0), end(3, 1);
  const Mark mk{0x5EEDC0DEF00DFACEull, 0xA5, 2};
  auto count = [&](long long t0, int n, bool f) { return (int32_t)(formant_emitted_upto(t0 + n, f) - formant_emitted_upto(t0, false)); };

  // a refused call of every kind moves no record and writes no count: a slot out of range, one named twice, another
  // key, id or strength on an open segment, a stride too small
  CHECK(call(g, {5}, {0}, N_IN, mk, WIDE).err.empty());
  const std::vector<PcmSeg> before = g;
  for (const Out& o : {call(g, {0, S}, {0, 0}, N_IN, mk, WIDE), call(g, {0, -1}, {0, 0}, N_IN, mk, WIDE), call(g, {1, 0, 1}, go, N_IN, mk, WIDE),
                       call(g, {0, 5}, {0, 0}, N_IN, Mark{mk.key + 1, mk.id, mk.strength}, WIDE),
                       call(g, {0, 5}, {0, 0}, N_IN, Mark{mk.key, mk.id ^ 1, mk.strength}, WIDE),
                       call(g, {0, 5}, {0, 0}, N_IN, Mark{mk.key, mk.id, 3}, WIDE), call(g, three, end, N_IN, mk, 4)}) {
    CHECK(!o.err.empty() && same(g, before) && o.launches.empty());
    for (int32_t n : o.n) CHECK(n == -7);
  }
  CHECK(call(g, {0, 5}, {1, 1}, N_IN, Mark{mk.key, mk.id, 3}, WIDE).err == "slot 5: its segment is open at another mark");

  // four calls: the counts are the closed form's, the buffers alternate, a call reads what the last wrote
  Out o = call(g, three, go, N_IN, mk, WIDE);
  CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, 0) && o.launches.size() == 1);  // (nothing out, a history kept)
  std::vector<int> first_in = o.in, last_out = o.out;
  for (int k = 1; k < 4; ++k) {
    o = call(g, three, go, N_IN, mk, WIDE);
    CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, count((long long)k * N_IN, N_IN, false)) && o.n[0] > 0);
    CHECK(o.in == last_out && (k % 2 ? o.out == first_in : o.in == first_in));
    for (int b = 0; b < 3; ++b)
      CHECK(o.in[b] != o.out[b] && o.out[b] >= 0 && g[b].t0 == (long long)(k + 1) * N_IN && g[b].key == mark_digest(mark_table(mk.key, mk.id), mk.strength));
    last_out = o.out;
  }
  // a stride one sample short of the final call's output is refused; the final call emits the rest and closes
  const int32_t rest = count(4 * N_IN, N_IN, true);
  CHECK(rest > N_IN && !call(g, three, end, N_IN, mk, 4ll * rest - 4).err.empty());
  o = call(g, three, end, N_IN, mk, 4ll * rest);
  CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, rest) && o.out == std::vector<int>(3, -1));
  for (int b = 0; b < 3; ++b) CHECK(g[b].t0 == 0 && g[b].key == PcmSeg::NONE);
  CHECK(call(g, three, end, N_IN, Mark{1, 2, 3}, WIDE).n == std::vector<int32_t>(3, N_IN));  // another mark may follow
  o = call(g, {5}, {1}, 0, mk, WIDE);  // (the slot the first step opened: a flush-only final)
  CHECK(o.err.empty() && o.n[0] == N_IN && o.launches.size() == 1);

  // 33 rows are packets of 32 and 1; a packet whose rows have nothing to emit or keep is not launched
  o = call(g, iota(33), Finals(33, 0), 2 * N_IN, mk, WIDE);
  CHECK(o.err.empty() && o.launches.size() == 2 && o.launches[0].rows == 32 && o.launches[1].rows == 1 && o.launches[1].first_row == 32);
  CHECK(o.launches[1].max_out == o.n[32] && o.n[32] == 512);
  o = call(g, iota(32), Finals(32, 1), 0, mk, WIDE);
  CHECK(o.err.empty() && o.launches.size() == 1 && o.n[0] == 2 * N_IN - 512);
  o = call(g, iota(33), Finals(33, 1), 0, mk, WIDE);
  CHECK(o.err.empty() && o.n[31] == 0 && o.n[32] == 2 * N_IN - 512 && o.launches.size() == 1 && o.launches[0].first_row == 32);
  CHECK(call(g, iota(33), Finals(33, 1), 0, mk, WIDE).launches.empty());
}

int main() {
  check_table();
  check_counts();
  check_skeleton();
  std::puts("mark host check: ok");
  return 0;
}
