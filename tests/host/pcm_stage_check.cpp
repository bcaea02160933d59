// Stand-alone check of the PCM stages' host skeleton (llmvox_amd/csrc/pcm_host.h): the planning, the commit and the
// packets of every stage without a device, the launches only recorded. Built and run by tests/test_pcm_stage_host.py
// with the system compiler under AddressSanitizer and UBSan; exit status 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <functional>

#include "pcm_host.h"

using namespace lvx;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: [%s] %s\n", __FILE__, __LINE__, g_stage, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static const char* g_stage = "";
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

static int row_in(const JoinRow& r) { return r.tail_in; }
template <class Row> int row_in(const Row& r) { return r.hist_in; }

// what an entry point does with the skeleton, the launch recorded instead of made
template <class Rows, class Row, class KeyText, class Plan>
Out run(std::vector<PcmSeg>& segs, int hist, const Slots& slots, const Finals& finals, int n_in, long long key, bool advance,
        bool launch, KeyText key_text, Plan plan) {
  Out o;
  const int B = (int)slots.size();
  o.n.assign(B, -7);
  std::vector<Row> rows;
  o.err = pcm_plan(segs, hist, B, n_in, slots.data(), finals.data(), o.n.data(), key, advance, key_text, rows, plan);
  if (!o.err.empty() || !launch) return o;
  for (const Row& r : rows) {
    o.in.push_back(row_in(r));
    o.out.push_back(row_kept(r));
  }
  pcm_chunks<Rows>(rows, [&](const Rows& pk, int nr, int max_out) { o.launches.push_back(Launch{nr, max_out, pk.r[0].row}); });
  return o;
}

static std::string plain(long long k) { return std::to_string(k); }

// a keyed stage: its call at a parameter and its closed form
struct Stage {
  const char* name;
  long long p, other, identity;
  bool identity_advances;
  std::function<Out(std::vector<PcmSeg>&, const Slots&, const Finals&, int, long long, long long)> call;
  std::function<long long(long long, long long, bool)> upto;
};

static const Stage kStages[] = {
    {"convert", 16000, 8000, 24000, true,
     [](std::vector<PcmSeg>& g, const Slots& sl, const Finals& fl, int n_in, long long rate, long long stride) {
       const PcmRate* pr = pcm_rate_of((int)rate);
       const bool launch = pr->N != 0;  // (f32le)
       return run<PcmRows, PcmRow>(g, PCM_HIST, sl, fl, n_in, rate, true, launch, plain,
                                   [&](const PcmCall& c, PcmRow& r) { return plan_convert(c, n_in, *pr, 4, launch, stride, r); });
     },
     [](long long rate, long long T, bool f) { return pcm_emitted_upto(*pcm_rate_of((int)rate), T, f); }},
    {"stretch", 130, 77, 100, false,
     [](std::vector<PcmSeg>& g, const Slots& sl, const Finals& fl, int n_in, long long pct, long long stride) {
       return run<StretchRows, StretchRow>(g, STR_HIST, sl, fl, n_in, pct, pct != 100, pct != 100, plain, [&](const PcmCall& c, StretchRow& r) {
         return plan_stretch(c, n_in, (int)pct, stride, false, 0, r);
       });
     },
     [](long long pct, long long T, bool f) { return stretch_emitted_upto((int)pct, T, f); }},
    {"ratio", ratio_key(4, 5), ratio_key(133, 120), ratio_key(1, 1), false,
     [](std::vector<PcmSeg>& g, const Slots& sl, const Finals& fl, int n_in, long long k, long long stride) {
       const int L = (int)(k >> 16), M = (int)(k & 0xffff);
       return run<RatioRows, RatioRow>(g, RAT_HIST, sl, fl, n_in, k, L != M, L != M, plain,
                                       [&](const PcmCall& c, RatioRow& r) { return plan_ratio(c, n_in, L, M, stride, r); });
     },
     [](long long k, long long T, bool f) {
       const int L = (int)(k >> 16), M = (int)(k & 0xffff);
       return pcm_emitted_upto(L, M, ratio_N(L, M), T, f);
     }},
    {"level", 250, 0, 100, false,
     [](std::vector<PcmSeg>& g, const Slots& sl, const Finals& fl, int n_in, long long pct, long long stride) {
       return run<PcmRows, PcmRow>(g, LVL_HIST, sl, fl, n_in, pct, pct != 100, pct != 100, plain, [&](const PcmCall& c, PcmRow& r) {
         return plan_level(c, n_in, (int)pct, stride, true, stride, r);
       });
     },
     [](long long pct, long long T, bool f) { return level_emitted_upto((int)pct, T, f); }},
};

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

static void check_stage(const Stage& st) {
  g_stage = st.name;
  std::vector<PcmSeg> g(S);
  const Slots three{0, 1, 2};
  const Finals go(3, 0), end(3, 1);
  auto count = [&](long long p, long long t0, int n, bool f) { return (int32_t)(st.upto(p, t0 + n, f) - st.upto(p, t0, false)); };

  // 1. a refused call of every kind moves no record and writes no count; the good call behind them is a first call
  CHECK(st.call(g, {5}, {0}, N_IN, st.p, WIDE).err.empty());
  const std::vector<PcmSeg> before = g;
  for (const Out& o : {st.call(g, {0, S}, {0, 0}, N_IN, st.p, WIDE), st.call(g, {0, -1}, {0, 0}, N_IN, st.p, WIDE),
                       st.call(g, {1, 0, 1}, go, N_IN, st.p, WIDE), st.call(g, {0, 5}, {0, 0}, N_IN, st.other, WIDE),
                       st.call(g, three, go, N_IN, st.p, 4)}) {
    CHECK(!o.err.empty() && same(g, before) && o.launches.empty());
    for (int32_t n : o.n) CHECK(n == -7);
  }
  CHECK(st.call(g, {0, 5}, {0, 0}, N_IN, st.other, WIDE).err.find("slot 5: its segment is open at ") == 0);
  Out o = st.call(g, three, go, N_IN, st.p, WIDE);
  CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, count(st.p, 0, N_IN, false)) && o.launches.size() == 1);

  // 2. two more calls: the counts are the closed form's, the buffers alternate, and a call reads what the last wrote
  std::vector<int> first_in = o.in, last_out = o.out;
  for (int k = 1; k < 3; ++k) {
    o = st.call(g, three, go, N_IN, st.p, WIDE);
    CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, count(st.p, (long long)k * N_IN, N_IN, false)));
    CHECK(o.n[0] > 0 && o.in == last_out && (k == 1 ? o.out == first_in : o.in == first_in));
    for (int b = 0; b < 3; ++b) CHECK(o.in[b] != o.out[b] && o.out[b] >= 0 && g[b].t0 == (long long)(k + 1) * N_IN && g[b].key == st.p);
    last_out = o.out;
  }

  // 3. a final call emits the rest and closes the segment (the buffers stay turned): another key may follow
  o = st.call(g, three, end, N_IN, st.p, WIDE);
  CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, count(st.p, 3 * N_IN, N_IN, true)));
  CHECK(st.upto(st.p, 0, false) == 0 && o.out == std::vector<int>(3, -1));
  for (int b = 0; b < 3; ++b) CHECK(g[b].t0 == 0 && g[b].aux == 0 && g[b].key == PcmSeg::NONE && g[b].par == 1);
  o = st.call(g, three, end, N_IN, st.other, WIDE);
  CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, count(st.other, 0, N_IN, true)));
  o = st.call(g, {5}, {1}, 0, st.p, WIDE);  // (the slot the first step opened)
  CHECK(o.err.empty() && o.n[0] == count(st.p, N_IN, 0, true) && o.n[0] > 0);

  // 4. 33 rows are packets of 32 and 1; a packet whose rows have nothing to emit or keep is not launched
  const Slots all = iota(33);
  o = st.call(g, all, Finals(33, 0), N_IN, st.p, WIDE);
  CHECK(o.err.empty() && o.launches.size() == 2);
  CHECK(o.launches[0].rows == 32 && o.launches[0].first_row == 0 && o.launches[1].rows == 1 && o.launches[1].first_row == 32);
  CHECK(o.launches[1].max_out == o.n[32]);
  o = st.call(g, iota(32), Finals(32, 1), 0, st.p, WIDE);
  CHECK(o.err.empty() && o.launches.size() == 1 && o.launches[0].rows == 32);
  o = st.call(g, all, Finals(33, 1), 0, st.p, WIDE);  // rows 0 .. 31 are closed: only row 32 has a rest
  CHECK(o.err.empty() && o.n[0] == 0 && o.n[31] == 0 && o.n[32] == count(st.p, N_IN, 0, true) && o.n[32] > 0);
  CHECK(o.launches.size() == 1 && o.launches[0].rows == 1 && o.launches[0].first_row == 32);
  o = st.call(g, all, Finals(33, 1), 0, st.p, WIDE);  // and now none has
  CHECK(o.err.empty() && o.launches.empty());

  // 5. the identity: the rows are the output; only the rate conversion's mirror advances
  const std::vector<PcmSeg> closed = g;
  o = st.call(g, three, go, N_IN, st.identity, 0);
  CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, N_IN) && o.launches.empty());
  if (st.identity_advances) {
    for (int b = 0; b < 3; ++b) CHECK(g[b].t0 == N_IN && g[b].key == st.identity && g[b].par == closed[b].par);
    CHECK(!st.call(g, three, go, N_IN, st.p, WIDE).err.empty());  // (open at 24 kHz)
  } else {
    CHECK(same(g, closed));
  }
  CHECK(st.call(g, three, end, 0, st.identity, 0).err.empty() && same(g, closed));
  CHECK(st.call(g, {7}, {0}, N_IN, st.p, WIDE).err.empty());
  CHECK(!st.call(g, {7}, {1}, N_IN, st.identity, 0).err.empty() && g[7].key == st.p);  // an identity call still minds the key
}

// 6. volume 0 is a volume: a slot open at 0 refuses 50 (the "none open" state is not 0)
static void check_level_zero() {
  g_stage = "level at 0";
  const Stage& st = kStages[3];
  std::vector<PcmSeg> g(S);
  Out o = st.call(g, {3}, {0}, N_IN, 0, WIDE);
  CHECK(o.err.empty() && g[3].key == 0 && o.n[0] == N_IN - 2 * LVL_A);
  o = st.call(g, {3}, {0}, N_IN, 50, WIDE);
  CHECK(o.err == "slot 3: its segment is open at 0" && g[3].t0 == N_IN);
  CHECK(st.call(g, {3}, {1}, N_IN, 0, WIDE).n[0] == N_IN + 2 * LVL_A);
}

// the join: no key, a tail kept by every call that is not final, and the counts of join_emitted
static void check_join() {
  g_stage = "join";
  std::vector<PcmSeg> g(S);
  auto call = [&](const Slots& sl, const Finals& fl, int n_in, int ctx, long long stride) {
    return run<JoinRows, JoinRow>(g, JOIN_HOLD, sl, fl, n_in, 0, true, true, plain,
                                  [&](const PcmCall& c, JoinRow& r) { return plan_join(c, n_in, ctx, stride, r); });
  };
  const Slots three{0, 1, 2};
  const Finals go(3, 0), end(3, 1);
  const std::vector<PcmSeg> before = g;
  for (const Out& o : {call({0, S}, {0, 0}, N_IN, 0, WIDE), call({1, 0, 1}, go, N_IN, 0, WIDE), call(three, go, N_IN, 0, 4),
                       call(three, go, N_IN + 1, 0, WIDE), call(three, go, N_IN, 1, WIDE)}) {  // (context on a closed segment)
    CHECK(!o.err.empty() && same(g, before) && o.launches.empty());
    for (int32_t n : o.n) CHECK(n == -7);
  }
  Out o = call(three, go, N_IN, 0, WIDE);
  CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, join_emitted(false, 0, N_IN, false)) && o.n[0] == N_IN - JOIN_HOLD);
  const std::vector<int> first_in = o.in;
  std::vector<int> last_out = o.out;
  o = call(three, go, JOIN_HOLD, 0, WIDE);  // one frame: it emits the held one and keeps its own
  CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, JOIN_HOLD) && o.in == last_out && o.out == first_in);
  last_out = o.out;
  o = call(three, go, N_IN, 1, WIDE);
  CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, join_emitted(true, 1, N_IN, false)) && o.in == last_out && o.in == first_in);
  o = call(three, end, N_IN, 0, WIDE);
  CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, join_emitted(true, 0, N_IN, true)) && o.n[0] == N_IN + JOIN_HOLD);
  for (int b = 0; b < 3; ++b) CHECK(g[b].key == PcmSeg::NONE && g[b].par == 1);
  CHECK(!call(three, go, N_IN, 1, WIDE).err.empty());  // closed again: no context
  o = call(iota(33), Finals(33, 0), N_IN, 0, WIDE);
  CHECK(o.err.empty() && o.launches.size() == 2 && o.launches[0].rows == 32 && o.launches[1].rows == 1 && o.launches[1].first_row == 32);
  o = call(iota(32), Finals(32, 1), 0, 0, WIDE);
  CHECK(o.err.empty() && o.launches.size() == 1 && o.n[0] == JOIN_HOLD);
  o = call(iota(33), Finals(33, 1), 0, 0, WIDE);  // the flush of 32 closed slots and an open one
  CHECK(o.err.empty() && o.n[31] == 0 && o.n[32] == JOIN_HOLD && o.launches.size() == 1 && o.launches[0].first_row == 32);
  CHECK(call(iota(33), Finals(33, 1), 0, 0, WIDE).launches.empty());
}

int main() {
  for (const Stage& st : kStages) check_stage(st);
  check_level_zero();
  check_join();
  std::puts("pcm stage host check: ok");
  return 0;
}
