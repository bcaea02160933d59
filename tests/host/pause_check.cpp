// Stand-alone check of the host side of the pause stage (llmvox_amd/csrc/pcm_host.h, "PCM pause" in include/llmvox.h):
// pause_slots (what lvx_pause_slots runs) over constructed sentences at every rate, encoding and length around a block's
// edge, held to llmvox.h's rule written here a second time (the textbook G.711 expansions, the f32 test in double, no
// shared arithmetic); the mark at the threshold's edges; the counts against brute force; the plan_pause rows of pcm_plan
// with the buffer turns; cap too small and the refusals, which move no slot's state. Built and run by
// tests/test_pause_host.py with the system compiler under AddressSanitizer and UBSan; exit status 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pcm_host.h"

using namespace lvx;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

// ---- the rule a second time ----
static int rule_ulaw(int c) {  // G.711's own expansion
  const int u = ~c & 0xFF;
  int t = ((u & 0x0F) << 3) + 0x84;
  t <<= (u & 0x70) >> 4;
  return (u & 0x80) ? 0x84 - t : t - 0x84;
}
static int rule_alaw(int c) {
  const int a = c ^ 0x55, seg = (a & 0x70) >> 4;
  int t = (a & 0x0F) << 4;
  if (seg == 0) t += 8;
  else if (seg == 1) t += 0x108;
  else t = (t + 0x108) << (seg - 1);
  return (a & 0x80) ? t : -t;
}
static bool rule_loud(int enc, const uint8_t* p) {
  if (enc == LVX_PCM_F32LE) {
    float v;
    std::memcpy(&v, p, 4);
    return std::isnan(v) || std::fabs((double)v) > 103.0 / 32768.0;
  }
  long q;
  if (enc == LVX_PCM_S16LE) {
    int16_t s;
    std::memcpy(&s, p, 2);
    q = s;
  } else {
    q = enc == LVX_PCM_ULAW ? rule_ulaw(*p) : rule_alaw(*p);
  }
  return std::labs(q) > 103;
}
static int rule_bytes(int enc) { return enc == LVX_PCM_F32LE ? 4 : enc == LVX_PCM_S16LE ? 2 : 1; }
static std::vector<uint8_t> rule_slots(int rate, int enc, const std::vector<uint8_t>& y, long long T, long long j0, long long j1) {
  const int bl = rate / 100, bps = rule_bytes(enc), slot = 8 + bl * bps;
  const uint8_t fill = enc == LVX_PCM_ULAW ? 0xFF : enc == LVX_PCM_ALAW ? 0xD5 : 0x00;
  std::vector<uint8_t> out;
  for (long long j = j0; j < j1; ++j) {
    const long long first = j * bl, end = std::min<long long>(first + bl, T);
    bool active = false;
    for (long long i = first; i < end; ++i) active = active || rule_loud(enc, &y[(size_t)i * bps]);
    const int n = (int)(end - first);
    out.push_back((uint8_t)(n & 0xFF));
    out.push_back((uint8_t)(n >> 8));
    out.push_back(active ? 1 : 0);
    out.push_back(end == T ? 1 : 0);
    out.insert(out.end(), 4, (uint8_t)0);
    out.insert(out.end(), y.begin() + (size_t)first * bps, y.begin() + (size_t)end * bps);
    out.insert(out.end(), (size_t)(bl - n) * bps, fill);
    CHECK((int)(out.size() % slot) == 0);
  }
  return out;
}
static long long brute_blocks(int bl, long long T, bool final) {
  long long k = 0;
  for (long long j = 0; j * bl < T; ++j)
    if (final || (j + 1) * bl < T) ++k;  // complete and followed by at least one more sample; a final call: every block
  return k;
}

// ---- the sentences ----
static unsigned g_lcg = 2463534242u;
static int rnd(int lo, int hi) {  // lo .. hi
  g_lcg = g_lcg * 1664525u + 1013904223u;
  return lo + (int)((g_lcg >> 8) % (unsigned)(hi - lo + 1));
}
static void put_sample(int enc, int q, std::vector<uint8_t>& y) {
  if (enc == LVX_PCM_F32LE) {
    const float v = (float)q / 32768.f;
    uint8_t b[4];
    std::memcpy(b, &v, 4);
    y.insert(y.end(), b, b + 4);
  } else if (enc == LVX_PCM_S16LE) {
    y.push_back((uint8_t)(q & 0xFF));
    y.push_back((uint8_t)((q >> 8) & 0xFF));
  } else {
    y.push_back((uint8_t)(enc == LVX_PCM_ULAW ? g711_ulaw(q) : g711_alaw(q)));
  }
}
// T samples; a block is noise of at most 60 on the 16-bit scale, and every other block (by `phase`) has one sample of 2,000 or more
static std::vector<uint8_t> sentence(int enc, int bl, long long T, int phase) {
  std::vector<uint8_t> y;
  for (long long i = 0; i < T; ++i) {
    const long long j = i / bl;
    const bool loud_block = ((j + phase) % 2) == 0, here = loud_block && (i % bl == (j * 7 + 3) % bl || i == T - 1);
    put_sample(enc, here ? rnd(2000, 30000) * (rnd(0, 1) ? 1 : -1) : rnd(-60, 60), y);
  }
  return y;
}

static const int kRates[] = {8000, 16000, 24000, 48000};
static const int kEncs[] = {LVX_PCM_F32LE, LVX_PCM_S16LE, LVX_PCM_ULAW, LVX_PCM_ALAW};

static void check_slots(int rate, int enc) {
  const int bl = pause_block(rate), bps = pcm_sample_bytes(enc), slot = pause_slot_bytes(bl, bps);
  CHECK(bl == rate / 100 && bps == rule_bytes(enc) && slot == LVX_PAUSE_SLOT(rate, bps) && slot % 8 == 0 && bl * bps <= PAUSE_HIST);
  const long long lengths[] = {1, bl - 1, bl, bl + 1, 2 * bl, 3 * bl + 7, 0};
  int marks[2] = {0, 0};
  for (long long T : lengths)
    for (int phase = 0; phase < 2; ++phase) {
      const std::vector<uint8_t> y = sentence(enc, bl, T, phase);
      const long long K = pause_blocks_upto(bl, T, true);
      CHECK(K == (T + bl - 1) / bl && K == brute_blocks(bl, T, true));
      const std::vector<uint8_t> want = rule_slots(rate, enc, y, T, 0, K);
      std::vector<uint8_t> got(want.size() + 8, 0xA5);
      CHECK(pause_slots(rate, enc, y.data(), T, 0, K, got.data(), (long long)want.size()) == (long long)want.size());
      CHECK(std::equal(want.begin(), want.end(), got.begin()));
      for (size_t i = want.size(); i < got.size(); ++i) CHECK(got[i] == 0xA5);
      for (long long j = 0; j < K; ++j) {
        ++marks[want[(size_t)j * slot + 2]];
        CHECK(want[(size_t)j * slot + 2] == (((j + phase) % 2) == 0 ? 1 : 0));
        CHECK(want[(size_t)j * slot + 3] == (j == K - 1 ? 1 : 0));
      }
      for (long long j0 = 0; j0 <= K; ++j0)  // any range of blocks is that part of the whole
        for (long long j1 = j0; j1 <= K; ++j1) {
          std::vector<uint8_t> part((size_t)(j1 - j0) * slot + 1, 0xA5);
          CHECK(pause_slots(rate, enc, y.data(), T, j0, j1, part.data(), (long long)part.size()) == (j1 - j0) * slot);
          CHECK(std::equal(part.begin(), part.end() - 1, want.begin() + (size_t)j0 * slot) && part.back() == 0xA5);
        }
      if (K > 0) {  // cap one byte short: nothing is written
        std::vector<uint8_t> small(want.size() - 1, 0xA5);
        CHECK(pause_slots(rate, enc, y.data(), T, 0, K, small.data(), (long long)small.size()) == LVX_E_CAPACITY);
        for (uint8_t v : small) CHECK(v == 0xA5);
        CHECK(pause_slots(rate, enc, y.data(), T, 0, K + 1, got.data(), 1 << 20) == LVX_E_ARG);
        CHECK(pause_slots(rate, enc, nullptr, T, 0, K, got.data(), 1 << 20) == LVX_E_ARG);
        CHECK(pause_slots(rate, enc, y.data(), T, 0, K, nullptr, 1 << 20) == LVX_E_ARG);
        CHECK(pause_slots(rate, enc, y.data(), T, 1, 0, got.data(), 1 << 20) == LVX_E_ARG);
      }
    }
  CHECK(marks[0] > 0 && marks[1] > 0);
  std::vector<uint8_t> one(4, 0), out(8 + 4 * 480, 0xA5);
  CHECK(pause_slots(44100, enc, one.data(), 1, 0, 1, out.data(), 4096) == LVX_E_ARG);
  CHECK(pause_slots(rate, 2, one.data(), 1, 0, 1, out.data(), 4096) == LVX_E_ARG);
  CHECK(pause_slots(rate, enc, one.data(), -1, 0, 0, out.data(), 4096) == LVX_E_ARG);
  CHECK(pause_slots(rate, enc, nullptr, 0, 0, 0, nullptr, 0) == 0);  // a sentence of no samples: no slot
  for (uint8_t v : out) CHECK(v == 0xA5);
}

static int mark_of(int enc, const std::vector<uint8_t>& y) {
  std::vector<uint8_t> out(8 + 80 * 4);
  CHECK(pause_slots(8000, enc, y.data(), (long long)y.size() / rule_bytes(enc), 0, 1, out.data(), (long long)out.size()) > 0);
  return out[2];
}

static void check_edges() {
  const int s16[][2] = {{103, 0}, {-103, 0}, {104, 1}, {-104, 1}, {-32768, 1}, {32767, 1}, {0, 0}};
  for (const auto& c : s16) {
    std::vector<uint8_t> y;
    put_sample(LVX_PCM_S16LE, 0, y);
    put_sample(LVX_PCM_S16LE, c[0], y);
    CHECK(mark_of(LVX_PCM_S16LE, y) == c[1]);
  }
  const float t = 103.f / 32768.f;
  CHECK((double)t == 0.003143310546875);
  const float fs[] = {t, -t, std::nextafterf(t, 1.f), -std::nextafterf(t, 1.f), std::nanf(""), -std::nanf(""), INFINITY, 0.f, -0.f,
                      std::nextafterf(t, 0.f)};
  const int fw[] = {0, 0, 1, 1, 1, 1, 1, 0, 0, 0};
  for (int k = 0; k < 10; ++k) {
    std::vector<uint8_t> y(8, 0);
    std::memcpy(&y[4], &fs[k], 4);
    CHECK(mark_of(LVX_PCM_F32LE, y) == fw[k]);
  }
  for (int law : {LVX_PCM_ULAW, LVX_PCM_ALAW}) {
    int below = 0, above = 1 << 20;
    for (int c = 0; c < 256; ++c) {
      const int lin = law == LVX_PCM_ULAW ? rule_ulaw(c) : rule_alaw(c), m = std::abs(lin);
      CHECK(lin == (law == LVX_PCM_ULAW ? g711_ulaw_linear(c) : g711_alaw_linear(c)));
      if (m <= 103) below = std::max(below, m);
      else above = std::min(above, m);
      CHECK(mark_of(law, std::vector<uint8_t>{(uint8_t)c}) == (m > 103 ? 1 : 0));
    }
    CHECK(below == (law == LVX_PCM_ULAW ? 96 : 88) && above == 104);
    CHECK(mark_of(law, std::vector<uint8_t>(5, (uint8_t)pause_silence(law))) == 0);
  }
  CHECK(pause_silence(LVX_PCM_ULAW) == 0xFF && pause_silence(LVX_PCM_ALAW) == 0xD5 && rule_alaw(0xD5) == 8 && rule_ulaw(0xFF) == 0);
}

static void check_plan(int rate, int enc) {
  const int bl = pause_block(rate), bps = pcm_sample_bytes(enc), slot = pause_slot_bytes(bl, bps), S = 6;
  const long long key = pause_key(rate, enc);
  std::vector<PcmSeg> segs(S);
  bool capacity = false;
  auto call = [&](const std::vector<int32_t>& sl, const std::vector<uint8_t>& fl, int n_in, int r, int e, long long in_stride,
                  long long out_stride, std::vector<PauseRow>& rows, std::vector<int32_t>& n) {
    n.assign(sl.size(), -7);
    capacity = false;
    return pcm_plan(segs, PAUSE_HIST, (int)sl.size(), n_in, sl.data(), fl.data(), n.data(), pause_key(r, e), true,
                    [](long long k) { return std::to_string(k >> 8) + " Hz"; }, rows,
                    [&](const PcmCall& c, PauseRow& row) { return plan_pause(c, n_in, r, e, in_stride, out_stride, &capacity, row); });
  };
  const long long WIDE = 1 << 24;
  std::vector<PauseRow> rows;
  std::vector<int32_t> n;
  const int steps[] = {1, 17, bl + 16, 1000, 0, bl - 1, bl, bl + 1, 3 * bl + 7};
  for (int step : steps) {
    long long T = 0, emitted = 0;
    uint8_t par = segs[2].par;
    const int calls = step == 1 ? 2 * bl + 3 : 7;
    for (int c = 0; c < calls; ++c) {
      const bool final = c == calls - 1;
      CHECK(call({4, 2}, {0, (uint8_t)final}, step, rate, enc, (long long)step * bps, WIDE, rows, n).empty());
      const long long want = brute_blocks(bl, T + step, final) - brute_blocks(bl, T, false);
      CHECK(n[1] == want && rows[1].n_out == want && rows[1].t0 == T && rows[1].j0 == emitted && rows[1].row == 1);
      CHECK(rows[1].last == (final ? 1 : 0) && rows[1].hist_in == (par * S + 2) * PAUSE_HIST);
      if (step > 0 && !final) {
        CHECK(rows[1].hist_out == ((1 - par) * S + 2) * PAUSE_HIST);
        par ^= 1;
      } else {
        CHECK(rows[1].hist_out == -1);
      }
      if (want > 0) {
        const long long last = final ? T + step - (emitted + want - 1) * bl : bl;
        CHECK(rows[1].last_n == last && last >= 1 && last <= bl);
      }
      CHECK(emitted * bl >= T - bl);  // the call's first block starts inside what the slot kept
      T += step;
      emitted += want;
      if (!final && T > 0) CHECK(T - emitted * bl >= 1 && T - emitted * bl <= bl);  // held back: 1 .. bl samples
      if (final) CHECK(emitted == (T + bl - 1) / bl);
      CHECK(final ? segs[2].key == PcmSeg::NONE && segs[2].t0 == 0 : segs[2].key == key && segs[2].t0 == T);
      CHECK(segs[2].par == par);
    }
    CHECK(call({4}, {1}, 0, rate, enc, 0, WIDE, rows, n).empty());  // (the companion's segment ends too)
  }
  // the refusals: no slot's state changes
  CHECK(call({1, 3}, {0, 0}, 40, rate, enc, 40ll * bps, WIDE, rows, n).empty());
  const std::vector<PcmSeg> before = segs;
  auto unchanged = [&] {
    for (int s = 0; s < S; ++s)
      CHECK(segs[s].t0 == before[s].t0 && segs[s].key == before[s].key && segs[s].par == before[s].par && segs[s].aux == before[s].aux);
    for (int32_t v : n) CHECK(v == -7);
  };
  const int other_rate = rate == 8000 ? 16000 : 8000, other_enc = enc == LVX_PCM_ULAW ? LVX_PCM_ALAW : LVX_PCM_ULAW;
  CHECK(!call({0, 1}, {0, 0}, 40, other_rate, enc, 160, WIDE, rows, n).empty() && !capacity);  // open at another rate
  unchanged();
  CHECK(!call({0, 1}, {0, 0}, 40, rate, other_enc, 160, WIDE, rows, n).empty() && !capacity);  // open at another encoding
  unchanged();
  CHECK(!call({0, 3, 0}, {0, 0, 0}, 40, rate, enc, 160, WIDE, rows, n).empty() && !capacity);  // named twice
  unchanged();
  CHECK(!call({0, S}, {0, 0}, 40, rate, enc, 160, WIDE, rows, n).empty() && !call({-1}, {0}, 40, rate, enc, 160, WIDE, rows, n).empty());
  unchanged();
  CHECK(!call({0, 1}, {0, 0}, 40, rate, enc, 40ll * bps - 1, WIDE, rows, n).empty() && !capacity);  // in_stride smaller than a row
  unchanged();
  CHECK(!call({0, 1}, {0, 1}, 3 * bl, rate, enc, 3ll * bl * bps, 4ll * slot - 8, rows, n).empty() && capacity);  // out_stride: the second row's four slots
  unchanged();
  CHECK(call({0, 1}, {0, 1}, 3 * bl, rate, enc, 3ll * bl * bps, 4ll * slot, rows, n).empty() && !capacity);
  CHECK(n[0] == 2 && n[1] == 4);  // the next call is the one it would have been: 3 bl fresh, and 40 + 3 bl to the end
}

int main() {
  for (int rate : kRates)
    for (int enc : kEncs) {
      check_slots(rate, enc);
      check_plan(rate, enc);
    }
  check_edges();
  CHECK(pause_block(44100) == 0 && pcm_sample_bytes(2) == 0);
  std::printf("pause host check: ok\n");
  return 0;
}
