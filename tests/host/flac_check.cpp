// Stand-alone check of the host side of the FLAC stage (llmvox_amd/csrc/pcm_host.h, "PCM FLAC" in include/llmvox.h):
// flac_subframe and flac_finish (what lvx_flac_subframe / lvx_flac_finish run) over the test signals at every frame
// length around the cuts, held to llmvox.h's rule written here a second time (bits in a vector<bool>, bitwise CRCs, no
// shared arithmetic); the plan_flac counts of pcm_plan against brute force, with the buffer turns; cap too small,
// n = 0 and the argument errors. Built and run by tests/test_flac_host.py with the system compiler under
// AddressSanitizer and UBSan; exit status 0 when every check holds.
#include <cstdio>
#include <cstdlib>

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
typedef std::vector<bool> BitVec;
static void put(BitVec& b, unsigned long long v, int len) {
  for (int i = len - 1; i >= 0; --i) b.push_back((v >> i) & 1);
}
static std::vector<uint8_t> pack(const BitVec& b) {
  std::vector<uint8_t> o((b.size() + 7) / 8, 0);
  for (size_t i = 0; i < b.size(); ++i)
    if (b[i]) o[i / 8] |= (uint8_t)(0x80 >> (i % 8));
  return o;
}

static std::vector<uint8_t> rule_subframe(const std::vector<int16_t>& x, int* kind) {
  const int n = (int)x.size();
  BitVec b;
  bool same = true;
  for (int i = 1; i < n; ++i) same = same && x[i] == x[0];
  if (same) {
    put(b, 0, 8);
    put(b, (uint16_t)x[0], 16);
    *kind = -1;
    return pack(b);
  }
  // the differences, one after another
  std::vector<std::vector<long long>> r(5, std::vector<long long>(n, 0));
  for (int i = 0; i < n; ++i) r[0][i] = x[i];
  for (int p = 1; p <= 4; ++p)
    for (int i = p; i < n; ++i) r[p][i] = r[p - 1][i] - r[p - 1][i - 1];
  int p = 0;
  long long best = -1;
  for (int q = 0; q <= 4; ++q) {
    long long e = 0;
    for (int i = 4; i < n; ++i) e += r[q][i] < 0 ? -r[q][i] : r[q][i];
    if (best < 0 || e < best) {
      best = e;
      p = q;
    }
  }
  int P = 0;
  while (P < 3 && n % (2 << P) == 0) ++P;
  while (P > 0 && (n >> P) < 16) --P;
  std::vector<unsigned long long> u(n, 0);
  for (int i = p; i < n; ++i) u[i] = r[p][i] >= 0 ? 2 * r[p][i] : -2 * r[p][i] - 1;
  BitVec f;
  put(f, (8u | (unsigned)p) << 1, 8);
  for (int i = 0; i < p; ++i) put(f, (uint16_t)x[i], 16);
  put(f, 0, 2);
  put(f, (unsigned)P, 4);
  const int len = n >> P;
  for (int j = 0; j < (1 << P); ++j) {
    const int lo = j == 0 ? p : j * len, hi = (j + 1) * len;
    int k = 0;
    unsigned long long least = 0;
    for (int t = 0; t <= 14; ++t) {
      unsigned long long c = 0;
      for (int i = lo; i < hi; ++i) c += (u[i] >> t) + 1 + t;
      if (t == 0 || c < least) {
        least = c;
        k = t;
      }
    }
    put(f, (unsigned)k, 4);
    for (int i = lo; i < hi; ++i) {
      for (unsigned long long z = u[i] >> k; z > 0; --z) f.push_back(false);
      f.push_back(true);
      put(f, u[i] & ((1ull << k) - 1), k);
    }
  }
  if (f.size() >= 8 + 16 * (size_t)n) {
    put(b, 0x02, 8);
    for (int i = 0; i < n; ++i) put(b, (uint16_t)x[i], 16);
    *kind = -2;
    return pack(b);
  }
  *kind = p;
  return pack(f);
}

static unsigned rule_crc(const uint8_t* p, size_t n, unsigned poly, int width) {
  unsigned c = 0;
  const unsigned top = 1u << (width - 1), mask = (1u << width) - 1u;
  for (size_t i = 0; i < n; ++i) {
    c ^= (unsigned)p[i] << (width - 8);
    for (int k = 0; k < 8; ++k) c = (c & top) ? ((c << 1) ^ poly) & mask : (c << 1) & mask;
  }
  return c;
}

static std::vector<uint8_t> rule_frame(int rate, const std::vector<int16_t>& x, unsigned long long no) {
  std::vector<uint8_t> o = {0xFF, 0xF9};
  o.push_back((uint8_t)(0x70 | (rate == 8000 ? 4 : rate == 16000 ? 5 : rate == 24000 ? 7 : 10)));
  o.push_back(0x08);
  if (no < 0x80) {
    o.push_back((uint8_t)no);
  } else {
    int bytes = 2;  // the payload bits of 2 .. 7 bytes: 11, 16, 21, 26, 31, 36
    const int room[8] = {0, 0, 11, 16, 21, 26, 31, 36};
    while (no >> room[bytes]) ++bytes;
    BitVec b;
    for (int i = 0; i < bytes; ++i) b.push_back(true);
    b.push_back(false);
    const int first = 7 - bytes;  // payload bits of the first byte
    put(b, no >> (6 * (bytes - 1)), first);
    for (int i = bytes - 2; i >= 0; --i) {
      put(b, 2, 2);
      put(b, (no >> (6 * i)) & 0x3F, 6);
    }
    const std::vector<uint8_t> v = pack(b);
    CHECK((int)v.size() == bytes);
    o.insert(o.end(), v.begin(), v.end());
  }
  const int n = (int)x.size();
  o.push_back((uint8_t)((n - 1) >> 8));
  o.push_back((uint8_t)(n - 1));
  o.push_back((uint8_t)rule_crc(o.data(), o.size(), 0x07, 8));
  int kind;
  const std::vector<uint8_t> sub = rule_subframe(x, &kind);
  o.insert(o.end(), sub.begin(), sub.end());
  const unsigned c = rule_crc(o.data(), o.size(), 0x8005, 16);
  o.push_back((uint8_t)(c >> 8));
  o.push_back((uint8_t)c);
  return o;
}

// ---- the signals ----
static unsigned g_lcg = 12345;
static int rnd(int lo, int hi) {  // lo .. hi
  g_lcg = g_lcg * 1664525u + 1013904223u;
  return lo + (int)((g_lcg >> 8) % (unsigned)(hi - lo + 1));
}
enum { SILENCE, CONSTANT, SINES, NOISE, ALTERNATING, RAMP, HISS, WALK, SMOOTH, N_SIGNALS };
static std::vector<int16_t> signal(int kind, int T) {
  std::vector<int16_t> x(T);
  long long walk = 2000, d1 = 0, d2 = 0, acc = 0;
  for (int i = 0; i < T; ++i) {
    long long v = 0;
    switch (kind) {
      case SILENCE: v = 0; break;
      case CONSTANT: v = -7; break;
      case SINES: v = std::lround(9000 * std::sin(0.031 * i) + 4000 * std::sin(0.27 * i + 1.0)) + rnd(-20, 20); break;
      case NOISE: v = rnd(-32768, 32767); break;
      case ALTERNATING: v = i % 2 == 0 ? 32767 : -32768; break;
      case RAMP: v = (5ll * i) % 30000 - 15000; break;
      case HISS: v = rnd(-300, 300); break;
      case WALK: walk = (walk + rnd(-40, 40) + 9000) % 9000; v = walk; break;
      default: {  // third difference +-1 in long runs
        const int ph = i % 96, s = (ph / 48 ? -1 : 1) * ((ph % 48) < 12 || (ph % 48) >= 36 ? 1 : -1);
        d2 += s;
        d1 += d2;
        acc += d1;
        v = acc;
      }
    }
    CHECK(v >= -32768 && v <= 32767);
    x[i] = (int16_t)v;
  }
  return x;
}

static int g_kinds[7];  // constant, verbatim, fixed 0 .. 4: how often each came

static void check_subframes(int rate) {
  const int bs = flac_block(rate);
  CHECK(bs == rate / 25 && flac_slot_bytes(bs) == LVX_FLAC_SLOT(rate) && flac_slot_bytes(bs) % 16 == 0);
  const int lens[] = {1, 2, 4, 5, 15, 16, 17, bs - 1, bs, bs + 15, 24, 32, 128, 333};
  for (int kind = 0; kind < N_SIGNALS; ++kind)
    for (int n : lens) {
      const std::vector<int16_t> x = signal(kind, n);
      int which;
      const std::vector<uint8_t> want = rule_subframe(x, &which);
      ++g_kinds[which + 2];
      CHECK((int)want.size() <= 1 + 2 * n);
      std::vector<uint8_t> got(want.size(), 0xA5);  // exactly sized: a byte too many is the sanitizer's to report
      CHECK(flac_subframe(x.data(), n, got.data(), (int)got.size()) == (int)want.size());
      CHECK(got == want);
      if (!want.empty()) {  // cap too small: nothing is written
        std::vector<uint8_t> small(want.size() - 1, 0xA5);
        CHECK(flac_subframe(x.data(), n, small.data(), (int)small.size()) == LVX_E_CAPACITY);
        for (uint8_t v : small) CHECK(v == 0xA5);
      }
      if (kind == NOISE && n >= 16) CHECK(which == -2 && (int)want.size() == 1 + 2 * n);
      if (kind <= CONSTANT) CHECK(which == -1 && want.size() == 3);
    }
}

// a sentence of T samples through flac_finish: slots as the device writes them, frames as the rule states them
static void check_finish(int rate, int kind, int T, unsigned long long first_no) {
  const int bs = flac_block(rate), slot = flac_slot_bytes(bs);
  const std::vector<int16_t> x = signal(kind, T);
  const int frames = (int)flac_frames_upto(bs, T, true);
  std::vector<uint8_t> slots((size_t)frames * slot, 0), want;
  unsigned long long no = first_no;
  for (int f = 0; f < frames; ++f) {
    const int at = f * bs, n = f == frames - 1 ? T - at : bs;
    CHECK(n >= 1 && n <= bs + 15 && (n >= 16 || T < 16));
    const std::vector<int16_t> fx(x.begin() + at, x.begin() + at + n);
    uint8_t* s = slots.data() + (size_t)f * slot;
    const int body = flac_subframe(fx.data(), n, s + 8, slot - 8);
    CHECK(body >= 3 && body <= 1 + 2 * n);
    s[0] = (uint8_t)n;
    s[1] = (uint8_t)(n >> 8);
    s[2] = (uint8_t)body;
    s[3] = (uint8_t)(body >> 8);
    const std::vector<uint8_t> fr = rule_frame(rate, fx, no);
    CHECK((int)fr.size() <= 2 * n + 17);
    want.insert(want.end(), fr.begin(), fr.end());
    no += n;
  }
  std::vector<uint8_t> got(want.size(), 0xA5);
  unsigned long long run = first_no;
  CHECK(flac_finish(rate, slots.data(), frames, &run, got.data(), (long long)got.size()) == (long long)want.size());
  CHECK(got == want && run == first_no + (unsigned long long)T);
  if (!want.empty()) {  // cap too small: nothing written, the number stays
    std::vector<uint8_t> small(want.size() - 1, 0xA5);
    run = first_no;
    CHECK(flac_finish(rate, slots.data(), frames, &run, small.data(), (long long)small.size()) == LVX_E_CAPACITY);
    CHECK(run == first_no);
    for (uint8_t v : small) CHECK(v == 0xA5);
  }
}

static void check_errors() {
  std::vector<int16_t> x(20, 3);
  x[7] = 9;
  std::vector<uint8_t> out(64, 0xA5);
  CHECK(flac_subframe(x.data(), 0, out.data(), 64) == LVX_E_ARG);  // n = 0: a frame has a sample
  CHECK(flac_subframe(x.data(), -1, out.data(), 64) == LVX_E_ARG);
  CHECK(flac_subframe(x.data(), FLAC_MAX_N + 1, out.data(), 64) == LVX_E_ARG);
  CHECK(flac_subframe(nullptr, 20, out.data(), 64) == LVX_E_ARG);
  CHECK(flac_subframe(x.data(), 20, nullptr, 64) == LVX_E_ARG);
  CHECK(flac_subframe(x.data(), 20, out.data(), -1) == LVX_E_ARG);
  for (uint8_t v : out) CHECK(v == 0xA5);
  unsigned long long no = 5;
  CHECK(flac_finish(8000, nullptr, 0, &no, nullptr, 0) == 0 && no == 5);  // no frames: no bytes
  std::vector<uint8_t> slot(LVX_FLAC_SLOT(8000), 0);
  slot[0] = 20;
  slot[2] = (uint8_t)flac_subframe(x.data(), 20, slot.data() + 8, (int)slot.size() - 8);
  CHECK(flac_finish(8000, slot.data(), 1, &no, out.data(), 64) > 0 && no == 25);
  std::fill(out.begin(), out.end(), (uint8_t)0xA5);
  CHECK(flac_finish(44100, slot.data(), 1, &no, out.data(), 64) == LVX_E_ARG);
  CHECK(flac_finish(8000, nullptr, 1, &no, out.data(), 64) == LVX_E_ARG);
  CHECK(flac_finish(8000, slot.data(), 1, nullptr, out.data(), 64) == LVX_E_ARG);
  CHECK(flac_finish(8000, slot.data(), 1, &no, nullptr, 64) == LVX_E_ARG);
  CHECK(flac_finish(8000, slot.data(), -1, &no, out.data(), 64) == LVX_E_ARG);
  CHECK(flac_finish(8000, slot.data(), 1, &no, out.data(), -1) == LVX_E_ARG);
  unsigned long long far = (1ull << 36) - 19;
  CHECK(flac_finish(8000, slot.data(), 1, &far, out.data(), 64) == LVX_E_ARG && far == (1ull << 36) - 19);
  far = (1ull << 36) - 20;  // the last number there is: 7 bytes
  CHECK(flac_finish(8000, slot.data(), 1, &far, out.data(), 64) > 0 && far == (1ull << 36) && out[4] == 0xFE);
  std::fill(out.begin(), out.end(), (uint8_t)0xA5);
  for (int bad = 0; bad < 4; ++bad) {  // records that are none of the stage's
    std::vector<uint8_t> s = slot;
    if (bad == 0) s[0] = 0;
    if (bad == 1) s[1] = 2;  // n = 532 > BS + 15
    if (bad == 2) s[2] = 200;  // body > 1 + 2 n
    if (bad == 3) s[5] = 1;
    CHECK(flac_finish(8000, s.data(), 1, &no, out.data(), 64) == LVX_E_ARG && no == 25);
  }
  for (uint8_t v : out) CHECK(v == 0xA5);
  uint8_t head[42];
  CHECK(flac_stream_header(16000, head) && !flac_stream_header(11025, head) && !flac_stream_header(8000, nullptr));
  CHECK(head[0] == 'f' && head[7] == 34 && head[9] == 16 && ((head[10] << 8) | head[11]) == 640 + 15);
  CHECK(((head[18] << 12) | (head[19] << 4) | (head[20] >> 4)) == 16000 && (head[20] & 15) == 0 && head[21] == 0xF0);
  CHECK(flac_crc8((const uint8_t*)"123456789", 9) == 0xF4 && flac_crc16((const uint8_t*)"123456789", 9) == 0xFEE8);
  CHECK(rule_crc((const uint8_t*)"123456789", 9, 0x07, 8) == 0xF4 && rule_crc((const uint8_t*)"123456789", 9, 0x8005, 16) == 0xFEE8);
}

// ---- plan_flac under pcm_plan: the counts against brute force, the buffer turns, the refusals ----
static int brute_frames(int bs, long long T, bool final) {
  int k = 0;
  while ((long long)(k + 1) * bs + 16 <= T) ++k;  // frame k is whole, and at least 16 samples follow it
  return k + (final && T > 0 ? 1 : 0);
}

static void check_plan(int rate) {
  const int bs = flac_block(rate), slot = flac_slot_bytes(bs), S = 6;
  std::vector<PcmSeg> segs(S);
  auto call = [&](const std::vector<int32_t>& sl, const std::vector<uint8_t>& fl, int n_in, int r, long long in_stride,
                  long long out_stride, std::vector<FlacRow>& rows, std::vector<int32_t>& n) {
    n.assign(sl.size(), -7);
    return pcm_plan(segs, FLAC_HIST, (int)sl.size(), n_in, sl.data(), fl.data(), n.data(), r, true,
                    [](long long k) { return std::to_string(k) + " Hz"; }, rows,
                    [&](const PcmCall& c, FlacRow& row) { return plan_flac(c, n_in, r, in_stride, out_stride, row); });
  };
  const long long WIDE = 1 << 24;
  std::vector<FlacRow> rows;
  std::vector<int32_t> n;
  const int steps[] = {1, 17, bs + 16, 1000, 0, 15, 16, bs - 1, 3 * bs + 7};
  for (int step : steps) {
    long long T = 0, emitted = 0;
    uint8_t par = segs[2].par;
    const int calls = step == 1 ? 2 * bs + 40 : 7;
    for (int c = 0; c < calls; ++c) {
      const bool final = c == calls - 1;
      CHECK(call({4, 2}, {0, (uint8_t)final}, step, rate, 2ll * step, WIDE, rows, n).empty());
      const int want = brute_frames(bs, T + step, final) - brute_frames(bs, T, false);
      CHECK(n[1] == want && rows[1].n_out == want && rows[1].t0 == T && rows[1].j0 == emitted && rows[1].row == 1);
      CHECK(n[1] == flac_frames_upto(bs, T + step, final) - flac_frames_upto(bs, T, false));
      CHECK(rows[1].hist_in == (par * S + 2) * FLAC_HIST);
      if (step > 0 && !final) {
        CHECK(rows[1].hist_out == ((1 - par) * S + 2) * FLAC_HIST);
        par ^= 1;
      } else {
        CHECK(rows[1].hist_out == -1);
      }
      if (want > 0) {
        const long long last = final ? T + step - (emitted + want - 1) * bs : bs;
        CHECK(rows[1].last_n == last && last >= 1 && last <= bs + 15);
      }
      T += step;
      emitted += want;
      CHECK(T - emitted * bs <= bs + 15 || final);  // what the slot keeps fits its history
      CHECK(final ? segs[2].key == PcmSeg::NONE && segs[2].t0 == 0 : segs[2].key == rate && segs[2].t0 == T);
      CHECK(segs[2].par == par);
    }
    CHECK(call({4}, {1}, 0, rate, 0, WIDE, rows, n).empty());  // (the companion's segment ends too)
  }
  // the refusals: no slot's state changes
  CHECK(call({1, 3}, {0, 0}, 40, rate, 80, WIDE, rows, n).empty());
  const std::vector<PcmSeg> before = segs;
  auto unchanged = [&] {
    for (int s = 0; s < S; ++s)
      CHECK(segs[s].t0 == before[s].t0 && segs[s].key == before[s].key && segs[s].par == before[s].par && segs[s].aux == before[s].aux);
  };
  const int other = rate == 8000 ? 16000 : 8000;
  CHECK(!call({0, 1}, {0, 0}, 40, other, 80, WIDE, rows, n).empty());  // open at another rate
  unchanged();
  CHECK(!call({0, 3, 0}, {0, 0, 0}, 40, rate, 80, WIDE, rows, n).empty());  // named twice
  unchanged();
  CHECK(!call({0, S}, {0, 0}, 40, rate, 80, WIDE, rows, n).empty() && !call({-1}, {0}, 40, rate, 80, WIDE, rows, n).empty());
  unchanged();
  CHECK(!call({0, 1}, {0, 0}, 40, rate, 78, WIDE, rows, n).empty());  // in_stride_bytes smaller than a row
  unchanged();
  CHECK(!call({0, 1}, {0, 1}, 3 * bs, rate, 6ll * bs, 3ll * slot - 4, rows, n).empty());  // out_stride_bytes smaller than the slots
  unchanged();
  CHECK(call({0, 1}, {0, 1}, 3 * bs, rate, 6ll * bs, 4ll * slot, rows, n).empty() && n[0] == 2 && n[1] == 4);
}

int main() {
  static_assert(flac_fold(0) == 0 && flac_fold(-1) == 1 && flac_fold(1) == 2 && flac_fold(-524288) == 1048575, "");
  static_assert(flac_partition_order(1920) == 3 && flac_partition_order(320 + 15) == 0 && flac_partition_order(64) == 2 &&
                    flac_partition_order(16) == 0 && flac_partition_order(8) == 0 && flac_partition_order(36) == 1,
                "");
  static_assert(flac_diff(4, 1, 0, 0, 0, 0) == 1 && flac_diff(3, 0, 1, 0, 0, 9) == -3 && flac_rice_bits(37, 3) == 8, "");
  static_assert(LVX_FLAC_SLOT(8000) == 688 && LVX_FLAC_SLOT(48000) == 3888, "");
  for (int rate : {8000, 16000, 24000, 48000}) {
    const int bs = rate / 25;
    check_subframes(rate);
    const int Ts[] = {1, 15, 16, 17, bs - 1, bs, bs + 15, bs + 16, bs + 17, 2 * bs + 15, 2 * bs + 16, 3 * bs + 7};
    for (int kind = 0; kind < N_SIGNALS; ++kind)
      for (int T : Ts) check_finish(rate, kind, T, rate == 8000 ? 0 : kind == SINES ? (1ull << 31) - 5 : 1000003ull * T);
    check_plan(rate);
  }
  for (int k = 0; k < 7; ++k) CHECK(g_kinds[k] > 0);  // every kind came: constant, verbatim, fixed 0 .. 4
  check_errors();
  std::printf("flac host check: ok\n");
  return 0;
}
