// Stand-alone check of the G.711 companding of llmvox_amd/csrc/pcm_host.h ("PCM G.711" in include/llmvox.h): all 65,536
// inputs and all 256 codes through g711_encode / g711_decode, held to llmvox.h's rule written here a second time with its
// loops, the properties the header states, n = 0 and the argument errors. Built and run by tests/test_g711_host.py with
// the system compiler under AddressSanitizer and UBSan; exit status 0 when every check holds.
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

// llmvox.h's rule as it is written there: the loops, no count of leading zeros
static int ulaw_rule(int q) {
  int a = ((q < 0 ? ~q : q) >> 2) + 33;
  if (a > 0x1FFF) a = 0x1FFF;
  int seg = 1;
  for (int t = a >> 6; t; t >>= 1) ++seg;
  return ((8 - seg) << 4) | (0xF - ((a >> seg) & 0xF)) | (q >= 0 ? 0x80 : 0);
}

static int alaw_rule(int q) {
  int x = (q < 0 ? ~q : q) >> 4;
  if (x > 15) {
    int e = 1;
    while (x > 31) {
      x >>= 1;
      e += 1;
    }
    x = x - 16 + (e << 4);
  }
  if (q >= 0) x |= 0x80;
  return x ^ 0x55;
}

static void check_law(int enc, int (*rule)(int), int silence, int zero_count, int bound_all, int no_round_trip) {
  constexpr int NQ = 65536;
  // exactly-sized heap buffers: a write or a read past either end is the sanitizer's to report
  std::vector<int16_t> q(NQ), back(NQ), lin(256);
  std::vector<uint8_t> code(NQ), all(256), again(256);
  for (int i = 0; i < NQ; ++i) q[i] = (int16_t)(i - 32768);
  for (int i = 0; i < 256; ++i) all[i] = (uint8_t)i;
  CHECK(g711_encode(enc, q.data(), NQ, code.data()) == LVX_OK);
  CHECK(g711_decode(enc, all.data(), 256, lin.data()) == LVX_OK);
  CHECK(g711_decode(enc, code.data(), NQ, back.data()) == LVX_OK);
  CHECK(g711_encode(enc, lin.data(), 256, again.data()) == LVX_OK);

  std::vector<int> seen(256, 0);
  int worst = 0;
  for (int i = 0; i < NQ; ++i) {
    const int v = q[i];
    CHECK(code[i] == rule(v));
    CHECK(code[i] == (enc == LVX_PCM_ULAW ? g711_ulaw(v) : g711_alaw(v)));
    CHECK(code[NQ - 1 - i] == (code[i] ^ 0x80));  // q[NQ - 1 - i] is ~q[i]
    CHECK(back[i] == lin[code[i]]);
    if (i > 0) CHECK(back[i] >= back[i - 1]);
    const int err = std::abs(back[i] - v);
    worst = std::max(worst, err);
    if (enc == LVX_PCM_ALAW || std::abs(v) <= 32124) CHECK(err <= 512);
    ++seen[code[i]];
  }
  CHECK(worst == bound_all);
  for (int c = 0; c < 256; ++c) {
    CHECK(seen[c] > 0);
    CHECK(again[c] == c || c == no_round_trip);
  }
  CHECK(code[32768] == silence && seen[silence] == zero_count && seen[silence ^ 0x80] == zero_count);
  CHECK(code[32767] == (silence ^ 0x80));  // q = -1
  if (no_round_trip >= 0) CHECK(lin[no_round_trip] == 0 && again[no_round_trip] == silence);

  // one sample at a time from buffers of one element, and n = 0 with and without pointers
  for (int i = 0; i < NQ; i += 257) {
    std::vector<int16_t> one(1, q[i]);
    std::vector<uint8_t> out(1, 0);
    CHECK(g711_encode(enc, one.data(), 1, out.data()) == LVX_OK && out[0] == code[i]);
  }
  CHECK(g711_encode(enc, nullptr, 0, nullptr) == LVX_OK && g711_decode(enc, nullptr, 0, nullptr) == LVX_OK);
  CHECK(g711_encode(enc, q.data(), 0, code.data()) == LVX_OK && g711_decode(enc, all.data(), 0, lin.data()) == LVX_OK);
  // the argument errors: nothing is written
  std::vector<uint8_t> guard(4, 0xA5);
  std::vector<int16_t> guard16(4, 0x5A5A);
  CHECK(g711_encode(enc, q.data(), -1, guard.data()) == LVX_E_ARG);
  CHECK(g711_encode(enc, nullptr, 4, guard.data()) == LVX_E_ARG);
  CHECK(g711_encode(enc, q.data(), 4, nullptr) == LVX_E_ARG);
  CHECK(g711_decode(enc, all.data(), -1, guard16.data()) == LVX_E_ARG);
  CHECK(g711_decode(enc, nullptr, 4, guard16.data()) == LVX_E_ARG);
  CHECK(g711_decode(enc, all.data(), 4, nullptr) == LVX_E_ARG);
  for (int bad : {LVX_PCM_F32LE, LVX_PCM_S16LE, 2, 3, 5, 8, -1}) {
    CHECK(g711_encode(bad, q.data(), 4, guard.data()) == LVX_E_ARG);
    CHECK(g711_decode(bad, all.data(), 4, guard16.data()) == LVX_E_ARG);
    CHECK(pcm_sample_bytes(bad) == (bad == LVX_PCM_F32LE ? 4 : bad == LVX_PCM_S16LE ? 2 : 0));
  }
  for (int k = 0; k < 4; ++k) CHECK(guard[k] == 0xA5 && guard16[k] == 0x5A5A);
  CHECK(pcm_sample_bytes(enc) == 1);
}

int main() {
  static_assert(LVX_PCM_ALAW == 6 && LVX_PCM_ULAW == 7, "the WAVE format tags");
  static_assert(g711_ulaw(0) == 0xFF && g711_ulaw(-1) == 0x7F && g711_ulaw(32767) == 0x80 && g711_ulaw(-32768) == 0x00, "");
  static_assert(g711_alaw(0) == 0xD5 && g711_alaw(-1) == 0x55 && g711_alaw(32767) == 0xAA && g711_alaw(-32768) == 0x2A, "");
  check_law(LVX_PCM_ULAW, ulaw_rule, 0xFF, 4, 644, 0x7F);
  check_law(LVX_PCM_ALAW, alaw_rule, 0xD5, 16, 512, -1);
  std::printf("g711 host check: ok\n");
  return 0;
}
