// Stand-alone check of the formant stage's host side (llmvox_amd/csrc/pcm_host.h): the integer plan against rational
// arithmetic written a second time, the streaming counts, the tables, and plan_formant through the skeleton pcm_plan /
// pcm_chunks without a device, the launches only recorded. Built and run by tests/test_formant_host.py with the system
// compiler under AddressSanitizer and UBSan; exit status 0 when every check holds.
#include <cstdio>
#include <cstdlib>

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

// what lvx_pcm_formant does with the skeleton, the launch recorded instead of made
static Out call(std::vector<PcmSeg>& g, const Slots& slots, const Finals& finals, int n_in, int Fn, int Fd, long long stride) {
  Out o;
  const int B = (int)slots.size();
  o.n.assign(B, -7);
  std::vector<PcmRow> rows;
  const bool launch = Fn != Fd;
  o.err = pcm_plan(
      g, FMT_HIST, B, n_in, slots.data(), finals.data(), o.n.data(), ratio_key(Fn, Fd), launch, [](long long k) { return std::to_string(k); },
      rows, [&](const PcmCall& c, PcmRow& r) { return plan_formant(c, n_in, Fn, Fd, stride, r); });
  if (!o.err.empty() || !launch) return o;
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

// every triple of percentages: valid exactly where the stretch exists and rho lies in 1/2 .. 2, and then Fn / Fd is
// rho in lowest terms
static void check_plan() {
  long long valid = 0;
  for (int speed = 48; speed <= 202; ++speed)
    for (int pitch = 48; pitch <= 202; ++pitch) {
      const bool in_range = speed >= 50 && speed <= 200 && pitch >= 50 && pitch <= 200;
      const int st = pitch > 0 ? (200 * speed + pitch) / (2 * pitch) : 0;
      for (int f = 48; f <= 202; ++f) {
        int Fn = -1, Fd = -1;
        const bool ok = formant_plan(speed, pitch, f, &Fn, &Fd);
        // rho = (100 speed) / (f st): the resampling's M / L is speed / st before it is reduced
        const long long num = 100ll * speed, den = (long long)f * st;
        const bool want = in_range && f >= 50 && f <= 200 && st >= 50 && st <= 200 && den <= 2 * num && num <= 2 * den;
        CHECK(ok == want);
        if (!ok) {
          CHECK(Fn == -1 && Fd == -1);
          continue;
        }
        ++valid;
        CHECK(formant_ok(Fn, Fd) && gcd_of(Fn, Fd) == 1 && (long long)Fn * den == (long long)Fd * num);
        if (100ll * speed == (long long)f * st) CHECK(Fn == 1 && Fd == 1);  // the formant is where the pitch put the envelope
      }
    }
  CHECK(valid > 100000);
  int Fn = 0, Fd = 0;
  CHECK(formant_plan(100, 125, 100, &Fn, &Fd) && Fn == 5 && Fd == 4);
  CHECK(formant_plan(100, 100, 90, &Fn, &Fd) && Fn == 10 && Fd == 9);
  CHECK(formant_plan(100, 100, 100, &Fn, &Fd) && Fn == 1 && Fd == 1);
  CHECK(!formant_plan(100, 200, 50, &Fn, &Fd));  // rho = 4
  CHECK(!formant_ok(2, 4) && !formant_ok(0, 1) && !formant_ok(1, 3) && !formant_ok(40001, 40000) && formant_ok(40000, 39999));
  CHECK(formant_ok(2, 1) && formant_ok(1, 2) && formant_ok(199, 200));
}

static void check_counts() {
  CHECK(formant_emitted_upto(0, false) == 0 && formant_emitted_upto(0, true) == 0);
  CHECK(formant_emitted_upto(1023, false) == 0 && formant_emitted_upto(1024, false) == 256 && formant_emitted_upto(1279, false) == 256);
  long long prev = 0;
  for (long long T = 0; T < 6000; ++T) {
    const long long m = formant_emitted_upto(T, false);
    CHECK(m >= prev && m % FMT_H == 0 && formant_emitted_upto(T, true) == T);
    // the last emitted block's last frame ends inside the input, and the next block's does not
    if (m > 0) CHECK((m / FMT_H - 1 + 4) * FMT_H <= T);
    CHECK((m / FMT_H + 4) * FMT_H > T);
    CHECK(T - m <= 4 * FMT_H - 1 && (T < 3 * FMT_H || T - m >= 3 * FMT_H));  // held back: 768 .. 1023
    prev = m;
  }
  // any cutting of T adds up to T
  unsigned seed = 12345;
  for (int T : {1, 255, 256, 257, 767, 768, 769, 1024, 3000, 100000}) {
    for (int rep = 0; rep < 20; ++rep) {
      long long t0 = 0, sum = 0;
      while (t0 < T) {
        seed = seed * 1664525u + 1013904223u;
        const long long n = std::min<long long>(T - t0, 1 + (seed >> 8) % 1500);
        const bool fin = t0 + n == T;
        sum += formant_emitted_upto(t0 + n, fin) - formant_emitted_upto(t0, false);
        t0 += n;
      }
      CHECK(sum == T);
    }
  }
}

static void check_tables() {
  std::vector<float> w(FMT_N), c(FMT_TAPS), tw(FMT_N);
  formant_design(w.data(), c.data(), tw.data());
  formant_design(nullptr, nullptr, nullptr);  // (every table is optional)
  double csum = 0;
  for (int d = 0; d < FMT_TAPS; ++d) {
    CHECK(c[d] > 0 && c[d] == c[FMT_TAPS - 1 - d]);
    csum += c[d];
  }
  CHECK(std::fabs(csum - 1.0) < 1e-6 && c[FMT_K] > c[FMT_K + 1]);
  for (int n = 0; n < FMT_N; ++n) CHECK(w[n] > 0 && w[n] <= 1 && w[n] == w[FMT_N - 1 - n]);
  for (int n = 0; n < FMT_H; ++n) {  // the four shifted w^2 sum to 1.5
    double s = 0;
    for (int q = 0; q < 4; ++q) s += (double)w[n + q * FMT_H] * w[n + q * FMT_H];
    CHECK(std::fabs(s - 1.5) < 1e-6);
  }
  CHECK(tw[0] == 1.f && tw[FMT_N / 2] == 0.f && std::signbit(tw[FMT_N / 2]) && tw[FMT_N / 2 + FMT_N / 4] == -1.f);
  for (int k = 0; k < FMT_N / 2; ++k) CHECK(std::fabs((double)tw[k] * tw[k] + (double)tw[FMT_N / 2 + k] * tw[FMT_N / 2 + k] - 1.0) < 1e-6);
}

static void check_skeleton() {
  std::vector<PcmSeg> g(S);
  const Slots three{0, 1, 2};
  const Finals go(3, 0), end(3, 1);
  auto count = [&](long long t0, int n, bool f) { return (int32_t)(formant_emitted_upto(t0 + n, f) - formant_emitted_upto(t0, false)); };

  // a refused call of every kind moves no record and writes no count
  CHECK(call(g, {5}, {0}, N_IN, 3, 2, WIDE).err.empty());
  const std::vector<PcmSeg> before = g;
  for (const Out& o : {call(g, {0, S}, {0, 0}, N_IN, 3, 2, WIDE), call(g, {0, -1}, {0, 0}, N_IN, 3, 2, WIDE),
                       call(g, {1, 0, 1}, go, N_IN, 3, 2, WIDE), call(g, {0, 5}, {0, 0}, N_IN, 2, 3, WIDE),
                       call(g, three, end, N_IN, 3, 2, 4)}) {
    CHECK(!o.err.empty() && same(g, before) && o.launches.empty());
    for (int32_t n : o.n) CHECK(n == -7);
  }
  CHECK(call(g, {0, 5}, {0, 0}, N_IN, 2, 3, WIDE).err.find("slot 5: its segment is open at ") == 0);

  // four calls: the counts are the closed form's, the buffers alternate, a call reads what the last wrote
  Out o = call(g, three, go, N_IN, 3, 2, WIDE);
  CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, 0) && o.launches.size() == 1);  // (nothing out, a history kept)
  std::vector<int> first_in = o.in, last_out = o.out;
  for (int k = 1; k < 4; ++k) {
    o = call(g, three, go, N_IN, 3, 2, WIDE);
    CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, count((long long)k * N_IN, N_IN, false)) && o.n[0] > 0);
    CHECK(o.in == last_out && (k % 2 ? o.out == first_in : o.in == first_in));
    for (int b = 0; b < 3; ++b) CHECK(o.in[b] != o.out[b] && o.out[b] >= 0 && g[b].t0 == (long long)(k + 1) * N_IN && g[b].key == ratio_key(3, 2));
    last_out = o.out;
  }
  // a stride one sample short of the final call's output is refused; the final call emits the rest and closes
  const int32_t rest = count(4 * N_IN, N_IN, true);
  CHECK(rest > N_IN && !call(g, three, end, N_IN, 3, 2, 4ll * rest - 4).err.empty());
  o = call(g, three, end, N_IN, 3, 2, 4ll * rest);
  CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, rest) && o.out == std::vector<int>(3, -1));
  for (int b = 0; b < 3; ++b) CHECK(g[b].t0 == 0 && g[b].key == PcmSeg::NONE);
  CHECK(call(g, three, end, N_IN, 2, 3, WIDE).n == std::vector<int32_t>(3, N_IN));  // another ratio may follow
  o = call(g, {5}, {1}, 0, 3, 2, WIDE);  // (the slot the first step opened)
  CHECK(o.err.empty() && o.n[0] == N_IN);

  // 33 rows are packets of 32 and 1; a packet whose rows have nothing to emit or keep is not launched
  o = call(g, iota(33), Finals(33, 0), 2 * N_IN, 199, 200, WIDE);
  CHECK(o.err.empty() && o.launches.size() == 2 && o.launches[0].rows == 32 && o.launches[1].rows == 1 && o.launches[1].first_row == 32);
  CHECK(o.launches[1].max_out == o.n[32] && o.n[32] == 512);
  o = call(g, iota(32), Finals(32, 1), 0, 199, 200, WIDE);
  CHECK(o.err.empty() && o.launches.size() == 1 && o.n[0] == 2 * N_IN - 512);
  o = call(g, iota(33), Finals(33, 1), 0, 199, 200, WIDE);
  CHECK(o.err.empty() && o.n[31] == 0 && o.n[32] == 2 * N_IN - 512 && o.launches.size() == 1 && o.launches[0].first_row == 32);
  CHECK(call(g, iota(33), Finals(33, 1), 0, 199, 200, WIDE).launches.empty());

  // 1 / 1: the rows are the output and no record moves, but an open segment's ratio is still minded
  const std::vector<PcmSeg> closed = g;
  o = call(g, three, go, N_IN, 1, 1, 0);
  CHECK(o.err.empty() && o.n == std::vector<int32_t>(3, N_IN) && o.launches.empty() && same(g, closed));
  CHECK(call(g, {7}, {0}, N_IN, 3, 2, WIDE).err.empty());
  CHECK(!call(g, {7}, {1}, N_IN, 1, 1, 0).err.empty() && g[7].key == ratio_key(3, 2));
}

int main() {
  check_plan();
  check_counts();
  check_tables();
  check_skeleton();
  std::puts("formant host check: ok");
  return 0;
}
