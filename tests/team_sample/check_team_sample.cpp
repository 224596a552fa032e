// The CPU proof of csrc/team_sample.hpp, built from that header alone (tests/test_team_sample_host.py: g++, address and
// undefined-behaviour sanitizers).  The header's schedule -- teamsort::step_at, the list of steps the device executes on
// registers -- runs here on plain arrays, for teams of W = 1, 4 and 16 lanes:
//   * every 0-1 input for every N <= 16, and for (W, N) = (4, 20): five blocks over four lanes, slots padded to a power of two --
//     by the 0-1 principle a comparator network that sorts every 0-1 input of a length sorts every input of that length;
//   * a NaN enters as +inf and comes out last;
//   * N in {33, 45, 100, 128, 257, 512} against std::sort on random inputs with duplicates, +-inf among them;
//   * the replicated fallback (W = 4, N = 257: more than 32 slots per lane) and W = 1, which forward to sabc::sort_ascending;
//   * the layout: every draw has a slot of its own below M on the lane that generates its block, draw_of inverts it;
//   * the SIGNED-VALUE executor (what the device does: sign flips by sign_mask, a cross-lane step as min(own, -partner's), an
//     in-lane step ascending on the stored values but for descending_slot_bit) gives the plain schedule's result bit for bit.
// Prints one line per failure and a summary; the exit status is the number of failures, capped at 1.
#include "team_sample.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

namespace {

namespace ts = sabc::teamsort;
int g_failures = 0, g_checks = 0;
const double kInf = std::numeric_limits<double>::infinity();

void fail(const char *what, int w, int n) {
  if (++g_failures <= 20) std::printf("FAIL %s W=%d N=%d\n", what, w, n);
}

uint64_t g_state = 0x9E3779B97F4A7C15ull;              // splitmix64, fixed seed
uint64_t next_u64() {
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static_assert(ts::slots(128, 16) == 8 && ts::slots(128, 4) == 32 && ts::slots(45, 16) == 4 && ts::slots(20, 4) == 8, "slots per lane");
static_assert(ts::slots(1, 16) == 2 && ts::slots(17, 16) == 2 && ts::slots(257, 16) == 32 && ts::slots(512, 16) == 32, "slots per lane");
static_assert(ts::spread(128, 4) && !ts::spread(257, 4) && !ts::spread(129, 4) && !ts::spread(8, 1) && ts::spread(512, 16) && !ts::spread(513, 16),
              "spread while a lane's slots fit the unrolled size");
static_assert(ts::step_count(16, 8) == 28 && ts::step_count(4, 32) == 28 && ts::step_count(4, 2) == 6, "log P (log P + 1) / 2 steps");
static_assert(ts::step_at(16, 8, 0).dist == 1 && !ts::step_at(16, 8, 0).cross && ts::step_at(16, 8, 0).stage == 2, "the first step");
static_assert(ts::step_at(16, 8, 6).cross && ts::step_at(16, 8, 6).dist == 1 && ts::step_at(16, 8, 6).stage == 16, "the first cross-lane step");

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// the steps of a team, listed once
struct Steps {
  int w = 0, m = 0, count = 0;
  ts::Step at[64];
  void list(const int w_, const int m_) {
    if (w == w_ && m == m_) return;
    w = w_; m = m_; count = ts::step_count(w, m);
    for (int i = 0; i < count; ++i) at[i] = ts::step_at(w, m, i);
  }
};
Steps g_steps;
constexpr int kMaxPositions = 16 * sabc::kSortUnrollMax;

// the device's executor in plain C++: y[q m + r] holds x or -x as sign_mask says
void run_signed(const Steps &st, double *y) {
  const int w = st.w, m = st.m;
  double t[kMaxPositions];
  int before = 0;
  for (int i = 0; i < st.count; ++i) {
    const ts::Step s = st.at[i];
    const int mask = ts::sign_mask(s, w, m);
    if (mask != before)
      for (int q = 0; q < w; ++q)
        if (__builtin_popcount(q & (mask ^ before)) & 1)
          for (int r = 0; r < m; ++r) y[q * m + r] = -y[q * m + r];
    before = mask;
    if (s.cross) {
      for (int p = 0; p < w * m; ++p) t[p] = y[p];
      for (int q = 0; q < w; ++q)
        for (int r = 0; r < m; ++r) y[q * m + r] = std::fmin(t[q * m + r], -t[(q ^ s.dist) * m + r]);
    } else {
      const int desc = ts::descending_slot_bit(s, m);
      for (int q = 0; q < w; ++q)
        for (int r = 0; r < m; ++r) {
          if (r & s.dist) continue;
          const double lo = std::fmin(y[q * m + r], y[q * m + (r | s.dist)]), hi = std::fmax(y[q * m + r], y[q * m + (r | s.dist)]);
          y[q * m + r] = (r & desc) ? hi : lo;
          y[q * m + (r | s.dist)] = (r & desc) ? lo : hi;
        }
    }
  }
  if (before != 0) fail("the last step's sign mask is not 0", w, m);
}

// Sample<n, w> as the header lays it out: fill in draw order, sort, read in rank order
std::vector<double> team_sort(const int w, const std::vector<double> &in, bool *signed_agrees = nullptr) {
  const int n = (int)in.size();
  std::vector<double> out(in);
  if (!ts::spread(n, w)) {                             // replicated: the array every lane holds, sabc::sort_ascending
    sabc::sort_ascending(out.data(), n);
    return out;
  }
  const int m = ts::slots(n, w), positions = w * m;
  g_steps.list(w, m);
  double x[kMaxPositions], y[kMaxPositions];
  char used[kMaxPositions] = {};
  for (int p = 0; p < positions; ++p) x[p] = kInf;
  for (int i = 0; i < n; ++i) {
    const int q = ts::draw_lane(i, w), r = ts::draw_slot(i, w);
    if (q < 0 || q >= w || r < 0 || r >= m || used[q * m + r] || ts::draw_of(q, r, w) != i) { fail("layout of the draws", w, n); return out; }
    used[q * m + r] = 1;
    x[q * m + r] = std::fmin(in[i], kInf);             // NaN -> +inf
  }
  for (int p = 0; p < positions; ++p) y[p] = x[p];
  for (int i = 0; i < g_steps.count; ++i) ts::run_step(g_steps.at[i], w, m, x);
  run_signed(g_steps, y);
  bool agree = true;
  for (int p = 0; p < positions; ++p) agree = agree && (same_bits(x[p], y[p]) || (x[p] == 0.0 && y[p] == 0.0));
  if (signed_agrees) *signed_agrees = agree;
  for (int i = 0; i < n; ++i) out[i] = x[ts::rank_lane(i, m) * m + ts::rank_slot(i, m)];
  for (int p = n; p < positions; ++p)
    if (x[p] != kInf) fail("a pad slot among the first N ranks", w, n);
  return out;
}

// ... and once through run_schedule itself, the loop over step_at the listing above takes apart
void whole_schedule(const int w, const int n) {
  if (!ts::spread(n, w)) return;
  const int m = ts::slots(n, w);
  std::vector<double> x((size_t)w * m), want;
  for (double &v : x) v = (double)(next_u64() % 1000);
  want = x;
  std::sort(want.begin(), want.end());
  ts::run_schedule(w, m, x.data());
  ++g_checks;
  if (x != want) fail("run_schedule", w, n);
}

void zero_one(const int w, const int n) {
  std::vector<double> in((size_t)n);
  for (uint32_t bits = 0; bits < (1u << n); ++bits) {
    int ones = 0;
    for (int i = 0; i < n; ++i) { in[i] = (double)((bits >> i) & 1u); ones += (int)((bits >> i) & 1u); }
    bool agree = true;
    const std::vector<double> out = team_sort(w, in, &agree);
    bool ok = agree;
    for (int i = 0; i < n; ++i) ok = ok && out[i] == (double)(i >= n - ones ? 1 : 0);
    ++g_checks;
    if (!ok) { fail(agree ? "0-1 input" : "0-1 input: the signed executor differs", w, n); return; }
  }
}

void against_std_sort(const int w, const int n) {
  for (int kind = 0; kind < 4; ++kind) {
    std::vector<double> in((size_t)n);
    for (int i = 0; i < n; ++i) {
      const uint64_t u = next_u64();
      switch (kind) {
        case 0: in[i] = (double)(int64_t)(u >> 11) * 0x1p-40 - 4096.0; break;            // random
        case 1: in[i] = (double)(u % 7) - 3.0; break;                                      // many duplicates
        case 2: in[i] = u % 5 == 0 ? kInf : u % 5 == 1 ? -kInf : (double)(u % 1000); break;   // infinities
        default: in[i] = (double)(n - i); break;                                           // reversed
      }
    }
    std::vector<double> want(in);
    std::sort(want.begin(), want.end());
    bool agree = true;
    const std::vector<double> out = team_sort(w, in, &agree);
    ++g_checks;
    if (!agree) fail("the signed executor differs from the schedule", w, n);
    if (!std::equal(want.begin(), want.end(), out.begin())) fail("against std::sort", w, n);
  }
}

void nan_policy(const int w, const int n) {
  std::vector<double> in((size_t)n);
  for (int i = 0; i < n; ++i) in[i] = (double)((i * 7) % n);
  in[n / 2] = std::numeric_limits<double>::quiet_NaN();
  in[0] = std::numeric_limits<double>::quiet_NaN();
  const std::vector<double> out = team_sort(w, in);
  ++g_checks;
  bool ok = out[n - 1] == kInf && out[n - 2] == kInf;
  for (int i = 0; i + 1 < n; ++i) ok = ok && out[i] <= out[i + 1];
  for (int i = 0; i < n - 2; ++i) ok = ok && out[i] < kInf;
  if (!ok) fail("NaN enters as +inf", w, n);
}

}  // namespace

int main() {
  for (const int w : {1, 4, 16}) {
    for (int n = 1; n <= 16; ++n) zero_one(w, n);
    for (const int n : {33, 45, 100, 128, 257, 512}) { against_std_sort(w, n); whole_schedule(w, n); }
    for (const int n : {3, 8, 17, 45, 128}) nan_policy(w, n);
  }
  zero_one(4, 20);                                     // five blocks over four lanes: six slots padded to eight
  against_std_sort(4, 257);                            // (named: the replicated fallback)
  std::printf("team_sample: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
