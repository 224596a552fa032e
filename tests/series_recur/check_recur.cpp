// The CPU proof of sabc::Series::recur (csrc/team_series.hpp), built from the headers alone (tests/test_series_recur_host.py: g++,
// address and undefined-behaviour sanitizers where their runtimes exist).  series::run_recur walks the relay on plain arrays of
// W M positions exactly as the device does -- phase p: every lane from the same carried state through its own M slots, lane p keeps
// the outputs, its state is handed on -- the evaluations that the other lanes discard included.  For teams of W = 4 and 16 lanes,
// every 1 <= N <= 40 and N = 45, 100, 128, 129 (129 on 16 lanes only: a quad holds it replicated), first = 0 and 2, and three maps
//   * the sum (State double: cumsum),
//   * the AR(2) map with explicit fmas (State Carry<2>),
//   * the GARCH(1,1) map (State double; two rounded products, two fmas),
// it checks that
//   * the outputs and the returned state have the bits of the sequential loop over x[t];
//   * positions >= N and times t < first are untouched, and the elements t < first did not touch the state;
//   * overwriting what the lanes q != p computed in phase p -- their outputs and their state -- with a poison value before the
//     select changes nothing: nothing a lane discards is ever read.
// Prints one line per failure and a summary; the exit status is 1 if anything failed.
#include "team_series.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

namespace {

namespace ts = sabc::teamsort;
namespace sr = sabc::series;
int g_failures = 0, g_checks = 0;

void fail(const char *what, const char *map, int w, int n, int first) {
  if (++g_failures <= 20) std::printf("FAIL %s (%s) W=%d N=%d first=%d\n", what, map, w, n, first);
}

uint64_t g_state = 0x9E3779B97F4A7C15ull;              // splitmix64, fixed seed
uint64_t next_u64() {
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double next_value() {                                  // values of mixed sign and magnitude: sums that round
  const double u = (double)(next_u64() >> 11) * 0x1p-53 - 0.5;
  return std::ldexp(u, (int)(next_u64() % 8) - 2);
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }
template <class State>
bool same_state(State a, State b) {
  for (int k = 0; k < sr::CarryOf<State>::size; ++k)
    if (!same_bits(sr::CarryOf<State>::at(a, k), sr::CarryOf<State>::at(b, k))) return false;
  return true;
}

static_assert(sr::CarryOf<double>::size == 1 && sr::CarryOf<sr::Carry<2>>::size == 2 && sr::CarryOf<sr::Carry<4>>::size == 4, "the states");
static_assert(sr::relay_lanes(45, 4) == 12 && sr::relay_lanes(45, 16) == 3 && sr::relay_lanes(129, 16) == 9 && sr::relay_lanes(1, 2) == 1 &&
              sr::relay_lanes(128, 8) == 16, "only the lanes that hold a time < N take a phase");
static_assert(ts::slots(129, 16) == 16 && ts::slots(128, 4) == 32 && !ts::spread(129, 4), "slots per lane");

const double kPoison = std::numeric_limits<double>::quiet_NaN();

template <class State, class F>
void check(const char *map, const int w, const int n, const int first, const State s0, F &&f) {
  const int m = ts::slots(n, w), P = w * m;
  std::vector<double> x(P), want(P), got(P, 123.0), spoiled(P, 123.0);
  for (int p = 0; p < P; ++p) x[p] = next_value();     // positions >= N hold something too: they must come back untouched
  // the sequential loop
  want = x;
  State s = s0;
  for (int t = first; t < n; ++t) want[t] = f(t, s, want[t]);
  const State got_state = sr::run_recur(w, m, n, first, s0, f, x.data(), got.data());
  const State spoiled_state = sr::run_recur(w, m, n, first, s0, f, x.data(), spoiled.data(), [&](int, int, double *kept, State &mine) {
    for (int r = 0; r < m; ++r) kept[r] = kPoison;
    for (int k = 0; k < sr::CarryOf<State>::size; ++k) sr::CarryOf<State>::at(mine, k) = kPoison;
  });
  ++g_checks;
  for (int p = 0; p < P; ++p) {
    if (!same_bits(got[p], want[p])) { fail(p >= n ? "a position >= N was touched" : p < first ? "a time < first was touched" : "outputs", map, w, n, first); break; }
  }
  if (!same_state(got_state, s)) fail("the returned state", map, w, n, first);
  for (int p = 0; p < P; ++p)
    if (!same_bits(spoiled[p], got[p])) { fail("a discarded output was read", map, w, n, first); break; }
  if (!same_state(spoiled_state, got_state)) fail("a discarded state was read", map, w, n, first);
  // in place
  std::vector<double> in_place = x;
  const State in_place_state = sr::run_recur(w, m, n, first, s0, f, in_place.data(), in_place.data());
  for (int p = 0; p < P; ++p)
    if (!same_bits(in_place[p], want[p])) { fail("in place", map, w, n, first); break; }
  if (!same_state(in_place_state, s)) fail("in place: the returned state", map, w, n, first);
}

}  // namespace

int main() {
  const int widths[2] = {4, 16};
  std::vector<int> sizes;
  for (int n = 1; n <= 40; ++n) sizes.push_back(n);
  for (const int n : {45, 100, 128, 129}) sizes.push_back(n);
  const double phi1 = 0.6, phi2 = -0.3, omega = 0.1, alpha = 0.15, beta = 0.8;
  const auto sum = [](const int, double &s, const double x) { s = s + x; return s; };
  const auto ar2 = [&](const int, sr::Carry<2> &s, const double x) {
    const double out = std::fma(phi1, s.v[0], std::fma(phi2, s.v[1], x));
    s.v[1] = s.v[0];
    s.v[0] = out;
    return out;
  };
  const auto garch = [&](const int, double &s, const double z) {
    const double zz = sr::rounded_product(z, z), r = sr::rounded_product(s, zz);
    s = std::fma(s, std::fma(alpha, zz, beta), omega);
    return r;
  };
  // a map that depends on t, so that a lane running with another lane's times would show
  const auto timed = [](const int t, double &s, const double x) { s = std::fma(0.5, s, x + 0.125 * (double)t); return s - x; };
  for (const int w : widths)
    for (const int n : sizes) {
      if (!ts::spread(n, w)) {
        if (!(w == 4 && n == 129)) fail("spread", "", w, n, 0);
        continue;
      }
      for (const int first : {0, 2}) {
        check("sum", w, n, first, 0.0, sum);
        check("ar2", w, n, first, sr::Carry<2>{{0.25, -0.5}}, ar2);
        check("garch", w, n, first, 0.7, garch);
        check("timed", w, n, first, 1.5, timed);
      }
    }
  std::printf("series_recur: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
