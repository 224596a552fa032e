// The CPU proof of csrc/sample_reduce.hpp, built from the headers alone (tests/test_sample_reduce_host.py: g++, address and
// undefined-behaviour sanitizers where their runtimes exist).
//   * THE CANONICAL SUM, restated here on its own (pad with +0.0 to a power of two, add neighbours level by level, + 0.0),
//     against sabc::tree_sum (the stack of partial sums: what a lane runs alone, W = 1 and the replicated store) and against a
//     plain-array model of the device's executor for W = 4 and 16 -- every lane adds the tree of its own M slots
//     (reduce::lane_tree, the function the device calls), the team follows with the butterfly over lane distances 1, 2, 4, 8 --
//     on the SORTED layout (position q M + r holds element q M + r, a pad slot adds +0.0): the same bits for every N <= 64 and
//     for N = 100, 128, 257, 1000, on inputs with heavy cancellation (+-1e16 among values of order 1), on all -0.0 and on
//     infinities; every lane of the model ends with the same bits.
//   * the DRAW layout (position q M + r holds draw_of(q, r, W)): |sum - exact| <= N 2^-53 sum |s_i|, exact = a compensated
//     sum in long double.
//   * count_less / count_less_equal (reduce::count_below) against std::lower_bound / std::upper_bound for m = 0, 1, 2, 3, 7, 8,
//     9, 1000 with duplicates and +-inf among the data, v every datum, values between, +-inf and NaN (which counts as +inf).
//   * the Kolmogorov-Smirnov numerators (reduce::ks_term with those counts) against the supremum over all pooled points,
//     as exact integers, on small integer samples: the values of x distinct (one of them +inf now and then), ties within y and
//     between the samples the rule -- equal; with ties within x as well: never below the supremum and at most
//     (longest run - 1) / n above it.
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
namespace rd = sabc::reduce;
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
double unit() { return (double)(next_u64() >> 11) * 0x1.0p-53; }

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// the definition, restated
double canonical(const std::vector<double> &s) {
  size_t p = 1;
  while (p < s.size()) p <<= 1;
  std::vector<double> a(s);
  a.resize(p, 0.0);
  for (; p > 1; p >>= 1)
    for (size_t i = 0; i < p / 2; ++i) a[i] = a[2 * i] + a[2 * i + 1];
  return a[0] + 0.0;
}

template <int M>
double lane_tree_of(const double *pos) {
  double t[M];
  for (int r = 0; r < M; ++r) t[r] = pos[r];
  return rd::lane_tree(t);
}
double lane_tree_m(const int m, const double *pos) {
  switch (m) {
    case 1: return lane_tree_of<1>(pos);
    case 2: return lane_tree_of<2>(pos);
    case 4: return lane_tree_of<4>(pos);
    case 8: return lane_tree_of<8>(pos);
    case 16: return lane_tree_of<16>(pos);
    case 32: return lane_tree_of<32>(pos);
  }
  return std::nan("");
}

// the device's executor on plain arrays: pos[q m + r] = what lane q holds in slot r (a pad slot: +0.0)
double team_model(const int w, const int m, const std::vector<double> &pos, bool *lanes_agree) {
  std::vector<double> s((size_t)w), next((size_t)w);
  for (int q = 0; q < w; ++q) s[(size_t)q] = lane_tree_m(m, &pos[(size_t)q * (size_t)m]);
  for (int dist = 1; dist < w; dist <<= 1) {
    for (int q = 0; q < w; ++q) next[(size_t)q] = s[(size_t)q] + s[(size_t)(q ^ dist)];
    s.swap(next);
  }
  for (int q = 1; q < w; ++q)
    if (!same_bits(s[0], s[(size_t)q])) *lanes_agree = false;
  return rd::finish_sum(s[0]);
}

std::vector<double> make_input(const int n, const int kind) {
  std::vector<double> s((size_t)n);
  for (int i = 0; i < n; ++i) {
    const uint64_t u = next_u64();
    double v = 4.0 * unit() - 2.0;
    if (kind == 1) v = (u & 3) == 0 ? 1e16 : (u & 3) == 1 ? -1e16 : v;             // heavy cancellation
    if (kind == 2) v = -0.0;                                                       // a sum that is a zero
    if (kind == 3) v = i == 0 || (u & 15) == 0 ? kInf : v;                                  // +inf among them
    if (kind == 4) v = std::ldexp(v, (int)(u % 80) - 40);                          // many magnitudes
    s[(size_t)i] = v;
  }
  return s;
}

void check_sums(const int n) {
  for (int kind = 0; kind < 5; ++kind) {
    const std::vector<double> s = make_input(n, kind);
    const double want = canonical(s);
    ++g_checks;
    if (!same_bits(want, sabc::tree_sum(s.data(), n))) fail("tree_sum(x, n)", 1, n);
    if (!same_bits(want, sabc::tree_sum(n, [&](const int i) { return s[(size_t)i]; }))) fail("tree_sum(n, g)", 1, n);
    if (kind == 2 && !same_bits(want, 0.0)) fail("a zero sum is +0.0", 1, n);
    long double exact = 0.0L, comp = 0.0L, mag = 0.0L;                               // Neumaier, in long double
    for (const double v : s) {
      const long double t = exact + (long double)v;
      comp += std::fabs(exact) >= std::fabs((long double)v) ? (exact - t) + (long double)v : ((long double)v - t) + exact;
      exact = t;
      mag += std::fabs((long double)v);
    }
    exact += comp;
    for (const int w : {4, 16}) {
      if (!ts::spread(n, w)) continue;
      const int m = ts::slots(n, w);
      std::vector<double> sorted_layout((size_t)(w * m), 0.0), draw_layout((size_t)(w * m), 0.0);
      for (int q = 0; q < w; ++q)
        for (int r = 0; r < m; ++r) {
          const int after = q * m + r, before = ts::draw_of(q, r, w);
          if (after < n) sorted_layout[(size_t)(q * m + r)] = s[(size_t)after];
          if (before < n) draw_layout[(size_t)(q * m + r)] = s[(size_t)before];
        }
      bool agree = true;
      ++g_checks;
      if (!same_bits(want, team_model(w, m, sorted_layout, &agree))) fail("the team's sum on the sorted layout", w, n);
      const double drawn = team_model(w, m, draw_layout, &agree);
      if (!agree) fail("the lanes of a team end with the same bits", w, n);
      if (kind != 3 && !(std::fabs((long double)drawn - exact) <= (long double)n * 0x1.0p-53L * mag)) fail("the bound on the draw layout", w, n);
      if (kind != 3 && !(std::fabs((long double)want - exact) <= (long double)n * 0x1.0p-53L * mag)) fail("the bound on the sorted layout", w, n);
      if (kind == 3 && !same_bits(drawn, want)) fail("infinities on the draw layout", w, n);
    }
  }
}

void check_counts(const int m) {
  for (int kind = 0; kind < 3; ++kind) {
    std::vector<double> y((size_t)m);
    for (double &v : y) v = kind == 0 ? 8.0 * unit() : std::floor(6.0 * unit());       // kind > 0: duplicates
    if (kind == 2 && m >= 2) { y[0] = -kInf; y[(size_t)m - 1] = kInf; }
    if (kind == 2 && m >= 7) { y[1] = -kInf; y[(size_t)m - 2] = kInf; }
    std::sort(y.begin(), y.end());
    std::vector<double> probes = {-kInf, kInf, std::nan(""), -1.0, 0.0, -0.0, 2.5, 100.0};
    for (size_t j = 0; j < y.size(); j += (m > 100 ? 7 : 1)) {
      probes.push_back(y[j]);
      probes.push_back(std::nextafter(y[j], kInf));
      probes.push_back(std::nextafter(y[j], -kInf));
    }
    const auto at = [&](const long long j) {
      if (j < 0 || j >= (long long)m) { fail("an index outside the data", 0, m); return 0.0; }
      return y[(size_t)j];
    };
    for (const double v : probes) {
      const double key = v != v ? kInf : v;
      const long long less = std::lower_bound(y.begin(), y.end(), key) - y.begin();
      const long long less_equal = std::upper_bound(y.begin(), y.end(), key) - y.begin();
      ++g_checks;
      if (rd::count_below<false>(v, m, at) != less) fail("count_less", kind, m);
      if (rd::count_below<true>(v, m, at) != less_equal) fail("count_less_equal", kind, m);
    }
  }
}

void check_ks(const int n, const int m, const bool distinct) {
  // x: distinct integers of [0, 2 n) (a simulated sample: continuous draws), or any of them (ties within x); y: any integers of
  // that range, so ties within y and between the samples are the rule
  std::vector<double> x, y((size_t)m);
  for (int v = 0; v < 2 * n && distinct; ++v) x.push_back((double)v);
  for (size_t i = 0; i < x.size(); ++i) std::swap(x[i], x[i + (size_t)(next_u64() % (x.size() - i))]);
  x.resize((size_t)n);
  for (double &v : x) v = distinct ? v : std::floor(2 * n * unit());
  for (double &v : y) v = std::floor(2 * n * unit());
  if (next_u64() & 1) x[0] = kInf;                                                  // a NaN draw that entered as +inf
  std::sort(x.begin(), x.end());
  std::sort(y.begin(), y.end());
  const auto at = [&](const long long j) { return y[(size_t)j]; };
  double top = 0.0;
  for (int i = 0; i < n; ++i)
    top = std::max(top, rd::ks_term(i, n, m, rd::count_below<false>(x[(size_t)i], m, at), rd::count_below<true>(x[(size_t)i], m, at)));
  std::vector<double> pooled(x);
  pooled.insert(pooled.end(), y.begin(), y.end());
  long long want = 0;                                                               // sup |F_x - F_y| n m over the pooled points
  for (const double t : pooled) {
    const long long cx = std::upper_bound(x.begin(), x.end(), t) - x.begin(), cy = std::upper_bound(y.begin(), y.end(), t) - y.begin();
    want = std::max(want, std::llabs(cx * m - cy * n));
  }
  long long run = 1, longest = 1;
  for (int i = 1; i < n; ++i) longest = std::max(longest, run = x[(size_t)i] == x[(size_t)i - 1] ? run + 1 : 1);
  ++g_checks;
  if (distinct ? top != (double)want : !(top >= (double)want && top <= (double)(want + (longest - 1) * m)))
    fail(distinct ? "the Kolmogorov-Smirnov numerator" : "the Kolmogorov-Smirnov numerator with ties in x", m, n);
}

}  // namespace

int main() {
  for (int n = 1; n <= 64; ++n) check_sums(n);
  for (const int n : {100, 128, 257, 1000}) check_sums(n);
  if (!same_bits(sabc::tree_sum(static_cast<const double *>(nullptr), 0), 0.0)) fail("an empty sum", 1, 0);
  for (const int m : {0, 1, 2, 3, 7, 8, 9, 1000}) check_counts(m);
  for (int trial = 0; trial < 4000; ++trial) check_ks(1 + (int)(next_u64() % 12), 1 + (int)(next_u64() % 12), (trial & 3) != 0);
  for (int trial = 0; trial < 50; ++trial) check_ks(45, 7 + (int)(next_u64() % 60), true);
  std::printf("sample_reduce: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
