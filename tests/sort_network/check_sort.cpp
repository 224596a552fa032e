// The CPU proof of csrc/sort_network.hpp, built from that header alone (tests/test_sort_network_host.py: g++ -O2).
//   * every 0-1 input: the loop form for n = 1..16, the template form for N in {1, 2, 3, 4, 5, 7, 8, 16} -- by the 0-1 principle
//     a comparator network that sorts every 0-1 input of a length sorts every input of that length;
//   * n in {17, 31, 32, 33, 64, 100, 128, 257, 1024} against std::sort: random doubles of a fixed seed, sorted, reversed, all-equal,
//     many duplicates, +-inf, denormals, a mix of -0.0 and +0.0 (compared with ==); the template form where N is one of them;
//   * k NaNs come out as k +inf at the end, the rest sorted;
//   * quantile and order_statistic at p in {0, 1/8, 0.5, 1 - 2^-53, 1}, n = 1, ranks 0 and n + 1;
//   * the float twins: the same checks.
// Prints one line per failure and a summary; the exit status is the number of failures, capped at 1.
#include "sort_network.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

namespace {

int g_failures = 0, g_checks = 0;

void fail(const char *what, int n, const char *type) {
  if (++g_failures <= 20) std::printf("FAIL %s n=%d %s\n", what, n, type);
}

template <class T> const char *type_name();
template <> const char *type_name<double>() { return "double"; }
template <> const char *type_name<float>() { return "float"; }

uint64_t g_state = 0x9E3779B97F4A7C15ull;              // splitmix64, fixed seed
uint64_t next_u64() {
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double next_unit() { return (double)(next_u64() >> 11) * 0x1p-53; }

// ---- every 0-1 input ----
template <class T>
void zero_one_loop(const int n) {
  T x[16];
  for (uint32_t bits = 0; bits < (1u << n); ++bits) {
    int ones = 0;
    for (int i = 0; i < n; ++i) { x[i] = (T)((bits >> i) & 1u); ones += (int)((bits >> i) & 1u); }
    sabc::sort_ascending(x, n);
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok && x[i] == (T)(i >= n - ones ? 1 : 0);
    ++g_checks;
    if (!ok) { fail("0-1 input, loop form", n, type_name<T>()); return; }
  }
}

template <class T, int N>
void zero_one_template() {
  T x[N];
  for (uint32_t bits = 0; bits < (1u << N); ++bits) {
    int ones = 0;
    for (int i = 0; i < N; ++i) { x[i] = (T)((bits >> i) & 1u); ones += (int)((bits >> i) & 1u); }
    sabc::sort_ascending(x);
    bool ok = true;
    for (int i = 0; i < N; ++i) ok = ok && x[i] == (T)(i >= N - ones ? 1 : 0);
    ++g_checks;
    if (!ok) { fail("0-1 input, template form", N, type_name<T>()); return; }
  }
}

// ---- larger sizes against std::sort ----
template <class T>
std::vector<T> make_input(const int kind, const int n) {
  const T inf = std::numeric_limits<T>::infinity(), tiny = std::numeric_limits<T>::denorm_min();
  std::vector<T> v((size_t)n);
  for (int i = 0; i < n; ++i) {
    const double u = next_unit();
    switch (kind) {
      case 0: v[i] = (T)((u - 0.5) * 2000.0); break;                           // random
      case 1: v[i] = (T)i - (T)7; break;                                       // sorted
      case 2: v[i] = (T)(n - i); break;                                        // reversed
      case 3: v[i] = (T)2.5; break;                                            // all equal
      case 4: v[i] = (T)(int)(u * 5.0); break;                                 // many duplicates
      case 5: v[i] = u < 0.2 ? inf : u < 0.4 ? -inf : (T)(u * 10.0); break;    // +-inf
      case 6: v[i] = (T)((int)(u * 64.0) - 32) * tiny; break;                  // denormals, both signs, and zeros
      default: v[i] = u < 0.35 ? (T)-0.0 : u < 0.7 ? (T)0.0 : (T)(u < 0.85 ? -1.0 : 1.0); break;   // -0.0 and +0.0
    }
  }
  return v;
}
const char *const kKinds[8] = {"random", "sorted", "reversed", "all equal", "duplicates", "infinities", "denormals", "signed zeros"};

template <class T>
bool same(const std::vector<T> &a, const std::vector<T> &b) {
  for (size_t i = 0; i < a.size(); ++i)
    if (!(a[i] == b[i])) return false;                 // ==: -0.0 and +0.0 may come out in either order
  return true;
}

template <class T, int N>
void against_std_sort_template(const std::vector<T> &in, const std::vector<T> &expect, const char *kind) {
  T x[N];
  for (int i = 0; i < N; ++i) x[i] = in[(size_t)i];
  sabc::sort_ascending(x);
  ++g_checks;
  if (!same(std::vector<T>(x, x + N), expect)) fail(kind, N, type_name<T>());
}

template <class T>
void against_std_sort(const int n) {
  for (int kind = 0; kind < 8; ++kind) {
    const std::vector<T> in = make_input<T>(kind, n);
    std::vector<T> expect = in, got = in;
    std::sort(expect.begin(), expect.end());
    sabc::sort_ascending(got.data(), n);
    ++g_checks;
    if (!same(got, expect)) fail(kKinds[kind], n, type_name<T>());
    // the template form at the sizes on both sides of its unrolled | loop boundary, and one well inside each
    if (n == 17) against_std_sort_template<T, 17>(in, expect, kKinds[kind]);
    if (n == 31) against_std_sort_template<T, 31>(in, expect, kKinds[kind]);
    if (n == 32) against_std_sort_template<T, 32>(in, expect, kKinds[kind]);
    if (n == 33) against_std_sort_template<T, 33>(in, expect, kKinds[kind]);
    if (n == 128) against_std_sort_template<T, 128>(in, expect, kKinds[kind]);
  }
}

// ---- NaN: k NaNs in, k +inf at the end, the rest sorted ----
template <class T, int N>
void nans_template(const std::vector<T> &in, const std::vector<T> &expect) {
  T x[N];
  for (int i = 0; i < N; ++i) x[i] = in[(size_t)i];
  sabc::sort_ascending(x);
  ++g_checks;
  if (!same(std::vector<T>(x, x + N), expect)) fail("NaN, template form", N, type_name<T>());
}

template <class T>
void nans(const int n, const int k) {
  std::vector<T> in = make_input<T>(0, n), rest;
  for (int j = 0; j < k; ++j) in[(size_t)((j * 7 + 3) % n)] = std::numeric_limits<T>::quiet_NaN();   // (7 and n coprime: k distinct places)
  for (const T v : in)
    if (v == v) rest.push_back(v);
  std::sort(rest.begin(), rest.end());
  const int k_in = n - (int)rest.size();
  std::vector<T> expect = rest;
  expect.resize((size_t)n, std::numeric_limits<T>::infinity());
  std::vector<T> got = in;
  sabc::sort_ascending(got.data(), n);
  ++g_checks;
  if (k_in != k || !same(got, expect)) fail("NaN, loop form", n, type_name<T>());
  if (n == 5) nans_template<T, 5>(in, expect);
  if (n == 32) nans_template<T, 32>(in, expect);
  if (n == 33) nans_template<T, 33>(in, expect);
}

// ---- quantile, order_statistic ----
void check(const bool ok, const char *what, const int n) {
  ++g_checks;
  if (!ok) fail(what, n, "double");
}

void quantiles() {
  const double inf = std::numeric_limits<double>::infinity();
  const double one[1] = {4.25};
  for (const double p : {0.0, 0.125, 0.5, 1.0 - 0x1p-53, 1.0, -3.0, 7.0}) check(sabc::quantile(one, 1, p) == 4.25, "quantile, n = 1", 1);
  check(sabc::order_statistic(one, 1, 1) == 4.25 && sabc::order_statistic(one, 1, 0) == inf && sabc::order_statistic(one, 1, 2) == inf,
        "order_statistic, n = 1", 1);
  for (const int n : {2, 9, 17, 100}) {
    std::vector<double> x = make_input<double>(0, n);
    std::sort(x.begin(), x.end());
    const double *s = x.data();
    check(sabc::quantile(s, n, 0.0) == s[0] && sabc::quantile(s, n, -1.0) == s[0], "quantile, p = 0", n);
    check(sabc::quantile(s, n, 1.0) == s[n - 1] && sabc::quantile(s, n, 2.0) == s[n - 1], "quantile, p = 1", n);
    for (const double p : {0.125, 0.5, 1.0 - 0x1p-53}) {
      // the definition, written out: h = (n - 1) p, i = floor(h), s[i] + (h - i) (s[i + 1] - s[i])
      const double h = (double)(n - 1) * p, fl = std::floor(h);
      const int i = (int)fl;
      const double expect = i >= n - 1 ? s[n - 1] : s[i] + (h - fl) * (s[i + 1] - s[i]);
      const double got = sabc::quantile(s, n, p);
      // one rounding of the product and one of the sum on either side (a compiler may contract one of them): 2 ulp of the larger neighbour
      const double tol = 4.0 * std::numeric_limits<double>::epsilon() * std::max(std::fabs(s[std::min(i + 1, n - 1)]), std::fabs(s[i]));
      check(std::fabs(got - expect) <= tol && got >= s[i] && got <= s[std::min(i + 1, n - 1)], "quantile, interior p", n);
    }
    if (n == 9) {                                      // h lands on a knot: (n - 1) / 8 and (n - 1) / 2 are whole
      check(sabc::quantile(s, n, 0.125) == s[1] && sabc::quantile(s, n, 0.5) == s[4], "quantile on a knot", n);
    }
    check(sabc::order_statistic(s, n, 0) == inf && sabc::order_statistic(s, n, n + 1) == inf && sabc::order_statistic(s, n, -5) == inf,
          "order_statistic outside [1, n]", n);
    bool all = true;
    for (int r = 1; r <= n; ++r) all = all && sabc::order_statistic(s, n, r) == s[r - 1];
    check(all, "order_statistic inside [1, n]", n);
  }
  // +inf at the end (what a NaN draw becomes): +inf from the first interval that touches it, never NaN
  const double tail[4] = {1.0, 2.0, inf, inf};
  check(sabc::quantile(tail, 4, 0.25) == 1.75 && sabc::quantile(tail, 4, 1.0 / 3.0) == 2.0 && sabc::quantile(tail, 4, 0.5) == inf &&
            sabc::quantile(tail, 4, 0.9) == inf && sabc::quantile(tail, 4, 1.0) == inf,
        "quantile with +inf at the end", 4);
  check(sabc::quantile(tail, 0, 0.5) == inf, "quantile, n = 0", 0);
}

template <class T>
void all_of_type() {
  for (int n = 1; n <= 16; ++n) zero_one_loop<T>(n);
  zero_one_template<T, 1>();
  zero_one_template<T, 2>();
  zero_one_template<T, 3>();
  zero_one_template<T, 4>();
  zero_one_template<T, 5>();
  zero_one_template<T, 7>();
  zero_one_template<T, 8>();
  zero_one_template<T, 16>();
  for (const int n : {17, 31, 32, 33, 64, 100, 128, 257, 1024}) against_std_sort<T>(n);
  for (const int n : {1, 2, 5, 17, 32, 33, 100})
    for (const int k : {1, 2, 5})
      if (k <= n) nans<T>(n, k);
  T none[1] = {(T)3};
  sabc::sort_ascending(none, 0);                       // n = 0: nothing is touched
  ++g_checks;
  if (none[0] != (T)3) fail("n = 0", 0, type_name<T>());
}

}  // namespace

int main() {
  all_of_type<double>();
  all_of_type<float>();
  quantiles();
  std::printf("comparators: n=2 %d, 4 %d, 8 %d, 16 %d, 32 %d, 64 %d, 128 %d\n", sabc::sortnet::comparators(2), sabc::sortnet::comparators(4),
              sabc::sortnet::comparators(8), sabc::sortnet::comparators(16), sabc::sortnet::comparators(32), sabc::sortnet::comparators(64),
              sabc::sortnet::comparators(128));
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
