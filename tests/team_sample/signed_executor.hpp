// What the CPU proofs of csrc/team_sample.hpp and csrc/team_sample_f32.hpp share, over the element type T (double: two normals to
// a Philox block, float: four): the SIGNED-VALUE EXECUTOR in plain C++ -- what the device does on T v[M]: sign flips by
// teamsort::sign_mask, a cross-lane step as min(own, -partner's), an in-lane step one min and one max ascending on the stored values
// but for descending_slot_bit -- and the checks that hold it to teamsort::run_schedule bit for bit: every 0-1 input of a length,
// random inputs against std::sort, the NaN policy.  Included by check_team_sample.cpp and ../team_sample_f32/check_team_sample_f32.cpp
// behind the header under test; one line per failure, counted in g_failures.
#pragma once
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

template <class T> bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }
template <class T> constexpr int kPer = sizeof(T) == 8 ? 2 : 4;      // normals to a Philox block
template <class T> constexpr T kInf = std::numeric_limits<T>::infinity();
constexpr int kMaxPositions = 16 * sabc::kSortUnrollMax;

// the device's executor in plain C++: y[q m + r] holds x or -x as sign_mask says (-y is the flip of the top bit)
template <class T>
void run_signed(const int w, const int m, T *y) {
  T t[kMaxPositions];
  int before = 0;
  for (int i = 0; i < ts::step_count(w, m); ++i) {
    const ts::Step s = ts::step_at(w, m, i);
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
          const T lo = std::fmin(y[q * m + r], y[q * m + (r | s.dist)]), hi = std::fmax(y[q * m + r], y[q * m + (r | s.dist)]);
          y[q * m + r] = (r & desc) ? hi : lo;
          y[q * m + (r | s.dist)] = (r & desc) ? lo : hi;
        }
    }
  }
  if (before != 0) fail("the last step's sign mask is not 0", w, m);
}

// Sample<n, w> / SampleF32<n, w> as the headers lay it out: fill in draw order (every draw a slot of its own below M, draw_of
// inverts it), sort by the schedule and by the signed executor, read the latter in rank order
template <class T>
std::vector<T> team_sort(const int w, const std::vector<T> &in, bool *signed_agrees) {
  constexpr int per = kPer<T>;
  const int n = (int)in.size();
  std::vector<T> out(in);
  if (!ts::spread(n, w, per)) {                        // replicated: the array every lane holds, sabc::sort_ascending
    sabc::sort_ascending(out.data(), n);
    return out;
  }
  const int m = ts::slots(n, w, per), positions = w * m;
  T x[kMaxPositions], y[kMaxPositions];
  char used[kMaxPositions] = {};
  for (int p = 0; p < positions; ++p) x[p] = kInf<T>;
  for (int i = 0; i < n; ++i) {
    const int q = ts::draw_lane(i, w, per), r = ts::draw_slot(i, w, per);
    if (q < 0 || q >= w || r < 0 || r >= m || used[q * m + r] || ts::draw_of(q, r, w, per) != i) { fail("layout of the draws", w, n); return out; }
    used[q * m + r] = 1;
    x[q * m + r] = std::fmin(in[(size_t)i], kInf<T>);  // NaN -> +inf
  }
  for (int p = 0; p < positions; ++p) y[p] = x[p];
  ts::run_schedule(w, m, x);
  run_signed(w, m, y);
  for (int p = 0; p < positions; ++p) *signed_agrees = *signed_agrees && (same_bits(x[p], y[p]) || (x[p] == 0 && y[p] == 0));
  for (int i = 0; i < n; ++i) out[(size_t)i] = y[ts::rank_lane(i, m) * m + ts::rank_slot(i, m)];
  for (int p = n; p < positions; ++p)
    if (x[p] != kInf<T> || y[p] != kInf<T>) fail("a pad slot among the first N ranks", w, n);
  return out;
}

template <class T>
void zero_one(const int w, const int n) {
  std::vector<T> in((size_t)n);
  for (uint32_t bits = 0; bits < (1u << n); ++bits) {
    int ones = 0;
    for (int i = 0; i < n; ++i) { in[(size_t)i] = (T)((bits >> i) & 1u); ones += (int)((bits >> i) & 1u); }
    bool agree = true;
    const std::vector<T> out = team_sort(w, in, &agree);
    bool ok = agree;
    for (int i = 0; i < n; ++i) ok = ok && out[(size_t)i] == (T)(i >= n - ones ? 1 : 0);
    ++g_checks;
    if (!ok) { fail(agree ? "0-1 input" : "0-1 input: the signed executor differs from the schedule", w, n); return; }
  }
}

template <class T>
void against_std_sort(const int w, const int n) {
  for (int kind = 0; kind < 4; ++kind) {
    std::vector<T> in((size_t)n);
    for (int i = 0; i < n; ++i) {
      const uint64_t u = next_u64();
      switch (kind) {
        case 0:                                                                                      // random
          if constexpr (sizeof(T) == 8) in[(size_t)i] = (double)(int64_t)(u >> 11) * 0x1p-40 - 4096.0;
          else in[(size_t)i] = (float)(int32_t)(u >> 40) * 0x1p-12f - 2048.0f;
          break;
        case 1: in[(size_t)i] = (T)(u % 7) - (T)3; break;                                            // many duplicates
        case 2: in[(size_t)i] = u % 5 == 0 ? kInf<T> : u % 5 == 1 ? -kInf<T> : (T)(u % 1000); break;   // infinities
        default: in[(size_t)i] = (T)(n - i); break;                                                  // reversed
      }
    }
    std::vector<T> want(in);
    std::sort(want.begin(), want.end());
    bool agree = true;
    const std::vector<T> out = team_sort(w, in, &agree);
    ++g_checks;
    if (!agree) fail("the signed executor differs from the schedule", w, n);
    if (!std::equal(want.begin(), want.end(), out.begin())) fail("against std::sort", w, n);
  }
}

template <class T>
void nan_policy(const int w, const int n) {
  std::vector<T> in((size_t)n);
  for (int i = 0; i < n; ++i) in[(size_t)i] = (T)((i * 7) % n);
  in[(size_t)(n / 2)] = std::numeric_limits<T>::quiet_NaN();
  in[0] = std::numeric_limits<T>::quiet_NaN();
  bool agree = true;
  const std::vector<T> out = team_sort(w, in, &agree);
  ++g_checks;
  bool ok = agree && out[(size_t)(n - 1)] == kInf<T> && out[(size_t)(n - 2)] == kInf<T>;
  for (int i = 0; i + 1 < n; ++i) ok = ok && out[(size_t)i] <= out[(size_t)(i + 1)];
  for (int i = 0; i < n - 2; ++i) ok = ok && out[(size_t)i] < kInf<T>;
  if (!ok) fail("NaN enters as +inf", w, n);
}

}  // namespace
