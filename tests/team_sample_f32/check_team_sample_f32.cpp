// The CPU proof of csrc/team_sample_f32.hpp, built from the headers alone (tests/test_team_sample_f32_host.py: g++, address and
// undefined-behaviour sanitizers where their runtimes exist).  For teams of W = 4 and 16 lanes:
//   * THE LAYOUT: for every N <= 132, draw -> (draw_lane_f32, draw_slot_f32) is injective, lands below M on the lane that generates
//     the draw's block of four, its image plus the pad slots is all W M positions, and draw_of_f32 inverts it;
//   * the spread / replicated boundary: N = 32 W is spread, N = 32 W + 1 is replicated, W = 1 always is;
//   * the FLOAT SIGNED-VALUE EXECUTOR in plain C++ -- what the device does on float v[M]: sign flips by teamsort::sign_mask on the
//     word's top bit, a cross-lane step as min(own, -partner's), an in-lane step one min and one max ascending on the stored
//     values but for descending_slot_bit -- against teamsort::run_schedule on the same floats, bit for bit: every 0-1 input for
//     every N <= 16 (by the 0-1 principle a proof for those sizes), and N = 45, 100, 128, 512 on random inputs, duplicates,
//     infinities and a reversed ramp, also against std::sort; 512 at W = 4 is the replicated store, sabc::sort_ascending(float *);
//   * a NaN enters as +inf and comes out last;
//   * THE f64 TREE over the widened floats -- every lane adds reduce::lane_tree of its M terms on the sorted layout, the team
//     follows with the butterfly over lane distances 1, 2, 4, 8 -- equals reduce::tree_sum_of bit for bit for every N <= 64 and
//     for 100 and 128, and every lane ends with the same bits.
// Prints one line per failure and a summary; the exit status is 1 if anything failed.
#include "team_sample_f32.hpp"

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
const float kInf = std::numeric_limits<float>::infinity();

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

static_assert(ts::slots_f32(128, 16) == 8 && ts::slots_f32(128, 4) == 32 && ts::slots_f32(45, 16) == 4 && ts::slots_f32(45, 4) == 16, "slots per lane");
static_assert(ts::slots_f32(1, 16) == 4 && ts::slots_f32(64, 16) == 4 && ts::slots_f32(65, 16) == 8 && ts::slots_f32(17, 4) == 8, "whole blocks of four");
static_assert(ts::spread_f32(128, 4) && !ts::spread_f32(129, 4) && ts::spread_f32(512, 16) && !ts::spread_f32(513, 16) && !ts::spread_f32(8, 1),
              "spread while a lane's slots fit the unrolled size");
static_assert(ts::blocks_f32(1) == 1 && ts::blocks_f32(4) == 1 && ts::blocks_f32(5) == 2 && ts::blocks_f32(128) == 32, "whole blocks");

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }
bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }
float flip_sign(float x) {                             // v_xor_b32 with 0x80000000
  uint32_t u;
  std::memcpy(&u, &x, 4);
  u ^= 0x80000000u;
  std::memcpy(&x, &u, 4);
  return x;
}

constexpr int kMaxPositions = 16 * sabc::kSortUnrollMax;

// the device's executor in plain C++: y[q m + r] holds x or -x as sign_mask says
void run_signed(const int w, const int m, float *y) {
  float t[kMaxPositions];
  int before = 0;
  for (int i = 0; i < ts::step_count(w, m); ++i) {
    const ts::Step s = ts::step_at(w, m, i);
    const int mask = ts::sign_mask(s, w, m);
    if (mask != before)
      for (int q = 0; q < w; ++q)
        if (__builtin_popcount(q & (mask ^ before)) & 1)
          for (int r = 0; r < m; ++r) y[q * m + r] = flip_sign(y[q * m + r]);
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
          const float lo = std::fmin(y[q * m + r], y[q * m + (r | s.dist)]), hi = std::fmax(y[q * m + r], y[q * m + (r | s.dist)]);
          y[q * m + r] = (r & desc) ? hi : lo;
          y[q * m + (r | s.dist)] = (r & desc) ? lo : hi;
        }
    }
  }
  if (before != 0) fail("the last step's sign mask is not 0", w, m);
}

void layout(const int w, const int n) {
  ++g_checks;
  const int m = ts::slots_f32(n, w);
  if (m < 4 || (m & (m - 1)) || w * m < n) { fail("slots per lane", w, n); return; }
  std::vector<int> owner((size_t)(w * m), -1);
  for (int i = 0; i < n; ++i) {
    const int q = ts::draw_lane_f32(i, w), r = ts::draw_slot_f32(i, w);
    if (q < 0 || q >= w || r < 0 || r >= m) { fail("a draw outside the team's slots", w, n); return; }
    if (q != (i / 4) % w || (r & 3) != (i & 3)) fail("a draw away from the lane that generates its block", w, n);
    if (owner[(size_t)(q * m + r)] != -1) { fail("two draws in one slot", w, n); return; }
    owner[(size_t)(q * m + r)] = i;
    if (ts::draw_of_f32(q, r, w) != i) fail("draw_of_f32 does not invert the layout", w, n);
  }
  int pads = 0;
  for (int q = 0; q < w; ++q)
    for (int r = 0; r < m; ++r) {
      const int i = ts::draw_of_f32(q, r, w);
      if (owner[(size_t)(q * m + r)] == -1) {
        ++pads;
        if (i < n) fail("a pad slot whose draw index is below N", w, n);
      } else if (owner[(size_t)(q * m + r)] != i) {
        fail("draw_of_f32 disagrees with the layout", w, n);
      }
    }
  if (pads + n != w * m) fail("draws plus pad slots are not all positions", w, n);
}

// SampleF32<n, w> as the header lays it out: fill in draw order, sort, read in rank order
std::vector<float> team_sort(const int w, const std::vector<float> &in, bool *signed_agrees = nullptr) {
  const int n = (int)in.size();
  std::vector<float> out(in);
  if (!ts::spread_f32(n, w)) {                         // replicated: the array every lane holds, sabc::sort_ascending
    sabc::sort_ascending(out.data(), n);
    return out;
  }
  const int m = ts::slots_f32(n, w), positions = w * m;
  float x[kMaxPositions], y[kMaxPositions];
  for (int p = 0; p < positions; ++p) x[p] = kInf;
  for (int i = 0; i < n; ++i) x[ts::draw_lane_f32(i, w) * m + ts::draw_slot_f32(i, w)] = std::fmin(in[(size_t)i], kInf);      // NaN -> +inf
  for (int p = 0; p < positions; ++p) y[p] = x[p];
  ts::run_schedule(w, m, x);
  run_signed(w, m, y);
  bool agree = true;
  for (int p = 0; p < positions; ++p) agree = agree && (same_bits(x[p], y[p]) || (x[p] == 0.0f && y[p] == 0.0f));
  if (signed_agrees) *signed_agrees = agree;
  for (int i = 0; i < n; ++i) out[(size_t)i] = y[ts::rank_lane(i, m) * m + ts::rank_slot(i, m)];
  for (int p = n; p < positions; ++p)
    if (y[p] != kInf) fail("a pad slot among the first N ranks", w, n);
  return out;
}

void zero_one(const int w, const int n) {
  std::vector<float> in((size_t)n);
  for (uint32_t bits = 0; bits < (1u << n); ++bits) {
    int ones = 0;
    for (int i = 0; i < n; ++i) { in[(size_t)i] = (float)((bits >> i) & 1u); ones += (int)((bits >> i) & 1u); }
    bool agree = true;
    const std::vector<float> out = team_sort(w, in, &agree);
    bool ok = agree;
    for (int i = 0; i < n; ++i) ok = ok && out[(size_t)i] == (float)(i >= n - ones ? 1 : 0);
    ++g_checks;
    if (!ok) { fail(agree ? "0-1 input" : "0-1 input: the signed executor differs from the schedule", w, n); return; }
  }
}

void against_std_sort(const int w, const int n) {
  for (int kind = 0; kind < 4; ++kind) {
    std::vector<float> in((size_t)n);
    for (int i = 0; i < n; ++i) {
      const uint64_t u = next_u64();
      switch (kind) {
        case 0: in[(size_t)i] = (float)(int32_t)(u >> 40) * 0x1p-12f - 2048.0f; break;             // random
        case 1: in[(size_t)i] = (float)(u % 7) - 3.0f; break;                                       // many duplicates
        case 2: in[(size_t)i] = u % 5 == 0 ? kInf : u % 5 == 1 ? -kInf : (float)(u % 1000); break;   // infinities
        default: in[(size_t)i] = (float)(n - i); break;                                            // reversed
      }
    }
    std::vector<float> want(in);
    std::sort(want.begin(), want.end());
    bool agree = true;
    const std::vector<float> out = team_sort(w, in, &agree);
    ++g_checks;
    if (!agree) fail("the signed executor differs from the schedule", w, n);
    if (!std::equal(want.begin(), want.end(), out.begin())) fail("against std::sort", w, n);
  }
}

void nan_policy(const int w, const int n) {
  std::vector<float> in((size_t)n);
  for (int i = 0; i < n; ++i) in[(size_t)i] = (float)((i * 7) % n);
  in[(size_t)(n / 2)] = std::numeric_limits<float>::quiet_NaN();
  in[0] = std::numeric_limits<float>::quiet_NaN();
  const std::vector<float> out = team_sort(w, in);
  ++g_checks;
  bool ok = out[(size_t)(n - 1)] == kInf && out[(size_t)(n - 2)] == kInf;
  for (int i = 0; i + 1 < n; ++i) ok = ok && out[(size_t)i] <= out[(size_t)(i + 1)];
  for (int i = 0; i < n - 2; ++i) ok = ok && out[(size_t)i] < kInf;
  if (!ok) fail("NaN enters as +inf", w, n);
}

template <int M>
double lane_tree_of(const double *pos) {
  double t[M];
  for (int r = 0; r < M; ++r) t[r] = pos[r];
  return rd::lane_tree(t);
}
double lane_tree_m(const int m, const double *pos) {
  switch (m) {
    case 4: return lane_tree_of<4>(pos);
    case 8: return lane_tree_of<8>(pos);
    case 16: return lane_tree_of<16>(pos);
    case 32: return lane_tree_of<32>(pos);
  }
  return std::nan("");
}

// SampleStoreF32::sum after sort(): position q m + r holds rank q m + r widened to double, a pad slot adds +0.0
void widened_tree(const int w, const int n) {
  if (!ts::spread_f32(n, w)) return;
  const int m = ts::slots_f32(n, w);
  for (int kind = 0; kind < 3; ++kind) {
    std::vector<float> x((size_t)n);
    for (int i = 0; i < n; ++i) {
      const uint64_t u = next_u64();
      x[(size_t)i] = kind == 0 ? (float)(int32_t)(u >> 40) * 0x1p-20f - 8.0f : kind == 1 ? (u % 9 == 0 ? 1e16f : u % 9 == 1 ? -1e16f : (float)(u % 100) * 0.37f) : -0.0f;
    }
    std::sort(x.begin(), x.end());
    const double want = rd::tree_sum_of(n, [&](const int i) { return (double)x[(size_t)i]; });
    std::vector<double> pos((size_t)(w * m), 0.0), s((size_t)w), next((size_t)w);
    for (int i = 0; i < n; ++i) pos[(size_t)i] = (double)x[(size_t)i];
    for (int q = 0; q < w; ++q) s[(size_t)q] = lane_tree_m(m, &pos[(size_t)(q * m)]);
    for (int dist = 1; dist < w; dist <<= 1) {
      for (int q = 0; q < w; ++q) next[(size_t)q] = s[(size_t)q] + s[(size_t)(q ^ dist)];
      s.swap(next);
    }
    ++g_checks;
    for (int q = 0; q < w; ++q)
      if (!same_bits(rd::finish_sum(s[(size_t)q]), want)) { fail("the f64 tree over the widened floats", w, n); break; }
  }
}

}  // namespace

int main() {
  for (const int w : {4, 16}) {
    for (int n = 1; n <= 132; ++n) layout(w, n);
    ++g_checks;
    if (!ts::spread_f32(32 * w, w) || ts::spread_f32(32 * w + 1, w) || ts::spread_f32(32 * w, 1)) fail("the spread / replicated boundary", w, 32 * w);
    for (int n = 1; n <= 16; ++n) zero_one(w, n);
    for (const int n : {45, 100, 128, 512}) against_std_sort(w, n);
    for (const int n : {3, 8, 17, 45, 128}) nan_policy(w, n);
    for (int n = 1; n <= 64; ++n) widened_tree(w, n);
    for (const int n : {100, 128}) widened_tree(w, n);
  }
  std::printf("team_sample_f32: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
