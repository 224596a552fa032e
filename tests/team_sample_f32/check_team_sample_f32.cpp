// The CPU proof of csrc/team_sample_f32.hpp, built from the headers alone (tests/test_team_sample_f32_host.py: g++, address and
// undefined-behaviour sanitizers where their runtimes exist).  For teams of W = 4 and 16 lanes:
//   * THE LAYOUT (teamsort's with four normals to a block): for every N <= 132, draw -> (draw_lane, draw_slot) is injective, lands
//     below M on the lane that generates the draw's block of four, its image plus the pad slots is all W M positions, and draw_of
//     inverts it;
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
// The executor's model and the checks on it are ../team_sample/signed_executor.hpp's, shared with the f64 proof; the layout for every
// N and the widened tree are here.  Prints one line per failure and a summary; the exit status is 1 if anything failed.
#include "team_sample_f32.hpp"

#include "../team_sample/signed_executor.hpp"

namespace {

namespace rd = sabc::reduce;

static_assert(ts::slots(128, 16, 4) == 8 && ts::slots(128, 4, 4) == 32 && ts::slots(45, 16, 4) == 4 && ts::slots(45, 4, 4) == 16, "slots per lane");
static_assert(ts::slots(1, 16, 4) == 4 && ts::slots(64, 16, 4) == 4 && ts::slots(65, 16, 4) == 8 && ts::slots(17, 4, 4) == 8, "whole blocks of four");
static_assert(ts::spread(128, 4, 4) && !ts::spread(129, 4, 4) && ts::spread(512, 16, 4) && !ts::spread(513, 16, 4) && !ts::spread(8, 1, 4),
              "spread while a lane's slots fit the unrolled size");
static_assert(ts::blocks(1, 4) == 1 && ts::blocks(4, 4) == 1 && ts::blocks(5, 4) == 2 && ts::blocks(128, 4) == 32, "whole blocks");

void layout(const int w, const int n) {
  ++g_checks;
  const int m = ts::slots(n, w, 4);
  if (m < 4 || (m & (m - 1)) || w * m < n) { fail("slots per lane", w, n); return; }
  std::vector<int> owner((size_t)(w * m), -1);
  for (int i = 0; i < n; ++i) {
    const int q = ts::draw_lane(i, w, 4), r = ts::draw_slot(i, w, 4);
    if (q < 0 || q >= w || r < 0 || r >= m) { fail("a draw outside the team's slots", w, n); return; }
    if (q != (i / 4) % w || (r & 3) != (i & 3)) fail("a draw away from the lane that generates its block", w, n);
    if (owner[(size_t)(q * m + r)] != -1) { fail("two draws in one slot", w, n); return; }
    owner[(size_t)(q * m + r)] = i;
    if (ts::draw_of(q, r, w, 4) != i) fail("draw_of does not invert the layout", w, n);
  }
  int pads = 0;
  for (int q = 0; q < w; ++q)
    for (int r = 0; r < m; ++r) {
      const int i = ts::draw_of(q, r, w, 4);
      if (owner[(size_t)(q * m + r)] == -1) {
        ++pads;
        if (i < n) fail("a pad slot whose draw index is below N", w, n);
      } else if (owner[(size_t)(q * m + r)] != i) {
        fail("draw_of disagrees with the layout", w, n);
      }
    }
  if (pads + n != w * m) fail("draws plus pad slots are not all positions", w, n);
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

// SampleF32's sum after sort(): position q m + r holds rank q m + r widened to double, a pad slot adds +0.0
void widened_tree(const int w, const int n) {
  if (!ts::spread(n, w, 4)) return;
  const int m = ts::slots(n, w, 4);
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
    if (!ts::spread(32 * w, w, 4) || ts::spread(32 * w + 1, w, 4) || ts::spread(32 * w, 1, 4)) fail("the spread / replicated boundary", w, 32 * w);
    for (int n = 1; n <= 16; ++n) zero_one<float>(w, n);
    for (const int n : {45, 100, 128, 512}) against_std_sort<float>(w, n);
    for (const int n : {3, 8, 17, 45, 128}) nan_policy<float>(w, n);
    for (int n = 1; n <= 64; ++n) widened_tree(w, n);
    for (const int n : {100, 128}) widened_tree(w, n);
  }
  std::printf("team_sample_f32: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
