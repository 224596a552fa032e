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
// The executor's model and the checks on it are signed_executor.hpp's, shared with the binary32 proof; the whole schedule is here.
// Prints one line per failure and a summary; the exit status is the number of failures, capped at 1.
#include "team_sample.hpp"

#include "signed_executor.hpp"

namespace {

static_assert(ts::slots(128, 16) == 8 && ts::slots(128, 4) == 32 && ts::slots(45, 16) == 4 && ts::slots(20, 4) == 8, "slots per lane");
static_assert(ts::slots(1, 16) == 2 && ts::slots(17, 16) == 2 && ts::slots(257, 16) == 32 && ts::slots(512, 16) == 32, "slots per lane");
static_assert(ts::spread(128, 4) && !ts::spread(257, 4) && !ts::spread(129, 4) && !ts::spread(8, 1) && ts::spread(512, 16) && !ts::spread(513, 16),
              "spread while a lane's slots fit the unrolled size");
static_assert(ts::step_count(16, 8) == 28 && ts::step_count(4, 32) == 28 && ts::step_count(4, 2) == 6, "log P (log P + 1) / 2 steps");
static_assert(ts::step_at(16, 8, 0).dist == 1 && !ts::step_at(16, 8, 0).cross && ts::step_at(16, 8, 0).stage == 2, "the first step");
static_assert(ts::step_at(16, 8, 6).cross && ts::step_at(16, 8, 6).dist == 1 && ts::step_at(16, 8, 6).stage == 16, "the first cross-lane step");

// run_schedule itself on all W M positions of a team, no pad among them
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

}  // namespace

int main() {
  for (const int w : {1, 4, 16}) {
    for (int n = 1; n <= 16; ++n) zero_one<double>(w, n);
    for (const int n : {33, 45, 100, 128, 257, 512}) { against_std_sort<double>(w, n); whole_schedule(w, n); }
    for (const int n : {3, 8, 17, 45, 128}) nan_policy<double>(w, n);
  }
  zero_one<double>(4, 20);                             // five blocks over four lanes: six slots padded to eight
  against_std_sort<double>(4, 257);                    // (named: the replicated fallback)
  std::printf("team_sample: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
