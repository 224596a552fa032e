// team_series.hpp -- sabc::Series<N, W>: one particle's time series x_0 .. x_{N-1} of doubles, in time order, on the W lanes that
// run the particle; element t meets element t - L across the lanes of the team.
//
// team_sample.hpp holds a SAMPLE: what it computes is symmetric in its elements (order statistics, distances between sorted
// samples), and before the sort an element lies where its Philox block was generated.  A series is compared through lagged
// summaries -- autocovariances of an MA(q) or AR model, the lag statistics of Ricker or Lotka-Volterra --, so it lies in time
// order from the start, in the layout Sample has AFTER its sort:
//
//   M = teamsort::slots(N, W); time t on lane t / M in slot t mod M: position p = q M + r.  Positions >= N hold 0.0 and take part
//   in nothing.  Spread over the team when teamsort::spread(N, W); else (W = 1, or M > 32) REPLICATED, a plain double x[N] per
//   lane with the same results, so any N compiles for any W.
//
//   fill_normals: lane q generates the blocks q M / 2 + a, a < M / 2, that exist (< ceil(N / 2)) and keeps both normals of each:
//   block b IS normals 2 b and 2 b + 1, so they land in slots 2 a and 2 a + 1 -- nothing moves between lanes.  (Sample deals its
//   blocks round-robin, block b to lane b mod W; here a lane's blocks are consecutive.)  The stream advances by ceil(N / 2): the
//   blocks and values a lane gets from rng.for_pairs plus an odd last draw, which is what the replicated form does.
//
//   lag<L>: position p reads position p - L.  With L = a M + b, b < M, slot r reads slot r - b of lane q - a where r >= b, and
//   slot r - b + M of lane q - a - 1 where r < b: source slot and lane distance are compile-time constants per slot, at most
//   two distances per L (series::lag_source).  Distance 0 is a register move; distance d one row_shr:d DPP move per 32-bit
//   half -- a quad is aligned inside its row of 16, so the same instruction serves W = 4 --, and the lanes q < d, whose source
//   would lie before the series (or in the neighbouring team), take `before`.  p < L holds exactly on those lanes.
//
//   Reductions: the canonical sum of sample_reduce.hpp over the time index -- a lane adds the tree of its own M slots, the team
//   follows with the xor_lane butterfly, then finish_sum.  Position equals index for every W, so sum, lagged_sum and
//   autocovariance give the same bits for 1, 4 and 16 lanes, for the replicated store and for the NumPy restatement, always (a
//   Sample only after its sort).  No LDS memory, no barrier, no atomic; a read-out returns the same value on every lane.
//
// A series is not sorted, so there is no NaN policy: values pass through unchanged.
//
//   recur / recur_with / cumsum: a state carried from t = 0 upwards, one application of f per time step -- THE SEQUENTIAL LOOP,
//   whose bits are those of the plain `for` over x[t] for every W by construction: no order of association is chosen.  A team
//   runs it as a RELAY over the ceil(N / M) lanes that hold a time < N, in lane order.  In phase p every lane of the team starts
//   from the same carried state and runs its own M slots in order through f, with its own times and its own elements; lane p
//   alone keeps the outputs (a select behind the computation, no branch around it), and its state is handed to every lane with
//   team_pick_ct<W, p> per component: the carry of phase p + 1 and, behind the last phase, the value returned.  The pick is
//   issued by every lane in uniform control flow, and nothing uninitialised is read: the other lanes compute f on the true carry
//   and their own real elements and discard the result.  So every lane issues N evaluations of f, as a lane alone does -- the
//   recurrence is not divided; the draws, maps, zips, summaries and registers around it are.  series::run_recur is the schedule
//   on plain arrays.
//
//   Count draws (state-space models with count observations: Ricker, branching processes, chain-binomial epidemics in time
//   order).  NormalStream::poisson / binomial consume a data-dependent number of blocks of the ONE sequential counter, so a draw
//   at time t cannot start before the draw at t - 1 has ended, and inside map / fill / zip -- a lane runs its own slots only --
//   the lanes of a team would make different requests of the shared generator.  A series draws its counts KEYED BY THE TIME STEP
//   instead (CountDraws, device_rng.hpp): cd = rng.reserve_counts(N) gives draw index t the 64 blocks base + 64 t .. + 63, and
//   cd.poisson(t, lambda) / cd.binomial(t, n, p) are pure functions of their arguments that the calling lane computes alone.
//   In map / fill / zip a lane draws for the slots it holds: the draws of a series are DIVIDED among the team (the replicated
//   store: every lane all N).  map_poisson(rng, scale) is x_t <- Poisson(scale x_t) with index t, the slot loop rolled.
//   Inside recur / recur_with f may call the const members of a CountDraws -- they are pure, the relay's discarded evaluations
//   are harmless -- and still may not draw from rng.  The recurrence is NOT divided: every lane issues all N draws, a row of 16
//   lanes sixteen times the draws of one lane.
//
// Out of scope: a parallel scan for associative operations (its rounding would depend on the order of association, other bits
// than the loop's); a binary32 twin; lags between two series other than through lag<L>() followed by zip.
//
// The layout, the lag schedule and the block ownership are constexpr and compile with a plain C++ compiler, as
// teamsort::step_at does; tests/team_series/check_series.cpp runs them on plain arrays of W M positions.
#pragma once
#include "team_sample.hpp"

namespace sabc {
namespace series {

constexpr int time_lane(int t, int m) { return t / m; }
constexpr int time_slot(int t, int m) { return t & (m - 1); }
constexpr int time_of(int lane, int slot, int m) { return lane * m + slot; }

// slot r of lane q takes, for lag l, slot `slot` of lane q - dist (dist may reach w: then no lane has a source)
struct Source {
  int slot, dist;
};
constexpr Source lag_source(int r, int l, int m) {
  return r >= (l & (m - 1)) ? Source{r - (l & (m - 1)), l / m} : Source{r - (l & (m - 1)) + m, l / m + 1};
}

// fill_normals: the a-th block of lane q (a < m / 2), and whether it is one of the stream's ceil(n / 2)
constexpr int block_of(int lane, int a, int m) { return lane * (m / 2) + a; }
constexpr bool owns_block(int lane, int a, int n, int m) { return block_of(lane, a, m) < teamsort::blocks(n); }

// (x - c)(y - c) rounded on its own: a product that the canonical tree's additions cannot fuse with, so every width and the NumPy
// restatement agree to the bit.  The pragma is what the language offers; a compiler told -ffp-contract=fast (the run-time
// compiler is) fuses whatever it sees regardless, so on the device the product also passes through an empty asm, behind which
// the compiler sees no product.
SABC_SORT_HD double rounded_product(const double a, const double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double p = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(p));
#endif
  return p;
}

// ---- the schedule on plain arrays of w m positions (the CPU proof; the definitions the device's members are held to) ----
// out[p] = in[p - l] where a source exists, `before` on the lanes in front of it, 0.0 at positions >= n
SABC_SORT_HD void run_lag(const int w, const int m, const int n, const int l, const double before, const double *in, double *out) {
  for (int q = 0; q < w; ++q)
    for (int r = 0; r < m; ++r) {
      const Source s = lag_source(r, l, m);
      const double v = q < s.dist ? before : in[time_of(q - s.dist, s.slot, m)];
      out[time_of(q, r, m)] = time_of(q, r, m) < n ? v : 0.0;
    }
}
// the team's sum of the terms at its w m positions: every lane the tree of its own slots, then the butterfly over the lane
// distances 1, 2, .., w / 2, then finish_sum; lane 0's value (sums[] of w entries is scratch: every lane ends with the same bits)
SABC_SORT_HD double run_team_sum(const int w, const int m, double *term, double *sums) {
  for (int q = 0; q < w; ++q) {
    for (int d = 1; d < m; d <<= 1)
      for (int r = 0; r < m; r += 2 * d) term[q * m + r] = term[q * m + r] + term[q * m + r + d];
    sums[q] = term[q * m];
  }
  for (int d = 1; d < w; d <<= 1)
    for (int q = 0; q < w; ++q)
      if (!(q & d)) sums[q] = sums[q | d] = sums[q] + sums[q | d];
  return reduce::finish_sum(sums[0]);
}
// lagged_sum<L>(g, first) on a plain array x of w m positions, through run_lag and run_team_sum (lagged, term: w m entries each)
template <class G>
SABC_SORT_HD double run_lagged_sum(const int w, const int m, const int n, const int l, const int first, G &&g, const double *x,
                                   double *lagged, double *term, double *sums) {
  if (l > 0) run_lag(w, m, n, l, 0.0, x, lagged);
  for (int p = 0; p < w * m; ++p) term[p] = p < n && p >= first + l ? g(p, x[p], l > 0 ? lagged[p] : x[p]) : 0.0;
  return run_team_sum(w, m, term, sums);
}


// ---- recurrences ----
// the state of a recurrence with K components, 1 <= K <= 4 (a plain double is the other State)
template <int K>
struct Carry {
  static_assert(K >= 1 && K <= 4, "a Carry holds 1 to 4 doubles");
  double v[K];
};
template <class State>
struct CarryOf {
  static_assert(sizeof(State) == 0, "the State of a recurrence is double or sabc::series::Carry<K>, 1 <= K <= 4");
};
template <>
struct CarryOf<double> {
  static constexpr int size = 1;
  static SABC_SORT_HD double &at(double &s, int) { return s; }
};
template <int K>
struct CarryOf<Carry<K>> {
  static constexpr int size = K;
  static SABC_SORT_HD double &at(Carry<K> &s, const int k) { return s.v[k]; }
};
// the lanes of the relay: those that hold a time < n
constexpr int relay_lanes(int n, int m) { return (n + m - 1) / m; }

// One lane's share of one phase: from the carried state s through its own m slots in order, out[r] = f(t, s, x[r]) and s advanced
// where first <= t < n, x[r] and s as they were elsewhere.  f is evaluated at every slot and chosen behind the evaluation.
template <class State, class F>
SABC_SORT_HD void recur_lane(const int q, const int m, const int n, const int first, State &s, F &&f, const double *x, double *out) {
  for (int r = 0; r < m; ++r) {
    const int t = time_of(q, r, m);
    const bool live = first <= t && t < n;
    State next = s;
    const double o = f(t, next, x[r]);
    for (int k = 0; k < CarryOf<State>::size; ++k) CarryOf<State>::at(s, k) = live ? CarryOf<State>::at(next, k) : CarryOf<State>::at(s, k);
    out[r] = live ? o : x[r];
  }
}
// recur(s0, f, first) on plain arrays of w m positions, x -> out (they may be the same array), phase by phase as the device
// walks them, the evaluations of the lanes that discard theirs included: `discarded(p, q, out_of_lane_q, state_of_lane_q)` sees
// what lane q != p computed in phase p before the select (the CPU proof overwrites it and finds nothing changed).
template <class State, class F, class D>
SABC_SORT_HD State run_recur(const int w, const int m, const int n, const int first, State s, F &&f, const double *x, double *out,
                             D &&discarded) {
  for (int p = 0; p < w * m; ++p) out[p] = x[p];
  for (int p = 0; p < relay_lanes(n, m); ++p) {
    State handed = s;
    for (int q = 0; q < w; ++q) {
      State mine = s;
      double kept[kSortUnrollMax];
      recur_lane(q, m, n, first, mine, f, out + q * m, kept);
      if (q != p) discarded(p, q, kept, mine);
      for (int r = 0; r < m; ++r) out[q * m + r] = q == p ? kept[r] : out[q * m + r];
      if (q == p) handed = mine;                       // team_pick_ct<W, p>
    }
    s = handed;
  }
  return s;
}
template <class State, class F>
SABC_SORT_HD State run_recur(const int w, const int m, const int n, const int first, State s, F &&f, const double *x, double *out) {
  return run_recur(w, m, n, first, s, f, x, out, [](int, int, double *, State &) {});
}

}  // namespace series
}  // namespace sabc

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
// ---- the device's half: included from the end of device_rng.hpp, behind team_sample.hpp whose Element<double>::select_slot,
// team_add, team_extreme, array_extreme and Summaries it uses ----
namespace sabc {
namespace series {

// v from lane - D of the row of 16 (control_kernel.hpp: dpp_row_shr has this shape); 0 where the row has no such lane
template <int D>
__device__ __forceinline__ double row_shr(const double v) {
  static_assert(D >= 1 && D <= 15, "a lane of the own row of 16");
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x110 + D, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x110 + D, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// ---- spread over the team ----
template <int N, int W, bool SPREAD>
struct SeriesStore {
  static constexpr int M = teamsort::slots(N, W);
  static_assert(W == 4 || W == 16, "a quad or a row of 16 lanes");
  double v[M];

  static __device__ __forceinline__ int lane() { return (int)(threadIdx.x & (unsigned)(W - 1)); }

  template <class F>
  __device__ __forceinline__ void fill_normals(NormalStream &rng, F &&f) {
    const int q = lane();
#pragma unroll
    for (int a = 0; a < M / 2; ++a) {
      v[2 * a] = v[2 * a + 1] = 0.0;
      if (owns_block(0, a, N, M)) {                      // (a constant: some lane of the team has an a-th block)
        double z0, z1;
        box_muller(stream_block(rng.seed, rng.pid, rng.purpose, rng.iter, rng.k + (uint32_t)block_of(q, a, M)), z0, z1);
        const int t = 2 * block_of(q, a, M);
        if (t < N) v[2 * a] = f(t, z0);
        if (t + 1 < N) v[2 * a + 1] = f(t + 1, z1);
      }
    }
    rng.k += (uint32_t)teamsort::blocks(N);
  }
  template <class G>
  __device__ __forceinline__ void fill(G &&g) {
    const int q = lane();
#pragma unroll
    for (int r = 0; r < M; ++r) {
      v[r] = 0.0;
      if (time_of(q, r, M) < N) v[r] = g(time_of(q, r, M));
    }
  }
  template <class G>
  __device__ __forceinline__ void map(G &&g) {
    const int q = lane();
#pragma unroll
    for (int r = 0; r < M; ++r)
      if (time_of(q, r, M) < N) v[r] = g(time_of(q, r, M), v[r]);
  }
  template <class G>
  __device__ __forceinline__ void zip(const SeriesStore &other, G &&g) {
    const int q = lane();
#pragma unroll
    for (int r = 0; r < M; ++r)
      if (time_of(q, r, M) < N) v[r] = g(time_of(q, r, M), v[r], other.v[r]);
  }
  // map with the slot loop ROLLED, for a g whose text is long (a count draw is a few hundred instructions, and map's unrolled
  // loop would hold up to 32 copies of it): ONE copy of g; the slot of the trip is read and written through selects against the
  // trip's number (select_slot and its mirror image, 4 M v_cndmask_b32 per trip), so the values stay in registers.
  template <class G>
  __device__ __forceinline__ void map_rolled(G &&g) {
    const int q = lane();
#pragma unroll 1
    for (int r = 0; r < M; ++r) {
      const int t = time_of(q, r, M);
      const double x = teamsort::Element<double>::select_slot<M>(v, r);
      const double y = t < N ? g(t, x) : x;
#pragma unroll
      for (int j = 0; j < M; ++j) v[j] = j == r ? y : v[j];
    }
  }
  __device__ __forceinline__ double at(const int t) const {
    return team_pick<W>(teamsort::Element<double>::select_slot<M>(v, time_slot(t, M)), (uint32_t)time_lane(t, M));
  }
  __device__ __forceinline__ void emit(NormalStream &rng, const long long first_output, const int first) const {
    if (!emitting(rng)) return;
    const int q = lane();
#pragma unroll
    for (int r = 0; r < M; ++r) {
      const int t = time_of(q, r, M);
      if (t < N && t >= first) sabc::emit(rng, first_output + (t - first), v[r]);
    }
  }

  template <int L, int R>
  __device__ __forceinline__ double lagged_slot(const int q, const double before) const {
    constexpr Source s = lag_source(R, L, M);
    double x;
    if constexpr (s.dist == 0) x = v[s.slot];
    else if constexpr (s.dist >= W) x = before;
    else {
      // the move first, by every lane of the team, the choice after it: inside the conditional's arm it would run with the lanes
      // q < dist switched off, and a DPP move reads 0 from a lane that is
      const double shifted = row_shr<s.dist>(v[s.slot]);
      x = q < s.dist ? before : shifted;
    }
    if constexpr (time_of(W - 1, R, M) >= N) x = time_of(q, R, M) < N ? x : 0.0;
    return x;
  }
  template <int L, int... R>
  __device__ __forceinline__ void lag_into(SeriesStore &out, const double before, sortnet::seq<R...>) const {
    const int q = lane();
    ((out.v[R] = lagged_slot<L, R>(q, before)), ...);
  }
  template <int L>
  __device__ __forceinline__ void lag_store(SeriesStore &out, const double before) const {
    lag_into<L>(out, before, typename sortnet::make_seq<M>::type{});
  }

  // the canonical sum of g(t, x_t, x_{t-L}) over first + L <= t < N, +0.0 elsewhere
  template <int L, class G>
  __device__ __forceinline__ double lagged_sum_store(G &&g, const int first) const {
    const int q = lane();
    double term[M];
    if constexpr (L == 0) {
#pragma unroll
      for (int r = 0; r < M; ++r) {
        const int t = time_of(q, r, M);
        term[r] = t < N && t >= first ? g(t, v[r], v[r]) : 0.0;
      }
    } else {
      SeriesStore back;
      lag_store<L>(back, 0.0);
#pragma unroll
      for (int r = 0; r < M; ++r) {
        const int t = time_of(q, r, M);
        term[r] = t < N && t >= first + L ? g(t, v[r], back.v[r]) : 0.0;
      }
    }
    return reduce::finish_sum(teamsort::team_add<W>(reduce::lane_tree(term)));
  }
  template <bool MAX, class G>
  __device__ __forceinline__ double extreme(G &&g) const {
    const int q = lane();
    double s = MAX ? -sortnet::inf_(0.0) : sortnet::inf_(0.0);
#pragma unroll
    for (int r = 0; r < M; ++r) {
      const int t = time_of(q, r, M);
      if (t < N) s = MAX ? sortnet::max_(s, g(t, v[r])) : sortnet::min_(s, g(t, v[r]));
    }
    return teamsort::team_extreme<W, MAX>(s);
  }

  // the relay: phase P.  Every lane from the same carry through its own slots; lane P keeps the outputs; its state to all.
  template <int P, class State, class F>
  __device__ __forceinline__ void recur_phase(State &s, F &&f, const int first, const int q) {
    State mine = s;
    double kept[M];
#pragma unroll
    for (int r = 0; r < M; ++r) {
      const int t = time_of(q, r, M);
      const bool live = first <= t && t < N;
      State next = mine;
      const double o = f(t, next, r);
#pragma unroll
      for (int k = 0; k < CarryOf<State>::size; ++k)
        CarryOf<State>::at(mine, k) = live ? CarryOf<State>::at(next, k) : CarryOf<State>::at(mine, k);
      kept[r] = live ? o : v[r];
    }
#pragma unroll
    for (int r = 0; r < M; ++r) v[r] = q == P ? kept[r] : v[r];
    // by every lane of the team, in uniform control flow: a DPP move reads 0 from a lane that is switched off
#pragma unroll
    for (int k = 0; k < CarryOf<State>::size; ++k) CarryOf<State>::at(s, k) = team_pick_ct<W, P>(CarryOf<State>::at(mine, k));
  }
  template <class State, class F, int... P>
  __device__ __forceinline__ void recur_phases(State &s, F &&f, const int first, sortnet::seq<P...>) {
    const int q = lane();
    (recur_phase<P>(s, f, first, q), ...);
  }
  // f(t, State &s, slot r): the members below bind the slot to this series' element (and another's)
  template <class State, class F>
  __device__ __forceinline__ State recur_store(State s, F &&f, const int first) {
    recur_phases(s, f, first, typename sortnet::make_seq<relay_lanes(N, M)>::type{});
    return s;
  }
  template <class State, class F>
  __device__ __forceinline__ State recur_one(State s, F &&f, const int first) {
    return recur_store(s, [&](const int t, State &c, const int r) { return f(t, c, v[r]); }, first);
  }
  template <class State, class F>
  __device__ __forceinline__ State recur_two(const SeriesStore &other, State s, F &&f, const int first) {
    return recur_store(s, [&](const int t, State &c, const int r) { return f(t, c, v[r], other.v[r]); }, first);
  }
  // The same relay with the loops over phases and slots ROLLED, for an f whose text is long (one that draws counts: the
  // unrolled relay holds relay_lanes M copies of f, 128 count draws at N = 128): ONE copy of f.  The slot of the trip is read
  // and written through selects against the trip's number, as in map_rolled, and the phase's lane is picked at run time
  // (team_pick<W>, a branch per bit of the phase, uniform over the team).  f at slot r reads slot r alone, so writing the kept
  // output at once is what recur_phase does behind its loop.  The same applications of f to the same arguments: the same bits.
  template <class State, class F>
  __device__ __forceinline__ State recur_store_rolled(State s, F &&f, const int first) {
    const int q = lane();
#pragma unroll 1
    for (int p = 0; p < relay_lanes(N, M); ++p) {
      State mine = s;
#pragma unroll 1
      for (int r = 0; r < M; ++r) {
        const int t = time_of(q, r, M);
        const bool live = first <= t && t < N;
        const double x = teamsort::Element<double>::select_slot<M>(v, r);
        State next = mine;
        const double o = f(t, next, r, x);
#pragma unroll
        for (int k = 0; k < CarryOf<State>::size; ++k)
          CarryOf<State>::at(mine, k) = live ? CarryOf<State>::at(next, k) : CarryOf<State>::at(mine, k);
        const double keep = live && q == p ? o : x;
#pragma unroll
        for (int j = 0; j < M; ++j) v[j] = j == r ? keep : v[j];
      }
      // by every lane of the team, in uniform control flow
#pragma unroll
      for (int k = 0; k < CarryOf<State>::size; ++k) CarryOf<State>::at(s, k) = team_pick<W>(CarryOf<State>::at(mine, k), (uint32_t)p);
    }
    return s;
  }
  template <class State, class F>
  __device__ __forceinline__ State recur_one_rolled(State s, F &&f, const int first) {
    return recur_store_rolled(s, [&](const int t, State &c, const int, const double x) { return f(t, c, x); }, first);
  }
};

// ---- replicated: a lane per particle, or a series too long for the team's registers ----
template <int N, int W>
struct SeriesStore<N, W, false> {
  static_assert(W == 1 || W == 4 || W == 16, "a lane, a quad or a row of 16 lanes");
  double x[N];

  template <class F>
  __device__ __forceinline__ void fill_normals(NormalStream &rng, F &&f) {
    int at_ = 0;
    rng.for_pairs(N >> 1, [&](const double z0, const double z1) {
      x[at_] = f(at_, z0);
      x[at_ + 1] = f(at_ + 1, z1);
      at_ += 2;
    });
    if (N & 1) {
      double z0, z1;
      rng.pair(z0, z1);
      x[N - 1] = f(N - 1, z0);
    }
  }
  template <class G>
  __device__ __forceinline__ void fill(G &&g) {
    for (int t = 0; t < N; ++t) x[t] = g(t);
  }
  template <class G>
  __device__ __forceinline__ void map(G &&g) {
    for (int t = 0; t < N; ++t) x[t] = g(t, x[t]);
  }
  template <class G>
  __device__ __forceinline__ void zip(const SeriesStore &other, G &&g) {
    for (int t = 0; t < N; ++t) x[t] = g(t, x[t], other.x[t]);
  }
  template <class G>
  __device__ __forceinline__ void map_rolled(G &&g) {
#pragma unroll 1
    for (int t = 0; t < N; ++t) x[t] = g(t, x[t]);
  }
  __device__ __forceinline__ double at(const int t) const { return x[t]; }
  __device__ __forceinline__ void emit(NormalStream &rng, const long long first_output, const int first) const {
    if (!emitting(rng) || (threadIdx.x & (unsigned)(W - 1)) != 0) return;
    for (int t = first > 0 ? first : 0; t < N; ++t) sabc::emit(rng, first_output + (t - first), x[t]);
  }
  template <int L>
  __device__ __forceinline__ void lag_store(SeriesStore &out, const double before) const {
    for (int t = 0; t < N; ++t) out.x[t] = t >= L ? x[t >= L ? t - L : 0] : before;
  }
  template <int L, class G>
  __device__ __forceinline__ double lagged_sum_store(G &&g, const int first) const {
    return reduce::tree_sum_of(N, [&](const int t) { return t >= first + L ? g(t, x[t], x[t >= L ? t - L : 0]) : 0.0; });
  }
  template <bool MAX, class G>
  __device__ __forceinline__ double extreme(G &&g) const { return teamsort::array_extreme<MAX>(x, g); }
  // the plain loop
  template <class State, class F>
  __device__ __forceinline__ State recur_one(State s, F &&f, const int first) {
    for (int t = first > 0 ? first : 0; t < N; ++t) x[t] = f(t, s, x[t]);
    return s;
  }
  template <class State, class F>
  __device__ __forceinline__ State recur_two(const SeriesStore &other, State s, F &&f, const int first) {
    for (int t = first > 0 ? first : 0; t < N; ++t) x[t] = f(t, s, x[t], other.x[t]);
    return s;
  }
  // (the plain loop is rolled as it stands)
  template <class State, class F>
  __device__ __forceinline__ State recur_one_rolled(State s, F &&f, const int first) { return recur_one(s, f, first); }
};

}  // namespace series

// One particle's series of N doubles in time order on the W = 1 | 4 | 16 lanes that run the particle (a simulator from source
// gets W as the template argument of sabc_user_simulate_team<W>).  All lanes of a team make the same calls in the same order;
// a read-out returns the same value on every lane of the team.
//   fill_normals(rng, f): x_t = f(t, normal t of the stream), ceil(N / 2) whole blocks consumed; fill(g): x_t = g(t);
//   map(g): x_t <- g(t, x_t); zip(other, g): x_t <- g(t, x_t, other_t), in-lane; at(t): x_t, t uniform over the team;
//   emit(rng, first_output, first = 0): x_t, t >= first, to output first_output + t - first, each value written once.
//   lag<L>(before = 0.0), 1 <= L < N: the series whose element t is x_{t-L}, `before` for t < L.
//   lagged_sum<L>(g, first = 0): the canonical sum over t = 0 .. N-1 of g(t, x_t, x_{t-L}) for t >= first + L, +0.0 otherwise.
//   autocovariance<L>(center = 0.0, first = 0), 0 <= L < N: that sum of (x_t - c)(x_{t-L} - c), each product rounded on its own
//   (series::rounded_product), divided by N - first.
//   sum(g), max(g), min(g) over g(t, x_t); sum(), mean(); moments(mean, var): Sample's definitions over the time index.
//   recur(s0, f, first = 0): for t = first .. N-1 in time order x_t <- f(t, s, x_t), where f takes `State &s` and may change it;
//   returns the state behind t = N-1, the same value on every lane.  recur_with(other, s0, f, first = 0): the same with
//   f(t, s, x_t, other_t).  cumsum(): recur(0.0, s = s + x).  State is double or sabc::series::Carry<K> (double v[K], 1 <= K <= 4).
//   Elements t < first are left as they are and do not touch the state.  The bits are the sequential loop's for every W.
//   THE CONTRACT ON f: a pure function of its arguments.  The library may evaluate it on lanes that discard the result (the relay
//   at the head of this file), so f has no side effects: it does not call emit, does not draw from rng and does not use the
//   state as an index into memory.  f MAY call the const members of a sabc::CountDraws (cd.poisson(t, lambda),
//   cd.binomial(t, n, p) with cd = rng.reserve_counts(N) taken in front of the recurrence): they are pure and total.  THE COST:
//   the recurrence is not divided, so every lane of the team issues all N draws -- a row of 16 lanes 16 times the draws of one.
//   recur_rolled(s0, f, first = 0): recur with the relay's loops rolled, ONE copy of f in the text where recur holds
//   one per time step (a count draw is a few hundred instructions); the same bits.  The form for an f that draws.
//   map_poisson(rng, scale = 1.0): x_t <- Poisson(scale x_t), the draw keyed by t (reserves N indices itself); a lane draws for
//   its own slots (spread) or for all N (replicated).  The plain spelling through map gives the same values:
//   cd = rng.reserve_counts(N); x.map([&](int t, double v) { return (double)cd.poisson(t, rounded_product(scale, v)); }).
//   ROUNDING IS THE CALLER'S: the run-time compiler is told -ffp-contract=fast, so an a * b + c inside f may fuse on the device
//   and not in a transcription.  f writes fma(...) where it wants one and series::rounded_product where it wants a product
//   rounded on its own.  cumsum only adds.
// Values pass through unchanged: no NaN policy.  The same bits for every W.
template <int N, int W>
struct Series : series::SeriesStore<N, W, teamsort::spread(N, W)>, teamsort::Summaries<Series<N, W>, N> {
  static_assert(N >= 1, "a series holds at least one value");
  static constexpr int size = N, lanes = W;
  static constexpr bool spread = teamsort::spread(N, W);
  using Store = series::SeriesStore<N, W, teamsort::spread(N, W)>;

  __device__ __forceinline__ void emit(NormalStream &rng, const long long first_output, const int first = 0) const {
    Store::emit(rng, first_output, first);
  }
  template <int L>
  __device__ __forceinline__ Series lag(const double before = 0.0) const {
    static_assert(L >= 1 && L < N, "1 <= L < N");
    Series out;
    Store::template lag_store<L>(out, before);
    return out;
  }
  template <int L, class G>
  __device__ __forceinline__ double lagged_sum(G &&g, const int first = 0) const {
    static_assert(L >= 1 && L < N, "1 <= L < N");
    return Store::template lagged_sum_store<L>(g, first);
  }
  template <int L>
  __device__ __forceinline__ double autocovariance(const double center = 0.0, const int first = 0) const {
    static_assert(L >= 0 && L < N, "0 <= L < N");
    return Store::template lagged_sum_store<L>([&](const int, const double a, const double b) {
      return series::rounded_product(a - center, b - center);
    }, first) / (double)(N - first);
  }
  template <class G> __device__ __forceinline__ double sum(G &&g) const {
    return Store::template lagged_sum_store<0>([&](const int t, const double a, const double) { return g(t, a); }, 0);
  }
  using teamsort::Summaries<Series, N>::sum;           // sum(), and with it max(g), min(g), mean(), moments(mean, var)

  template <class State, class F>
  __device__ __forceinline__ State recur(const State s0, F &&f, const int first = 0) {
    static_assert(series::CarryOf<State>::size >= 1, "double or Carry<K>");
    return Store::recur_one(s0, f, first);
  }
  template <class State, class F>
  __device__ __forceinline__ State recur_with(const Series &other, const State s0, F &&f, const int first = 0) {
    static_assert(series::CarryOf<State>::size >= 1, "double or Carry<K>");
    return Store::recur_two(other, s0, f, first);
  }
  // recur for an f whose text is long -- one that draws counts --: one copy of f in the text where recur holds one
  // per time step a lane walks (N of them), the same bits
  template <class State, class F>
  __device__ __forceinline__ State recur_rolled(const State s0, F &&f, const int first = 0) {
    static_assert(series::CarryOf<State>::size >= 1, "double or Carry<K>");
    return Store::recur_one_rolled(s0, f, first);
  }
  __device__ __forceinline__ void cumsum() {
    recur(0.0, [](const int, double &s, const double x) { s = s + x; return s; });
  }
  // x_t <- Poisson(scale x_t) for every t < N, the draw keyed by t: reserves N draw indices (64 N blocks of counter space, none
  // generated unless a trial asks for it) and draws with index t, the product scale x_t rounded on its own.  The same values as
  //   cd = rng.reserve_counts(N); x.map([&](int t, double v) { return (double)cd.poisson(t, rounded_product(scale, v)); })
  // with one copy of the draw in the text where map would hold one per slot.
  __device__ __forceinline__ void map_poisson(NormalStream &rng, const double scale = 1.0) {
    const CountDraws cd = rng.template reserve_counts<N>();
    Store::map_rolled([&](const int t, const double v) { return (double)cd.poisson(t, series::rounded_product(scale, v)); });
  }
};

}  // namespace sabc
#endif
