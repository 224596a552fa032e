// team_sample.hpp -- sabc::Sample<N, W>: one particle's sample of N doubles, drawn and sorted by the W lanes that run the particle.
//
// sort_network.hpp sorts an array that every lane holds whole: in a team of lanes per particle (update_kernel.hpp: LANES; a quad,
// a row of 16) every lane of the team sorts all N values and applies the draw's transform to all of them, and above 32 values
// the network loops over private memory.  Here the sample is SPREAD over the team, the layout of the built-in g-and-k kernel
// (device_models.hpp: gk_simulate_rows4): lane q of the team (q = threadIdx.x & (W - 1)) holds M slots in registers, the team
// W M >= N of them, the rest +inf.
//
//   M = pow2ceil(2 ceil(ceil(N / 2) / W)): the normals come in blocks of two and a lane keeps BOTH normals of the blocks it
//   generates (nothing is broadcast), so a lane holds a whole number of blocks.  That is pow2ceil(ceil(N / W)) except for the
//   smallest samples (N = 16, W = 16: 2 slots, not 1).  M <= kSortUnrollMax = 32, i.e. N <= 32 W.
//
//   W = 1, or M > 32: the REPLICATED form -- every lane holds all N values in an array, filled from the stream as a simulator
//   does by hand (for_pairs, an odd last draw from one more block) and sorted by sabc::sort_ascending: what a lane per particle
//   costs today, the same bits.  So any N compiles for any W.
//
// Before the sort, draw i = normal i of the stream lies on the lane that generated its block b = i / 2 -- lane b mod W, the
// assignment of NormalStream::for_team<double, W> -- in slot 2 (b / W) + (i & 1).  After it, rank i lies on lane i / M in slot
// i mod M: position p = q M + r.  A sorting network is oblivious to where its inputs start, so no value moves between the two.
//
// The network is the bitonic one on P = W M positions: stages k = 2, 4, .., P, in each the steps j = k / 2, .., 1 that order
// positions p and p ^ j -- ascending where (p & k) == 0.  Steps with j < M pair two registers of a lane (one min and one max);
// steps with j >= M pair the lanes at distance j / M of the team, through DPP (1, 2) or ds_swizzle (4, 8): no LDS memory, no
// barrier, no atomic.  THE SCHEDULE -- teamsort::step_at: kind, distance and stage of every step -- is constexpr and compiles
// with a plain C++ compiler; tests/team_sample/check_team_sample.cpp runs it on plain arrays (every 0-1 input for small N, which
// by the 0-1 principle proves those sizes), the device executes the same list on registers.
//
// A cross-lane step is ONE v_min_f64 per element by the signed-value scheme of gk_cross_step: a lane stores y = -x where
// sign_mask(step) says so -- in an in-lane step the lanes that order descending (then every in-lane step orders ascending), in a
// cross-lane step the lanes that keep the maximum (then both sides evaluate min(own, -partner's): min(x_a, x_b) below,
// -max(x_a, x_b) above, already in the sign that lane stores).  Between two steps whose masks differ the lanes that change
// sign flip it: one v_xor_b32 on the high word per element.  The mask is the XOR of at most two lane bits, and 0 after the last
// step.  (min and max are inline asm, as gk_min / gk_max: a __builtin_fmin of a shuffled value is preceded by a canonicalising
// v_max_f64 x, x.  The values are never NaN: a NaN enters as +inf at fill time -- min(x, +inf) --, the policy of gk_datum and of
// sort_network.hpp.)
//
// All lanes of a team hold the same particle and make the same calls in the same order -- the rule NormalStream states --, and a
// read-out returns the same value on every lane of the team.  A rank known only at run time (uniform over the team) selects
// over the slots and picks the lane by DPP: the slots stay registers.
//
// Reductions (sample_reduce.hpp has the definition): sum(g), max(g), min(g) over g(i, value) with i the element's index in the
// current order.  A lane adds the tree of its own M slots (r and r ^ 1, then ^ 2, ..), the team follows with a butterfly over
// the lane distances 1, 2, 4, 8 -- xor_lane and one v_add_f64 per step, a + b == b + a to the bit, so every lane ends with the
// same value; no LDS, no barrier, no atomic.  A slot whose element index is >= N adds +0.0 and takes no part in a maximum.
// After sort() position q M + r holds rank q M + r: in-lane levels are the low bits, the lanes the high bits of the canonical
// tree over the rank, whatever W is -- the same bits for 1, 4 and 16 lanes and for the replicated store.
//
// All of this is written ONCE for the element types double and float: the layout functions take the normals per block, and the
// device's executor, store, summaries and distances are templates over teamsort::Element<T>, which holds what the type decides
// (below; Element<float> and what it changes in the paragraphs above: team_sample_f32.hpp).  Sample<N, W> is the instance for
// doubles.  The team's f64 butterflies (team_add, team_extreme) and the Summaries also serve sabc::Series (team_series.hpp).
#pragma once
#include "sample_reduce.hpp"
#include "sort_network.hpp"

namespace sabc {
namespace teamsort {

constexpr int pow2ceil(int x) { int p = 1; while (p < x) p <<= 1; return p; }
constexpr int ilog2(int x) { return x <= 1 ? 0 : 1 + ilog2(x >> 1); }
// The layout for `per` normals to a Philox block, a power of two: 2 for doubles, 4 for binary32 values (team_sample_f32.hpp)
constexpr int blocks(int n, int per = 2) { return (n + per - 1) / per; }                 // whole Philox blocks of n normals
constexpr int slots(int n, int w, int per = 2) { return pow2ceil(per * ((blocks(n, per) + w - 1) / w)); }      // M
constexpr bool spread(int n, int w, int per = 2) { return w > 1 && slots(n, w, per) <= kSortUnrollMax; }

// where draw i lies before the sort, where rank i lies after it
constexpr int draw_lane(int i, int w, int per = 2) { return (i >> ilog2(per)) & (w - 1); }
constexpr int draw_slot(int i, int w, int per = 2) { return per * ((i >> ilog2(per)) / w) + (i & (per - 1)); }
constexpr int draw_of(int lane, int slot, int w, int per = 2) {
  return per * (lane + w * (slot >> ilog2(per))) + (slot & (per - 1));
}
constexpr int rank_lane(int i, int m) { return i / m; }
constexpr int rank_slot(int i, int m) { return i & (m - 1); }

// One step of the schedule: positions p (without the bit of the distance) and p ^ distance meet, distance = dist slots of
// one lane (cross = false) or dist lanes (cross = true: dist M positions); the lower position keeps the minimum where
// (p & stage) == 0, else the maximum (stage = P: nowhere, the final merge).
struct Step {
  bool cross;
  int dist, stage;
};
constexpr int step_count(int w, int m) { return ilog2(w * m) * (ilog2(w * m) + 1) / 2; }
constexpr Step step_at(int w, int m, int i) {
  for (int k = 2; k <= w * m; k <<= 1)
    for (int j = k >> 1; j >= 1; j >>= 1, --i)
      if (i == 0) return j >= m ? Step{true, j / m, k} : Step{false, j, k};
  return Step{false, 0, 0};
}
constexpr int position_distance(const Step s, int m) { return s.cross ? s.dist * m : s.dist; }
// the signed-value scheme: the lanes q with an odd number of bits in q & sign_mask store -x during this step ...
constexpr int descending_lane_bit(const Step s, int w, int m) { return (s.stage / m) & (w - 1); }
constexpr int sign_mask(const Step s, int w, int m) { return descending_lane_bit(s, w, m) ^ (s.cross ? s.dist : 0); }
// ... and an in-lane step of a stage inside the lane orders descending the pairs whose lower slot has this bit
constexpr int descending_slot_bit(const Step s, int m) { return s.stage & (m - 1); }

// the schedule on a plain array of w m positions (the CPU proof; the definition the device's executor is held to)
template <class T>
SABC_SORT_HD void run_step(const Step s, const int w, const int m, T *x) {
  const int j = position_distance(s, m);
  for (int p = 0; p < w * m; ++p) {
    if (p & j) continue;
    const T lo = sortnet::min_(x[p], x[p | j]), hi = sortnet::max_(x[p], x[p | j]);
    const bool ascending = (p & s.stage) == 0;
    x[p] = ascending ? lo : hi;
    x[p | j] = ascending ? hi : lo;
  }
}
template <class T>
SABC_SORT_HD void run_schedule(const int w, const int m, T *x) {
  for (int i = 0; i < step_count(w, m); ++i) run_step(step_at(w, m, i), w, m, x);
}

}  // namespace teamsort
}  // namespace sabc

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
// ---- the device's half: included from the end of device_rng.hpp, whose NormalStream, box_muller, team_pick and emit it uses
namespace sabc {
namespace teamsort {

// What the element type of a sample decides -- all of it: the executor, the store and the summaries below are written once over
// Element<T>.  Specialisations of one template, not overloads: a dependent call on a fundamental type gets no argument-dependent
// lookup, so an overload declared behind the template that calls it (team_sample_f32.hpp's) would not be found.
//   per_block: normals to a Philox block;  inf()
//   Slots<N, W, M>: the spread store's members v[M] and sorted with its fill_normals, the base of SampleStore.  (Per type, in the
//   text it had and called by the simulator itself: as one loop over the normals of a block the f64 form's i + 1 < N is no longer
//   folded into a comparison of the lane with a constant, the two types transform and store in different orders, and behind one
//   more call the same text is scheduled differently.)
//   xor_lane<DIST>(v): v from lane ^ DIST of the row;  vmin, vmax, vmin_neg(a, b) = min(a, -b);  flip_sign(v, bit 31 or 0)
//   select_slot(v, slot): a slot known at run time (the lane known at run time is device_rng.hpp's team_pick<W>, one text for both)
//   the replicated store's fill_normals, order_statistic and quantile, as a simulator writes them by hand for this type
template <class T>
struct Element;
template <int W>
__device__ __forceinline__ int team_lane() { return (int)(threadIdx.x & (unsigned)(W - 1)); }      // q, the lane's place in the team

template <>
struct Element<double> {
  static constexpr int per_block = 2;
  static __device__ __forceinline__ double inf() { return sortnet::inf_(0.0); }
  template <int N, int W, int M>
  struct Slots {
    double v[M];
    bool sorted;
    template <class F>
    __device__ __forceinline__ void fill_normals(NormalStream &rng, F &&f) {
      const int q = team_lane<W>();
#pragma unroll
      for (int a = 0; a < M / 2; ++a) {
        if (a * W < blocks(N)) {                         // (a constant: some lane of the team has a block a)
          double z0, z1;
          box_muller(stream_block(rng.seed, rng.pid, rng.purpose, rng.iter, rng.k + (uint32_t)(a * W + q)), z0, z1);
          const double x0 = f(z0), x1 = f(z1);
          const int i = 2 * (a * W + q);
          v[2 * a] = i < N ? sortnet::min_(x0, sortnet::inf_(0.0)) : sortnet::inf_(0.0);
          v[2 * a + 1] = i + 1 < N ? sortnet::min_(x1, sortnet::inf_(0.0)) : sortnet::inf_(0.0);
        } else {
          v[2 * a] = v[2 * a + 1] = sortnet::inf_(0.0);
        }
      }
      rng.k += (uint32_t)blocks(N);
      sorted = false;
    }
  };

  // (device_models.hpp: xor_lane, restated where hipRTC sees it) DPP quad_perm for 1 and 2, ds_swizzle in bit-mask mode for 4 and 8
  template <int DIST>
  static __device__ __forceinline__ double xor_lane(const double v) {
    static_assert(DIST == 1 || DIST == 2 || DIST == 4 || DIST == 8, "a lane of the own row of 16");
    int lo = __double2loint(v), hi = __double2hiint(v);
    if constexpr (DIST == 1) {
      lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true);           // quad_perm [1,0,3,2]
      hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true);
    } else if constexpr (DIST == 2) {
      lo = __builtin_amdgcn_mov_dpp(lo, 0x4E, 0xF, 0xF, true);           // quad_perm [2,3,0,1]
      hi = __builtin_amdgcn_mov_dpp(hi, 0x4E, 0xF, 0xF, true);
    } else {
      constexpr int pattern = 0x1F | (DIST << 10);                        // and_mask 0x1f, or 0, xor DIST
      lo = __builtin_amdgcn_ds_swizzle(lo, pattern);
      hi = __builtin_amdgcn_ds_swizzle(hi, pattern);
    }
    return __hiloint2double(hi, lo);
  }
  static __device__ __forceinline__ double vmin(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
  static __device__ __forceinline__ double vmax(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
  static __device__ __forceinline__ double vmin_neg(double a, double b) { double r; asm("v_min_f64 %0, %1, -%2" : "=v"(r) : "v"(a), "v"(b)); return r; }
  static __device__ __forceinline__ double flip_sign(const double v, const int flip) { return __hiloint2double(__double2hiint(v) ^ flip, __double2loint(v)); }

  // a select per slot, no indexed access (the array stays in registers).  Chosen by 32-bit halves, the two v_cndmask_b32 a select
  // of doubles is anyway: a select between two LOADED doubles is turned into a load from a selected address while the array is
  // still memory to the compiler, and that leaves it in scratch.
  template <int M>
  static __device__ __forceinline__ double select_slot(const double (&v)[M], const int slot) {
    int lo = __double2loint(v[0]), hi = __double2hiint(v[0]);
#pragma unroll
    for (int r = 1; r < M; ++r) {
      lo = slot == r ? __double2loint(v[r]) : lo;
      hi = slot == r ? __double2hiint(v[r]) : hi;
    }
    return __hiloint2double(hi, lo);
  }

  template <int N, class F>
  static __device__ __forceinline__ void fill_normals(NormalStream &rng, double (&x)[N], F &&f) {
    int at_ = 0;
    rng.for_pairs(N >> 1, [&](const double z0, const double z1) {
      x[at_] = f(z0);
      x[at_ + 1] = f(z1);
      at_ += 2;
    });
    if (N & 1) {
      double z0, z1;
      rng.pair(z0, z1);
      x[N - 1] = f(z0);
    }
  }
  template <int N>
  static __device__ __forceinline__ double order_statistic(const double (&x)[N], const int rank) {
    return sabc::order_statistic(x, N, rank);
  }
  template <int N>
  static __device__ __forceinline__ double quantile(const double (&x)[N], const double p) { return sabc::quantile(x, N, p); }
};

template <class T, int W, int M, int I>
__device__ __forceinline__ void run_step_device(T (&v)[M], const int q) {
  using E = Element<T>;
  constexpr Step s = step_at(W, M, I);
  constexpr int mask = sign_mask(s, W, M), before = I > 0 ? sign_mask(step_at(W, M, I > 0 ? I - 1 : 0), W, M) : 0;
  if constexpr (mask != before) {
    const int flip = (__builtin_popcount(q & (mask ^ before)) & 1) << 31;
#pragma unroll
    for (int r = 0; r < M; ++r) v[r] = E::flip_sign(v[r], flip);
  }
  if constexpr (s.cross) {
    T p[M];
#pragma unroll
    for (int r = 0; r < M; ++r) p[r] = E::template xor_lane<s.dist>(v[r]);
#pragma unroll
    for (int r = 0; r < M; ++r) v[r] = E::vmin_neg(v[r], p[r]);
  } else {
    constexpr int desc = descending_slot_bit(s, M);
#pragma unroll
    for (int r = 0; r < M; ++r) {
      if (r & s.dist) continue;
      const T lo = E::vmin(v[r], v[r | s.dist]), hi = E::vmax(v[r], v[r | s.dist]);
      v[r] = (r & desc) ? hi : lo;
      v[r | s.dist] = (r & desc) ? lo : hi;
    }
  }
}
template <class T, int W, int M, int... I>
__device__ __forceinline__ void run_schedule_device(T (&v)[M], const int q, sortnet::seq<I...>) {
  (run_step_device<T, W, M, I>(v, q), ...);
  static_assert(sign_mask(step_at(W, M, step_count(W, M) - 1), W, M) == 0, "the last step leaves the values themselves");
}

// the type-7 quantile of sort_network.hpp (sabc::quantile: the same arithmetic, the same handling of infinities) over a
// read-out at(i) instead of an array; both neighbours are read before the first decision, so the team takes them together
template <int N, class At>
__device__ __forceinline__ double quantile_at(At &&at, double p) {
  p = p > 0.0 ? (p < 1.0 ? p : 1.0) : 0.0;
  const double h = (double)(N - 1) * p;
  const bool last = !(h < (double)(N - 1));
  const int i = last ? N - 1 : (h > 0.0 ? (int)h : 0);
  const double a = at(i), b = at(i + 1 < N ? i + 1 : N - 1);
  const double g = h - (double)i;
  if (last || g == 0.0 || a == b) return a;
  const double d = b - a;
  return d - d == 0.0 ? a + g * d : (1.0 - g) * a + g * b;
}

// the team's butterflies over the lane distances 1, 2, 4, 8, in f64 whatever the element type: every lane ends with the same bits
template <int W>
__device__ __forceinline__ double team_add(double s) {
  s = s + Element<double>::xor_lane<1>(s);
  s = s + Element<double>::xor_lane<2>(s);
  if constexpr (W == 16) {
    s = s + Element<double>::xor_lane<4>(s);
    s = s + Element<double>::xor_lane<8>(s);
  }
  return s;
}
template <int W, bool MAX>
__device__ __forceinline__ double team_extreme(double s) {
  const auto pick = [](const double a, const double b) { return MAX ? sortnet::max_(a, b) : sortnet::min_(a, b); };
  s = pick(s, Element<double>::xor_lane<1>(s));
  s = pick(s, Element<double>::xor_lane<2>(s));
  if constexpr (W == 16) {
    s = pick(s, Element<double>::xor_lane<4>(s));
    s = pick(s, Element<double>::xor_lane<8>(s));
  }
  return s;
}
// the extreme of g(i, x[i]) over an array a lane holds whole
template <bool MAX, int N, class T, class G>
__device__ __forceinline__ double array_extreme(const T (&x)[N], G &&g) {
  double s = MAX ? -sortnet::inf_(0.0) : sortnet::inf_(0.0);
  for (int i = 0; i < N; ++i) s = MAX ? sortnet::max_(s, (double)g(i, x[i])) : sortnet::min_(s, (double)g(i, x[i]));
  return s;
}

// ---- spread over the team: T v[M] per lane, P = Element<T>::per_block normals to a block (v, sorted, fill_normals: Slots') ----
template <class T, int N, int W, bool SPREAD>
struct SampleStore : Element<T>::template Slots<N, W, slots(N, W, Element<T>::per_block)> {
  using E = Element<T>;
  static constexpr int P = E::per_block, M = slots(N, W, P);
  static_assert(W == 4 || W == 16, "a quad or a row of 16 lanes");
  static_assert(M >= P && M <= kSortUnrollMax, "whole blocks in a lane's registers");
  using Slots = typename E::template Slots<N, W, M>;
  using Slots::v;
  using Slots::sorted;

  static __device__ __forceinline__ int lane() { return team_lane<W>(); }
  __device__ __forceinline__ int element(const int q, const int r) const { return sorted ? q * M + r : draw_of(q, r, W, P); }

  template <class G>
  __device__ __forceinline__ void fill(G &&g) {
    const int q = lane();
#pragma unroll
    for (int r = 0; r < M; ++r) {
      const int i = draw_of(q, r, W, P);
      v[r] = E::inf();
      if (i < N) {
        const T x = g(i);
        v[r] = sortnet::min_(x, E::inf());
      }
    }
    sorted = false;
  }
  __device__ __forceinline__ void sort() {
    run_schedule_device<T, W, M>(v, lane(), typename sortnet::make_seq<step_count(W, M)>::type{});
    sorted = true;
  }
  __device__ __forceinline__ T drawn(const int i) const {
    return team_pick<W>(E::template select_slot<M>(v, draw_slot(i, W, P)), (uint32_t)draw_lane(i, W, P));
  }
  __device__ __forceinline__ T at(const int i) const {
    return team_pick<W>(E::template select_slot<M>(v, rank_slot(i, M)), (uint32_t)rank_lane(i, M));
  }
  __device__ __forceinline__ T order_statistic(const int rank) const {
    const T x = at(rank >= 1 && rank <= N ? rank - 1 : 0);             // (uniform over the team: every lane takes part)
    return rank >= 1 && rank <= N ? x : E::inf();
  }
  __device__ __forceinline__ double quantile(const double p) const {
    return quantile_at<N>([&](const int i) { return (double)at(i); }, p);
  }
  template <class G>
  __device__ __forceinline__ double sum(G &&g) const {
    const int q = lane();
    double t[M];
#pragma unroll
    for (int r = 0; r < M; ++r) {
      const int i = element(q, r);
      t[r] = i < N ? g(i, v[r]) : 0.0;
    }
    return reduce::finish_sum(team_add<W>(reduce::lane_tree(t)));
  }
  template <bool MAX, class G>
  __device__ __forceinline__ double extreme(G &&g) const {
    const int q = lane();
    double s = MAX ? -sortnet::inf_(0.0) : sortnet::inf_(0.0);
#pragma unroll
    for (int r = 0; r < M; ++r) {
      const int i = element(q, r);
      if (i < N) s = MAX ? sortnet::max_(s, (double)g(i, v[r])) : sortnet::min_(s, (double)g(i, v[r]));
    }
    return team_extreme<W, MAX>(s);
  }
  __device__ __forceinline__ void emit(NormalStream &rng, const long long first_output) const {
    if (!emitting(rng)) return;
    const int q = lane();
#pragma unroll
    for (int r = 0; r < M; ++r) {
      const int i = element(q, r);
      if (i < N) sabc::emit(rng, first_output + i, (double)v[r]);
    }
  }
};

// ---- replicated: a lane per particle, or a sample too long for the team's registers ----
template <class T, int N, int W>
struct SampleStore<T, N, W, false> {
  using E = Element<T>;
  static_assert(W == 1 || W == 4 || W == 16, "a lane, a quad or a row of 16 lanes");
  T x[N];

  template <class F>
  __device__ __forceinline__ void fill_normals(NormalStream &rng, F &&f) { E::fill_normals(rng, x, f); }
  template <class G>
  __device__ __forceinline__ void fill(G &&g) {
    for (int i = 0; i < N; ++i) x[i] = g(i);
  }
  __device__ __forceinline__ void sort() { sort_ascending(x); }          // (a NaN enters as +inf there)
  __device__ __forceinline__ T drawn(const int i) const { return x[i]; }
  __device__ __forceinline__ T at(const int i) const { return x[i]; }
  __device__ __forceinline__ T order_statistic(const int rank) const { return E::order_statistic(x, rank); }
  __device__ __forceinline__ double quantile(const double p) const { return E::quantile(x, p); }
  template <class G>
  __device__ __forceinline__ double sum(G &&g) const {
    return reduce::tree_sum_of(N, [&](const int i) { return (double)g(i, x[i]); });
  }
  template <bool MAX, class G>
  __device__ __forceinline__ double extreme(G &&g) const { return array_extreme<MAX>(x, g); }
  __device__ __forceinline__ void emit(NormalStream &rng, const long long first_output) const {
    if (!emitting(rng) || (threadIdx.x & (unsigned)(W - 1)) != 0) return;
    for (int i = 0; i < N; ++i) sabc::emit(rng, first_output + i, (double)x[i]);
  }
};

// max(g), min(g), sum(), mean() and moments(mean, var) of a container C of N elements that has sum(g) and extreme<MAX>(g)
// (Sample, SampleF32, Series): an element widens to double on its way in
template <class C, int N>
struct Summaries {
  __device__ __forceinline__ const C &self() const { return static_cast<const C &>(*this); }
  template <class G> __device__ __forceinline__ double max(G &&g) const { return self().template extreme<true>(g); }
  template <class G> __device__ __forceinline__ double min(G &&g) const { return self().template extreme<false>(g); }
  __device__ __forceinline__ double sum() const { return self().sum([](const int, const auto x) { return (double)x; }); }
  __device__ __forceinline__ double mean() const { return sum() / (double)N; }
  __device__ __forceinline__ void moments(double &mean_out, double &var_out) const {
    const double m = mean();
    mean_out = m;
    var_out = N > 1 ? self().sum([&](const int, const auto x) { return ((double)x - m) * ((double)x - m); }) / (double)(N > 1 ? N - 1 : 1)
                    : 0.0;
  }
};

// sabc::Sample and sabc::SampleF32: the store, the summaries and the distances to observed data (doubles, as every data segment)
template <class T, int N, int W>
struct SampleOf : SampleStore<T, N, W, spread(N, W, Element<T>::per_block)>, Summaries<SampleOf<T, N, W>, N> {
  static_assert(N >= 1, "a sample holds at least one value");
  static constexpr int size = N, lanes = W;
  static constexpr bool spread = teamsort::spread(N, W, Element<T>::per_block);
  using Store = SampleStore<T, N, W, spread>;
  using Store::sum;
  using Summaries<SampleOf, N>::sum;

  __device__ __forceinline__ double wasserstein1(const int seg = 0) const {
    return Store::sum([&](const int i, const T x) { return __builtin_fabs((double)x - data_at(i, seg)); }) / (double)N;
  }
  __device__ __forceinline__ double wasserstein2_squared(const int seg = 0) const {
    return Store::sum([&](const int i, const T x) { const double d = (double)x - data_at(i, seg); return d * d; }) / (double)N;
  }
  __device__ __forceinline__ double ks(const int seg = 0) const {
    const long long m = data_len(seg);
    const double top = Store::template extreme<true>([&](const int i, const T x) {
      return reduce::ks_term(i, N, m, count_less((double)x, seg), count_less_equal((double)x, seg));
    });
    return top / ((double)N * (double)m);
  }
};

}  // namespace teamsort

// One particle's sample of N doubles on the W = 1 | 4 | 16 lanes that run the particle (a simulator from source gets W as the
// template argument of sabc_user_simulate_team<W>).  fill_normals(rng, f): element i = f(normal i of the stream), ceil(N / 2)
// whole blocks consumed; fill(g): element i = g(i); drawn(i): element i before the sort; sort(): ascending, a NaN as +inf;
// at(i) (rank i, 0-based), order_statistic(rank) (1-based, +inf outside [1, N]), quantile(p) (type 7) after it;
// emit(rng, first_output): element r of the current order -- draw order before the sort, rank order after -- to output
// first_output + r, each value written once.
// Reductions, the same value on every lane of the team (sample_reduce.hpp: the canonical tree; i = the element's index in the
// current order, draw index before the sort, 0-based rank after it): sum(g), max(g), min(g) over g(i, value); sum(), mean();
// moments(mean, var): two passes, var = sum (x - mean)^2 / (N - 1), 0 for N = 1.  After sort() sum gives the same bits for every
// W; max and min always do.  Distances to an ascending observed sample in data segment seg, after sort():
// wasserstein1(seg) = sum_i |x_(i) - y_i| / N and wasserstein2_squared(seg) = sum_i (x_(i) - y_i)^2 / N (data_len(seg) == N: each
// lane reads its own M consecutive observations), ks(seg) the Kolmogorov-Smirnov distance for any data_len(seg) >= 1
// (N data_len(seg) < 2^53).
template <int N, int W>
using Sample = teamsort::SampleOf<double, N, W>;

}  // namespace sabc
#endif
