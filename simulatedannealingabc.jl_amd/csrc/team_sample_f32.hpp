// team_sample_f32.hpp -- sabc::SampleF32<N, W>: one particle's sample of N binary32 values, drawn four to a Philox block and sorted
// by the W lanes that run the particle.  The float twin of sabc::Sample<N, W> (team_sample.hpp), a type of its own: Sample's text
// and instructions stay what they are.
//
// What is shared with Sample, unchanged: THE SCHEDULE (teamsort::step_at, sign_mask, descending_slot_bit: it depends on (W, M)
// alone), the signed-value scheme of a cross-lane step, the rule that all lanes of a team make the same calls in the same order,
// and the reductions' definition (sample_reduce.hpp: reduce::lane_tree, the f64 butterfly, finish_sum).  What differs:
//
//   Layout.  The normals come in blocks of FOUR (NormalStream::quad_f32) and a lane keeps all four normals of the blocks it
//   generates: M = pow2ceil(4 ceil(ceil(N / 4) / W)) slots per lane, M <= kSortUnrollMax = 32, i.e. N <= 32 W as for doubles.  Draw
//   i is normal i & 3 of block b = i >> 2 and lies on lane b mod W -- the assignment of NormalStream::for_quads_team / tail_f32 --
//   in slot 4 (b / W) + (i & 3); after the sort rank i lies on lane i / M in slot i mod M.  Pad slots hold +inf.
//   W = 1, or M > 32: the REPLICATED form, float x[N] filled through rng.for_quads_f32 and sorted by sabc::sort_ascending.
//   Either way fill_normals consumes the ceil(N / 4) whole blocks rng.for_quads_f32(ceil(N / 4), ..) would, in that order.
//
//   A slot is ONE register, and a cross-lane exchange moves one word: per element a DPP move (lane distance 1, 2: quad_perm;
//   8: row_ror:8, which is lane ^ 8 within a row of 16) or a ds_swizzle (4: one instruction where DPP needs two bank-masked
//   rotations), then ONE v_min_f32 against the negated partner.  In-lane steps are a v_min_f32 and a v_max_f32, the sign flip
//   where the mask changes one v_xor_b32 per element.  No LDS memory, no barrier, no atomic.
//   The min is inline asm beside a DPP move the compiler emits (two VALU instructions per element at distance 1 and 2), NOT a
//   v_min_f32 with a DPP operand (one): __builtin_fminf of a value that came through a DPP builtin -- the int form behind
//   bitcasts, the float overload, the negation in front of or behind the move -- is preceded by a canonicalising v_max_f32 -p, -p
//   (three per element), and with that instruction between the move and the min the DPP combine has nothing to fold; the
//   compiler takes no per-function promise that a value is no signalling NaN (#pragma float_control is refused for this target).
//   A DPP instruction written in asm is not an option: the compiler does not cover the write-then-DPP-read wait states of an asm
//   text.  (DESIGN.md section 3 has the counts.)
//
//   Values are never NaN inside the network: a NaN enters as +inf at fill time, min(x, +inf), Sample's policy.
//
//   Read-outs return float (drawn, at, order_statistic: a select over the slots, then team_pick_f32 -- no indexed access, the
//   slots stay registers); quantile(p) returns double, teamsort::quantile_at over the values widened to double (exact), the type-7
//   arithmetic of the f64 form; emit writes (double)value.
//
//   Reductions accumulate in f64: g(i, value) takes the float and returns double, a lane adds the tree of its M terms, the team
//   follows with Sample's butterfly (xor_lane and v_add_f64) -- after sort() the canonical tree over the rank, the same bits for
//   W = 1, 4 and 16, for the replicated store and for NumPy applied to the emitted (widened) sample.  ks counts (double)value in
//   the data segment, which stays double, as every data segment.
//
// The layout functions are constexpr and compile with a plain C++ compiler; tests/team_sample_f32/check_team_sample_f32.cpp
// checks them, and a plain-C++ model of the float executor against teamsort::run_schedule.
#pragma once
#include "team_sample.hpp"

namespace sabc {
namespace teamsort {

constexpr int blocks_f32(int n) { return (n + 3) / 4; }                                          // whole Philox blocks of n binary32 normals
constexpr int slots_f32(int n, int w) { return pow2ceil(4 * ((blocks_f32(n) + w - 1) / w)); }    // M
constexpr bool spread_f32(int n, int w) { return w > 1 && slots_f32(n, w) <= kSortUnrollMax; }

// where draw i lies before the sort (after it: rank_lane, rank_slot of team_sample.hpp)
constexpr int draw_lane_f32(int i, int w) { return (i >> 2) & (w - 1); }
constexpr int draw_slot_f32(int i, int w) { return 4 * ((i >> 2) / w) + (i & 3); }
constexpr int draw_of_f32(int lane, int slot, int w) { return 4 * (lane + w * (slot >> 2)) + (slot & 3); }

}  // namespace teamsort
}  // namespace sabc

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
// ---- the device's half: included from the end of device_rng.hpp, behind team_sample.hpp ----
namespace sabc {
namespace teamsort {

// v from lane ^ DIST of the row: one instruction per value
template <int DIST>
__device__ __forceinline__ float xor_lane_f32(const float v) {
  static_assert(DIST == 1 || DIST == 2 || DIST == 4 || DIST == 8, "a lane of the own row of 16");
  const int x = __float_as_int(v);
  if constexpr (DIST == 1) return __int_as_float(__builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, true));         // quad_perm [1,0,3,2]
  else if constexpr (DIST == 2) return __int_as_float(__builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
  else if constexpr (DIST == 8) return __int_as_float(__builtin_amdgcn_mov_dpp(x, 0x128, 0xF, 0xF, true));   // row_ror:8
  else return __int_as_float(__builtin_amdgcn_ds_swizzle(x, 0x1F | (DIST << 10)));                          // and 0x1f, or 0, xor 4
}
__device__ __forceinline__ float vmin_f32(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmax_f32(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmin_neg_f32(float a, float b) { float r; asm("v_min_f32 %0, %1, -%2" : "=v"(r) : "v"(a), "v"(b)); return r; }

template <int W, int M, int I>
__device__ __forceinline__ void run_step_device(float (&v)[M], const int q) {
  constexpr Step s = step_at(W, M, I);
  constexpr int mask = sign_mask(s, W, M), before = I > 0 ? sign_mask(step_at(W, M, I > 0 ? I - 1 : 0), W, M) : 0;
  if constexpr (mask != before) {
    const int flip = (__builtin_popcount(q & (mask ^ before)) & 1) << 31;
#pragma unroll
    for (int r = 0; r < M; ++r) v[r] = __int_as_float(__float_as_int(v[r]) ^ flip);
  }
  if constexpr (s.cross) {
    float p[M];
#pragma unroll
    for (int r = 0; r < M; ++r) p[r] = xor_lane_f32<s.dist>(v[r]);
#pragma unroll
    for (int r = 0; r < M; ++r) v[r] = vmin_neg_f32(v[r], p[r]);
  } else {
    constexpr int desc = descending_slot_bit(s, M);
#pragma unroll
    for (int r = 0; r < M; ++r) {
      if (r & s.dist) continue;
      const float lo = vmin_f32(v[r], v[r | s.dist]), hi = vmax_f32(v[r], v[r | s.dist]);
      v[r] = (r & desc) ? hi : lo;
      v[r | s.dist] = (r & desc) ? lo : hi;
    }
  }
}
template <int W, int M, int... I>
__device__ __forceinline__ void run_schedule_device(float (&v)[M], const int q, sortnet::seq<I...>) {
  (run_step_device<W, M, I>(v, q), ...);
  static_assert(sign_mask(step_at(W, M, step_count(W, M) - 1), W, M) == 0, "the last step leaves the values themselves");
}

// slot `slot` of v, the slot known at run time: a select per slot on the words, no indexed access (select_slot of team_sample.hpp)
template <int M>
__device__ __forceinline__ float select_slot_f32(const float (&v)[M], const int slot) {
  int x = 0;
#pragma unroll
  for (int r = 0; r < M; ++r) x = slot == r ? __float_as_int(v[r]) : x;
  return __int_as_float(x);
}

// ---- spread over the team ----
template <int N, int W, bool SPREAD>
struct SampleStoreF32 {
  static constexpr int M = slots_f32(N, W);
  static_assert(W == 4 || W == 16, "a quad or a row of 16 lanes");
  static_assert(M >= 4 && M <= kSortUnrollMax, "whole blocks of four in a lane's registers");
  using Butterfly = SampleStore<1, W, true>;           // team_add: Sample's f64 butterfly, a static member that does not depend on N
  float v[M];
  bool sorted;

  static __device__ __forceinline__ int lane() { return (int)(threadIdx.x & (unsigned)(W - 1)); }
  __device__ __forceinline__ int element(const int q, const int r) const { return sorted ? q * M + r : draw_of_f32(q, r, W); }

  template <class F>
  __device__ __forceinline__ void fill_normals(NormalStream &rng, F &&f) {
    const int q = lane();
#pragma unroll
    for (int a = 0; a < M / 4; ++a) {
      if (a * W < blocks_f32(N)) {                       // (a constant: some lane of the team has a block a)
        float z[4];
        f32::box_muller_quad(stream_block(rng.seed, rng.pid, rng.purpose, rng.iter, rng.k + (uint32_t)(a * W + q)), z[0], z[1], z[2], z[3]);
        const int i = 4 * (a * W + q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float x = f(z[j]);
          v[4 * a + j] = i + j < N ? sortnet::min_(x, sortnet::inf_(0.0f)) : sortnet::inf_(0.0f);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * a + j] = sortnet::inf_(0.0f);
      }
    }
    rng.k += (uint32_t)blocks_f32(N);
    sorted = false;
  }
  template <class G>
  __device__ __forceinline__ void fill(G &&g) {
    const int q = lane();
#pragma unroll
    for (int r = 0; r < M; ++r) {
      const int i = draw_of_f32(q, r, W);
      v[r] = sortnet::inf_(0.0f);
      if (i < N) {
        const float x = g(i);
        v[r] = sortnet::min_(x, sortnet::inf_(0.0f));
      }
    }
    sorted = false;
  }
  __device__ __forceinline__ void sort() {
    run_schedule_device<W, M>(v, lane(), typename sortnet::make_seq<step_count(W, M)>::type{});
    sorted = true;
  }
  __device__ __forceinline__ float drawn(const int i) const {
    return team_pick_f32<W>(select_slot_f32<M>(v, draw_slot_f32(i, W)), (uint32_t)draw_lane_f32(i, W));
  }
  __device__ __forceinline__ float at(const int i) const {
    return team_pick_f32<W>(select_slot_f32<M>(v, rank_slot(i, M)), (uint32_t)rank_lane(i, M));
  }
  __device__ __forceinline__ float order_statistic(const int rank) const {
    const float x = at(rank >= 1 && rank <= N ? rank - 1 : 0);         // (uniform over the team: every lane takes part)
    return rank >= 1 && rank <= N ? x : sortnet::inf_(0.0f);
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
    return reduce::finish_sum(Butterfly::team_add(reduce::lane_tree(t)));
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
    return Butterfly::template team_extreme<MAX>(s);
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
template <int N, int W>
struct SampleStoreF32<N, W, false> {
  static_assert(W == 1 || W == 4 || W == 16, "a lane, a quad or a row of 16 lanes");
  float x[N];

  template <class F>
  __device__ __forceinline__ void fill_normals(NormalStream &rng, F &&f) {
    int at_ = 0;
    rng.for_quads_f32(blocks_f32(N), [&](const float z0, const float z1, const float z2, const float z3) {
      const float z[4] = {z0, z1, z2, z3};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (at_ + j < N) x[at_ + j] = f(z[j]);
      at_ += 4;
    });
  }
  template <class G>
  __device__ __forceinline__ void fill(G &&g) {
    for (int i = 0; i < N; ++i) x[i] = g(i);
  }
  __device__ __forceinline__ void sort() { sort_ascending(x); }          // (a NaN enters as +inf there)
  __device__ __forceinline__ float drawn(const int i) const { return x[i]; }
  __device__ __forceinline__ float at(const int i) const { return x[i]; }
  __device__ __forceinline__ float order_statistic(const int rank) const { return rank >= 1 && rank <= N ? x[rank - 1] : sortnet::inf_(0.0f); }
  __device__ __forceinline__ double quantile(const double p) const {
    return quantile_at<N>([&](const int i) { return (double)x[i]; }, p);
  }
  template <class G>
  __device__ __forceinline__ double sum(G &&g) const {
    return reduce::tree_sum_of(N, [&](const int i) { return (double)g(i, x[i]); });
  }
  template <bool MAX, class G>
  __device__ __forceinline__ double extreme(G &&g) const {
    double s = MAX ? -sortnet::inf_(0.0) : sortnet::inf_(0.0);
    for (int i = 0; i < N; ++i) s = MAX ? sortnet::max_(s, (double)g(i, x[i])) : sortnet::min_(s, (double)g(i, x[i]));
    return s;
  }
  __device__ __forceinline__ void emit(NormalStream &rng, const long long first_output) const {
    if (!emitting(rng) || (threadIdx.x & (unsigned)(W - 1)) != 0) return;
    for (int i = 0; i < N; ++i) sabc::emit(rng, first_output + i, (double)x[i]);
  }
};

}  // namespace teamsort

// One particle's sample of N binary32 values on the W = 1 | 4 | 16 lanes that run the particle: Sample<N, W> with a register per
// slot and four normals per Philox block.  fill_normals(rng, f): element i = f(normal i of the stream's binary32 draws), f(float) ->
// float, the ceil(N / 4) whole blocks of rng.for_quads_f32(ceil(N / 4), ..) consumed in that order; fill(g): element i = g(i), a
// float; drawn(i): element i before the sort; sort(): ascending, a NaN as +inf; at(i) (rank i, 0-based), order_statistic(rank)
// (1-based, +inf outside [1, N]) return float, quantile(p) (type 7, on the values widened to double) returns double;
// emit(rng, first_output): (double)element r of the current order to output first_output + r, each value written once.
// Reductions accumulate in double and give the same value on every lane of the team (sample_reduce.hpp: the canonical tree; i =
// the element's index in the current order): sum(g), max(g), min(g) over g(i, value) with value a float and the result a double;
// sum(), mean(); moments(mean, var): two passes, var = sum (x - mean)^2 / (N - 1), 0 for N = 1.  After sort() sum gives the same
// bits for every W -- those of Sample's sum over the widened values --; max and min always do.  Distances to an ascending
// observed sample in data segment seg (doubles, as every data segment), after sort(): wasserstein1(seg), wasserstein2_squared(seg)
// (data_len(seg) == N) and ks(seg) (any data_len(seg) >= 1, N data_len(seg) < 2^53), as Sample's.
template <int N, int W>
struct SampleF32 : teamsort::SampleStoreF32<N, W, teamsort::spread_f32(N, W)> {
  static_assert(N >= 1, "a sample holds at least one value");
  static constexpr int size = N, lanes = W;
  static constexpr bool spread = teamsort::spread_f32(N, W);
  using Store = teamsort::SampleStoreF32<N, W, teamsort::spread_f32(N, W)>;
  using Store::sum;

  template <class G> __device__ __forceinline__ double max(G &&g) const { return Store::template extreme<true>(g); }
  template <class G> __device__ __forceinline__ double min(G &&g) const { return Store::template extreme<false>(g); }
  __device__ __forceinline__ double sum() const { return Store::sum([](const int, const float x) { return (double)x; }); }
  __device__ __forceinline__ double mean() const { return sum() / (double)N; }
  __device__ __forceinline__ void moments(double &mean_out, double &var_out) const {
    const double m = mean();
    mean_out = m;
    var_out = N > 1 ? Store::sum([&](const int, const float x) { return ((double)x - m) * ((double)x - m); }) / (double)(N > 1 ? N - 1 : 1) : 0.0;
  }
  __device__ __forceinline__ double wasserstein1(const int seg = 0) const {
    return Store::sum([&](const int i, const float x) { return __builtin_fabs((double)x - data_at(i, seg)); }) / (double)N;
  }
  __device__ __forceinline__ double wasserstein2_squared(const int seg = 0) const {
    return Store::sum([&](const int i, const float x) { const double d = (double)x - data_at(i, seg); return d * d; }) / (double)N;
  }
  __device__ __forceinline__ double ks(const int seg = 0) const {
    const long long m = data_len(seg);
    const double top = Store::template extreme<true>([&](const int i, const float x) {
      return reduce::ks_term(i, N, m, count_less((double)x, seg), count_less_equal((double)x, seg));
    });
    return top / ((double)N * (double)m);
  }
};

}  // namespace sabc
#endif
