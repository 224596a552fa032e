// team_sample_f32.hpp -- sabc::SampleF32<N, W>: one particle's sample of N binary32 values, drawn four to a Philox block and sorted
// by the W lanes that run the particle.  The float twin of sabc::Sample<N, W>: team_sample.hpp has the scheme and the one text of
// layout, executor, store, summaries and distances; this header has teamsort::Element<float>, WHAT DIFFERS:
//
//   Layout.  The normals come in blocks of FOUR (NormalStream::quad_f32) and a lane keeps all four normals of the blocks it
//   generates: M = pow2ceil(4 ceil(ceil(N / 4) / W)) slots per lane, M <= kSortUnrollMax = 32, i.e. N <= 32 W as for doubles.  Draw
//   i is normal i & 3 of block b = i >> 2 and lies on lane b mod W -- the assignment of NormalStream::for_team<float, W> / tail --
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
//   Read-outs return float (drawn, at, order_statistic: a select over the slots, then team_pick -- no indexed access, the
//   slots stay registers); quantile(p) returns double, teamsort::quantile_at over the values widened to double (exact), the type-7
//   arithmetic of the f64 form; emit writes (double)value.
//
//   Reductions accumulate in f64: g(i, value) takes the float and returns double, a lane adds the tree of its M terms, the team
//   follows with the f64 butterfly (teamsort::team_add) -- after sort() the canonical tree over the rank, the same bits for
//   W = 1, 4 and 16, for the replicated store and for NumPy applied to the emitted (widened) sample.  ks counts (double)value in
//   the data segment, which stays double, as every data segment.
//
// tests/team_sample_f32/check_team_sample_f32.cpp checks the layout with four normals to a block, and a plain-C++ model of the
// float executor against teamsort::run_schedule.
#pragma once
#include "team_sample.hpp"

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
// ---- the device's half: included from the end of device_rng.hpp, behind team_sample.hpp ----
namespace sabc {
namespace teamsort {

template <>
struct Element<float> {
  static constexpr int per_block = 4;
  static __device__ __forceinline__ float inf() { return sortnet::inf_(0.0f); }
  template <int N, int W, int M>
  struct Slots {
    float v[M];
    bool sorted;
    template <class F>
    __device__ __forceinline__ void fill_normals(NormalStream &rng, F &&f) {
      const int q = team_lane<W>();
#pragma unroll
      for (int a = 0; a < M / 4; ++a) {
        if (a * W < blocks(N, 4)) {                      // (a constant: some lane of the team has a block a)
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
      rng.k += (uint32_t)blocks(N, 4);
      sorted = false;
    }
  };

  // one instruction per value
  template <int DIST>
  static __device__ __forceinline__ float xor_lane(const float v) {
    static_assert(DIST == 1 || DIST == 2 || DIST == 4 || DIST == 8, "a lane of the own row of 16");
    const int x = __float_as_int(v);
    if constexpr (DIST == 1) return __int_as_float(__builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, true));         // quad_perm [1,0,3,2]
    else if constexpr (DIST == 2) return __int_as_float(__builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    else if constexpr (DIST == 8) return __int_as_float(__builtin_amdgcn_mov_dpp(x, 0x128, 0xF, 0xF, true));   // row_ror:8
    else return __int_as_float(__builtin_amdgcn_ds_swizzle(x, 0x1F | (DIST << 10)));                          // and 0x1f, or 0, xor 4
  }
  static __device__ __forceinline__ float vmin(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
  static __device__ __forceinline__ float vmax(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
  static __device__ __forceinline__ float vmin_neg(float a, float b) { float r; asm("v_min_f32 %0, %1, -%2" : "=v"(r) : "v"(a), "v"(b)); return r; }
  static __device__ __forceinline__ float flip_sign(const float v, const int flip) { return __int_as_float(__float_as_int(v) ^ flip); }

  // a select per slot on the words, from a constant over every slot: started from v[0] as Element<double>'s, which selects 32-bit
  // halves, it is turned into a load from a selected address and leaves the slots in scratch
  template <int M>
  static __device__ __forceinline__ float select_slot(const float (&v)[M], const int slot) {
    int x = 0;
#pragma unroll
    for (int r = 0; r < M; ++r) x = slot == r ? __float_as_int(v[r]) : x;
    return __int_as_float(x);
  }

  template <int N, class F>
  static __device__ __forceinline__ void fill_normals(NormalStream &rng, float (&x)[N], F &&f) {
    int at_ = 0;
    rng.for_quads_f32(blocks(N, 4), [&](const float z0, const float z1, const float z2, const float z3) {
      const float z[4] = {z0, z1, z2, z3};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (at_ + j < N) x[at_ + j] = f(z[j]);
      at_ += 4;
    });
  }
  template <int N>
  static __device__ __forceinline__ float order_statistic(const float (&x)[N], const int rank) {
    return rank >= 1 && rank <= N ? x[rank - 1] : inf();
  }
  template <int N>
  static __device__ __forceinline__ double quantile(const float (&x)[N], const double p) {
    return quantile_at<N>([&](const int i) { return (double)x[i]; }, p);
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
using SampleF32 = teamsort::SampleOf<float, N, W>;

}  // namespace sabc
#endif
