// sort_network.hpp -- order statistics for simulators from source: sabc::sort_ascending, sabc::order_statistic, sabc::quantile.
//
// A simulator is the body of a loop over particles that the lanes of a wave run side by side, so a sort inside it must be
// DATA-OBLIVIOUS: which elements are compared, and in which order, depends on the array's length alone.  Every lane then
// indexes its private array with the same index at the same time -- private memory is interleaved per lane, so such an access
// is one coalesced line per wave, and with compile-time indices the array needs no memory at all -- and no lane waits for
// another's data-dependent loop.  It also makes the result the same bits whichever kernel form runs the simulator (a lane, a
// quad or a row of 16 lanes per particle): a sorted array is unique.
//
// The network is Batcher's odd-even merge sort, written for the power of two P >= n with every comparator whose upper index
// is >= n left out.  All its comparators are ascending (the minimum goes to the lower index), so with +inf imagined behind the
// end such a comparator is a no-op, and a length that is no power of two needs no padding.  Comparators: n = 2: 1, 4: 5, 8: 19,
// 16: 63, 32: 191, 64: 543, 128: 1471 (a bitonic network of 32: 240, of 128: 1792); tests/sort_network/check_sort.cpp runs every
// 0-1 input for n <= 16, which by the 0-1 principle proves those sizes.
//
//   template <int N> sort_ascending(double (&x)[N])   N <= kSortUnrollMax = 32: the network as straight-line code with compile-time
//                                                     indices; an array the caller also indexes with constants never leaves
//                                                     the registers (2 N VGPRs), one that it indexes at run time is read
//                                                     once into registers and written back once.  N > 32: the loop form.
//   sort_ascending(double *x, int n)                  any n >= 0; loops whose bounds and indices depend on n alone.
//   float twins of both.
//
// A compare-exchange is one min and one max of the pair (v_min_f64 + v_max_f64), never a branch.  In the unrolled form the values
// stay in registers between comparators and only the first use of each pays the canonicalising v_max_f64 x, x that the compiler
// puts in front of a min/max of a value it knows nothing about (bitonic_step of device_models.hpp records that cost); in the loop
// form every comparator reads its pair from memory and pays it again -- two of its six VALU instructions, beside two loads and
// two stores.
//
// NaN: the policy of gk_datum (device_models.hpp).  A NaN enters as +inf, in ONE pass over the array before the network
// (x = min(x, +inf): minNum returns the operand that is a number): the reference's sort puts NaN last, where +inf ties with it.
// Inside a min/max network a NaN would duplicate one value and lose another.  So an input with k NaNs comes out with k more
// +inf at its end.  Signed zeros: -0.0 and +0.0 compare equal; they may come out in either order and with either sign.
//
// The same text compiles for the device (hipcc, hipRTC: namespace sabc of every simulator from source) and with a plain C++
// compiler for the host (the CPU proof): nothing here is a HIP builtin.
#pragma once

#if defined(__HIPCC__) || defined(__HIPCC_RTC__) || defined(__HIP__)
#define SABC_SORT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SABC_SORT_HD inline
#endif

namespace sabc {

constexpr int kSortUnrollMax = 32;                     // the largest N the template form unrolls (191 comparators, 64 VGPRs of f64)

namespace sortnet {

SABC_SORT_HD double min_(double a, double b) { return __builtin_fmin(a, b); }
SABC_SORT_HD double max_(double a, double b) { return __builtin_fmax(a, b); }
SABC_SORT_HD float min_(float a, float b) { return __builtin_fminf(a, b); }
SABC_SORT_HD float max_(float a, float b) { return __builtin_fmaxf(a, b); }
SABC_SORT_HD double inf_(double) { return __builtin_huge_val(); }
SABC_SORT_HD float inf_(float) { return __builtin_huge_valf(); }

template <class T>
SABC_SORT_HD void compare_exchange(T &a, T &b) {
  const T lo = min_(a, b), hi = max_(a, b);
  a = lo;
  b = hi;
}

// The comparators of the network for n elements in the order they are applied: merges of runs of p = 1, 2, 4, ... elements,
// each in steps of distance k = p, p/2, ..., 1.  visit(lo, hi) with lo < hi < n.  The one enumeration both forms use: the loop
// form calls it with the exchange itself, the unrolled form at compile time to write the comparators down.
// (Kept loops on the device even where n is a constant -- the template form above kSortUnrollMax: unrolled by the compiler, 128
// elements are 1471 comparators of straight-line code in each of a unit's sixteen kernels.  2 p = 2^s: the run an element lies
// in is a shift, not a division.)
#if defined(__clang__)
#define SABC_SORT_LOOP _Pragma("nounroll")
#else
#define SABC_SORT_LOOP
#endif
template <class F>
constexpr SABC_SORT_HD void for_each_comparator(const int n, F &&visit) {
  SABC_SORT_LOOP
  for (int p = 1, s = 1; p < n; p <<= 1, ++s) {
    SABC_SORT_LOOP
    for (int k = p; k >= 1; k >>= 1) {
      SABC_SORT_LOOP
      for (int j = k & (p - 1); j + k < n; j += 2 * k) {
        SABC_SORT_LOOP
        for (int i = 0; i < k && i + j + k < n; ++i)
          if (((i + j) >> s) == ((i + j + k) >> s)) visit(i + j, i + j + k);
      }
    }
  }
}

struct Count {
  int n = 0;
  constexpr void operator()(int, int) { ++n; }
};
constexpr int comparators(const int n) {
  Count c;
  for_each_comparator(n, c);
  return c.n;
}

template <int M>
struct Table {
  int lo[M + 1] = {}, hi[M + 1] = {};
  int at = 0;
  constexpr void operator()(int a, int b) { lo[at] = a; hi[at] = b; ++at; }
};
template <int N>
constexpr Table<comparators(N)> table() {
  Table<comparators(N)> t;
  for_each_comparator(N, t);
  return t;
}
template <int N>
struct Network {
  static constexpr int count = comparators(N);
  static constexpr Table<count> value = table<N>();
};

template <int... I> struct seq {};
template <int M, int... I> struct make_seq : make_seq<M - 1, M - 1, I...> {};
template <int... I> struct make_seq<0, I...> { using type = seq<I...>; };

template <int N, int I, class T>
SABC_SORT_HD void step(T (&x)[N]) {
  constexpr int lo = Network<N>::value.lo[I], hi = Network<N>::value.hi[I];
  static_assert(0 <= lo && lo < hi && hi < N, "a comparator of the network");
  compare_exchange(x[lo], x[hi]);
}
template <int N, class T, int... I>
SABC_SORT_HD void unrolled(T (&x)[N], seq<I...>) {
  (step<N, I>(x), ...);
}

template <class T>
struct Exchange {
  T *x;
  SABC_SORT_HD void operator()(int lo, int hi) { compare_exchange(x[lo], x[hi]); }
};

template <class T>
SABC_SORT_HD void sort_loop(T *x, const int n) {
  for (int i = 0; i < n; ++i) x[i] = min_(x[i], inf_(T()));      // NaN -> +inf
  Exchange<T> e{x};
  for_each_comparator(n, e);
}

template <int N, class T>
SABC_SORT_HD void sort_array(T (&x)[N]) {
  if constexpr (N > kSortUnrollMax) {
    sort_loop(&x[0], N);
  } else {
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < N; ++i) x[i] = min_(x[i], inf_(T()));    // NaN -> +inf
    unrolled(x, typename make_seq<Network<N>::count>::type{});
  }
}

}  // namespace sortnet

template <int N> SABC_SORT_HD void sort_ascending(double (&x)[N]) { sortnet::sort_array(x); }
template <int N> SABC_SORT_HD void sort_ascending(float (&x)[N]) { sortnet::sort_array(x); }
SABC_SORT_HD void sort_ascending(double *x, int n) { sortnet::sort_loop(x, n); }
SABC_SORT_HD void sort_ascending(float *x, int n) { sortnet::sort_loop(x, n); }

// x_(rank) of an ascending array, rank 1-based as the built-in g-and-k model counts; +inf for a rank outside [1, n]
SABC_SORT_HD double order_statistic(const double *sorted, int n, int rank) {
  return rank >= 1 && rank <= n ? sorted[rank - 1] : __builtin_huge_val();
}

// The p-quantile of an ascending array by Julia's default definition (type 7; NumPy's "linear"): h = (n - 1) p, i = floor(h),
// sorted[i] + (h - i) (sorted[i + 1] - sorted[i]); p clamped to [0, 1] (a NaN p: 0); n = 1: the single value; n < 1: +inf.
// Where the difference of the neighbours is not finite (an infinite one, or an overflow) the weighted mean
// (1 - g) a + g b stands in, and a zero weight never multiplies an infinity: the quantile of data holding +inf is +inf from
// the first interval that touches one, never NaN.
SABC_SORT_HD double quantile(const double *sorted, int n, double p) {
  if (n < 1) return __builtin_huge_val();
  p = p > 0.0 ? (p < 1.0 ? p : 1.0) : 0.0;
  const double h = (double)(n - 1) * p;
  if (!(h < (double)(n - 1))) return sorted[n - 1];
  const int i = h > 0.0 ? (int)h : 0;                  // 0 <= h < n - 1: the truncation is the floor
  const double g = h - (double)i, a = sorted[i], b = sorted[i + 1];
  if (g == 0.0 || a == b) return a;
  const double d = b - a;
  return d - d == 0.0 ? a + g * d : (1.0 - g) * a + g * b;
}

}  // namespace sabc

#include "sample_reduce.hpp"   // sabc::tree_sum, count_less, count_less_equal: what a sorted sample is summed and compared with
