// sample_reduce.hpp -- sums, extrema and two-sample distances for simulators from source: sabc::tree_sum, sabc::count_less,
// sabc::count_less_equal, and the definitions sabc::Sample<N, W>::sum / max / min / moments / wasserstein1 / ks are held to.
//
// THE CANONICAL SUM of s_0 .. s_{n-1} is the balanced binary tree over the element index, low bits first: s_{2i} + s_{2i+1},
// then neighbouring results, and so on, the sequence padded with +0.0 to a power of two; and, last, + 0.0 once.  t + 0.0 == t,
// so how far the padding reaches does not matter to the value -- but (-0.0) + 0.0 is +0.0, and the closing + 0.0 makes that
// hold for the bits too: a sum that is a zero is +0.0 whichever form computed it, with padding or without.  Every form below
// -- the stack of partial sums a lane runs alone (tree_sum), the partial tree of a lane's slots followed by the butterfly over
// the team's lanes (team_sample.hpp: SampleStore::sum), the NumPy restatement of the tests (pad, reshape(-1, 2), add) -- gives
// these bits whenever element i sits at position i: after Sample::sort(), for every team width.  Before the sort a team holds
// its sample in the layout of the draws, which depends on the width, and the sum is a tree over THAT order: the same value up
// to rounding, |sum - exact| <= n 2^-53 sum |s_i| (the bound of any order of summation), not the same bits.
// Rounding of the tree itself: log2(n) additions deep, so |sum - exact| <= ceil(log2 n) 2^-53 sum |s_i| to first order.
//
// tree_sum keeps one partial sum per set bit of the count of elements seen so far -- a sum of 2^a elements waits until its
// right-hand neighbour of 2^a elements is complete --: no copy of the sequence, kTreeLevels entries, n < 2^31.  (A source's
// g(i) that is a product contracts into the addition under -ffp-contract=fast where the compiler sees both: sums of products
// are held to a tolerance, sums of differences and absolute values to bits.)
//
// COUNTS in an ascending sequence y_0 <= .. <= y_{m-1}: count_less(v) = #{j: y_j < v}, count_less_equal(v) = #{j: y_j <= v} by a
// binary search without a branch on the data: the trip count depends on m alone (uniform over the wave where m is), v may
// differ per lane, a NaN v counts as +inf (the policy of the sort: a NaN enters as +inf), m = 0 gives 0.
//
// KOLMOGOROV-SMIRNOV between a sorted sample x_(0) <= .. <= x_(n-1) and y: D = sup_t |F_x(t) - F_y(t)|.  Between two points of
// x, F_x is constant and F_y monotone, so the supremum is reached at a point of x, from the right or from the left:
//   D = max_i max(|(i + 1) m - c<=(x_(i)) n|, |i m - c<(x_(i)) n|) / (n m)
// (ks_term: the numerator of element i, exact integers; one maximum over i; one division).  (i + 1) / n and i / n ARE F_x at
// x_(i) and just below it where the values of x are distinct -- a simulated sample of continuous draws --; ties within y and
// between x and y are covered by the two counts (tests/sample_reduce/check_reduce.cpp: equal to the supremum over all pooled
// points).  Within a run of r equal values of x -- duplicates planted through fill(g), several NaN draws that entered as +inf
// -- the inner members pair a level of F_x inside its jump with F_y beside it: the result is never below D and at most
// (r - 1) / n above it.  Supported: n m < 2^53, where the integers are exact as doubles.
//
// The same text compiles for the device and with a plain C++ compiler (the CPU proof); the part at the end that reads a data
// segment (sabc::data_at, sabc::data_len: what every source-compiled unit sees) is the device's.
#pragma once
#include "sort_network.hpp"

namespace sabc {
namespace reduce {

constexpr int kTreeLevels = 32;

SABC_SORT_HD double finish_sum(const double t) { return t + 0.0; }

// the canonical sum of g(0) .. g(n - 1)
template <class G>
SABC_SORT_HD double tree_sum_of(const int n, G &&g) {
  double part[kTreeLevels];
  int top = 0;
  for (int i = 0; i < n; ++i) {
    double t = g(i);
    for (unsigned c = (unsigned)i; c & 1u; c >>= 1) t = part[--top] + t;       // i ends in a ones: a left neighbours are complete
    part[top++] = t;
  }
  if (top == 0) return 0.0;
  double t = part[--top];                              // the padding: t + 0.0 up to the size of the next partial sum
  while (top > 0) t = part[--top] + t;
  return finish_sum(t);
}

// the tree over the M = 2^a values of an array, in place, every index a compile-time constant (a lane's slots: registers);
// the result is t[0]
template <int M>
SABC_SORT_HD double lane_tree(double (&t)[M]) {
  static_assert(M >= 1 && (M & (M - 1)) == 0, "a power of two");
#if defined(__clang__)
#pragma unroll
#endif
  for (int d = 1; d < M; d <<= 1) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int r = 0; r < M; r += 2 * d) t[r] = t[r] + t[r + d];
  }
  return t[0];
}

// #{j < m: at(j) < v} (or_equal: <= v) in an ascending sequence
template <bool OR_EQUAL, class At>
SABC_SORT_HD long long count_below(double v, const long long m, At &&at) {
  if (m <= 0) return 0;
  v = sortnet::min_(v, sortnet::inf_(0.0));            // NaN -> +inf
  long long base = 0;
  for (long long len = m; len > 1;) {                  // the answer lies in [base, base + len]
    const long long half = len >> 1;
    const double y = at(base + half - 1);
    base += (OR_EQUAL ? y <= v : y < v) ? half : 0;
    len -= half;
  }
  const double y = at(base);
  return base + ((OR_EQUAL ? y <= v : y < v) ? 1 : 0);
}

// the numerator of element i (0-based rank) in the Kolmogorov-Smirnov distance above, >= 0 and exact for n m < 2^53
SABC_SORT_HD double ks_term(const long long i, const long long n, const long long m, const long long c_less, const long long c_less_equal) {
  const long long right = (i + 1) * m - c_less_equal * n, left = i * m - c_less * n;
  const long long a = right < 0 ? -right : right, b = left < 0 ? -left : left;
  return (double)(a > b ? a : b);
}

}  // namespace reduce

// The array twins of Sample::sum for a source that holds its sample whole: the canonical sum of x[0..n) and of g(0) .. g(n - 1)
// (n >= 0; 0 elements: +0.0) -- the bits Sample<N, W>::sum gives after sort() for every W.
SABC_SORT_HD double tree_sum(const double *x, const int n) {
  return reduce::tree_sum_of(n, [&](const int i) { return x[i]; });
}
template <class G>
SABC_SORT_HD double tree_sum(const int n, G &&g) { return reduce::tree_sum_of(n, g); }

}  // namespace sabc

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
namespace sabc {
// what a source-compiled unit defines ahead of the user's text (rtc.cpp: the observed data of the handle)
__device__ long long data_len(int segment);
__device__ double data_at(long long i, int segment);

// counts in data segment `segment`, which must be ascending (the model class checks that; no index is checked here)
__device__ inline __attribute__((always_inline)) long long count_less(const double v, const int segment = 0) {
  return reduce::count_below<false>(v, data_len(segment), [&](const long long j) { return data_at(j, segment); });
}
__device__ inline __attribute__((always_inline)) long long count_less_equal(const double v, const int segment = 0) {
  return reduce::count_below<true>(v, data_len(segment), [&](const long long j) { return data_at(j, segment); });
}
}  // namespace sabc
#endif
