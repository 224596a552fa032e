// sabc::Series<128, W> on its own, for tests/test_team_series_isa.py: a team of W lanes fills the series from a counter that is a
// kernel argument (nothing folds away), forms the MA(2) series from lag<1> and lag<2> with two zips, takes the autocovariances at
// lags 0, 1 and 2 and reads ONE element whose time is a kernel argument -- an index the compiler cannot know.  The slots must
// not leave the registers: no indexed access, a select over the slots instead.
#include "device_rng.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

template <int W>
__device__ __forceinline__ void probe(const uint64_t counter, const double t1, const double t2, const int when, const int64_t teams,
                                      double *__restrict__ out) {
  const int64_t team = ((int64_t)blockIdx.x * 256 + threadIdx.x) / W;
  if (team >= teams) return;                           // (uniform over a team)
  sabc::Series<128, W> e;
  e.fill([&](const int t) {
    const uint64_t c = (counter + (uint64_t)team * 128u + (uint64_t)t) * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(c >> 11);
  });
  sabc::Series<128, W> y = e;
  y.zip(e.template lag<1>(), [&](const int, const double a, const double b) { return fma(t1, b, a); });
  y.zip(e.template lag<2>(), [&](const int, const double a, const double b) { return fma(t2, b, a); });
  const double a0 = y.template autocovariance<0>(0.0, 2), a1 = y.template autocovariance<1>(0.0, 2), a2 = y.template autocovariance<2>(0.0, 2);
  const double picked = y.at(when);
  if ((threadIdx.x & (W - 1)) == 0) {
    out[4 * team] = a0;
    out[4 * team + 1] = a1;
    out[4 * team + 2] = a2;
    out[4 * team + 3] = picked;
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_team_series_probe_16(const uint64_t counter, const double t1, const double t2, const int when, const int64_t teams, double *__restrict__ out) {
  probe<16>(counter, t1, t2, when, teams, out);
}

extern "C" __global__ void __launch_bounds__(256)
k_team_series_probe_4(const uint64_t counter, const double t1, const double t2, const int when, const int64_t teams, double *__restrict__ out) {
  probe<4>(counter, t1, t2, when, teams, out);
}
