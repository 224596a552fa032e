// sabc::Sample<128, W> on its own, for tests/test_team_sample_isa.py: a team of W lanes fills the sample from a counter that is
// a kernel argument (nothing folds away), sorts it and reads ONE quantile whose probability is a kernel argument -- a rank the
// compiler cannot know.  The slots must not leave the registers: no indexed access, a select over the slots instead.
#include "device_rng.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

template <int W>
__device__ __forceinline__ void probe(const uint64_t counter, const double p, const int64_t teams, double *__restrict__ out) {
  const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) / W;
  if (t >= teams) return;                              // (uniform over a team)
  sabc::Sample<128, W> x;
  x.fill([&](const int i) {
    const uint64_t c = (counter + (uint64_t)t * 128u + (uint64_t)i) * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(c >> 11);
  });
  x.sort();
  const double q = x.quantile(p);
  if ((threadIdx.x & (W - 1)) == 0) out[t] = q;
}

extern "C" __global__ void __launch_bounds__(256)
k_team_sort_probe_16(const uint64_t counter, const double p, const int64_t teams, double *__restrict__ out) {
  probe<16>(counter, p, teams, out);
}

extern "C" __global__ void __launch_bounds__(256)
k_team_sort_probe_4(const uint64_t counter, const double p, const int64_t teams, double *__restrict__ out) {
  probe<4>(counter, p, teams, out);
}
