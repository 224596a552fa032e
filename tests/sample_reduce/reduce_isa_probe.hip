// sabc::Sample<128, W> with its reductions on its own, for tests/test_sample_reduce_isa.py: a team of W lanes fills the sample
// from a counter that is a kernel argument (nothing folds away), sorts it and takes sum(), wasserstein1 and ks against an
// observed sample in memory.  The slots must not leave the registers: the reductions index them with constants only.
// A source-compiled unit gets sabc::data_at / data_len from the run-time compiler's preamble; here they read two module
// variables.
#include "device_rng.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ const double *probe_obs;
__device__ long long probe_obs_len;
namespace sabc {
__device__ __forceinline__ long long data_len(int) { return probe_obs_len; }
__device__ __forceinline__ double data_at(long long i, int) { return probe_obs[i]; }
}  // namespace sabc

template <int W>
__device__ __forceinline__ void probe(const uint64_t counter, const int64_t teams, double *__restrict__ out) {
  const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) / W;
  if (t >= teams) return;                              // (uniform over a team)
  sabc::Sample<128, W> x;
  x.fill([&](const int i) {
    const uint64_t c = (counter + (uint64_t)t * 128u + (uint64_t)i) * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(c >> 11);
  });
  x.sort();
  const double s = x.sum(), w1 = x.wasserstein1(0), ks = x.ks(0);
  if ((threadIdx.x & (W - 1)) == 0) {
    out[3 * t] = s;
    out[3 * t + 1] = w1;
    out[3 * t + 2] = ks;
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_reduce_probe_16(const uint64_t counter, const int64_t teams, double *__restrict__ out) {
  probe<16>(counter, teams, out);
}

extern "C" __global__ void __launch_bounds__(256)
k_reduce_probe_4(const uint64_t counter, const int64_t teams, double *__restrict__ out) {
  probe<4>(counter, teams, out);
}
