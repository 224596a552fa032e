// sabc::Series<128, W>::map_poisson on its own, for tests/test_series_counts_isa.py: a team of W lanes fills the series from a
// counter that is a kernel argument, and sums it -- with (k_series_counts_probe_W) and without (k_series_counts_base_W) the
// map_poisson in between.  The draws are lane-local: what the map adds holds no barrier, no DPP move and no ds_swizzle.  Both
// kernels load the elementary functions' tables first (rng_tables_init: the one barrier of either), as every kernel that draws
// does.
#include "device_rng.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

template <int W, bool DRAW>
__device__ __forceinline__ void probe(const uint64_t seed, const uint64_t counter, const double scale, const int64_t teams, double *__restrict__ out) {
  sabc::rng_tables_init();
  const int64_t team = ((int64_t)blockIdx.x * 256 + threadIdx.x) / W;
  if (team >= teams) return;                           // (uniform over a team)
  sabc::Series<128, W> x;
  x.fill([&](const int t) {
    const uint64_t c = (counter + (uint64_t)team * 128u + (uint64_t)t) * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(c >> 11) * 0x1p-48;      // [0, 32): both branches of the draw
  });
  if constexpr (DRAW) {
    sabc::NormalStream rng(seed, (uint64_t)team, sabc::PURPOSE_SIM, counter, W);
    x.map_poisson(rng, scale);
  }
  const double sum = x.sum();
  if ((threadIdx.x & (W - 1)) == 0) out[team] = sum;
}

#define PROBE_KERNEL(NAME, W, DRAW)                                                                                              \
  extern "C" __global__ void __launch_bounds__(256)                                                                              \
  NAME(const uint64_t seed, const uint64_t counter, const double scale, const int64_t teams, double *__restrict__ out) {         \
    probe<W, DRAW>(seed, counter, scale, teams, out);                                                                            \
  }
PROBE_KERNEL(k_series_counts_probe_16, 16, true)
PROBE_KERNEL(k_series_counts_base_16, 16, false)
PROBE_KERNEL(k_series_counts_probe_4, 4, true)
PROBE_KERNEL(k_series_counts_base_4, 4, false)
