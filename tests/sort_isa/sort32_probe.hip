// sabc::sort_ascending's unrolled form on its own, for tests/test_sort_isa.py: a lane fills double x[32] from a counter that is
// a kernel argument (nothing folds away), sorts it with the template form and stores it, one array per lane, element j of lane
// i at out[j * lanes + i].  Every index is a compile-time constant: the array must not leave the registers.
#include "sort_network.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" __global__ void __launch_bounds__(256)
k_sort32_probe(const uint64_t counter, const int64_t lanes, double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= lanes) return;
  double x[32];
  uint64_t c = counter + (uint64_t)i;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    c = c * 6364136223846793005ull + 1442695040888963407ull;
    x[j] = (double)(int64_t)(c >> 11);
  }
  sabc::sort_ascending(x);
#pragma unroll
  for (int j = 0; j < 32; ++j) out[(int64_t)j * lanes + i] = x[j];
}
