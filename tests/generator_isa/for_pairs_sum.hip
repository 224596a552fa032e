// The generator's hot loop on its own, for tests/test_generator_isa.py: a lane per particle sums n pairs drawn through
// NormalStream::for_pairs -- the path the built-in simulators and k_rng_peak take.  n, seed and iteration are kernel
// arguments, so nothing folds away; the test compiles this file to gfx950 assembly and counts the loop's instructions.
#include "device_rng.hpp"

extern "C" __global__ void __launch_bounds__(256)
k_for_pairs_sum(const uint64_t seed, const uint64_t iter, const int n, const int64_t lanes, double *__restrict__ out) {
  sabc::rng_tables_init();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= lanes) return;
  sabc::NormalStream ns(seed, (uint64_t)i, sabc::PURPOSE_SIM, iter);
  double acc = 0.0;
  ns.for_pairs(n, [&](const double z0, const double z1) {
    acc += z0;
    acc += z1;
  });
  out[i] = acc;
}
