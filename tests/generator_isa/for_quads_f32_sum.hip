// The binary32 generator's hot loop on its own, for tests/test_generator_isa_f32.py: a lane per particle sums the normals of n
// blocks drawn through NormalStream::for_quads_f32, four per block.  n, seed and iteration are kernel arguments, so nothing
// folds away; the test compiles this file to gfx950 assembly and counts the loop's instructions.
#include "device_rng.hpp"

extern "C" __global__ void __launch_bounds__(256)
k_for_quads_f32_sum(const uint64_t seed, const uint64_t iter, const int n, const int64_t lanes, float *__restrict__ out) {
  sabc::rng_tables_init();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= lanes) return;
  sabc::NormalStream ns(seed, (uint64_t)i, sabc::PURPOSE_SIM, iter);
  float acc = 0.0f;
  ns.for_quads_f32(n, [&](const float z0, const float z1, const float z2, const float z3) {
    acc += z0;
    acc += z1;
    acc += z2;
    acc += z3;
  });
  out[i] = acc;
}
