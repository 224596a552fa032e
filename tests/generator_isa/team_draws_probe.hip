// Every public draw member of NormalStream on its own, for tests/test_team_draws_isa.py: one kernel per way of sharing a stream
// -- a lane per particle (coop = 0), a quad and a row of 16 lanes per particle (4, 16), and a lane per particle with the plain
// loops (kCoopPlainLoop) -- sums n pairs through for_pairs, m blocks through for_quads_f32, one call each of pair, uniform_pair,
// quad_f32, uniform_quad_f32 and next, and a Poisson count whose mean is one of the draws.  n, m, seed and iteration are kernel
// arguments, so nothing folds away and both loops run their whole groups AND their tails; the test compiles this file to
// gfx950 assembly and reads each kernel's registers and scratch.
#include "device_rng.hpp"

template <int COOP>
__global__ void __launch_bounds__(256)
k_team_draws(const uint64_t seed, const uint64_t iter, const int n, const int m, const int64_t particles, double *__restrict__ out) {
  constexpr int W = COOP > 0 ? COOP : 1;
  sabc::rng_tables_init();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t p = t / W;
  if (p >= particles) return;                          // (uniform over a team)
  sabc::NormalStream ns(seed, (uint64_t)p, sabc::PURPOSE_SIM, iter, COOP);
  double acc = 0.0;
  float facc = 0.0f;
  ns.for_pairs(n, [&](const double z0, const double z1) {
    acc += z0;
    acc += z1;
  });
  ns.for_quads_f32(m, [&](const float z0, const float z1, const float z2, const float z3) {
    facc += z0;
    facc += z1;
    facc += z2;
    facc += z3;
  });
  double z0, z1, u0, u1;
  ns.pair(z0, z1);
  ns.uniform_pair(u0, u1);
  acc += z0 + z1 + u0 + u1;
  float f0, f1, f2, f3, g0, g1, g2, g3;
  ns.quad_f32(f0, f1, f2, f3);
  ns.uniform_quad_f32(g0, g1, g2, g3);
  facc += f0 + f1 + f2 + f3 + g0 + g1 + g2 + g3;
  acc += ns.next();
  acc += (double)ns.poisson(20.0 * u0);               // both branches of the count draw: inversion below 10, PTRS above
  out[t] = acc + (double)facc;
}

template __global__ void k_team_draws<0>(uint64_t, uint64_t, int, int, int64_t, double *);
template __global__ void k_team_draws<4>(uint64_t, uint64_t, int, int, int64_t, double *);
template __global__ void k_team_draws<16>(uint64_t, uint64_t, int, int, int64_t, double *);
template __global__ void k_team_draws<sabc::kCoopPlainLoop>(uint64_t, uint64_t, int, int, int64_t, double *);
