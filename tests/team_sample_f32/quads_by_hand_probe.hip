// The stream definition SampleF32::fill_normals is held to, for tests/test_gpu_team_sample_f32.py: a source registered the plain way
// (a lane per row) fills float x[4 HAND_BLOCKS] by hand with rng.for_quads_f32 -- z0..z3 of block 0, then of block 1, .. -- and
// emits it.  Draw i of a SampleF32<N, W> is output i of this probe for every N <= 4 HAND_BLOCKS and every W.  The test prepends
// #define HAND_BLOCKS <blocks>.
#if !defined(HAND_BLOCKS)
#error "quads_by_hand_probe.hip: HAND_BLOCKS is defined by the test in front of this text"
#endif
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  constexpr int B = HAND_BLOCKS;
  float x[4 * B];
  int at = 0;
  rng.for_quads_f32(B, [&](const float z0, const float z1, const float z2, const float z3) {
    x[at] = z0;
    x[at + 1] = z1;
    x[at + 2] = z2;
    x[at + 3] = z3;
    at += 4;
  });
  for (int i = 0; i < 4 * B; ++i) sabc::emit(rng, i, (double)x[i]);
  rho[0] = fabs((double)x[0]) + 0.0 * (theta[0] + p[0]);
}
