// The f_dist of the reference's getting-started example (docs/src/usage.md:15-35) on the device:
//     y_sim = rand(Normal(theta[1], theta[2]), length(y_obs))
//     rho   = (|mean(y_obs) - mean(y_sim)|, |sum(abs2, y_obs) - sum(abs2, y_sim)|)
// theta = (mu, sigma); y_obs is data segment 0 (sabc_set_device_data), read in place: no parameter is used.  The draws are the
// pairs of the particle's simulation stream in order (for_pairs), an odd last draw being the first normal of one more block.
// The two observed moments are summed from the data in index order on every call, as the reference recomputes them: the
// loop's index is the same in every lane, so a point of y_obs costs one scalar load per wave.
// Outputs (sabc::emit, a forward run only): output j = y_sim[j].  The forward run has a loop of its own, whose lambda keeps the
// index and hands the draws out; it is dead code wherever nothing is emitted, and the loop of the update kernels is the loop it
// always was, text and instructions (a lambda that captures `rng` for emit costs the team kernels registers even when every
// emit folds away: tools/rtc_unit_isa.py + tools/kernel_isa_diff.py show it).
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const long long n = sabc::data_len();
  const double mu = theta[0], sd = theta[1];
  double s1 = 0.0, s2 = 0.0;
  if (sabc::emitting(rng)) {
    long long at = 0;
    rng.for_pairs((int)(n >> 1), [&](const double z0, const double z1) {
      const double y0 = mu + sd * z0, y1 = mu + sd * z1;
      s1 += y0;
      s2 += y0 * y0;
      s1 += y1;
      s2 += y1 * y1;
      sabc::emit(rng, at, y0);
      sabc::emit(rng, at + 1, y1);
      at += 2;
    });
  } else {
    rng.for_pairs((int)(n >> 1), [&](const double z0, const double z1) {
      const double y0 = mu + sd * z0, y1 = mu + sd * z1;
      s1 += y0;
      s2 += y0 * y0;
      s1 += y1;
      s2 += y1 * y1;
    });
  }
  if (n & 1) {
    double z0, z1;
    rng.pair(z0, z1);
    const double y0 = mu + sd * z0;
    s1 += y0;
    s2 += y0 * y0;
    sabc::emit(rng, n - 1, y0);
  }
  double o1 = 0.0, o2 = 0.0;
  for (long long j = 0; j < n; ++j) {
    const double y = sabc::data_at(j);
    o1 += y;
    o2 += y * y;
  }
  rho[0] = fabs(o1 / (double)n - s1 / (double)n);
  rho[1] = fabs(o2 - s2);
}
