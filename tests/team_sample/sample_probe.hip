// A team-aware probe source for tests/test_team_sample_compile.py and tests/test_gpu_team_sample.py: it calls every member of
// sabc::Sample.  The tests prepend  #define PROBE_N <sample size>  and, for the planted form,  #define PROBE_PLANTED 1.
//   drawn form:   outputs 0..N-1 = the sample as drawn (x.emit before the sort), N..2N-1 = sorted (x.emit after it);
//                 rho[0] = |x.at(0) - x.order_statistic(1)| + |x.drawn(0) - first normal| = 0 when the read-outs agree,
//                 rho[1] = x.quantile(params[0]).
//   planted form: x.fill(g) with g(i) = data_at(i) (a NaN and duplicates planted by the test), the same outputs.
// theta is not used: the sample is the stream's normals themselves.
#if !defined(PROBE_N)
#error "sample_probe.hip: PROBE_N is defined by the test in front of this text"
#endif
template <int W>
__device__ void sabc_user_simulate_team(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  constexpr int N = PROBE_N;
  sabc::Sample<N, W> x;
#if defined(PROBE_PLANTED)
  x.fill([&](const int i) { return sabc::data_at(i, 0); });
#else
  x.fill_normals(rng, [&](const double z) { return z; });
#endif
  const double first = x.drawn(0);
  x.emit(rng, 0);
  x.sort();
  x.emit(rng, N);
  rho[0] = fabs(x.at(0) - x.order_statistic(1)) + (x.order_statistic(N + 1) == __builtin_huge_val() ? 0.0 : 1.0) + 0.0 * theta[0];
  rho[1] = sabc::finite_or_big(fabs(x.quantile(p[0]))) + (first == first ? 0.0 : 0.0);
}
