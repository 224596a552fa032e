// A team-aware probe source for tests/test_sample_reduce_compile.py and tests/test_gpu_sample_reduce.py: it calls every
// reduction and distance of sabc::Sample (csrc/team_sample.hpp, csrc/sample_reduce.hpp) and both count functions.  The tests
// prepend  #define PROBE_N <sample size>  and, for the planted form,  #define PROBE_PLANTED 1.
//   drawn form:   the sample is the stream's normals; data segment 0 = an ascending observed sample of PROBE_N values,
//                 segment 1 = a short ascending one (any length >= 1).
//   planted form: x.fill(g) with g(i) = data_at(i, 0) (duplicates, ties with the observed sample and a NaN planted by the
//                 test); the observed samples are segments 1 and 2.
// Outputs 0..N-1 = the sorted sample, then at N + k:
//   0 sum() before the sort      1 sum() after it             2 wasserstein1(obs)        3 max of the values, before the sort
//   4 min of the values, after   5, 6 moments: mean, var      7 ks(obs)                  8 ks(short)
//   9 wasserstein2_squared(obs) 10 sum(|v| + i), after       11 mean()                  12 max(|v| + i), after    13 min(v - i), before
// and at N + 16 + i: the sample as drawn (the drawn form); count_less of rank i in the short segment, count_less_equal at
// 2 N + 16 + i (the planted form).
// rho[0] = ks(obs).  theta is not used.
#if !defined(PROBE_N)
#error "reduce_probe.hip: PROBE_N is defined by the test in front of this text"
#endif
template <int W>
__device__ void sabc_user_simulate_team(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  constexpr int N = PROBE_N;
  sabc::Sample<N, W> x;
#if defined(PROBE_PLANTED)
  constexpr int OBS = 1;
  x.fill([&](const int i) { return sabc::data_at(i, 0); });
#else
  constexpr int OBS = 0;
  x.fill_normals(rng, [&](const double z) { return z; });
  x.emit(rng, N + 16);
#endif
  const auto value = [](const int, const double v) { return v; };
  const double sum_drawn = x.sum();
  const double max_drawn = x.max(value);
  const double min_shifted = x.min([](const int i, const double v) { return v - (double)i; });
  x.sort();
  x.emit(rng, 0);
  double mean, var;
  x.moments(mean, var);
  const double ks = x.ks(OBS);
  sabc::emit(rng, N + 0, sum_drawn);
  sabc::emit(rng, N + 1, x.sum());
  sabc::emit(rng, N + 2, x.wasserstein1(OBS));
  sabc::emit(rng, N + 3, max_drawn);
  sabc::emit(rng, N + 4, x.min(value));
  sabc::emit(rng, N + 5, mean);
  sabc::emit(rng, N + 6, var);
  sabc::emit(rng, N + 7, ks);
  sabc::emit(rng, N + 8, x.ks(OBS + 1));
  sabc::emit(rng, N + 9, x.wasserstein2_squared(OBS));
  sabc::emit(rng, N + 10, x.sum([](const int i, const double v) { return fabs(v) + (double)i; }));
  sabc::emit(rng, N + 11, x.mean());
  sabc::emit(rng, N + 12, x.max([](const int i, const double v) { return fabs(v) + (double)i; }));
  sabc::emit(rng, N + 13, min_shifted);
#if defined(PROBE_PLANTED)
  for (int i = 0; i < N; ++i) {
    const double v = x.at(i);
    sabc::emit(rng, N + 16 + i, (double)sabc::count_less(v, OBS + 1));
    sabc::emit(rng, 2 * N + 16 + i, (double)sabc::count_less_equal(v, OBS + 1));
  }
#endif
  rho[0] = sabc::finite_or_big(ks) + 0.0 * (theta[0] + p[0]);
}
