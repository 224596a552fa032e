// A team-aware probe source for tests/test_team_sample_f32_compile.py and tests/test_gpu_team_sample_f32.py: it calls every
// member of sabc::SampleF32 (csrc/team_sample_f32.hpp).  The tests prepend  #define PROBE_N <sample size>  and, for the planted
// form,  #define PROBE_PLANTED 1.
//   drawn form:   the sample is the stream's binary32 normals themselves (fill_normals with the identity); data segment 0 = an
//                 ascending observed sample of PROBE_N doubles, segment 1 = a short ascending one (any length >= 1).
//   planted form: x.fill(g) with g(i) = (float)data_at(i, 0) (a NaN, duplicates and ties with the observed sample planted by the
//                 test); the observed samples are segments 1 and 2.
// Outputs 0..N-1 = the sample as drawn (x.emit before the sort), N..2N-1 = sorted (x.emit after it), then at 2 N + k:
//   0 sum() before the sort      1 sum() after it             2 wasserstein1(obs)        3 max of the values, before the sort
//   4 min of the values, after   5, 6 moments: mean, var      7 ks(obs)                  8 ks(short)
//   9 wasserstein2_squared(obs) 10 sum(|v| + i), after       11 mean()                  12 max(|v| + i), after    13 min(v - i), before
//  14 quantile(params[0])       15 drawn(0), read before the sort                        16 at(N - 1)
//  17 |at(0) - order_statistic(1)| + (order_statistic(N + 1) == +inf ? 0 : 1) + (order_statistic(0) == +inf ? 0 : 1): 0 when the
//     read-outs agree
// rho[0] = ks(obs), rho[1] = |quantile(params[0])|.  theta is not used.
#if !defined(PROBE_N)
#error "sample_probe_f32.hip: PROBE_N is defined by the test in front of this text"
#endif
template <int W>
__device__ void sabc_user_simulate_team(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  constexpr int N = PROBE_N;
  sabc::SampleF32<N, W> x;
  static_assert(sabc::SampleF32<N, W>::size == N && sabc::SampleF32<N, W>::lanes == W, "the type says what it holds");
#if defined(PROBE_PLANTED)
  constexpr int OBS = 1;
  x.fill([&](const int i) { return (float)sabc::data_at(i, 0); });
#else
  constexpr int OBS = 0;
  x.fill_normals(rng, [&](const float z) { return z; });
#endif
  const float first = x.drawn(0);
  x.emit(rng, 0);
  const auto value = [](const int, const float v) { return (double)v; };
  const double sum_drawn = x.sum();
  const double max_drawn = x.max(value);
  const double min_shifted = x.min([](const int i, const float v) { return (double)v - (double)i; });
  x.sort();
  x.emit(rng, N);
  double mean, var;
  x.moments(mean, var);
  const double ks = x.ks(OBS), q = x.quantile(p[0]);
  constexpr int R = 2 * N;
  sabc::emit(rng, R + 0, sum_drawn);
  sabc::emit(rng, R + 1, x.sum());
  sabc::emit(rng, R + 2, x.wasserstein1(OBS));
  sabc::emit(rng, R + 3, max_drawn);
  sabc::emit(rng, R + 4, x.min(value));
  sabc::emit(rng, R + 5, mean);
  sabc::emit(rng, R + 6, var);
  sabc::emit(rng, R + 7, ks);
  sabc::emit(rng, R + 8, x.ks(OBS + 1));
  sabc::emit(rng, R + 9, x.wasserstein2_squared(OBS));
  sabc::emit(rng, R + 10, x.sum([](const int i, const float v) { return fabs((double)v) + (double)i; }));
  sabc::emit(rng, R + 11, x.mean());
  sabc::emit(rng, R + 12, x.max([](const int i, const float v) { return fabs((double)v) + (double)i; }));
  sabc::emit(rng, R + 13, min_shifted);
  sabc::emit(rng, R + 14, q);
  sabc::emit(rng, R + 15, (double)first);
  sabc::emit(rng, R + 16, (double)x.at(N - 1));
  sabc::emit(rng, R + 17, fabs((double)x.at(0) - (double)x.order_statistic(1)) + (x.order_statistic(N + 1) == __builtin_huge_valf() ? 0.0 : 1.0) +
                              (x.order_statistic(0) == __builtin_huge_valf() ? 0.0 : 1.0));
  rho[0] = sabc::finite_or_big(ks) + 0.0 * theta[0];
  rho[1] = sabc::finite_or_big(fabs(q));
}
