// A team-aware probe source for tests/test_team_series_compile.py and tests/test_gpu_team_series.py: it calls every member of
// sabc::Series (csrc/team_series.hpp).  The tests prepend  #define PROBE_N <series length>  and, for the planted form,
// #define PROBE_PLANTED 1.
//   drawn form:   x_t = normal t of the stream.
//   planted form: x.fill(g) with g(t) = data_at(t, 0) (a NaN and an infinity planted by the test).
// FIRST = 2 for N > 2, else 0.  params[0] = a time index known at run time only.  Outputs:
//   0 .. N-1                the series
//   N + k, k < 16:          0 sum()   1 mean()   2, 3 moments: mean, var   4 max(|v| + t)   5 min(v - t)   6 sum(|v| + t)
//                           7 autocovariance<0>()   8 autocovariance<0>(0.25, FIRST)   9 at(params[0])
//   N + 16 .. 2 N + 15      z with z_t = (x_t + t) - 2 x_t: map, then zip with x
//   2 N + 16 ..             for each lag L of (1, 2 at N = 3 only, 3, 4, 5, 9, 44) with L < N, N + 4 values:
//                           lag<L>(-7.0) whole, lagged_sum<L>(|a - b|), lagged_sum<L>(|a - b|, FIRST), autocovariance<L>(),
//                           autocovariance<L>(0.25, FIRST)
//   then N - FIRST values:  emit(rng, ., FIRST): x_FIRST .. x_{N-1}
//   then N values:          at(t) for every t (a loop: t is a run-time value)
// rho[0] = |sum()| (1e30 where that is not finite).  theta is not used.
#if !defined(PROBE_N)
#error "series_probe.hip: PROBE_N is defined by the test in front of this text"
#endif
template <int L, int N, class X>
__device__ __forceinline__ void probe_lag(const X &x, sabc::NormalStream &rng, long long &o, const int first) {
  if constexpr (L >= 1 && L < N) {
    const auto distance = [](const int, const double a, const double b) { return fabs(a - b); };
    x.template lag<L>(-7.0).emit(rng, o);
    o += N;
    sabc::emit(rng, o++, x.template lagged_sum<L>(distance));
    sabc::emit(rng, o++, x.template lagged_sum<L>(distance, first));
    sabc::emit(rng, o++, x.template autocovariance<L>());
    sabc::emit(rng, o++, x.template autocovariance<L>(0.25, first));
  }
}
template <int W>
__device__ void sabc_user_simulate_team(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  constexpr int N = PROBE_N, FIRST = N > 2 ? 2 : 0;
  sabc::Series<N, W> x;
#if defined(PROBE_PLANTED)
  x.fill([&](const int t) { return sabc::data_at(t, 0); });
#else
  x.fill_normals(rng, [](const int, const double z) { return z; });
#endif
  x.emit(rng, 0);
  double mean, var;
  x.moments(mean, var);
  const double sum = x.sum();
  sabc::emit(rng, N + 0, sum);
  sabc::emit(rng, N + 1, x.mean());
  sabc::emit(rng, N + 2, mean);
  sabc::emit(rng, N + 3, var);
  sabc::emit(rng, N + 4, x.max([](const int t, const double v) { return fabs(v) + (double)t; }));
  sabc::emit(rng, N + 5, x.min([](const int t, const double v) { return v - (double)t; }));
  sabc::emit(rng, N + 6, x.sum([](const int t, const double v) { return fabs(v) + (double)t; }));
  sabc::emit(rng, N + 7, x.template autocovariance<0>());
  sabc::emit(rng, N + 8, x.template autocovariance<0>(0.25, FIRST));
  sabc::emit(rng, N + 9, x.at((int)p[0]));
  sabc::Series<N, W> z = x;
  z.map([](const int t, const double v) { return v + (double)t; });
  z.zip(x, [](const int, const double a, const double b) { return a - 2.0 * b; });
  z.emit(rng, N + 16);
  long long o = 2 * N + 16;
  probe_lag<1, N>(x, rng, o, FIRST);
  probe_lag<(N == 3 ? 2 : 0), N>(x, rng, o, FIRST);
  probe_lag<3, N>(x, rng, o, FIRST);
  probe_lag<4, N>(x, rng, o, FIRST);
  probe_lag<5, N>(x, rng, o, FIRST);
  probe_lag<9, N>(x, rng, o, FIRST);
  probe_lag<44, N>(x, rng, o, FIRST);
  x.emit(rng, o, FIRST);
  o += N - FIRST;
  if (sabc::emitting(rng))
    for (int t = 0; t < N; ++t) sabc::emit(rng, o + t, x.at(t));
  rho[0] = sabc::finite_or_big(fabs(sum)) + 0.0 * (theta[0] + p[0]);
}
