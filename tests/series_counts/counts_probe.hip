// A team-aware probe source for tests/test_series_counts_compile.py and tests/test_gpu_series_counts.py: count draws keyed by an
// index (sabc::CountDraws, csrc/device_rng.hpp) on a sabc::Series (csrc/team_series.hpp).  The tests prepend
// #define PROBE_N <series length>.  x_t = normal t of the stream (ceil(N / 2) blocks); then three reservations of N indices each.
// Data: segment 0 the ramp lambda_t, segment 1 the trial counts n_t (doubles), segment 2 the probabilities p_t, N values each.
// theta[0] = m, the mean offspring of the branching process; params = [s0, scale].  Outputs:
//   0 .. N-1            (a) cd_a.poisson(t, lambda_t), drawn inside fill: a lane of the team draws for the times it holds
//   N .. 2 N - 1        (b) cd_b.binomial(t, n_t, p_t), likewise
//   2 N, 2 N + 1        (c) the pair() drawn behind the three reservations: block ceil(N / 2) + 64 * 3 N of the stream
//   2 N + 2 .. 3 N + 2  (d) the branching process s <- cd_d.poisson(t, fma(m, s, |x_t|)) from s0, a recurrence whose f draws
//                           (recur_rolled: one copy of the draw; with  #define PROBE_PLAIN_RECUR 1  recur itself): the series
//                           whole, then the returned state
//   3 N + 3 .. 4 N + 2  (e) y_t = 8 |x_t|, then y.map_poisson(rng, scale): its own reservation, behind the pair's block
// rho[0] = the returned state of (d) (1e30 where that is not finite).
#if !defined(PROBE_N)
#error "counts_probe.hip: PROBE_N is defined by the test in front of this text"
#endif
template <int W>
__device__ void sabc_user_simulate_team(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  constexpr int N = PROBE_N;
  const double m = theta[0], s0 = p[0], scale = p[1];
  sabc::Series<N, W> x;
  x.fill_normals(rng, [](const int, const double z) { return z; });
  const sabc::CountDraws cd_a = rng.reserve_counts(N), cd_b = rng.template reserve_counts<N>(), cd_d = rng.reserve_counts(N);

  sabc::Series<N, W> a;
  a.fill([&](const int t) { return (double)cd_a.poisson(t, sabc::data_at(t, 0)); });
  a.emit(rng, 0);
  sabc::Series<N, W> b;
  b.fill([&](const int t) { return (double)cd_b.binomial(t, sabc::data_at(t, 1), sabc::data_at(t, 2)); });
  b.emit(rng, N);

  double z0, z1;
  rng.pair(z0, z1);
  sabc::emit(rng, 2 * N, z0);
  sabc::emit(rng, 2 * N + 1, z1);

  sabc::Series<N, W> d = x;
  const auto offspring = [&](const int t, double &s, const double v) {
    s = (double)cd_d.poisson(t, fma(m, s, fabs(v)));
    return s;
  };
#if defined(PROBE_PLAIN_RECUR)
  const double end = d.recur(s0, offspring);           // the unrolled relay: a copy of the draw per time step (the tests: N = 3)
#else
  const double end = d.recur_rolled(s0, offspring);
#endif
  d.emit(rng, 2 * N + 2);
  sabc::emit(rng, 3 * N + 2, end);

  sabc::Series<N, W> y = x;
  y.map([](const int, const double v) { return 8.0 * fabs(v); });
  y.map_poisson(rng, scale);
  y.emit(rng, 3 * N + 3);
  rho[0] = sabc::finite_or_big(end);
}
