// A team-aware probe source for tests/test_series_recur_compile.py and tests/test_gpu_series_recur.py: the recurrences of
// sabc::Series (csrc/team_series.hpp).  The tests prepend  #define PROBE_N <series length>.  x_t = normal t of the stream;
// params = [phi1, phi2].  Outputs, N > 2 (at N <= 2 the block with first = 2 is absent):
//   0 .. N-1                the series
//   N .. 2 N                cumsum() whole, then the state recur(0.0, s = s + x) returns
//   2 N + 1 .. 3 N + 2      the AR(2) recurrence, State Carry<2> from (0.25, -0.5): out = fma(phi1, s.v[0], fma(phi2, s.v[1], x)),
//                           the state becomes (out, s.v[0]); whole, then both components of the returned state
//   3 N + 3 .. 4 N + 4      the same with first = 2
//   then N values           recur_with against the ramp o_t = 0.125 t, State double from 1.5: s = fma(0.5, s, x);
//                           out = rounded_product(exp_tab(0.25 s), o_t)
// rho[0] = |the sum's state| (1e30 where that is not finite).  theta is not used.
#if !defined(PROBE_N)
#error "recur_probe.hip: PROBE_N is defined by the test in front of this text"
#endif
template <int W>
__device__ void sabc_user_simulate_team(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  constexpr int N = PROBE_N;
  using Pair = sabc::series::Carry<2>;
  const double phi1 = p[0], phi2 = p[1];
  sabc::Series<N, W> x;
  x.fill_normals(rng, [](const int, const double z) { return z; });
  x.emit(rng, 0);
  long long o = N;

  sabc::Series<N, W> c = x;
  c.cumsum();
  c.emit(rng, o);
  c = x;
  const double total = c.recur(0.0, [](const int, double &s, const double v) { s = s + v; return s; });
  sabc::emit(rng, o + N, total);
  o += N + 1;

  const auto ar2 = [&](const int, Pair &s, const double v) {
    const double out = fma(phi1, s.v[0], fma(phi2, s.v[1], v));
    s.v[1] = s.v[0];
    s.v[0] = out;
    return out;
  };
  sabc::Series<N, W> a = x;
  Pair end = a.recur(Pair{{0.25, -0.5}}, ar2);
  a.emit(rng, o);
  sabc::emit(rng, o + N, end.v[0]);
  sabc::emit(rng, o + N + 1, end.v[1]);
  o += N + 2;
  if constexpr (N > 2) {
    a = x;
    end = a.recur(Pair{{0.25, -0.5}}, ar2, 2);
    a.emit(rng, o);
    sabc::emit(rng, o + N, end.v[0]);
    sabc::emit(rng, o + N + 1, end.v[1]);
    o += N + 2;
  }

  sabc::Series<N, W> ramp;
  ramp.fill([](const int t) { return 0.125 * (double)t; });
  sabc::Series<N, W> e = x;
  e.recur_with(ramp, 1.5, [](const int, double &s, const double v, const double r) {
    s = fma(0.5, s, v);
    return sabc::series::rounded_product(sabc::exp_tab(0.25 * s), r);
  });
  e.emit(rng, o);
  rho[0] = sabc::finite_or_big(fabs(total)) + 0.0 * theta[0];
}
