// MA(2) with autocovariance summaries, the canonical ABC benchmark (Marin, Pudlo, Robert, Ryder 2012):
//     y_t = e_{t+2} + theta1 e_{t+1} + theta2 e_t,  t = 0 .. N-1,  e_0 .. e_{N+1} ~ N(0, 1) the stream's normals in order,
// computed as y_t = fma(theta2, e_t, fma(theta1, e_{t+1}, e_{t+2})) -- explicit fmas, so a transcription with a correctly rounded
// fma gives the bits.  Summaries: tau_j = sum_{t >= j} y_t y_{t-j} / N for j = 0 .. MA2_N_LAGS, the canonical sum of
// csrc/sample_reduce.hpp with every product rounded on its own; rho[j] = |tau_j - acov_obs[j]| against data segment 0, the
// MA2_N_LAGS + 1 observed autocovariances (the class checks the length; the source checks no index).
// theta = (theta1, theta2); params = [n_obs, n_lags].  The class prepends  #define MA2_N_OBS <N>,  #define MA2_N_LAGS <q>
// (q <= 7) and, for the team-aware form,  #define MA2_TEAM 1.  Both forms run the same text on sabc::Series<N + 2, W>
// (csrc/team_series.hpp) -- the plain form with W = 1, a private array per lane -- and give the same bits.
// The series is held at the innovations' times: element s = t + 2 of `y` is y_t, so e_{t+1} and e_t are lags 1 and 2 of the
// innovations and every summary starts at first = 2.  Outputs (sabc::emit, a forward run only): output t = y_t,
// n_outputs = MA2_N_OBS.
#if !defined(MA2_N_OBS) || !defined(MA2_N_LAGS)
#error "ma2.hip: MA2_N_OBS and MA2_N_LAGS are defined by the model class in front of this text"
#endif
#if MA2_N_LAGS < 0 || MA2_N_LAGS > 7 || MA2_N_LAGS >= MA2_N_OBS
#error "ma2.hip: 0 <= MA2_N_LAGS <= 7 and MA2_N_LAGS < MA2_N_OBS"
#endif
template <int J, class Y>
__device__ __forceinline__ void ma2_summaries(const Y &y, double *rho) {
  rho[J] = sabc::finite_or_big(fabs(y.template autocovariance<J>(0.0, 2) - sabc::data_at(J, 0)));
  if constexpr (J < MA2_N_LAGS) ma2_summaries<J + 1>(y, rho);
}
template <int W>
__device__ __forceinline__ void ma2_simulate(const double *theta, sabc::NormalStream &rng, double *rho) {
  const double t1 = theta[0], t2 = theta[1];
  sabc::Series<MA2_N_OBS + 2, W> e;
  e.fill_normals(rng, [](const int, const double z) { return z; });
  sabc::Series<MA2_N_OBS + 2, W> y = e;
  y.zip(e.template lag<1>(), [&](const int, const double a, const double b) { return fma(t1, b, a); });
  y.zip(e.template lag<2>(), [&](const int, const double a, const double b) { return fma(t2, b, a); });
  ma2_summaries<0>(y, rho);
  y.emit(rng, 0, 2);
}
#if defined(MA2_TEAM)
template <int W>
__device__ void sabc_user_simulate_team(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  ma2_simulate<W>(theta, rng, rho);
}
#else
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  ma2_simulate<1>(theta, rng, rho);
}
#endif
