// GARCH(1,1) (Bollerslev 1986) with moment summaries of the squared returns:
//     y_t = sigma_t z_t,  sigma^2_{t+1} = omega + alpha y_t^2 + beta sigma^2_t,  t = 0 .. N-1,
// z_0 .. z_{N-1} ~ N(0, 1) the stream's normals in order, sigma^2_0 = params[2] (a positive number; the class's from_observations
// sets it to the mean of y_obs^2).  One recurrence over the series of normals (sabc::Series::recur, csrc/team_series.hpp), the
// state s = sigma^2_t, the element becoming r_t = y_t^2:
//     zz = rounded_product(z, z);  r_t = rounded_product(s, zz);  s = fma(s, fma(alpha, zz, beta), omega)
// -- two products rounded on their own and two explicit fmas, so a transcription with a correctly rounded fma gives the bits.
// Summaries, against data segment 0 (n_lags + 2 values; the class checks the length, the source checks no index):
//     rho[0] = |mean(r) - obs[0]|,  rho[1 + j] = |autocovariance<j>(r, mean(r)) - obs[1 + j]|,  j = 0 .. GARCH11_N_LAGS,
// the canonical sum of csrc/sample_reduce.hpp with every product rounded on its own.
// theta = (omega, alpha, beta); params = [n_obs, n_lags, sigma2_0].  The class prepends  #define GARCH11_N_OBS <N>,
// #define GARCH11_N_LAGS <q>  (q <= 7) and, for the team-aware form,  #define GARCH11_TEAM 1.  Both forms run the same text on
// sabc::Series<N, W> -- the plain form with W = 1, a private array per lane -- and give the same bits.
// Outputs (sabc::emit, a forward run only): output t = y_t = copysign(sqrt_fast(r_t), z_t), the returns; n_outputs = N.  With
// #define GARCH11_EMIT_SQUARES 1  in front of the text (the tests' direct look at the recurrence) also output N + t = r_t.
#if !defined(GARCH11_N_OBS) || !defined(GARCH11_N_LAGS)
#error "garch11.hip: GARCH11_N_OBS and GARCH11_N_LAGS are defined by the model class in front of this text"
#endif
#if GARCH11_N_LAGS < 0 || GARCH11_N_LAGS > 7 || GARCH11_N_LAGS >= GARCH11_N_OBS
#error "garch11.hip: 0 <= GARCH11_N_LAGS <= 7 and GARCH11_N_LAGS < GARCH11_N_OBS"
#endif
template <int J, class R>
__device__ __forceinline__ void garch11_summaries(const R &r, const double center, double *rho) {
  rho[1 + J] = sabc::finite_or_big(fabs(r.template autocovariance<J>(center) - sabc::data_at(1 + J, 0)));
  if constexpr (J < GARCH11_N_LAGS) garch11_summaries<J + 1>(r, center, rho);
}
template <int W>
__device__ __forceinline__ void garch11_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const double omega = theta[0], alpha = theta[1], beta = theta[2];
  sabc::Series<GARCH11_N_OBS, W> z;
  z.fill_normals(rng, [](const int, const double v) { return v; });
  sabc::Series<GARCH11_N_OBS, W> r = z;
  r.recur(p[2], [&](const int, double &s, const double v) {
    const double zz = sabc::series::rounded_product(v, v);
    const double r_t = sabc::series::rounded_product(s, zz);
    s = fma(s, fma(alpha, zz, beta), omega);
    return r_t;
  });
  const double center = r.mean();
  rho[0] = sabc::finite_or_big(fabs(center - sabc::data_at(0, 0)));
  garch11_summaries<0>(r, center, rho);
  if (sabc::emitting(rng)) {
#if defined(GARCH11_EMIT_SQUARES)
    r.emit(rng, GARCH11_N_OBS);
#endif
    r.zip(z, [](const int, const double a, const double b) { return copysign(sabc::sqrt_fast(a), b); });
    r.emit(rng, 0);
  }
}
#if defined(GARCH11_TEAM)
template <int W>
__device__ void sabc_user_simulate_team(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  garch11_simulate<W>(theta, p, rng, rho);
}
#else
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  garch11_simulate<1>(theta, p, rng, rho);
}
#endif
