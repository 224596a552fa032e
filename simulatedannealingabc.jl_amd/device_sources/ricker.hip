// The Ricker map with Poisson observations (Wood 2010, the standard benchmark of ABC and synthetic likelihood), a state-space
// model with COUNT observations:
//     N_{t+1} = r N_t exp(-N_t + sigma z_t),  y_t ~ Poisson(phi N_{t+1}),  t = 0 .. N-1,  N = RICKER_BURN_IN + RICKER_N_OBS,
// z_0 .. z_{N-1} ~ N(0, 1) the stream's normals in order, N_0 = params[3].  theta = (log r, sigma, phi).
//   1. e_t = rounded_product(sigma, z_t)                             (fill_normals; the product rounded on its own)
//   2. one recurrence (sabc::Series::recur, csrc/team_series.hpp), the state s = N_t, the element becoming N_{t+1}:
//          g = exp_tab((log r - s) + e_t);  s = rounded_product(s, g)            -- both additions in that order
//   3. y = the latent series;  y.map_poisson(rng, phi): y_t = Poisson(rounded_product(phi, N_{t+1})), the draw KEYED by t
//      (sabc::CountDraws, csrc/device_rng.hpp: index t owns 64 blocks of the counter behind the normals', so a lane of a team
//      draws for the times it holds and every width gives the same counts).
// so a transcription with exp_tab's restatement and plain float64 products gives the bits.  An overflowing latent state gives
// lambda = inf or NaN, which the count draw takes as 2^30 or 0: no draw can spin, and the distances pass through finite_or_big.
// Summaries over the n_obs times t >= RICKER_BURN_IN, against data segment 0 (n_lags + 3 values; the class checks the length,
// the source checks no index):
//     rho[0] = |mean(y) - obs[0]|,  rho[1] = |#{t: y_t = 0} - obs[1]| (a canonical sum of exact 0 / 1 terms),
//     rho[2 + j] = |autocovariance<j>(y, mean(y), burn_in) - obs[2 + j]|,  j = 0 .. RICKER_N_LAGS,
// the canonical sum of csrc/sample_reduce.hpp over all N times, +0.0 where t < burn_in, divided by n_obs.
// params = [n_obs, burn_in, n_lags, n0].  The class prepends  #define RICKER_N_OBS <n>,  #define RICKER_BURN_IN <b>,
// #define RICKER_N_LAGS <q>  (q <= 7) and, for the team-aware form,  #define RICKER_TEAM 1.  Both forms run the same text on
// sabc::Series<N, W> -- the plain form with W = 1, a private array per lane -- and give the same bits.
// Outputs (sabc::emit, a forward run only): output i = y_{burn_in + i}, the observed counts; n_outputs = n_obs.  With
// #define RICKER_EMIT_LATENT 1  in front of the text (the tests' direct look at the recurrence) also output n_obs + t = N_{t+1}
// for every t < N, the burn-in included.
#if !defined(RICKER_N_OBS) || !defined(RICKER_BURN_IN) || !defined(RICKER_N_LAGS)
#error "ricker.hip: RICKER_N_OBS, RICKER_BURN_IN and RICKER_N_LAGS are defined by the model class in front of this text"
#endif
#if RICKER_N_LAGS < 0 || RICKER_N_LAGS > 7 || RICKER_N_LAGS >= RICKER_N_OBS || RICKER_BURN_IN < 0
#error "ricker.hip: 0 <= RICKER_N_LAGS <= 7, RICKER_N_LAGS < RICKER_N_OBS and RICKER_BURN_IN >= 0"
#endif
#define RICKER_N (RICKER_BURN_IN + RICKER_N_OBS)
template <int J, class Y>
__device__ __forceinline__ void ricker_summaries(const Y &y, const double center, double *rho) {
  rho[2 + J] = sabc::finite_or_big(fabs(y.template autocovariance<J>(center, RICKER_BURN_IN) - sabc::data_at(2 + J, 0)));
  if constexpr (J < RICKER_N_LAGS) ricker_summaries<J + 1>(y, center, rho);
}
template <int W>
__device__ __forceinline__ void ricker_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const double logr = theta[0], sigma = theta[1], phi = theta[2];
  sabc::Series<RICKER_N, W> latent;
  latent.fill_normals(rng, [&](const int, const double v) { return sabc::series::rounded_product(sigma, v); });
  latent.recur(p[3], [&](const int, double &s, const double e) {
    const double g = sabc::exp_tab((logr - s) + e);
    s = sabc::series::rounded_product(s, g);
    return s;
  });
  sabc::Series<RICKER_N, W> y = latent;
  y.map_poisson(rng, phi);
  const double center = y.sum([](const int t, const double v) { return t >= RICKER_BURN_IN ? v : 0.0; }) / (double)RICKER_N_OBS;
  const double zeros = y.sum([](const int t, const double v) { return t >= RICKER_BURN_IN && v == 0.0 ? 1.0 : 0.0; });
  rho[0] = sabc::finite_or_big(fabs(center - sabc::data_at(0, 0)));
  rho[1] = sabc::finite_or_big(fabs(zeros - sabc::data_at(1, 0)));
  ricker_summaries<0>(y, center, rho);
  if (sabc::emitting(rng)) {
    y.emit(rng, 0, RICKER_BURN_IN);
#if defined(RICKER_EMIT_LATENT)
    latent.emit(rng, RICKER_N_OBS);
#endif
  }
}
#if defined(RICKER_TEAM)
template <int W>
__device__ void sabc_user_simulate_team(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  ricker_simulate<W>(theta, p, rng, rho);
}
#else
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  ricker_simulate<1>(theta, p, rng, rho);
}
#endif
