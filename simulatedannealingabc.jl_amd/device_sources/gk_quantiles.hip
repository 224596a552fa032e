// g-and-k compared at quantiles: x = A + B (1 + c tanh(g z / 2)) (1 + z^2)^k z, z ~ N(0, 1), GKQ_N_DRAWS draws;
//     rho_j = |quantile(sort(x), probs[j]) - q_obs[j]|,   j < GKQ_N_STATS
// theta = (A, B, g, k); params = [n_draws, c]; data segment 0 = probs, segment 1 = q_obs (GKQ_N_STATS values each: the class
// checks it wherever data enter, the source checks no index).  The class prepends the two #defines: the sample's length is a
// compile-time constant, so sabc::sort_ascending is its template form -- up to 32 draws the network as straight-line code
// on registers, above that the loop form.  The quantile is Julia's default (type 7; NumPy's "linear"), sabc::quantile.
// The draws are the pairs of the particle's simulation stream in order (for_pairs), an odd last draw being the first normal of
// one more block, as in normal_moments.hip.  The sample is indexed by the loop's counter while it is drawn and by the
// quantiles' ranks afterwards, so it lives in the lane's private memory (8 GKQ_N_DRAWS bytes; the same index in every lane:
// one line per wave and access); the unrolled network reads it once and writes it back once.
// tanh, exp and log are device_rng.hpp's (tanh_abs_tab: 2.8e-16 absolutely; exp_tab_upto<710>, neg2_log_tab: 2 ulp): a power
// that overflows is +-inf as the definition's, a NaN draw (0 times inf) sorts as +inf, and a quantile that touches one is a
// distance of 1e30 (finite_or_big), as in the built-in g-and-k model.
// Outputs (sabc::emit, a forward run only): output i = the i-th smallest draw, n_outputs = GKQ_N_DRAWS.
#if !defined(GKQ_N_DRAWS) || !defined(GKQ_N_STATS)
#error "gk_quantiles.hip: GKQ_N_DRAWS and GKQ_N_STATS are defined by the model class in front of this text"
#endif
#if defined(GKQ_TEAM)
// The team-aware form (GandKQuantiles(..., team_lanes=)): the same draws, statistics and outputs through sabc::Sample<N, W>
// (csrc/team_sample.hpp) -- each of the W lanes that run the particle generates its own blocks of the stream, applies the
// quantile function to its own normals only and keeps the results; the team sorts them in registers, and every lane reads the
// same quantiles.  W = 1, or more than 32 values per lane: the sample every lane holds whole, as below.
template <int W>
__device__ void sabc_user_simulate_team(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  constexpr int N = GKQ_N_DRAWS;
  const double A = theta[0], B = theta[1], g = theta[2], k = theta[3], c = p[1];
  const auto draw = [&](const double z) {
    const double w = sabc::exp_tab_upto<710>(-0.5 * k * sabc::neg2_log_tab(fma(z, z, 1.0)));     // (1 + z^2)^k
    return A + B * (1.0 + c * sabc::tanh_abs_tab(g * z / 2.0)) * w * z;
  };
  sabc::Sample<N, W> x;
  x.fill_normals(rng, draw);
  x.sort();
#pragma unroll
  for (int j = 0; j < GKQ_N_STATS; ++j) rho[j] = sabc::finite_or_big(fabs(x.quantile(sabc::data_at(j, 0)) - sabc::data_at(j, 1)));
  x.emit(rng, 0);
}
#else
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  constexpr int N = GKQ_N_DRAWS;
  const double A = theta[0], B = theta[1], g = theta[2], k = theta[3], c = p[1];
  const auto draw = [&](const double z) {
    const double w = sabc::exp_tab_upto<710>(-0.5 * k * sabc::neg2_log_tab(fma(z, z, 1.0)));     // (1 + z^2)^k
    return A + B * (1.0 + c * sabc::tanh_abs_tab(g * z / 2.0)) * w * z;
  };
  double x[N];
  int at = 0;
  rng.for_pairs(N >> 1, [&](const double z0, const double z1) {
    x[at] = draw(z0);
    x[at + 1] = draw(z1);
    at += 2;
  });
  if (N & 1) {
    double z0, z1;
    rng.pair(z0, z1);
    x[N - 1] = draw(z0);
  }
  sabc::sort_ascending(x);
#pragma unroll
  for (int j = 0; j < GKQ_N_STATS; ++j) rho[j] = sabc::finite_or_big(fabs(sabc::quantile(x, N, sabc::data_at(j, 0)) - sabc::data_at(j, 1)));
  if (sabc::emitting(rng))
    for (int i = 0; i < N; ++i) sabc::emit(rng, i, x[i]);
}
#endif
