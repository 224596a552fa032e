// g-and-k compared with the observed sample itself: x = A + B (1 + c tanh(g z / 2)) (1 + z^2)^k z, z ~ N(0, 1), GKS_N_DRAWS draws,
// sorted, against data segment 0 = the observed sample y, ascending (the class sorts it and checks it wherever data enter; the
// source checks no index):
//     wasserstein: rho = sum_i |x_(i) - y_i| / N                     (len(y) == N; the canonical sum of csrc/sample_reduce.hpp)
//     ks:          rho = sup_t |F_x(t) - F_y(t)|                     (any len(y) >= 1; sabc::count_less / count_less_equal)
// theta = (A, B, g, k); params = [n_draws, c].  The class prepends  #define GKS_N_DRAWS <N>  and, for each distance it was asked
// for, the index of its statistic:  #define GKS_WASSERSTEIN <j>,  #define GKS_KS <j>  (one or both; n_stats = how many), and
// #define GKS_TEAM 1  for the team-aware form.  Both forms give the same bits: the sum is the same tree over the rank, the
// Kolmogorov-Smirnov numerators are integers.
// The draws are those of gk_quantiles.hip: the pairs of the particle's simulation stream in order, an odd last draw the first
// normal of one more block; a NaN draw (0 times inf) sorts as +inf, and a distance that touches an infinity is 1e30
// (finite_or_big).  Outputs (sabc::emit, a forward run only): output i = the i-th smallest draw, n_outputs = GKS_N_DRAWS.
#if !defined(GKS_N_DRAWS) || !(defined(GKS_WASSERSTEIN) || defined(GKS_KS))
#error "gk_sample.hip: GKS_N_DRAWS and GKS_WASSERSTEIN and / or GKS_KS are defined by the model class in front of this text"
#endif
#if defined(GKS_TEAM)
// GandKSample(..., team_lanes=): sabc::Sample<N, W> (csrc/team_sample.hpp) -- every lane of the team draws, transforms and keeps
// its own share of the sample, and after the sort compares its own M consecutive ranks with the M observations beside them.
template <int W>
__device__ void sabc_user_simulate_team(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  constexpr int N = GKS_N_DRAWS;
  const double A = theta[0], B = theta[1], g = theta[2], k = theta[3], c = p[1];
  const auto draw = [&](const double z) {
    const double w = sabc::exp_tab_upto<710>(-0.5 * k * sabc::neg2_log_tab(fma(z, z, 1.0)));     // (1 + z^2)^k
    return A + B * (1.0 + c * sabc::tanh_abs_tab(g * z / 2.0)) * w * z;
  };
  sabc::Sample<N, W> x;
  x.fill_normals(rng, draw);
  x.sort();
#if defined(GKS_WASSERSTEIN)
  rho[GKS_WASSERSTEIN] = sabc::finite_or_big(x.wasserstein1(0));
#endif
#if defined(GKS_KS)
  rho[GKS_KS] = sabc::finite_or_big(x.ks(0));
#endif
  x.emit(rng, 0);
}
#else
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  constexpr int N = GKS_N_DRAWS;
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
#if defined(GKS_WASSERSTEIN)
  rho[GKS_WASSERSTEIN] = sabc::finite_or_big(sabc::tree_sum(N, [&](const int i) { return fabs(x[i] - sabc::data_at(i, 0)); }) / (double)N);
#endif
#if defined(GKS_KS)
  {
    const long long m = sabc::data_len(0);
    double top = 0.0;
    for (int i = 0; i < N; ++i)
      top = fmax(top, sabc::reduce::ks_term(i, N, m, sabc::count_less(x[i], 0), sabc::count_less_equal(x[i], 0)));
    rho[GKS_KS] = sabc::finite_or_big(top / ((double)N * (double)m));
  }
#endif
  if (sabc::emitting(rng))
    for (int i = 0; i < N; ++i) sabc::emit(rng, i, x[i]);
}
#endif
