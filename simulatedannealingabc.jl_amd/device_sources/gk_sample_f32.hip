// gk_sample.hip's team-aware form on a binary32 sample: x = A + B (1 + c tanh(g z / 2)) (1 + z^2)^k z with z one of the stream's
// binary32 normals (four per Philox block, |z| <= 6.7637), GKS_N_DRAWS draws, kept and sorted as floats in sabc::SampleF32<N, W>
// (csrc/team_sample_f32.hpp), against data segment 0 = the observed sample y, ascending doubles (the class sorts it and checks it
// wherever data enter; the source checks no index):
//     wasserstein: rho = sum_i |x_(i) - y_i| / N                     (len(y) == N; the canonical sum of csrc/sample_reduce.hpp, in f64)
//     ks:          rho = sup_t |F_x(t) - F_y(t)|                     (any len(y) >= 1; sabc::count_less / count_less_equal)
// theta = (A, B, g, k); params = [n_draws, c].  The class prepends  #define GKS_N_DRAWS <N>  and, for each distance it was asked
// for, the index of its statistic:  #define GKS_WASSERSTEIN <j>,  #define GKS_KS <j>  (one or both; n_stats = how many).
// The transform is gk_sample.hip's, in f64 on the normal widened to double (exact), and its result is rounded to binary32 ONCE:
// what is binary32 here is the noise and the sample, not the arithmetic between them.  Every lane of the team draws, transforms
// and keeps its own share; teams of 1, 4 and 16 lanes give the same bits.  A NaN draw (0 times inf) sorts as +inf, and a distance
// that touches an infinity is 1e30 (finite_or_big).  Outputs (sabc::emit, a forward run only): output i = the i-th smallest draw,
// a binary32 value written as a double, n_outputs = GKS_N_DRAWS.
#if !defined(GKS_N_DRAWS) || !(defined(GKS_WASSERSTEIN) || defined(GKS_KS))
#error "gk_sample_f32.hip: GKS_N_DRAWS and GKS_WASSERSTEIN and / or GKS_KS are defined by the model class in front of this text"
#endif
template <int W>
__device__ void sabc_user_simulate_team(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  constexpr int N = GKS_N_DRAWS;
  const double A = theta[0], B = theta[1], g = theta[2], k = theta[3], c = p[1];
  const auto draw = [&](const float zf) {
    const double z = (double)zf;
    const double w = sabc::exp_tab_upto<710>(-0.5 * k * sabc::neg2_log_tab(fma(z, z, 1.0)));     // (1 + z^2)^k
    return (float)(A + B * (1.0 + c * sabc::tanh_abs_tab(g * z / 2.0)) * w * z);
  };
  sabc::SampleF32<N, W> x;
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
