// The Gillespie epidemic of sir.hip (docs/src/example.md:75-173 of the reference), compared with a whole observed curve
// instead of three summaries.  theta = (beta, gamma); params = [S0, I0, R0, t_max]; the observation is the handle's data
// (sabc_set_device_data): segment 0 = t_obs, increasing, segment 1 = I_obs, as many values.
// One statistic: the mean over k of |I(t_k) - I_obs[k]|, I(t_k) being the number infected just before the first event later
// than t_k, and the final number for every t_k no event comes after.  Event j of a simulation is block j of the particle's
// simulation stream, exactly as in sir.hip; the curve is compared on the fly, nothing of it is stored.
// Outputs (sabc::emit, a forward run only): output k = I(t_k), one per observation time.
// The observation index differs from particle to particle: these reads are vector loads (the data sit in L2 after the first).
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const double beta = theta[0], gamma = theta[1];
  const int S0 = (int)p[0], I0 = (int)p[1], R0 = (int)p[2];
  const double t_max = p[3];
  const double N = (double)(S0 + I0 + R0);
  const long long K = sabc::data_len(0);
  int S = S0, I = I0;
  double t = 0.0, acc = 0.0;
  long long k = 0;
  if (t < t_max && I > 0) {
    rng.while_events(2 * S0 + I0, [&](const double e, const double u) {
      const double infection_rate = beta * (double)S * (double)I / N;
      const double recovery_rate = gamma * (double)I;
      const double total_rate = infection_rate + recovery_rate;
      if (!(total_rate > 0.0)) return false;
      t += e / total_rate;
      while (k < K && sabc::data_at(k, 0) < t) {     // observation times this event is the first to lie after
        acc += fabs((double)I - sabc::data_at(k, 1));
        sabc::emit(rng, k, (double)I);
        ++k;
      }
      if (u < infection_rate / total_rate) {
        S -= 1;
        I += 1;
      } else {
        I -= 1;
      }
      return t < t_max && I > 0;
    });
  }
  for (; k < K; ++k) {
    acc += fabs((double)I - sabc::data_at(k, 1));
    sabc::emit(rng, k, (double)I);
  }
  rho[0] = acc / (double)K;
}
