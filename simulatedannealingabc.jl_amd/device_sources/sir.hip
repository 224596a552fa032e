// The stochastic SIR epidemic of the reference's documentation (docs/src/example.md:75-173), simulated with Gillespie's direct
// method on the device.  theta = (beta, gamma); params = [S0, I0, R0, t_max, obs_total, obs_peak, obs_t_peak].
// Event j of a simulation is block j of the particle's simulation stream: the waiting time from its first uniform, the choice
// between infection and recovery from its second (NormalStream::while_events).  Every event takes one from S or from I, so a
// run has at most 2 S0 + I0 events: the loop's bound is exact.
// SIR_N_STATS (defined in front of this text by the bindings): 3 = the squared differences of final R, peak I and the time of
// the peak to the observation, one distance each; 1 = their sum.
// Outputs (sabc::emit, a forward run only): 0 = final R (total_infected), 1 = peak I (peak_infected), 2 = t_peak.
#ifndef SIR_N_STATS
#define SIR_N_STATS 3
#endif

__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const double beta = theta[0], gamma = theta[1];
  const int S0 = (int)p[0], I0 = (int)p[1], R0 = (int)p[2];
  const double t_max = p[3];
  const double N = (double)(S0 + I0 + R0);
  int S = S0, I = I0, R = R0;
  double t = 0.0;
  int peak = I0;                                   // maximum(sim.I) and sim.time[argmax(sim.I)]: the first maximum wins
  double t_peak = 0.0;
  if (t < t_max && I > 0) {
    rng.while_events(2 * S0 + I0, [&](const double e, const double u) {
      const double infection_rate = beta * (double)S * (double)I / N;
      const double recovery_rate = gamma * (double)I;
      const double total_rate = infection_rate + recovery_rate;
      if (!(total_rate > 0.0)) return false;       // nothing can happen any more (its block is drawn and unused)
      t += e / total_rate;                         // rand(Exponential(1 / total_rate))
      if (u < infection_rate / total_rate) {
        S -= 1;
        I += 1;
      } else {
        I -= 1;
        R += 1;
      }
      if (I > peak) {
        peak = I;
        t_peak = t;
      }
      return t < t_max && I > 0;                   // the event that carried t past t_max is applied, as in the reference
    });
  }
  const double d0 = (double)R - p[4], d1 = (double)peak - p[5], d2 = t_peak - p[6];
#if SIR_N_STATS == 3
  rho[0] = d0 * d0;
  rho[1] = d1 * d1;
  rho[2] = d2 * d2;
#else
  rho[0] = d0 * d0 + d1 * d1 + d2 * d2;
#endif
  sabc::emit(rng, 0, (double)R);                   // outputs (a forward run only): total_infected, peak_infected, t_peak
  sabc::emit(rng, 1, (double)peak);
  sabc::emit(rng, 2, t_peak);
}
