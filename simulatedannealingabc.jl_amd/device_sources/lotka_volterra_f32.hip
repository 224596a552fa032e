// The stochastic Lotka-Volterra model of the built-in simulator (device_models.hpp: Sim<SABC_MODEL_LV>) with its noise, its
// state and its step in binary32: theta = (a, b, c), dX = (a X - b X Y) dt + sigma X dW1, dY = (b X Y - c Y) dt + sigma Y dW2
// by the same factored Euler-Maruyama step, both species from the old state, and the same four statistics -- mean and
// standard deviation of each path -- as absolute differences to the observed ones.
//   params = (n_steps, dt, sigma, x0, y0, obs[0..3]); LV_N_STATS (1..4, #defined in front of this text) statistics are returned
// Two steps come from each Philox block (NormalStream::for_quads_f32: four binary32 normals per block, half the generator's
// instructions per normal of the f64 loop).  The running sums are sums of DEVIATIONS from the initial state -- of the order of
// the path's spread, not of its level, so 256 of them keep six digits in binary32 -- and the statistics are formed from them in
// double at the end; theta, params and rho stay double.  Every operation is an explicit fma, product or sum, so
// tests/elementary_f32_ref.py restates a run bit for bit.  Outputs (sabc::emit): the two paths, X at 0..n_steps-1, Y behind it.
#ifndef LV_N_STATS
#define LV_N_STATS 4
#endif

__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const int n_steps = (int)p[0];
  const float dt = (float)p[1], sdt = (float)(p[2] * sqrt(p[1]));
  const float a = (float)theta[0], b = (float)theta[1], c = (float)theta[2];
  const float X0 = (float)p[3], Y0 = (float)p[4];
  float X = X0, Y = Y0, SX = 0.f, QX = 0.f, SY = 0.f, QY = 0.f;
  int step = 0;
  auto advance = [&](const float z1, const float z2) {
    const float fx = fmaf(sdt, z1, fmaf(-b, Y, a) * dt);
    const float fy = fmaf(sdt, z2, fmaf(b, X, -c) * dt);
    X = fmaxf(fmaf(X, fx, X), 0.f);
    Y = fmaxf(fmaf(Y, fy, Y), 0.f);
    const float dx = X - X0, dy = Y - Y0;
    SX += dx;
    QX = fmaf(dx, dx, QX);
    SY += dy;
    QY = fmaf(dy, dy, QY);
    if (sabc::emitting(rng)) {
      sabc::emit(rng, step, (double)X);
      sabc::emit(rng, n_steps + step, (double)Y);
    }
    ++step;
  };
  rng.for_quads_f32(n_steps / 2, [&](const float z0, const float z1, const float z2, const float z3) {
    advance(z0, z1);
    advance(z2, z3);
  });
  if (n_steps & 1) {                      // an odd step takes the first pair of one more block
    float z0, z1, z2, z3;
    rng.quad_f32(z0, z1, z2, z3);
    advance(z0, z1);
  }
  const double n = (double)n_steps;
  const double mdX = (double)SX / n, mdY = (double)SY / n;               // mean deviation
  const double vX = fma(-(double)SX, mdX, (double)QX) / (n - 1.0), vY = fma(-(double)SY, mdY, (double)QY) / (n - 1.0);
  const double st[4] = {(double)X0 + mdX, sqrt(fmax(vX, 0.0)), (double)Y0 + mdY, sqrt(fmax(vY, 0.0))};
  for (int j = 0; j < LV_N_STATS; ++j) {
    const double d = fabs(st[j] - p[5 + j]);
    rho[j] = d < 1e300 ? d : 1e300;       // NaN and inf (a path that blew up) count as far away
  }
}
