"""Host-side example models, written the way a user of the reference writes `f_dist` (plain Python / NumPy, no device
code): used by `bench.py --config host` and the tests of the host-callback path."""
from __future__ import annotations

import numpy as np


def gaussian_mean_batched(obs_mean, n_obs=100, seed=0):
    """BASELINE config 2's simulator as a vectorised NumPy callable: for every proposal theta the distance
    |mean(x) - mean(y_obs)| with x_1..n_obs ~ N(theta, 1), drawn through its sufficient statistic
    (mean(x) ~ N(theta, 1 / n_obs)).  `fn(Theta)` takes the m proposals at once (HostDistance(batched=True))."""
    rng = np.random.default_rng(seed)
    sd = 1.0 / np.sqrt(n_obs)

    def fn(theta):
        theta = np.asarray(theta, dtype=np.float64)
        return np.abs(theta + sd * rng.standard_normal(theta.shape[0]) - obs_mean)

    return fn


def sir_gillespie(seed=11, N=100, i0=5, t_max=30.0, n_grid=16):
    """The reference's documentation example (docs/src/example.md:75-173): a stochastic SIR epidemic simulated with
    Gillespie's algorithm, observed on a time grid.  Returns (simulate(beta, gamma) -> infected on the grid,
    f_dist(theta, data) -> root-mean-square distance)."""
    rng = np.random.default_rng(seed)
    grid = np.linspace(0.0, t_max, n_grid)

    def simulate(beta, gamma):
        s, i, t, k = N - i0, i0, 0.0, 0
        out = np.zeros(len(grid))
        while k < len(grid):
            rate_inf, rate_rec = beta * s * i / N, gamma * i
            total = rate_inf + rate_rec
            t_next = t + rng.exponential(1 / total) if total > 0 else np.inf
            while k < len(grid) and grid[k] < t_next:
                out[k] = i
                k += 1
            if not np.isfinite(t_next):
                break
            t = t_next
            if rng.random() < rate_inf / total:
                s, i = s - 1, i + 1
            else:
                i -= 1
        return out

    def f_dist(theta, data):
        return float(np.sqrt(np.mean((simulate(theta[0], theta[1]) - data) ** 2)))

    return simulate, f_dist


def sir_series_observation(theta=(0.3, 0.1), t_obs=None, S0=99, I0=1, R0=0, t_max=160.0, seed=123):
    """An observation for `StochasticSIRSeries`: one Gillespie run at theta = (beta, gamma) with NumPy's generator, observed at
    the increasing times `t_obs` (default: 0, 5, ..., 155) the way device_sources/sir_series.hip observes a simulation -- I(t_k)
    is the number infected just before the first event later than t_k, the final number once no event follows.
    Returns (t_obs, I_obs) as float64 arrays."""
    rng = np.random.default_rng(seed)
    t_obs = np.arange(0.0, 160.0, 5.0) if t_obs is None else np.asarray(t_obs, dtype=np.float64).reshape(-1)
    beta, gamma = float(theta[0]), float(theta[1])
    N = S0 + I0 + R0
    S, I, t, k = int(S0), int(I0), 0.0, 0
    I_obs = np.empty(len(t_obs))
    while t < t_max and I > 0:
        infection_rate, recovery_rate = beta * S * I / N, gamma * I
        total_rate = infection_rate + recovery_rate
        if not total_rate > 0.0:
            break
        t += rng.exponential(1.0 / total_rate)
        while k < len(t_obs) and t_obs[k] < t:
            I_obs[k] = I
            k += 1
        if rng.random() < infection_rate / total_rate:
            S, I = S - 1, I + 1
        else:
            I -= 1
    I_obs[k:] = I
    return t_obs, I_obs


def sir_observation(theta=(0.3, 0.1), S0=99, I0=1, R0=0, t_max=160.0, seed=123):
    """An observation for `StochasticSIR` made the way the reference's documentation makes one (docs/src/example.md:75-148):
    one Gillespie run at theta = (beta, gamma) with NumPy's generator, summarised as
    dict(total_infected, peak_infected, t_peak).  (The seed decides whether the epidemic takes off at all.)"""
    rng = np.random.default_rng(seed)
    beta, gamma = float(theta[0]), float(theta[1])
    N = S0 + I0 + R0
    S, I, R, t = int(S0), int(I0), int(R0), 0.0
    peak, t_peak = I, 0.0
    while t < t_max and I > 0:
        infection_rate, recovery_rate = beta * S * I / N, gamma * I
        total_rate = infection_rate + recovery_rate
        if not total_rate > 0.0:
            break
        t += rng.exponential(1.0 / total_rate)
        if rng.random() < infection_rate / total_rate:
            S, I = S - 1, I + 1
        else:
            I, R = I - 1, R + 1
        if I > peak:
            peak, t_peak = I, t
    return dict(total_infected=float(R), peak_infected=float(peak), t_peak=float(t_peak))
