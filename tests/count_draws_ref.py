"""sabc::CountDraws (csrc/device_rng.hpp) -- count draws keyed by an index -- and device_sources/ricker.hip, restated in Python.

CountDraws(O, seed, pid, it, purpose, base): draw index i owns blocks base + 64 i .. base + 64 i + 63 of the stream (seed, pid,
purpose, it); trial j of a draw reads block base + 64 i + j and takes the uniforms uniform_pair() would return for it.  The
algorithms are tests/discrete_draws_ref.py's (NormalStream::poisson / binomial, constant for constant), written here over the
functions a draw calls, so that they run with the device's own elementary functions -- tests/elementary_ref.py's exp_tab,
log_fast, log_factorial, u52 (FUNCTIONS_TABLE, the default) -- or with math.exp / math.log / math.lgamma as discrete_draws_ref.py
has them (FUNCTIONS_MATH): with those, CountDraws.poisson(i, lam) IS discrete_draws_ref.Stream(k = base + 64 i).poisson(lam),
which tests/test_count_draws.py asserts.  The degenerate arguments are the header's: lam NaN or <= 0 gives 0, lam > 2^30 counts
as 2^30, n_trials is clamped to [0, 2^30] (a NaN to 0), p NaN or <= 0 gives 0, p >= 1 the clamped n_trials -- none computes a block
(`blocks` counts every block a draw computed).

What is NOT restated: the run-time compiler may contract a product into the addition behind it (b = 0.931 + 2.53 sqrt(lam),
c += p in the inversion), and log_fast / log_factorial start from the device's reciprocal seed.  Either moves a compared value
in its last place; a count changes only where a uniform falls within that last place of a threshold, a chance of about 1e-15
per comparison.  The tests hold the counts to this file exactly.

The Ricker transcription: the latent state by the sequential loop with E.exp_tab and a product rounded on its own, the counts
keyed by the time step behind the normals' blocks, the summaries through tree_sum / team_series_ref.autocovariance."""
import math

import numpy as np

from tests import elementary_ref as E
from tests import team_series_ref as T
from tests.sample_reduce_ref import tree_sum

COUNT_BLOCKS = 64
MAX_COUNT = 2.0 ** 30
MAX_COUNT_DRAWS = 1 << 20

FUNCTIONS_TABLE = dict(exp=E.exp_tab, log=E.log_fast, log_factorial=E.log_factorial)
FUNCTIONS_MATH = dict(exp=math.exp, log=math.log, log_factorial=lambda k: math.lgamma(k + 1.0))


def poisson_from(lam, nxt, exp, log, log_factorial):
    """count::poisson_from: 0 < lam <= 2^30, nxt() -> (u, v) the uniforms of the next trial's block."""
    if lam < 10.0:
        u, _ = nxt()
        p = exp(-lam)
        c, k = p, 0
        while u >= c and k < 1000:
            k += 1
            p *= lam / k
            c += p
        return k
    b = 0.931 + 2.53 * math.sqrt(lam)
    a = -0.059 + 0.02483 * b
    inv_alpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    log_lam, log_inv_alpha = log(lam), log(inv_alpha)
    for _ in range(COUNT_BLOCKS):
        u, v = nxt()
        U = u - 0.5
        us = 0.5 - abs(U)
        k = math.floor((2.0 * a / us + b) * U + lam + 0.43)
        if us >= 0.07 and v <= vr:
            return k
        if k < 0 or (us < 0.013 and v > us):
            continue
        if log(v) + log_inv_alpha - log(a / (us * us) + b) <= -lam + k * log_lam - log_factorial(float(k)):
            return k
    return math.floor(lam)


def binomial_lower_from(n, p, nxt, exp, log, log_factorial):
    """count::binomial_lower_from: n >= 1, 0 < p <= 1/2."""
    q = 1.0 - p
    r = p / q
    nd = float(n)
    if nd * p < 10.0:
        u, _ = nxt()
        pk = exp(nd * log(q))
        c, k = pk, 0
        while u >= c and k < n and k < 1000:
            k += 1
            pk *= r * float(n - k + 1) / float(k)
            c += pk
        return k
    spq = math.sqrt(nd * p * q)
    b = 1.15 + 2.53 * spq
    a = -0.0873 + 0.0248 * b + 0.01 * p
    c = nd * p + 0.5
    vr = 0.92 - 4.2 / b
    alpha = (2.83 + 5.1 / b) * spq
    m = math.floor((nd + 1.0) * p)
    log_r = log(r)
    for _ in range(COUNT_BLOCKS):
        u, v = nxt()
        U = u - 0.5
        us = 0.5 - abs(U)
        k = math.floor((2.0 * a / us + b) * U + c)
        if us >= 0.07 and v <= vr:
            return k
        if k < 0 or k > n:
            continue
        lf = log_factorial(float(m)) + log_factorial(nd - m) - log_factorial(float(k)) - log_factorial(nd - k)
        if log(v * alpha / (a / (us * us) + b)) <= lf + (k - m) * log_r:
            return k
    return m


class CountDraws:
    """NormalStream::reserve_counts's handle on (seed, pid, purpose, it) from block `base`.  `blocks`: the blocks computed so
    far, as (index, trial) pairs."""

    def __init__(self, O, seed, pid, it, purpose=None, base=0, functions=None):
        self.O, self.seed, self.pid, self.it, self.base = O, int(seed), int(pid), int(it), int(base)
        self.purpose = O.PURPOSE_SIM if purpose is None else purpose
        self.functions = FUNCTIONS_TABLE if functions is None else functions
        self.blocks = []

    def block_of(self, i, trial):
        return (self.base + COUNT_BLOCKS * int(i) + trial) & 0xFFFFFFFF

    def trials(self, i):
        at = [0]

        def nxt():
            w = self.O.stream_block(self.seed, self.pid, self.purpose, self.it, self.block_of(i, at[0]))
            self.blocks.append((int(i), at[0]))
            at[0] += 1
            return E.u52(int(w[0]), int(w[1])), E.u52(int(w[2]), int(w[3]))
        return nxt

    def poisson(self, i, lam):
        lam = float(lam)
        if not lam > 0.0:                                # NaN, 0, negative
            return 0
        return int(poisson_from(min(lam, MAX_COUNT), self.trials(i), **self.functions))

    def binomial(self, i, n_trials, p):
        n_trials, p = float(n_trials), float(p)
        n = 0 if math.isnan(n_trials) else int(min(max(n_trials, 0.0), MAX_COUNT))
        if n <= 0 or not p > 0.0:
            return 0
        if p >= 1.0:
            return n
        if p > 0.5:
            return n - int(binomial_lower_from(n, 1.0 - p, self.trials(i), **self.functions))
        return int(binomial_lower_from(n, p, self.trials(i), **self.functions))


def reserve_counts(O, seed, pid, it, purpose, k, n, functions=None):
    """(the handle, the stream's counter behind the reservation): k advances by 64 n, n clamped to [0, 2^20]."""
    n = min(max(int(n), 0), MAX_COUNT_DRAWS)
    return CountDraws(O, seed, pid, it, purpose, k, functions), (int(k) + COUNT_BLOCKS * n) & 0xFFFFFFFF


# ---------------------------------------------------------------- device_sources/ricker.hip
def ricker_latent(theta, z, n0):
    """N_1 .. N_N for ONE sequence of normals z: e_t = sigma z_t; g = exp_tab((log r - s) + e_t); s = s g, from s = n0."""
    logr, sigma = float(theta[0]), float(theta[1])
    s, out = float(n0), []
    for v in z:
        e = sigma * float(v)
        g = E.exp_tab((logr - s) + e)
        s = s * g
        out.append(s)
    return np.array(out, dtype=np.float64)


def ricker_counts(cd, phi, latent):
    """y_t = cd.poisson(t, phi N_{t+1}), the product one float64 multiplication: Series::map_poisson(rng, phi)."""
    phi = float(phi)
    return np.array([cd.poisson(t, phi * float(v)) for t, v in enumerate(latent)], dtype=np.float64)


def ricker_summaries_of_series(y_all, n_lags, burn_in):
    """mean, number of zeros and autocovariances about the mean at lags 0 .. n_lags over the times t >= burn_in of the WHOLE
    series y_all [..., burn_in + n_obs], as ricker.hip computes them: the canonical sums over all times, +0.0 before burn_in."""
    y = np.asarray(y_all, dtype=np.float64)
    n_obs = y.shape[-1] - burn_in
    flat = y.reshape(-1, y.shape[-1])
    out = []
    for row in flat:
        live = np.arange(len(row)) >= burn_in
        mean = float(tree_sum(np.where(live, row, 0.0))) / float(n_obs)
        zeros = float(tree_sum(np.where(live & (row == 0.0), 1.0, 0.0)))
        out.append([mean, zeros] + [float(T.autocovariance(row, j, mean, burn_in)) for j in range(n_lags + 1)])
    return np.array(out, dtype=np.float64).reshape(y.shape[:-1] + (n_lags + 3,))


def ricker_summaries(y_obs, n_lags, burn_in):
    """... of the observed counts alone [..., n_obs]: they sit behind burn_in times that add +0.0 (any values there do: those
    terms are not read)."""
    y = np.asarray(y_obs, dtype=np.float64)
    return ricker_summaries_of_series(np.concatenate([np.zeros(y.shape[:-1] + (int(burn_in),)), y], axis=-1), n_lags, burn_in)


def ricker_simulation(O, seed, pid, it, purpose, theta, n_obs, burn_in, n0, normals=None):
    """One run of ricker.hip on the stream (seed, pid, purpose, it): (latent N_1 .. N_N, counts y_0 .. y_{N-1}).  The normals
    are blocks 0 .. ceil(N / 2) - 1, the counts' reservation starts behind.  The normals are the device's BIT FOR BIT -- the
    Python transcription of the table-driven Box-Muller pair (tests/test_f32_draws.f64_pair), or `normals` where the caller has
    them --, not the oracle's O.normal_pair, which agrees with the device to 1e-9 only: at log r above 2.7 the map is chaotic, a
    last-place difference in one normal grows to another trajectory within a few steps, and the counts are discrete."""
    n = burn_in + n_obs
    blocks = (n + 1) // 2
    if normals is None:
        from tests.test_f32_draws import f64_pair
        normals = np.array([f64_pair(O.stream_block(seed, pid, purpose, it, b)) for b in range(blocks)]).reshape(-1)[:n]
    latent = ricker_latent(theta, normals, n0)
    cd, _ = reserve_counts(O, seed, pid, it, purpose, blocks, n)
    return latent, ricker_counts(cd, theta[2], latent)


def finite_or_big(v):
    return np.where(np.isfinite(v), v, 1e30)


def ricker_distances(y_all, obs, n_lags, burn_in):
    return finite_or_big(np.abs(ricker_summaries_of_series(y_all, n_lags, burn_in) - np.asarray(obs, dtype=np.float64)))
