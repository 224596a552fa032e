"""sabc::Series::recur, recur_with and cumsum (csrc/team_series.hpp) restated as the Python loop they are defined to be -- a state
carried from t = first upwards, one application of f per time step -- and device_sources/garch11.hip on top of it: the fmas
through tests/elementary_ref.fma, the products plain float64 multiplications (the device rounds them on their own:
series::rounded_product), the summaries through tests/team_series_ref.autocovariance and tests/sample_reduce_ref.tree_sum.
Every width of the team, the replicated store and this file give the same bits: there is no order of association to choose."""
import numpy as np

from tests import elementary_ref as E
from tests import team_series_ref as T
from tests.sample_reduce_ref import tree_sum


def recur(x, s0, f, first=0, other=None):
    """x_t <- f(t, s, x_t) -> (x_t, s) for t = first .. N-1 in time order along the last axis, every row from the state s0 (a float,
    or a tuple of floats for a Carry<K>); with `other`, f(t, s, x_t, other_t).  Elements t < first are left as they are.
    Returns (the series, the states behind t = N-1: [..., K] for a tuple, [...] for a float)."""
    x = np.array(x, dtype=np.float64)
    flat = x.reshape(-1, x.shape[-1])
    oth = None if other is None else np.broadcast_to(np.asarray(other, dtype=np.float64), x.shape).reshape(flat.shape)
    states = []
    for row in range(flat.shape[0]):
        s = s0
        for t in range(max(first, 0), flat.shape[1]):
            v, s = f(t, s, float(flat[row, t])) if oth is None else f(t, s, float(flat[row, t]), float(oth[row, t]))
            flat[row, t] = v
        states.append(s)
    return x, np.array(states, dtype=np.float64).reshape(x.shape[:-1] + ((len(s0),) if isinstance(s0, tuple) else ()))


def cumsum(x):
    """s = s + x_t from s = 0.0, in time order: one rounding per step."""
    def add(t, s, v):
        s = s + v
        return s, s
    return recur(x, 0.0, add)[0]


def ar2(phi1, phi2, fma=E.fma):
    """The AR(2) map of the probes: out = fma(phi1, s[0], fma(phi2, s[1], x)); the state becomes (out, s[0])."""
    def f(t, s, v):
        out = fma(phi1, s[0], fma(phi2, s[1], v))
        return out, (out, s[0])
    return f


def damped_exp(t, s, v, o):
    """The recur_with map of the probes: s = fma(0.5, s, x); out = exp_tab(0.25 s) o_t, the product rounded on its own."""
    s = E.fma(0.5, s, v)
    return E.exp_tab(0.25 * s) * o, s


def garch11_squared_returns(theta, z, sigma2_0, fma=E.fma):
    """r_t = y_t^2 for normals z [..., N]: zz = z z; r_t = s zz; s = fma(s, fma(alpha, zz, beta), omega), from s = sigma2_0."""
    omega, alpha, beta = (float(v) for v in theta)
    z = np.asarray(z, dtype=np.float64)
    out = np.empty(z.shape)
    for row, dst in zip(z.reshape(-1, z.shape[-1]).tolist(), out.reshape(-1, z.shape[-1])):
        s, r = float(sigma2_0), []
        for v in row:                                  # (recur with this map, written out: the oracle runs it per simulation)
            zz = v * v
            r.append(s * zz)
            s = fma(s, fma(alpha, zz, beta), omega)
        dst[:] = r
    return out


def garch11_summaries_of_squares(r, n_lags):
    """mean(r) and the autocovariances of r about it at lags 0 .. n_lags, as garch11.hip computes them: [..., n_lags + 2]."""
    r = np.asarray(r, dtype=np.float64)
    mean = tree_sum(r) / float(r.shape[-1])
    acov = [[T.autocovariance(row, j, float(c)) for j in range(n_lags + 1)] for row, c in zip(r.reshape(-1, r.shape[-1]), np.reshape(mean, -1))]
    return np.concatenate([np.reshape(mean, -1)[:, None], np.array(acov, dtype=np.float64).reshape(-1, n_lags + 1)], axis=1).reshape(r.shape[:-1] + (n_lags + 2,))


def garch11_summaries(y, n_lags):
    """... of a series of returns y: squared first, each square one float64 multiplication."""
    y = np.asarray(y, dtype=np.float64)
    return garch11_summaries_of_squares(y * y, n_lags)


def garch11_returns(r, z):
    """y_t = copysign(sqrt(r_t), z_t) with the correctly rounded sqrt (the device's sqrt_fast is held to 1 ulp of it)."""
    return np.copysign(np.sqrt(np.asarray(r, dtype=np.float64)), z)
