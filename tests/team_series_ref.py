"""csrc/team_series.hpp restated in NumPy: lag, lagged_sum and autocovariance of sabc::Series<N, W> -- what every width and the
replicated store give, bit for bit (float64 additions and multiplications are IEEE in both; a product is rounded on its own
before it enters the tree) -- and device_sources/ma2.hip on top of them, its fmas through tests/elementary_ref.py."""
import numpy as np

from tests import elementary_ref as E
from tests.sample_reduce_ref import tree_sum


def lag(x, L, before=0.0):
    """Element t is x_{t-L} for t >= L, `before` for t < L.  Along the last axis."""
    x = np.asarray(x, dtype=np.float64)
    assert 1 <= L < x.shape[-1]
    out = np.full(x.shape, float(before))
    out[..., L:] = x[..., :-L]
    return out


def lagged_sum(x, L, g, first=0):
    """The canonical sum over t = 0 .. N-1 of g(t, x_t, x_{t-L}) for t >= first + L, +0.0 otherwise; g takes arrays."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    assert 0 <= L < n
    terms = np.zeros(x.shape)
    lo = first + L
    if lo < n:
        terms[..., lo:] = g(np.arange(lo, n), x[..., lo:], x[..., lo - L:n - L])
    return tree_sum(terms)


def autocovariance(x, L, center=0.0, first=0):
    """lagged_sum of (x_t - c)(x_{t-L} - c), each product one float64 multiplication, divided by N - first."""
    n = np.asarray(x).shape[-1]
    return lagged_sum(x, L, lambda t, a, b: (a - center) * (b - center), first) / float(n - first)


def ma2_series(theta, e, fma=E.fma):
    """y_t = fma(theta2, e_t, fma(theta1, e_{t+1}, e_{t+2})), t = 0 .. len(e) - 3, for ONE innovation sequence e."""
    t1, t2 = float(theta[0]), float(theta[1])
    e = [float(v) for v in e]
    return np.array([fma(t2, e[t], fma(t1, e[t + 1], e[t + 2])) for t in range(len(e) - 2)])


def ma2_summaries(y, n_lags):
    """tau_0 .. tau_n_lags as ma2.hip computes them: the series sits at the innovations' times, two leading positions that add
    +0.0 (first = 2), and the sum is divided by n_obs."""
    y = np.asarray(y, dtype=np.float64)
    held = np.concatenate([np.zeros(y.shape[:-1] + (2,)), y], axis=-1)
    return np.stack([autocovariance(held, j, 0.0, 2) for j in range(n_lags + 1)], axis=-1)
