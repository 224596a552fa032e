"""csrc/sample_reduce.hpp restated in NumPy: the canonical sum, the counts in a sorted sample and the Kolmogorov-Smirnov
distance -- what sabc::tree_sum, sabc::count_less / count_less_equal and sabc::Sample<N, W>::sum / wasserstein1 / ks give, bit
for bit (float64 additions are IEEE in both; the KS numerators are integers)."""
import numpy as np


def tree_sum(s):
    """The balanced binary tree over the index, low bits first: pad with +0.0 to a power of two, add neighbours level by
    level; + 0.0 last (a sum that is a zero is +0.0).  Along the last axis."""
    a = np.asarray(s, dtype=np.float64)
    n = a.shape[-1]
    p = 1
    while p < n:
        p *= 2
    a = np.concatenate([a, np.zeros(a.shape[:-1] + (p - n,))], axis=-1)
    while a.shape[-1] > 1:
        a = a.reshape(a.shape[:-1] + (-1, 2))
        a = a[..., 0] + a[..., 1]
    return a[..., 0] + 0.0


def count_less(v, y_sorted):
    """#{j: y_j < v}, a NaN v as +inf"""
    return np.searchsorted(y_sorted, np.where(np.isnan(v), np.inf, v), side="left")


def count_less_equal(v, y_sorted):
    """#{j: y_j <= v}, a NaN v as +inf"""
    return np.searchsorted(y_sorted, np.where(np.isnan(v), np.inf, v), side="right")


def wasserstein1(x_sorted, y_sorted):
    x = np.asarray(x_sorted, dtype=np.float64)
    assert x.shape[-1] == len(y_sorted)
    return tree_sum(np.abs(x - y_sorted)) / float(x.shape[-1])


def ks(x_sorted, y_sorted):
    """max_i max(|(i + 1) m - c<=(x_(i)) n|, |i m - c<(x_(i)) n|) / (n m): integers, one maximum, one division.  Along the last
    axis of x_sorted."""
    x = np.asarray(x_sorted, dtype=np.float64)
    n, m = x.shape[-1], len(y_sorted)
    assert n * m < 2 ** 53
    i = np.arange(n, dtype=np.int64)
    right = np.abs((i + 1) * m - count_less_equal(x, y_sorted).astype(np.int64) * n)
    left = np.abs(i * m - count_less(x, y_sorted).astype(np.int64) * n)
    return np.maximum(right, left).max(axis=-1).astype(np.float64) / (float(n) * float(m))
