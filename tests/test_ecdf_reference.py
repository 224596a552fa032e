"""The NumPy ECDF reference of tests/ecdf_ref.py against the oracle, the tables it generates, and proof that its checkers tell a
right lookup from a wrong one.  CPU only: the device side is tests/test_gpu_ecdf_paths.py."""
import numpy as np
import pytest

from tests import ecdf_ref as E

N_BIG = 40_001                 # the population the device tests reach every regime at
REGIMES = ("lds", "block", "mid")
PATTERNS = ("runs", "dominant", "spread")


def discrete_pool(rng, m=5000, q=64):
    """Distances of a count-like simulator: |N(0.8, 1)| on the grid of 1/q, zeros included."""
    return np.floor(np.abs(rng.normal(0.8, 1.0, m)) * q) / q


def tables(s, n=N_BIG):
    rng = np.random.default_rng(11 + s)
    pool = discrete_pool(rng)
    out = []
    for reg in REGIMES:
        L = E.regime_length(reg, s, n)
        if L is None:
            continue
        for pat in PATTERNS:
            out.append((reg, pat, E.make_table(L, pool, 64, pat, rng)))
    return out


@pytest.mark.parametrize("seed", range(4))
def test_build_cdf_ref_is_the_oracle_bit_for_bit(O, seed):
    rng = np.random.default_rng(seed)
    x = np.concatenate([discrete_pool(rng, 3000), rng.exponential(1.0, 500), [0.0] * 40, -rng.random(7)])
    x = rng.permutation(x)
    if seed == 3:
        x = np.abs(x)                                  # no zeros at all: nothing dropped
    np.testing.assert_array_equal(E.build_cdf_ref(x), O.build_cdf(x))
    with pytest.raises(ValueError):
        E.build_cdf_ref([0.0, -1.0])


@pytest.mark.parametrize("s", [1, 3, 12])
def test_cdf_ref_is_the_oracle_on_the_generated_tables(O, s):
    for reg, pat, T in tables(s, n=4001 if s > 1 else N_BIG)[::2]:
        q = E.probes(T)
        q = np.concatenate([q[:: max(1, len(q) // 4000)], [np.nan]])
        got, want = E.cdf_ref(T, q), O.cdf_apply(T, q)
        assert np.isnan(got[-1]) and np.isnan(want[-1])
        np.testing.assert_allclose(got[:-1], want[:-1], rtol=0, atol=E.U_TOL, err_msg=f"{reg}/{pat}")


def test_cdf_ref_edges():
    T = np.array([0.0, 0.5, 0.5, 0.5, 1.0, 1.5])
    u = E.cdf_ref(T, np.array([-1.0, 0.0, 0.25, 0.5, 0.75, 1.5, 2.0, np.inf, -np.inf, np.nan]))
    np.testing.assert_array_equal(u[:8], [0.0, 0.0, 0.1, 0.2, 0.7, 1.0, 1.0, 1.0])
    assert u[8] == 0.0 and np.isnan(u[9])
    # the first knot of a run: the rank counts the knots strictly below (F's left limit at the jump)
    assert E.cdf_ref(T, np.array([0.5]), side="right")[0] == pytest.approx(0.6)


@pytest.mark.parametrize("s", [1, 2, 8, 9, 12, 48])
def test_each_regime_reaches_its_shift(s):
    """The lengths follow build_coarse with the coarse sizes of kernels.hpp: retuning them moves the tables too."""
    nc = E.coarse_entries(s)
    assert nc in (E.coarse_sizes()[0], E.coarse_sizes()[1], E.coarse_sizes()[1] // 2)
    for v in range(4):
        assert E.shift_of(E.regime_length("lds", s, N_BIG, v), s) == 0
        assert 1 <= E.shift_of(E.regime_length("block", s, N_BIG, v), s) <= 4
        assert E.shift_of(E.regime_length("mid", s, N_BIG, v), s) >= 5
    assert {E.shift_of(E.regime_length("block", s, N_BIG, v), s) for v in range(4)} == {1, 2, 3, 4}
    assert all(E.regime_length(r, s, N_BIG, v) <= E.knot_stride(N_BIG) for r in REGIMES for v in range(4))
    assert E.regime_length("mid", s, 2001) is None                 # a small handle cannot hold a mid-level table


@pytest.mark.parametrize("s", [1, 3, 12])
def test_the_tables_have_runs_across_every_boundary(s):
    for reg, pat, T in tables(s):
        assert np.all(np.diff(T) >= 0) and T[0] == 0.0 and T[-1] == 1.5 * T[-2]
        assert np.all(T[1:-1] * 2.0 ** 20 == np.round(T[1:-1] * 2.0 ** 20))          # on a power-of-two grid
        runs = E.run_lengths(T)
        if pat == "spread":
            assert runs.max() == 2 and np.mean(runs[1:-1] == 1) > 0.5, (reg, runs.max())
            continue
        sh = E.shift_of(len(T), s)
        for period in {E.LINE, 1 << sh} - {1}:                      # lines / mid entries, coarse entries
            across, starting = E.runs_across(T, period)
            assert across > 0, (reg, pat, period)
        if pat == "dominant":
            assert runs.max() >= 0.75 * (len(T) - 2)


@pytest.mark.parametrize("s", [1, 3, 12])
def test_the_checker_refuses_a_wrong_rank_on_every_table(s):
    """On every regime and pattern: the last-duplicate convention (<= in the search) and a rank off by one are caught, on the
    probes of the table and on a discrete simulator's distances alike.  The right lookup passes."""
    rng = np.random.default_rng(5)
    for reg, pat, T in tables(s):
        rho = discrete_pool(rng, 20_000)
        for q, what in ((E.probes(T), "probes"), (rho, "rho")):
            assert len(E.u_mismatch(T, q, E.cdf_ref(T, q))) == 0
            assert len(E.u_mismatch(T, q, E.cdf_ref(T, q) + 0.5 * E.U_TOL)) == 0
            assert len(E.u_mismatch(T, q, E.cdf_ref(T, q, side="right"))) > 0, (reg, pat, what, "<=")
            for d in (-1, 1):
                assert len(E.u_mismatch(T, q, E.cdf_ref(T, q, rank_shift=d))) > 0, (reg, pat, what, d)
            u = E.cdf_ref(T, q)
            u[len(u) // 2] = np.nan                                 # a NaN where the reference has none
            assert len(E.u_mismatch(T, q, u)) == 1


@pytest.mark.parametrize("n", [130, 2001, 16_001, 40_001, 400_003])
def test_the_sums_checker_refuses_a_dropped_block(n):
    """A reduction that lost one block of 64 particles -- the first, one inside, or the ragged tail -- is caught at every size
    the device tests use, for u (rel 1e-12) and rho (rel 1e-10)."""
    rng = np.random.default_rng(n)
    u = rng.random((3, n))
    rho = np.floor(np.abs(rng.normal(0.8, 1.0, (3, n))) * 64) / 64
    mu = np.array([E.fsum_mean(r) for r in u])
    assert len(E.mean_mismatch(mu, u, 1e-12)) == 0
    nb = (n + 63) // 64
    for b in sorted({0, nb // 2, nb - 1}):
        assert len(E.mean_mismatch(E.drop_block(u, b), u, 1e-12)) == 3, b
        assert len(E.mean_mismatch(E.drop_block(rho, b), rho, 1e-10)) >= 2, b


def test_cov_ref_is_the_oracle_formula():
    rng = np.random.default_rng(3)
    th = 1e6 + 1e-2 * rng.random((3, 5000))
    c = E.cov_ref(th, 0.8)
    want = 0.8 * (np.cov(th - 1e6) + 1e-8 * np.eye(3))       # shifted exactly (1e6 is a float): the same covariance
    np.testing.assert_allclose(np.asarray(c, dtype=np.float64), want, rtol=1e-12)
    one = E.cov_ref(th[:1], 0.8)
    assert one.shape == (1, 1) and float(one[0, 0]) == pytest.approx(0.8 * np.var(th[0] - 1e6, ddof=1), rel=1e-12)
