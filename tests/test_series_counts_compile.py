"""Count draws on a sabc::Series and the Ricker model through the compiler stage (hipRTC needs no device), the model class's
argument checks and its summaries against the restatement.

tests/series_counts/counts_probe.hip calls reserve_counts in both forms, cd.poisson and cd.binomial inside fill, a recurrence
whose f draws (recur_rolled, and recur itself at 3 and 45 values) and map_poisson from sabc_user_simulate_team<W>; it compiles as a
team-aware source, whose unit holds W = 1, 4 and 16, with one value, with three, spread for both widths (45, 128), and spread over
a row of 16 while replicated in a quad (129).  Ricker compiles through the model class in both forms and with every lag; the
sequential rng.poisson / rng.binomial keep compiling unchanged; a reservation of more than 2^20 indices is a compile error
with the header's own message."""
import os

import numpy as np
import pytest

from tests import count_draws_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = open(os.path.join(ROOT, "tests", "series_counts", "counts_probe.hip")).read()
PROBE_PARAMS = [5.0, 1.5]          # s0 of the branching process, map_poisson's scale


def probe_outputs(n):
    """what counts_probe.hip emits at length n: (a) n, (b) n, (c) 2, (d) n + 1, (e) n"""
    return 4 * n + 3


def probe_data(n):
    """The probe's three data segments at length n: the ramp of lambda -- 0, a negative value, NaN, 9.99, 10, 10.01, one above
    2^30, then values in (0, 10) and up to 3000 --, and (n_t, p_t) across the degenerate cases, inversion, BTRS and reflection."""
    lam = np.concatenate([[0.0, -1.5, np.nan, 9.99, 10.0, 10.01, 2.0 ** 31, 0.05, 3.7], np.geomspace(0.1, 9.9, 40), np.geomspace(10.5, 3000.0, 80)])
    trials = np.concatenate([[0.0, -3.0, np.nan, 7.0, 7.0, 7.0, 7.9, 2.0 ** 31, 40.0, 40.0, 40.0, 40.0], np.tile([40.0, 1000.0, 25.0, 1e6, 10.0], 21), np.full(12, 300.0)])
    prob = np.concatenate([[0.5, 0.5, 0.5, 0.0, np.nan, 1.0, 1.5, 0.25, 0.1, 0.4, 0.6, 0.9], np.linspace(0.002, 0.998, 105), np.linspace(-0.1, 1.1, 12)])
    assert len(lam) == len(trials) == len(prob) == 129
    return [lam[:n], trials[:n], prob[:n]]


def probe_model(S, n, lanes, head=""):
    return S.DeviceSource(f"#define PROBE_N {n}\n" + head + PROBE_SRC, 1, 1, PROBE_PARAMS, data=probe_data(n), n_outputs=probe_outputs(n),
                          team_lanes=lanes)


@pytest.mark.parametrize("n", [1, 3, 45, 128, 129])
def test_a_probe_that_draws_keyed_counts_compiles(S, n):
    # one unit holds sabc_user_simulate_team<1>, <4> and <16>: the width is no part of the text or of the compiler stage
    assert probe_model(S, n, 16).compile_check()


@pytest.mark.parametrize("n", [3, 45])
def test_a_draw_inside_the_unrolled_recur_compiles(S, n):
    assert probe_model(S, n, 4, "#define PROBE_PLAIN_RECUR 1\n").compile_check()


def test_ricker_compiles_in_both_forms(S):
    obs = [4.0, 12.0, 30.0, 5.0, -3.0]
    plain = S.Ricker(obs, n_obs=40, burn_in=5, n_lags=2)
    assert plain.source.startswith("#define RICKER_N_OBS 40\n#define RICKER_BURN_IN 5\n#define RICKER_N_LAGS 2\n// The Ricker map")
    assert (plain.n_stats, plain.n_para, plain.n_obs, plain.burn_in, plain.n_lags, plain.n0, plain.n_outputs, plain.data_names, plain.team_lanes) == \
        (5, (3,), 40, 5, 2, 1.0, 40, ("summaries_obs",), None)
    assert plain.params == [40.0, 5.0, 2.0, 1.0]
    np.testing.assert_array_equal(plain.data[0], obs)
    assert plain.compile_check()
    team = S.Ricker(obs, n_obs=40, burn_in=5, n_lags=2, n0=0.5, team_lanes=16)
    assert team.source.startswith("#define RICKER_N_OBS 40\n#define RICKER_BURN_IN 5\n#define RICKER_N_LAGS 2\n#define RICKER_TEAM 1\n// The Ricker map")
    assert team.params == [40.0, 5.0, 2.0, 0.5]
    assert team.compile_check()
    for lanes in (1, 4):
        other = S.Ricker(obs, n_obs=40, burn_in=5, n_lags=2, n0=0.5, team_lanes=lanes)
        assert other.source == team.source and other.team_lanes == lanes
    assert "sabc::Series<RICKER_N, W>" in plain.source and ".map_poisson(" in plain.source and ".recur(" in plain.source and "Ricker" in S.__all__
    defaults = S.Ricker()
    assert (defaults.n_obs, defaults.burn_in, defaults.n_lags, defaults.n_stats, defaults.n0, defaults.data, defaults.team_lanes) == (50, 50, 5, 8, 1.0, None, None)


def test_ricker_with_every_lag_compiles(S):
    # seven lags on a short series without a burn-in: lag 7 of 10 times crosses three lanes of a row of 16 (two slots per lane)
    assert S.Ricker(np.ones(10), n_obs=10, burn_in=0, n_lags=7, team_lanes=4).compile_check()


def test_the_sequential_count_draws_keep_compiling(S):
    from tests.test_discrete_draws import CHAIN_BINOMIAL_PARAMS, CHAIN_BINOMIAL_SRC
    assert S.DeviceSource(CHAIN_BINOMIAL_SRC, 2, 2, CHAIN_BINOMIAL_PARAMS).compile_check()
    src = """__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const int a = rng.poisson(theta[0]);
  const sabc::CountDraws cd = rng.reserve_counts(2);
  rho[0] = (double)(a + cd.poisson(0, theta[0]) + cd.binomial(1, 40, 0.3) + cd.binomial(1, p[0], 0.3) + rng.poisson(theta[0]) + rng.binomial(40, 0.3));
}
"""
    assert S.DeviceSource(src, 1, 1, [40.0]).compile_check()


def test_a_reservation_beyond_the_bound_is_a_compile_error(S):
    src = """__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const sabc::CountDraws cd = rng.reserve_counts<(1 << 20) + 1>();
  rho[0] = (double)cd.poisson(0, theta[0]);
}
"""
    with pytest.raises(S._lib.SABCError, match="0 <= n <= 2\\^20"):
        S.DeviceSource(src, 1, 1, []).compile_check()


def test_ricker_checks_its_arguments(S):
    for bad in (-1, 8, 2.5, True, "2"):
        with pytest.raises((ValueError, TypeError), match="n_lags|int"):
            S.Ricker(n_lags=bad)
    for bad in (0, 2, 1025, 4.5, True, "50"):
        with pytest.raises(ValueError, match="n_obs"):
            S.Ricker(n_obs=bad, n_lags=2)
    for bad in (-1, 2.5, True, "5", 1000):
        with pytest.raises(ValueError, match="burn_in"):
            S.Ricker(burn_in=bad)
    for bad in (0, 2, 8, 32, "4", True):
        with pytest.raises(ValueError, match="team_lanes"):
            S.Ricker(team_lanes=bad)
    for bad in (0.0, -1.0, np.nan, np.inf, True, "1"):
        with pytest.raises(ValueError, match="n0"):
            S.Ricker(n0=bad)
    with pytest.raises(ValueError, match="n_lags \\+ 3 = 5"):
        S.Ricker([1.0, 0.5, 0.1, 0.0], n_lags=2)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            S.Ricker([1.0, bad, 0.2, 0.1, 0.0], n_lags=2)
    model = S.Ricker([1.0, 0.5, 0.2, 0.1, 0.0], n_lags=2)
    model.bind_data((), {"summaries_obs": [2.0, 1.0, 0.1, 0.0, 0.3]})
    with pytest.raises(ValueError, match="n_lags \\+ 3"):
        model.bind_data(([2.0, 1.0, 0.1],), {})
    with pytest.raises(ValueError, match="finite"):
        model.bind_data(([2.0, np.nan, 0.1, 0.0, 0.0],), {})
    with pytest.raises(TypeError, match="summaries_obs"):
        model.bind_data((), {"y_obs": [1.0, 2.0, 3.0, 4.0, 5.0]})
    with pytest.raises(ValueError, match="burn_in"):
        S.Ricker.from_observations(np.arange(40.0), burn_in=-1)


def test_summaries_and_from_observations_use_the_restatements_bits(S):
    y = np.random.default_rng(5).poisson(6.0, size=40).astype(np.float64)
    y[[3, 17]] = 0.0
    model = S.Ricker.from_observations(y, burn_in=5, n_lags=2, team_lanes=4)
    assert (model.n_obs, model.burn_in, model.n_lags, model.n_stats, model.team_lanes) == (40, 5, 2, 5, 4)
    np.testing.assert_array_equal(model.data[0], C.ricker_summaries(y, 2, 5))
    assert model.data[0][0] == y.sum() / 40.0 and model.data[0][1] == (y == 0).sum() >= 2
    for burn_in in (0, 5, 50):
        np.testing.assert_array_equal(S.Ricker.summaries(y, 7, burn_in), C.ricker_summaries(y, 7, burn_in))
    many = np.random.default_rng(6).poisson(3.0, size=(5, 3, 50)).astype(np.float64)
    np.testing.assert_array_equal(S.Ricker.summaries(many, 5, 50), C.ricker_summaries(many, 5, 50))
    # the values are the textbook ones up to rounding
    d = y - y.mean()
    for j in range(3):
        assert abs(model.data[0][2 + j] - np.dot(d[j:], d[:40 - j]) / 40) <= 1e-12 * np.abs(d).max() ** 2
    assert S.Ricker.from_observations(y).n_stats == 8 and S.Ricker.from_observations(y).burn_in == 50
