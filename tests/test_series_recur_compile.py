"""sabc::Series::recur and GARCH11 through the compiler stage (hipRTC needs no device), the model class's argument checks and the
restatement against itself.

tests/series_recur/recur_probe.hip calls cumsum, recur with a double and with a Carry<2> (first = 0 and 2) and recur_with from
sabc_user_simulate_team<W>; it compiles as a team-aware source, whose unit holds W = 1, 4 and 16, with one value, with three,
spread for both widths (45, 128), and spread over a row of 16 while replicated in a quad (129).  GARCH11 compiles through the
model class in both forms and with every lag; a Carry<5> is a compile error with the header's own message, not a crash; and
tests/series_recur_ref.py agrees with the direct definitions and with GARCH11.summaries."""
import os

import numpy as np
import pytest

from tests import series_recur_ref as R
from tests import team_series_ref as T
from tests.sample_reduce_ref import tree_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = open(os.path.join(ROOT, "tests", "series_recur", "recur_probe.hip")).read()
PHI = (0.6, -0.3)


def probe_outputs(n):
    """what recur_probe.hip emits at length n: the series, cumsum + 1, the AR(2) block (+ 2), its first = 2 twin where N > 2, and
    recur_with"""
    return n + (n + 1) + (n + 2) * (2 if n > 2 else 1) + n


@pytest.mark.parametrize("n", [1, 3, 45, 128, 129])
def test_a_probe_that_calls_every_recurrence_compiles(S, n):
    # one unit holds sabc_user_simulate_team<1>, <4> and <16>: the width is no part of the text or of the compiler stage
    assert S.DeviceSource(f"#define PROBE_N {n}\n" + PROBE_SRC, 1, 1, list(PHI), n_outputs=probe_outputs(n), team_lanes=16).compile_check()


def test_garch11_compiles_in_both_forms(S):
    obs = [1.2, 3.0, 0.7, 0.4]
    plain = S.GARCH11(obs, n_obs=45)
    assert plain.source.startswith("#define GARCH11_N_OBS 45\n#define GARCH11_N_LAGS 2\n// GARCH(1,1)")
    assert (plain.n_stats, plain.n_para, plain.n_obs, plain.n_lags, plain.sigma2_0, plain.n_outputs, plain.data_names, plain.team_lanes) == \
        (4, (3,), 45, 2, 1.0, 45, ("summaries_obs",), None)
    assert plain.params == [45.0, 2.0, 1.0]
    np.testing.assert_array_equal(plain.data[0], obs)
    assert plain.compile_check()
    team = S.GARCH11(obs, n_obs=45, sigma2_0=0.5, team_lanes=16)
    assert team.source.startswith("#define GARCH11_N_OBS 45\n#define GARCH11_N_LAGS 2\n#define GARCH11_TEAM 1\n// GARCH(1,1)")
    assert team.params == [45.0, 2.0, 0.5]
    assert team.compile_check()
    for lanes in (1, 4):
        other = S.GARCH11(obs, n_obs=45, team_lanes=lanes)
        assert other.source == team.source and other.team_lanes == lanes
    assert "sabc::Series<GARCH11_N_OBS, W>" in plain.source and ".recur(" in plain.source and "GARCH11" in S.__all__
    defaults = S.GARCH11()
    assert (defaults.n_obs, defaults.n_lags, defaults.n_stats, defaults.sigma2_0, defaults.data, defaults.team_lanes) == (100, 2, 4, 1.0, None, None)


def test_garch11_with_every_lag_compiles(S):
    # seven lags on a short series: lag 7 of 10 times crosses three lanes of a row of 16 (two slots per lane)
    assert S.GARCH11(np.ones(9), n_obs=10, n_lags=7, team_lanes=4).compile_check()


def test_garch11_checks_its_arguments(S):
    for bad in (-1, 8, 2.5, True, "2"):
        with pytest.raises((ValueError, TypeError), match="n_lags|int"):
            S.GARCH11(n_lags=bad)
    for bad in (0, 2, 1025, 4.5, True):
        with pytest.raises(ValueError, match="n_obs"):
            S.GARCH11(n_obs=bad, n_lags=2)
    for bad in (0, 2, 8, 32, "4", True):
        with pytest.raises(ValueError, match="team_lanes"):
            S.GARCH11(team_lanes=bad)
    for bad in (0.0, -1.0, np.nan, np.inf, True, "1"):
        with pytest.raises(ValueError, match="sigma2_0"):
            S.GARCH11(sigma2_0=bad)
    with pytest.raises(ValueError, match="n_lags \\+ 2 = 4"):
        S.GARCH11([1.0, 0.5, 0.1])
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            S.GARCH11([1.0, bad, 0.2, 0.1])
    model = S.GARCH11([1.0, 0.5, 0.2, 0.1])
    model.bind_data((), {"summaries_obs": [2.0, 1.0, 0.1, 0.0]})
    with pytest.raises(ValueError, match="n_lags \\+ 2"):
        model.bind_data(([2.0, 1.0, 0.1],), {})
    with pytest.raises(ValueError, match="finite"):
        model.bind_data(([2.0, np.nan, 0.1, 0.0],), {})
    with pytest.raises(TypeError, match="summaries_obs"):
        model.bind_data((), {"y_obs": [1.0, 2.0, 3.0, 4.0]})


def test_summaries_and_from_observations_use_the_restatements_bits(S):
    y = np.random.default_rng(5).normal(size=45) * 1.3
    model = S.GARCH11.from_observations(y, team_lanes=4)
    assert (model.n_obs, model.n_lags, model.n_stats, model.team_lanes) == (45, 2, 4, 4)
    np.testing.assert_array_equal(model.data[0], R.garch11_summaries(y, 2))
    assert model.sigma2_0 == model.data[0][0] == tree_sum(y * y) / 45.0
    np.testing.assert_array_equal(S.GARCH11.summaries(y, 7), R.garch11_summaries(y, 7))
    many = np.random.default_rng(6).normal(size=(5, 3, 100))
    np.testing.assert_array_equal(S.GARCH11.summaries(many, 2), R.garch11_summaries(many, 2))
    # the values are the textbook ones up to rounding
    r = y * y
    assert abs(model.data[0][0] - r.mean()) <= 45 * 2.0 ** -53 * r.sum()
    for j in range(3):
        d = r - r.mean()
        assert abs(model.data[0][1 + j] - np.dot(d[j:], d[:45 - j]) / 45) <= 1e-12 * np.abs(d).max() ** 2
    assert S.GARCH11.from_observations(y, n_lags=5).n_stats == 7


def test_the_restatement_against_the_direct_definitions():
    rng = np.random.default_rng(7)
    # small integers add exactly: the loop, np.cumsum and any other order agree
    for n in (1, 2, 3, 45, 128, 129):
        k = rng.integers(-50, 50, size=(4, n)).astype(np.float64)
        np.testing.assert_array_equal(R.cumsum(k), np.cumsum(k, axis=-1))
        x = rng.normal(size=(3, n))
        got = R.cumsum(x)
        for row in range(3):
            s = 0.0
            for t in range(n):
                s = s + float(x[row, t])
                assert got[row, t] == s
        # recur with a Carry<2>, first = 0 and 2: a hand loop
        for first in (0, 2):
            out, state = R.recur(x, (0.25, -0.5), R.ar2(0.6, -0.3), first)
            assert state.shape == (3, 2)
            for row in range(3):
                a, b = 0.25, -0.5
                for t in range(n):
                    if t < first:
                        assert out[row, t] == x[row, t]
                        continue
                    o = R.E.fma(0.6, a, R.E.fma(-0.3, b, float(x[row, t])))
                    a, b = o, a
                    assert out[row, t] == o
                assert (state[row, 0], state[row, 1]) == (a, b)
        # recur_with: the other series reaches f at its own time
        ramp = 0.125 * np.arange(n)
        out, state = R.recur(x, 1.5, R.damped_exp, other=ramp)
        s = 1.5
        for t in range(n):
            s = R.E.fma(0.5, s, float(x[0, t]))
            assert out[0, t] == R.E.exp_tab(0.25 * s) * ramp[t]
        assert state.shape == (3,) and state[0] == s
    # the input is left as it was
    x = rng.normal(size=(2, 9))
    before = x.copy()
    R.cumsum(x)
    np.testing.assert_array_equal(x, before)


def test_the_garch11_transcription_with_either_fma():
    from tests import elementary_ref as E
    z = np.random.default_rng(8).normal(size=45)
    theta = (0.2, 0.15, 0.7)
    r = R.garch11_squared_returns(theta, z, 0.9)
    np.testing.assert_array_equal(r, R.garch11_squared_returns(theta, z, 0.9, fma=E.fma_fraction))
    s, want = 0.9, []
    for v in z:
        want.append(s * v * v)
        s = theta[0] + theta[1] * (s * v * v) + theta[2] * s
    np.testing.assert_allclose(r, want, rtol=1e-12)                 # (the same model, rounded differently)
    y = R.garch11_returns(r, z)
    assert (np.sign(y) == np.sign(z)).all()
    np.testing.assert_allclose(y * y, r, rtol=4 * 2.0 ** -53)
    got = R.garch11_summaries_of_squares(r, 2)
    assert got.shape == (4,) and got[0] == tree_sum(r) / 45.0 and got[2] == T.autocovariance(r, 1, got[0])


def test_a_carry_of_five_is_a_compile_error(S):
    src = """template <int W>
__device__ void sabc_user_simulate_team(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  sabc::Series<8, W> x;
  x.fill([](const int t) { return (double)t; });
  sabc::series::Carry<5> s = x.recur(sabc::series::Carry<5>{}, [](const int, sabc::series::Carry<5> &c, const double v) { c.v[0] += v; return v; });
  rho[0] = s.v[0] + theta[0];
}
"""
    with pytest.raises(S._lib.SABCError, match="a Carry holds 1 to 4 doubles"):
        S.DeviceSource(src, 1, 1, [], team_lanes=4).compile_check()
    # ... and any other State than double or Carry<K>
    with pytest.raises(S._lib.SABCError, match="double or sabc::series::Carry"):
        S.DeviceSource(src.replace("sabc::series::Carry<5>{}", "0.0f").replace("sabc::series::Carry<5>", "float").replace("c.v[0]", "c")
                       .replace("s.v[0]", "(double)s"), 1, 1, [], team_lanes=4).compile_check()
