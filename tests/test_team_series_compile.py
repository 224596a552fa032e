"""sabc::Series and MA2 through the compiler stage (hipRTC needs no device), the model class's argument checks and the NumPy
restatement against itself.

tests/team_series/series_probe.hip calls every member of sabc::Series from sabc_user_simulate_team<W>; it compiles the way
tests/test_team_sample_compile.py compiles its probe -- as a team-aware source, whose unit holds W = 1, 4 and 16 -- with one value,
with three (a lag of N - 1 = 2), spread for both widths (45, 128), spread over a row of 16 and replicated in a quad (257), and in
the planted form.  MA2 compiles through the model class in both forms; team_series.hpp is one of the unit's headers, so an edit
of it is another cache key; and tests/team_series_ref.py agrees with the direct definitions and with MA2.autocovariances."""
import os
import shutil

import numpy as np
import pytest

from tests import team_series_ref as T
from tests.sample_reduce_ref import tree_sum
from tests.test_rtc_host import CSRC, rtc_check  # noqa: F401  (the fixture: tests/rtc_host/rtc_check.cpp built against rtc.cpp alone)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = open(os.path.join(ROOT, "tests", "team_series", "series_probe.hip")).read()
LAGS = (1, 3, 4, 5, 9, 44)


def probe_lags(n):
    """the lags series_probe.hip compiles at length n, in its order"""
    return [L for L in (1, 2 if n == 3 else 0, 3, 4, 5, 9, 44) if 1 <= L < n]


def probe_outputs(n):
    first = 2 if n > 2 else 0
    return 2 * n + 16 + len(probe_lags(n)) * (n + 4) + (n - first) + n


@pytest.mark.parametrize("n,planted", [(1, False), (3, False), (45, False), (128, False), (257, False), (12, True)])
def test_a_probe_that_calls_every_member_of_series_compiles(S, n, planted):
    head = f"#define PROBE_N {n}\n" + ("#define PROBE_PLANTED 1\n" if planted else "")
    # one unit holds sabc_user_simulate_team<1>, <4> and <16>: the width is no part of the text or of the compiler stage
    assert S.DeviceSource(head + PROBE_SRC, 1, 1, [0.0], n_outputs=probe_outputs(n), team_lanes=16).compile_check()


def test_ma2_compiles_in_both_forms(S):
    acov = [1.4, 0.7, 0.2]
    plain = S.MA2(acov, n_obs=43)
    assert plain.source.startswith("#define MA2_N_OBS 43\n#define MA2_N_LAGS 2\n// MA(2) with autocovariance summaries")
    assert (plain.n_stats, plain.n_para, plain.n_obs, plain.n_lags, plain.n_outputs, plain.data_names, plain.team_lanes) == \
        (3, (2,), 43, 2, 43, ("acov_obs",), None)
    assert plain.params == [43.0, 2.0]
    np.testing.assert_array_equal(plain.data[0], acov)
    assert plain.compile_check()
    team = S.MA2(acov, n_obs=43, team_lanes=16)
    assert team.source.startswith("#define MA2_N_OBS 43\n#define MA2_N_LAGS 2\n#define MA2_TEAM 1\n// MA(2)")
    assert team.compile_check()
    for lanes in (1, 4):
        other = S.MA2(acov, n_obs=43, team_lanes=lanes)
        assert other.source == team.source and other.team_lanes == lanes
    assert "sabc::Series<MA2_N_OBS + 2, W>" in plain.source and "MA2" in S.__all__
    defaults = S.MA2()
    assert (defaults.n_obs, defaults.n_lags, defaults.n_stats, defaults.data, defaults.team_lanes) == (100, 2, 3, None, None)


def test_ma2_with_every_lag_compiles(S):
    # seven lags on a short series: lag 7 of 12 held times crosses three lanes of a row of 16 (two slots per lane)
    assert S.MA2(np.ones(8), n_obs=10, n_lags=7, team_lanes=4).compile_check()


def test_ma2_checks_its_arguments(S):
    for bad in (-1, 8, 2.5, True, "2"):
        with pytest.raises((ValueError, TypeError), match="n_lags|int"):
            S.MA2(n_lags=bad)
    for bad in (0, 2, 1023, 4.5, True):
        with pytest.raises(ValueError, match="n_obs"):
            S.MA2(n_obs=bad, n_lags=2)
    for bad in (0, 2, 8, 32, "4", True):
        with pytest.raises(ValueError, match="team_lanes"):
            S.MA2(team_lanes=bad)
    with pytest.raises(ValueError, match="n_lags \\+ 1 = 3"):
        S.MA2([1.0, 0.5])
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            S.MA2([1.0, bad, 0.2])
    model = S.MA2([1.0, 0.5, 0.2])
    model.bind_data((), {"acov_obs": [2.0, 1.0, 0.1]})
    with pytest.raises(ValueError, match="n_lags \\+ 1"):
        model.bind_data(([2.0, 1.0, 0.1, 0.0],), {})
    with pytest.raises(ValueError, match="finite"):
        model.bind_data(([2.0, np.nan, 0.1],), {})
    with pytest.raises(TypeError, match="acov_obs"):
        model.bind_data((), {"y_obs": [1.0, 2.0, 3.0]})


def test_from_observations_uses_the_restatements_tree(S):
    y = np.random.default_rng(5).normal(size=43)
    model = S.MA2.from_observations(y, team_lanes=4)
    assert (model.n_obs, model.n_lags, model.n_stats, model.team_lanes) == (43, 2, 3, 4)
    np.testing.assert_array_equal(model.data[0], T.ma2_summaries(y, 2))
    np.testing.assert_array_equal(S.MA2.autocovariances(y, 7), T.ma2_summaries(y, 7))
    many = np.random.default_rng(6).normal(size=(5, 3, 100))
    np.testing.assert_array_equal(S.MA2.autocovariances(many, 2), T.ma2_summaries(many, 2))
    # the value is the textbook one up to rounding; the bits are the tree's over 45 positions, not those of a plain sum
    for j in range(3):
        assert abs(model.data[0][j] - np.dot(y[j:], y[:43 - j]) / 43) <= 45 * 2.0 ** -53 * np.abs(y[j:] * y[:43 - j]).sum()
    assert S.MA2.from_observations(y, n_lags=5).n_stats == 6


def test_the_restatement_against_the_direct_definitions():
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 5, 45, 128, 257):
        x = rng.normal(size=(4, n)) * 10.0 ** rng.integers(-3, 4, size=(4, n))
        for L in range(1, min(n, 50)):
            got = T.lag(x, L, -7.0)
            for t in range(n):
                np.testing.assert_array_equal(got[:, t], x[:, t - L] if t >= L else np.full(4, -7.0))
        for L in (0, 1, 2, 44):
            if L >= n:
                continue
            for first in (0, 2):
                if first >= n:
                    continue
                terms = np.array([[abs(x[r, t] - x[r, t - L]) if t >= first + L else 0.0 for t in range(n)] for r in range(4)])
                np.testing.assert_array_equal(T.lagged_sum(x, L, lambda t, a, b: np.abs(a - b), first), tree_sum(terms))
                prods = np.array([[(x[r, t] - 0.25) * (x[r, t - L] - 0.25) if t >= first + L else 0.0 for t in range(n)] for r in range(4)])
                np.testing.assert_array_equal(T.autocovariance(x, L, 0.25, first), tree_sum(prods) / float(n - first))


def test_the_ma2_transcription_with_either_fma():
    from tests import elementary_ref as E
    e = np.random.default_rng(8).normal(size=45)
    y = T.ma2_series((0.6, 0.2), e)
    assert y.shape == (43,)
    np.testing.assert_array_equal(y, T.ma2_series((0.6, 0.2), e, fma=E.fma_fraction))
    np.testing.assert_allclose(y, e[2:] + 0.6 * e[1:-1] + 0.2 * e[:-2], rtol=0, atol=1e-14)      # (the same model, rounded twice more)


def test_the_new_header_is_one_of_the_units_headers(rtc_check, tmp_path):
    """rtc.cpp finds the unit's headers by their #include lines: team_series.hpp is among them, and in a copy of csrc/ an edit of
    it alone is another hash."""
    assert os.path.realpath(os.path.join(CSRC, "team_series.hpp")) in [os.path.realpath(p) for p in rtc_check("headers", CSRC)[1:]]
    csrc = tmp_path / "simulatedannealingabc.jl_amd" / "csrc"
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so"))
    os.makedirs(tmp_path / "include")
    shutil.copy(os.path.join(ROOT, "include", "sabc_hip.h"), tmp_path / "include" / "sabc_hip.h")
    before = rtc_check("headers", csrc)[0]
    with open(csrc / "team_series.hpp", "a") as f:
        f.write("// an edit\n")
    assert rtc_check("headers", csrc)[0] != before
