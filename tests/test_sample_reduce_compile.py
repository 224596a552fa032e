"""The reductions and distances of sabc::Sample through the compiler stage (hipRTC needs no device), and GandKSample's
argument checks.

tests/sample_reduce/reduce_probe.hip calls every new member of sabc::Sample and both count functions from
sabc_user_simulate_team<W>; it compiles with a spread sample for both widths (N = 45) and with one that is replicated in a quad
(N = 257), in the drawn and in the planted form.  GandKSample compiles in its four forms: plain arrays, and teams of 1, 4 and
16 lanes, which are one text."""
import os
import shutil

import numpy as np
import pytest

from tests.test_rtc_host import CSRC, rtc_check  # noqa: F401  (the fixture: tests/rtc_host/rtc_check.cpp built against rtc.cpp alone)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = open(os.path.join(ROOT, "tests", "sample_reduce", "reduce_probe.hip")).read()
Y45 = np.sort(np.random.default_rng(3).normal(3.0, 2.0, 45))


@pytest.mark.parametrize("n,planted", [(45, False), (257, False), (8, True)])
def test_a_probe_that_calls_every_reduction_compiles(S, n, planted):
    head = f"#define PROBE_N {n}\n" + ("#define PROBE_PLANTED 1\n" if planted else "")
    assert S.DeviceSource(head + PROBE_SRC, 1, 1, [0.0], n_outputs=(3 if planted else 2) * n + 16, team_lanes=16).compile_check()


@pytest.mark.parametrize("team_lanes", [None, 16])
def test_gk_sample_compiles_in_its_four_forms(S, team_lanes):
    """Two units: plain arrays, and the team-aware text, which holds the widths 1, 4 and 16 (the width is no part of the text)."""
    model = S.GandKSample(Y45[::-1], team_lanes=team_lanes)
    head = "#define GKS_N_DRAWS 45\n#define GKS_WASSERSTEIN 0\n#define GKS_KS 1\n" + ("" if team_lanes is None else "#define GKS_TEAM 1\n")
    assert model.source.startswith(head + "//") and model.team_lanes == team_lanes
    assert (model.n_stats, model.n_para, model.n_draws, model.n_outputs, model.data_names) == (2, (4,), 45, 45, ("y_obs",))
    np.testing.assert_array_equal(model.data[0], Y45)                         # kept sorted
    assert model.compile_check()
    if team_lanes is not None:
        for lanes in (1, 4):
            other = S.GandKSample(Y45, team_lanes=lanes)
            assert other.source == model.source and other.team_lanes == lanes


def test_gk_sample_with_one_distance(S):
    ks = S.GandKSample(Y45[:7], distance="ks", n_draws=33)                      # any two lengths
    assert ks.n_stats == 1 and ks.distance == ("ks",) and ks.source.startswith("#define GKS_N_DRAWS 33\n#define GKS_KS 0\n//")
    both = S.GandKSample(Y45, distance=["ks", "wasserstein"])                   # the statistics in the order given
    assert both.source.startswith("#define GKS_N_DRAWS 45\n#define GKS_KS 0\n#define GKS_WASSERSTEIN 1\n//")
    one = S.GandKSample(Y45, distance=("wasserstein",))
    assert one.n_stats == 1 and one.source.startswith("#define GKS_N_DRAWS 45\n#define GKS_WASSERSTEIN 0\n//")


def test_gk_sample_checks_its_arguments(S):
    for bad in ("energy", ("ks", "ks"), (), ("wasserstein", "cramer")):
        with pytest.raises(ValueError, match="distance"):
            S.GandKSample(Y45, distance=bad)
    with pytest.raises(ValueError, match="must equal n_draws"):
        S.GandKSample(Y45, n_draws=44)                                          # "wasserstein" compares rank with rank
    with pytest.raises(ValueError, match="must equal n_draws"):
        S.GandKSample(Y45, distance="wasserstein", n_draws=46)
    assert S.GandKSample(Y45, distance="ks", n_draws=44).n_draws == 44
    for bad in (np.nan, np.inf, -np.inf):
        y = Y45.copy()
        y[7] = bad
        with pytest.raises(ValueError, match="finite"):
            S.GandKSample(y)
    for bad in (0, 2, 8, 32, -4, 4.5, "16", True):
        with pytest.raises(ValueError, match="team_lanes"):
            S.GandKSample(Y45, team_lanes=bad)
    for bad in (0, 1025, 4.5, True):
        with pytest.raises(ValueError, match="n_draws"):
            S.GandKSample(Y45, distance="ks", n_draws=bad)
    with pytest.raises(ValueError, match="at least one value"):
        S.GandKSample([])
    # data that enter later are checked the same way; they are not sorted for the caller
    model = S.GandKSample(Y45)
    model.bind_data((), {"y_obs": Y45 + 1.0})
    with pytest.raises(ValueError, match="ascending"):
        model.bind_data((Y45[::-1],), {})
    with pytest.raises(ValueError, match="must equal n_draws"):
        model.bind_data((Y45[:44],), {})
    with pytest.raises(ValueError, match="one segment"):
        model.validate_data([Y45, Y45])


def test_the_new_header_enters_the_code_object_cache_key(rtc_check, tmp_path):
    """rtc.cpp finds the unit's headers by their #include lines (tests/test_rtc_host.py checks the mechanism): sample_reduce.hpp
    is among them, and in a copy of csrc/ an edit of it alone is another hash."""
    assert os.path.realpath(os.path.join(CSRC, "sample_reduce.hpp")) in [os.path.realpath(p) for p in rtc_check("headers", CSRC)[1:]]
    csrc = tmp_path / "simulatedannealingabc.jl_amd" / "csrc"
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so"))
    os.makedirs(tmp_path / "include")
    shutil.copy(os.path.join(ROOT, "include", "sabc_hip.h"), tmp_path / "include" / "sabc_hip.h")
    before = rtc_check("headers", csrc)[0]
    with open(csrc / "sample_reduce.hpp", "a") as f:
        f.write("// an edit\n")
    assert rtc_check("headers", csrc)[0] != before
