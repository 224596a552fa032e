"""sabc::SampleF32 and GandKSampleF32 through the compiler stage (hipRTC needs no device), and the model class's argument checks.

tests/team_sample_f32/sample_probe_f32.hip calls every member of sabc::SampleF32 from sabc_user_simulate_team<W>; it compiles the
way tests/test_team_sample_compile.py compiles its probe -- as a team-aware source, whose unit holds W = 1, 4 and 16 -- with a
sample that is spread for both widths (N = 45), with one that is spread over a row of 16 and replicated in a quad (N = 129), and
in the planted form.  GandKSampleF32 compiles through the model class, checks its arguments as GandKSample does and refuses
team_lanes=None by name; and the new header is one of the unit's headers, so an edit of it is another cache key."""
import os
import shutil

import numpy as np
import pytest

from tests.test_rtc_host import CSRC, rtc_check  # noqa: F401  (the fixture: tests/rtc_host/rtc_check.cpp built against rtc.cpp alone)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = open(os.path.join(ROOT, "tests", "team_sample_f32", "sample_probe_f32.hip")).read()
Y45 = np.sort(np.random.default_rng(3).normal(3.0, 2.0, 45))


@pytest.mark.parametrize("n,planted", [(45, False), (129, False), (8, True)])
def test_a_probe_that_calls_every_member_of_sample_f32_compiles(S, n, planted):
    head = f"#define PROBE_N {n}\n" + ("#define PROBE_PLANTED 1\n" if planted else "")
    # one unit holds sabc_user_simulate_team<1>, <4> and <16>: the width is no part of the text or of the compiler stage
    assert S.DeviceSource(head + PROBE_SRC, 1, 2, [0.3], n_outputs=2 * n + 18, team_lanes=16).compile_check()


def test_gk_sample_f32_compiles_through_the_model_class(S):
    model = S.GandKSampleF32(Y45[::-1], team_lanes=16)
    assert model.source.startswith("#define GKS_N_DRAWS 45\n#define GKS_WASSERSTEIN 0\n#define GKS_KS 1\n// gk_sample.hip's team-aware form on a binary32")
    assert "sabc::SampleF32<N, W>" in model.source and "GKS_TEAM" not in model.source
    assert (model.n_stats, model.n_para, model.n_draws, model.n_outputs, model.data_names, model.team_lanes) == (2, (4,), 45, 45, ("y_obs",), 16)
    assert model.params == [45.0, 0.8]
    np.testing.assert_array_equal(model.data[0], Y45)                         # kept sorted
    assert model.compile_check()
    for lanes in (1, 4):
        other = S.GandKSampleF32(Y45, team_lanes=lanes)
        assert other.source == model.source and other.team_lanes == lanes
    assert S.GandKSampleF32(Y45).team_lanes == 4                               # the default
    assert isinstance(model, S.GandKSample) and "GandKSampleF32" in S.__all__


def test_gk_sample_f32_with_one_distance(S):
    ks = S.GandKSampleF32(Y45[:7], distance="ks", n_draws=33)                  # any two lengths
    assert ks.n_stats == 1 and ks.distance == ("ks",) and ks.source.startswith("#define GKS_N_DRAWS 33\n#define GKS_KS 0\n//")
    both = S.GandKSampleF32(Y45, distance=["ks", "wasserstein"])               # the statistics in the order given
    assert both.source.startswith("#define GKS_N_DRAWS 45\n#define GKS_KS 0\n#define GKS_WASSERSTEIN 1\n//")


def test_gk_sample_f32_checks_its_arguments(S):
    with pytest.raises(ValueError, match="GandKSample") as e:
        S.GandKSampleF32(Y45, team_lanes=None)
    assert "team_lanes" in str(e.value)
    for bad in (0, 2, 8, 32, -4, 4.5, "16", True):
        with pytest.raises(ValueError, match="team_lanes"):
            S.GandKSampleF32(Y45, team_lanes=bad)
    for bad in ("energy", ("ks", "ks"), (), ("wasserstein", "cramer")):
        with pytest.raises(ValueError, match="distance"):
            S.GandKSampleF32(Y45, distance=bad)
    with pytest.raises(ValueError, match="must equal n_draws"):
        S.GandKSampleF32(Y45, n_draws=44)                                      # "wasserstein" compares rank with rank
    assert S.GandKSampleF32(Y45, distance="ks", n_draws=44).n_draws == 44
    for bad in (np.nan, np.inf, -np.inf):
        y = Y45.copy()
        y[7] = bad
        with pytest.raises(ValueError, match="finite"):
            S.GandKSampleF32(y)
    for bad in (0, 1025, 4.5, True):
        with pytest.raises(ValueError, match="n_draws"):
            S.GandKSampleF32(Y45, distance="ks", n_draws=bad)
    with pytest.raises(ValueError, match="at least one value"):
        S.GandKSampleF32([])
    model = S.GandKSampleF32(Y45)
    model.bind_data((), {"y_obs": Y45 + 1.0})
    with pytest.raises(ValueError, match="ascending"):
        model.bind_data((Y45[::-1],), {})
    with pytest.raises(ValueError, match="must equal n_draws"):
        model.bind_data((Y45[:44],), {})


def test_the_existing_model_keeps_its_text(S):
    """GandKSample reads its source's name and its team switch from class attributes now: the text it hands on is what it was."""
    assert S.GandKSample(Y45).source.startswith("#define GKS_N_DRAWS 45\n#define GKS_WASSERSTEIN 0\n#define GKS_KS 1\n// g-and-k compared")
    assert S.GandKSample(Y45, team_lanes=4).source.startswith("#define GKS_N_DRAWS 45\n#define GKS_WASSERSTEIN 0\n#define GKS_KS 1\n#define GKS_TEAM 1\n// g-and-k")


def test_the_new_header_is_one_of_the_units_headers(rtc_check, tmp_path):
    """rtc.cpp finds the unit's headers by their #include lines: team_sample_f32.hpp is among them, and in a copy of csrc/ an
    edit of it alone is another hash."""
    assert os.path.realpath(os.path.join(CSRC, "team_sample_f32.hpp")) in [os.path.realpath(p) for p in rtc_check("headers", CSRC)[1:]]
    csrc = tmp_path / "simulatedannealingabc.jl_amd" / "csrc"
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so"))
    os.makedirs(tmp_path / "include")
    shutil.copy(os.path.join(ROOT, "include", "sabc_hip.h"), tmp_path / "include" / "sabc_hip.h")
    before = rtc_check("headers", csrc)[0]
    with open(csrc / "team_sample_f32.hpp", "a") as f:
        f.write("// an edit\n")
    assert rtc_check("headers", csrc)[0] != before
