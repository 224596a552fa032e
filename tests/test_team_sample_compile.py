"""Team-aware simulators from source through the compiler stage (hipRTC needs no device), and the argument checks.

tests/team_sample/sample_probe.hip calls every member of sabc::Sample from sabc_user_simulate_team<W>; it compiles as a
team-aware source -- with a spread sample and with one too long for a quad's registers, the replicated fallback -- and so does
the shipped model, GandKQuantiles(..., team_lanes=16).  Registered the old way the same probe fails, and the log names the
entry point it lacks, sabc_user_simulate."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = open(os.path.join(ROOT, "tests", "team_sample", "sample_probe.hip")).read()


def probe(S, n, team_lanes):
    return S.DeviceSource(f"#define PROBE_N {n}\n" + PROBE_SRC, 1, 2, [0.3], n_outputs=2 * n, team_lanes=team_lanes)


@pytest.mark.parametrize("n", [45, 257])
def test_a_probe_that_calls_every_member_of_sample_compiles(S, n):
    # 45: spread for both widths; 257: spread over a row of 16 (32 slots per lane), replicated in a quad
    assert probe(S, n, 16).compile_check()


def test_gk_quantiles_compiles_in_its_team_aware_form(S):
    model = S.GandKQuantiles((0.25, 0.5, 0.75), (1.0, 2.0, 3.0), n_draws=45, team_lanes=16)
    assert model.source.startswith("#define GKQ_N_DRAWS 45\n#define GKQ_N_STATS 3\n#define GKQ_TEAM 1\n")
    assert model.compile_check()


def test_the_probe_registered_the_old_way_lacks_its_entry_point(S):
    with pytest.raises(S.SABCError, match="sabc_user_simulate") as e:
        probe(S, 45, None).compile_check()
    assert "sabc_user_simulate_team" not in str(e.value).replace("sabc_user_simulate_team<", "")     # the plain entry point is named


def test_team_lanes_is_checked(S):
    for bad in (0, 2, 8, 32, 64, -4, 4.5, "16", True):
        with pytest.raises(ValueError, match="team_lanes"):
            probe(S, 8, bad)
        with pytest.raises(ValueError, match="team_lanes"):
            S.GandKQuantiles((0.5,), (1.0,), n_draws=8, team_lanes=bad)
    for ok in (None, 1, 4, 16):
        assert probe(S, 8, ok).team_lanes == ok
    model = S.GandKQuantiles((0.25, 0.5), (1.0, 2.0), n_draws=8)
    assert model.team_lanes is None and model.source.startswith("#define GKQ_N_DRAWS 8\n#define GKQ_N_STATS 2\n//")
    y = [0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5, 8.5]
    assert S.GandKQuantiles.from_observations(y, team_lanes=4).team_lanes == 4
    assert S.GandKQuantiles.from_observations(y).team_lanes is None


def test_a_team_aware_source_has_no_wide_form(S):
    with pytest.raises(ValueError, match="16 statistics"):
        S.DeviceSource(PROBE_SRC, 1, 17, [0.3], team_lanes=4)
    assert S.DeviceSource(PROBE_SRC, 1, 17, [0.3]).team_lanes is None        # the ordinary entry point keeps its 64
    # ... and the library says so too, whoever calls it
    import ctypes as C
    from sabc_amd import _lib
    log = C.create_string_buffer(4096)
    rc = _lib.lib().sabc_op_compile_device_simulator_team(b"#define PROBE_N 8\n" + PROBE_SRC.encode(), 1, 17, log, len(log))
    assert rc == -8 and b"no wide form" in log.value                          # SABC_ERR_BAD_CONFIG
