"""csrc/team_sample.hpp and its kernel table on the CPU.

The proof: tests/team_sample/check_team_sample.cpp, a stand-alone program built with g++ from that header alone, runs the
header's schedule -- the list of steps the device executes on registers -- on plain arrays for teams of 1, 4 and 16 lanes:
every 0-1 input for every N <= 16 and for (W, N) = (4, 20), by the 0-1 principle a proof for those sizes; larger sizes
against std::sort; the NaN policy; the replicated fallback; the layout of the draws; and a plain-C++ model of the device's
signed-value executor against the schedule.  Built with the address and undefined-behaviour sanitizers where the compiler
has their runtimes.

The kernel table: tests/team_sample/team_names.cpp, built against rtc.cpp alone like tests/rtc_host/rtc_check.cpp, prints a
team-aware unit's names in the documented order, and the names of a unit that is not team-aware are those
tests/test_rtc_host.py lists."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simulatedannealingabc.jl_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH") or "/opt/rocm"
SRC = os.path.join(ROOT, "tests", "team_sample", "check_team_sample.cpp")


def build(out, *flags):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", *flags, f"-I{CSRC}", SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_the_schedule_sorts_on_the_host(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    out = str(tmp_path / "check_team_sample")
    r = build(out, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout or r.returncode != 0 and "asan" in r.stderr:
        r = build(out)                                 # a g++ without the sanitizers' runtimes: the plain program
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    run = subprocess.run([out], capture_output=True, text=True, timeout=600)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert " 0 failures" in run.stdout


@pytest.fixture(scope="module")
def team_names(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    out = str(tmp_path_factory.mktemp("team_names") / "team_names")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include",
           os.path.join(ROOT, "tests", "team_sample", "team_names.cpp"), os.path.join(CSRC, "rtc.cpp"), "-o", out,
           f"-L{ROCM}/lib", f"-Wl,-rpath,{ROCM}/lib", "-lamdhip64", "-ldl"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(*args):
        r = subprocess.run([out] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (args, r.stderr[-2000:])
        return r.stdout.splitlines()
    return run


def plain_names(u, d, s, one_launch):
    ds = f"{d}, {s}"
    chain = [f"sabc::k_prior_simulate<{u}, {ds}>", f"sabc::k_update<{u}, {ds}, 0>", f"sabc::k_update<{u}, {ds}, 1>", f"sabc::k_update<{u}, {ds}, 2>",
             f"sabc::k_simulate_batch<{u}, {ds}>", f"sabc::k_stats<{ds}>", f"sabc::k_prior_op_t<{d}>"]
    teams = [f"sabc::k_update_persistent<{u}, {ds}, {p}{lanes}>" for lanes in ("", ", 4", ", 16") for p in range(3)]
    return chain + (teams if one_launch else [])


def test_a_team_aware_unit_appends_its_kernels_in_the_documented_order(team_names):
    u = re.search(r"SABC_MODEL_USER\s*=\s*(\d+)", open(os.path.join(ROOT, "include", "sabc_hip.h")).read()).group(1)
    appended = ([f"sabc::k_update_team<{u}, 2, 3, {p}, {lanes}>" for lanes in (4, 16) for p in range(3)] +
                [f"sabc::k_simulate_batch_team<{u}, 2, 3, {lanes}>" for lanes in (4, 16)])
    assert len(appended) == 8
    for one_launch in (0, 1):
        plain = team_names(2, 3, one_launch, 0)
        assert plain == plain_names(u, 2, 3, one_launch)                    # what tests/test_rtc_host.py lists, unchanged
        assert team_names(2, 3, one_launch, 1) == plain + appended
    # the wide form has no team kernels (a team-aware registration is refused there): its table is the plain one
    assert team_names(3, 48, 0, 1) == team_names(3, 48, 0, 0) and len(team_names(3, 48, 0, 0)) == 7
