"""sabc::Series::recur on the CPU (csrc/team_series.hpp).

tests/series_recur/check_recur.cpp, a stand-alone program built with g++ from the headers alone: series::run_recur -- the relay
over the lanes of a team on plain arrays of W M positions, phase by phase as the device walks it, the evaluations that the other
lanes discard included -- against the sequential loop for every N <= 40 (and 45, 100, 128, 129) on 4 and 16 lanes, first = 0 and
2, the states double and Carry<2>, and the sum, the AR(2) map, the GARCH(1,1) map and a map that reads t: equal bits for the
outputs and the returned state, positions >= N and times < first untouched, and a poison value written over everything a lane
discards changes nothing.  Built with the address and undefined-behaviour sanitizers where the compiler has their runtimes, as
tests/test_team_series_host.py builds its program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simulatedannealingabc.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "series_recur", "check_recur.cpp")


def build(out, *flags):
    # -ffp-contract=off: the sequential loop and the relay inline the same map twice; neither copy may fuse on its own
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off", *flags, f"-I{CSRC}", SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_the_relay_gives_the_sequential_loops_bits_on_the_host(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    out = str(tmp_path / "check_recur")
    r = build(out, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout or r.returncode != 0 and "asan" in r.stderr:
        r = build(out)                                 # a g++ without the sanitizers' runtimes: the plain program
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    run = subprocess.run([out], capture_output=True, text=True, timeout=600)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert " 0 failures" in run.stdout
