"""csrc/team_series.hpp on the CPU.

tests/team_series/check_series.cpp, a stand-alone program built with g++ from the headers alone: the time-order layout of
sabc::Series for every N <= 40 (and 45, 100, 128) on 4 and 16 lanes, the constexpr lag schedule on plain arrays of W M positions --
lag<L> equal to the direct definition for every 1 <= L < N, `before` included, and which (lane distance, source slot) each slot
reads --, lagged_sum and autocovariance with first = 0 and 2 against reduce::tree_sum_of over the whole array, and the block
ownership of fill_normals.  Built with the address and undefined-behaviour sanitizers where the compiler has their runtimes, as
tests/test_team_sample_f32_host.py builds its program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simulatedannealingabc.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "team_series", "check_series.cpp")


def build(out, *flags):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", *flags, f"-I{CSRC}", SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_the_lag_schedule_and_the_sums_on_the_host(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    out = str(tmp_path / "check_series")
    r = build(out, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout or r.returncode != 0 and "asan" in r.stderr:
        r = build(out)                                 # a g++ without the sanitizers' runtimes: the plain program
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    run = subprocess.run([out], capture_output=True, text=True, timeout=600)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert " 0 failures" in run.stdout
