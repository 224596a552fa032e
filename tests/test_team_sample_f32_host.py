"""csrc/team_sample_f32.hpp on the CPU.

tests/team_sample_f32/check_team_sample_f32.cpp, a stand-alone program built with g++ from the headers alone: the layout of the
binary32 draws (blocks of four) for every N <= 132 on 4 and 16 lanes, the spread / replicated boundary at N = 32 W, a plain-C++
model of the float signed-value executor against teamsort::run_schedule -- every 0-1 input for N <= 16, sizes 45, 100, 128 and 512
against std::sort --, the NaN policy, and the f64 tree over the widened floats against reduce::tree_sum_of.  Built with the
address and undefined-behaviour sanitizers where the compiler has their runtimes, as tests/test_team_sample_host.py builds its
program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simulatedannealingabc.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "team_sample_f32", "check_team_sample_f32.cpp")


def build(out, *flags):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", *flags, f"-I{CSRC}", SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_the_float_executor_sorts_on_the_host(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    out = str(tmp_path / "check_team_sample_f32")
    r = build(out, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout or r.returncode != 0 and "asan" in r.stderr:
        r = build(out)                                 # a g++ without the sanitizers' runtimes: the plain program
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    run = subprocess.run([out], capture_output=True, text=True, timeout=600)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert " 0 failures" in run.stdout
