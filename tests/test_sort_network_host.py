"""csrc/sort_network.hpp on the CPU: tests/sort_network/check_sort.cpp, a stand-alone program built with g++ from that header
alone (the same text every simulator from source sees in namespace sabc).  It runs every 0-1 input through the loop form for
n = 1..16 and through the template form for N in {1, 2, 3, 4, 5, 7, 8, 16} -- by the 0-1 principle a proof for those sizes --,
larger sizes against std::sort on random, sorted, reversed, all-equal, duplicate-heavy, infinite, denormal and signed-zero
inputs, the NaN policy (k NaNs in, k +inf at the end), quantile / order_statistic at their edges, and the float twins.
Built with the address and undefined-behaviour sanitizers where the compiler has their runtimes: a comparator that indexed
past the array would be reported, not merely survive."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simulatedannealingabc.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "sort_network", "check_sort.cpp")


def build(out, *flags):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", *flags, f"-I{CSRC}", SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_sort_network_on_the_host(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    out = str(tmp_path / "check_sort")
    r = build(out, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout or r.returncode != 0 and "asan" in r.stderr:
        r = build(out)                                 # a g++ without the sanitizers' runtimes: the plain program
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    run = subprocess.run([out], capture_output=True, text=True, timeout=300)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert " 0 failures" in run.stdout
