"""csrc/sample_reduce.hpp on the CPU.

The proof: tests/sample_reduce/check_reduce.cpp, a stand-alone program built with g++ from the headers alone -- the canonical
sum against the stack form and against a plain-array model of the device's executor (a lane's partial tree, the butterfly over
the team) for teams of 4 and 16 lanes, the rounding bound on the draw layout, the counts against std::lower_bound /
std::upper_bound, the Kolmogorov-Smirnov numerators against the supremum over all pooled points.  Built with the address and
undefined-behaviour sanitizers where the compiler has their runtimes.

The NumPy restatement the GPU tests compare with (tests/sample_reduce_ref.py) is held to the same definitions here: the tree
against math.fsum within the tree's bound and against a plain recursion bit for bit, the Kolmogorov-Smirnov formula against
the supremum over the pooled points."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import sample_reduce_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simulatedannealingabc.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "sample_reduce", "check_reduce.cpp")


def build(out, *flags):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", *flags, f"-I{CSRC}", SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_the_reductions_on_the_host(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    out = str(tmp_path / "check_reduce")
    r = build(out, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if r.returncode != 0 and "sanitize" in r.stderr + r.stdout or r.returncode != 0 and "asan" in r.stderr:
        r = build(out)                                 # a g++ without the sanitizers' runtimes: the plain program
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    run = subprocess.run([out], capture_output=True, text=True, timeout=600)
    print(run.stdout[-2000:])
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert " 0 failures" in run.stdout


def recursive_tree(s):
    if len(s) == 1:
        return s[0]
    half = 1 << ((len(s) - 1).bit_length() - 1)         # the left subtree: the largest power of two below the length
    right = s[half:]
    return recursive_tree(s[:half]) + (recursive_tree(right) if len(right) else 0.0)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 45, 100, 128, 257, 1000])
def test_the_numpy_tree_is_the_canonical_sum(n):
    rng = np.random.default_rng(n)
    s = rng.normal(size=n) * np.where(rng.random(n) < 0.2, 1e16, 1.0)
    got = float(R.tree_sum(s))
    assert got == float(recursive_tree(list(s))) + 0.0
    assert abs(got - math.fsum(s)) <= max(1, math.ceil(math.log2(n))) * 2.0 ** -53 * math.fsum(np.abs(s)) * 1.01
    rows = rng.normal(size=(7, n))
    np.testing.assert_array_equal(R.tree_sum(rows), [R.tree_sum(r) for r in rows])
    assert np.signbit(R.tree_sum(np.full(n, -0.0))) == False                      # noqa: E712


def test_the_numpy_ks_is_the_supremum_over_the_pooled_points():
    rng = np.random.default_rng(5)
    for _ in range(300):
        n, m = rng.integers(1, 13, 2)
        x = np.sort(rng.choice(2 * n, n, replace=False).astype(float))          # distinct, as continuous draws are
        y = np.sort(rng.integers(0, 2 * n, m).astype(float))                     # ties within y and with x
        pooled = np.concatenate([x, y])
        sup = max(abs(np.searchsorted(x, t, "right") * m - np.searchsorted(y, t, "right") * n) for t in pooled)
        assert R.ks(x, y) == sup / (float(n) * float(m))
    assert R.ks(np.array([1.0, np.inf]), np.array([0.0, 1.0, 2.0])) == 0.5
    assert R.count_less(np.array([np.nan, 1.0]), np.array([0.0, 1.0, 1.0])).tolist() == [3, 1]
    assert R.count_less_equal(np.array([np.nan, 1.0]), np.array([0.0, 1.0, 1.0])).tolist() == [3, 3]
