"""The host side of the run-time compiled path (csrc/rtc.cpp) from a plain C++ program, tests/rtc_host/rtc_check.cpp, built
with g++ against rtc.cpp alone: no device, no Python binding in between.  What the disk cache of compiled simulators rests on:
the headers whose text keys it are FOUND by following the unit's #include "..." lines -- they must cover what the
preprocessor reads, and an edit to any of them, listed by nobody, must change the key --, and the one table of the unit's
kernels must yield the names and the order that cached files and code objects depend on."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simulatedannealingabc.jl_amd")
CSRC = os.path.join(PKG, "csrc")
ROCM = os.environ.get("ROCM_PATH") or "/opt/rocm"


@pytest.fixture(scope="module")
def rtc_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    out = str(tmp_path_factory.mktemp("rtc_host") / "rtc_check")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include",
           os.path.join(ROOT, "tests", "rtc_host", "rtc_check.cpp"), os.path.join(CSRC, "rtc.cpp"), "-o", out,
           f"-L{ROCM}/lib", f"-Wl,-rpath,{ROCM}/lib", "-lamdhip64", "-ldl"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(*args):
        r = subprocess.run([out] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (args, r.stderr[-2000:])
        return r.stdout.splitlines()
    return run


def test_the_scanned_headers_cover_what_the_preprocessor_reads(rtc_check, tmp_path):
    """The unit's two headers through the device preprocessor: every file of this repository its line markers name is among
    the files the hash covers (today 13: the former hand-kept list and rtc.hpp), and every file the scan lists exists."""
    clang = os.path.join(ROCM, "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        pytest.skip("the ROCm clang++ was not found")
    unit = tmp_path / "unit.hip"
    unit.write_text('#include "update_kernel.hpp"\n#include "persistent_kernel.hpp"\n')
    r = subprocess.run([clang, "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", "-nogpulib", "-std=c++17", "-I", CSRC,
                        "-I", f"{ROCM}/include", "-E", str(unit)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = {os.path.realpath(m.group(1)) for m in re.finditer(r'^# \d+ "([^"<][^"]*)"', r.stdout, re.M)}
    ours = {p for p in seen if p.startswith(os.path.realpath(ROOT) + os.sep)}
    listed = rtc_check("headers", CSRC)[1:]
    print(len(ours), "files of the repository through the preprocessor,", len(listed), "scanned")
    assert {os.path.join(os.path.realpath(CSRC), f) for f in ("update_kernel.hpp", "persistent_kernel.hpp", "device_models.hpp")} <= ours
    assert ours <= {os.path.realpath(p) for p in listed}, sorted(ours - {os.path.realpath(p) for p in listed})
    assert len(listed) == len(set(listed)) and all(os.path.isfile(p) for p in listed), listed


def test_an_edit_to_any_included_file_changes_the_hash(rtc_check, tmp_path):
    """In a copy of csrc/ and include/sabc_hip.h with the same relative layout (a fresh process per state: the hash is memoised
    per directory): an edit to a header changes the hash, undoing it restores it, and so does a header NOBODY listed -- one
    that device_models.hpp starts to include, and then an edit to that file alone."""
    csrc = tmp_path / "simulatedannealingabc.jl_amd" / "csrc"
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so"))
    os.makedirs(tmp_path / "include")
    shutil.copy(os.path.join(ROOT, "include", "sabc_hip.h"), tmp_path / "include" / "sabc_hip.h")

    def state():
        return rtc_check("headers", csrc)[0]
    h0 = state()
    assert re.fullmatch(r"[0-9a-f]{16}", h0)
    rng_text = (csrc / "device_rng.hpp").read_text()
    (csrc / "device_rng.hpp").write_text(rng_text + "// an edit\n")
    assert state() != h0
    (csrc / "device_rng.hpp").write_text(rng_text)
    assert state() == h0
    (csrc / "extra_probe.hpp").write_text("#pragma once\n// text that moved out of device_models.hpp\n")
    with open(csrc / "device_models.hpp", "a") as f:
        f.write('#include "extra_probe.hpp"\n')
    h4 = state()
    assert h4 != h0
    assert os.path.realpath(csrc / "extra_probe.hpp") in rtc_check("headers", csrc)[1:]
    with open(csrc / "extra_probe.hpp", "a") as f:
        f.write("// an edit\n")
    assert state() not in (h0, h4)


def test_the_kernel_table_yields_the_names_cached_files_depend_on(rtc_check):
    """Name expressions and their order, written out: the seven kernels of the launch chain, then the one-launch form for teams
    of 1, 4 and 16 lanes x three proposals; the wide forms above 16 statistics, which have no one-launch form."""
    user = int(re.search(r"SABC_MODEL_USER\s*=\s*(\d+)", open(os.path.join(ROOT, "include", "sabc_hip.h")).read()).group(1))
    u = str(user)
    chain = ["sabc::k_prior_simulate<" + u + ", 2, 3>",
             "sabc::k_update<" + u + ", 2, 3, 0>", "sabc::k_update<" + u + ", 2, 3, 1>", "sabc::k_update<" + u + ", 2, 3, 2>",
             "sabc::k_simulate_batch<" + u + ", 2, 3>", "sabc::k_stats<2, 3>", "sabc::k_prior_op_t<2>"]
    one_launch = ["sabc::k_update_persistent<" + u + ", 2, 3, 0>", "sabc::k_update_persistent<" + u + ", 2, 3, 1>",
                  "sabc::k_update_persistent<" + u + ", 2, 3, 2>",
                  "sabc::k_update_persistent<" + u + ", 2, 3, 0, 4>", "sabc::k_update_persistent<" + u + ", 2, 3, 1, 4>",
                  "sabc::k_update_persistent<" + u + ", 2, 3, 2, 4>",
                  "sabc::k_update_persistent<" + u + ", 2, 3, 0, 16>", "sabc::k_update_persistent<" + u + ", 2, 3, 1, 16>",
                  "sabc::k_update_persistent<" + u + ", 2, 3, 2, 16>"]
    assert rtc_check("names", 2, 3, 1) == chain + one_launch and len(chain + one_launch) == 16
    assert rtc_check("names", 2, 3, 0) == chain
    wide = ["sabc::k_prior_simulate_wide<" + u + ", 3, 48>",
            "sabc::k_update_wide<" + u + ", 3, 48, 0>", "sabc::k_update_wide<" + u + ", 3, 48, 1>", "sabc::k_update_wide<" + u + ", 3, 48, 2>",
            "sabc::k_simulate_batch_wide<" + u + ", 3, 48>", "sabc::k_stats_wide<3, 48>", "sabc::k_prior_op_t<3>"]
    assert rtc_check("names", 3, 48, 0) == wide
    assert rtc_check("names", 3, 48, 1) == wide
