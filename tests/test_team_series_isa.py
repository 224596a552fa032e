"""sabc::Series<128, W> stays in registers (CPU only: hipcc cross-compiles for gfx950 without a GPU).

tests/team_series/series_isa_probe.hip fills a series of 128 doubles over a team of 16 lanes (8 slots per lane) and of 4 lanes
(32 slots per lane), forms the MA(2) series from lag<1>, lag<2> and two zips, takes autocovariance<0>, <1> and <2> and reads ONE
element whose time is a kernel argument: the index is known at run time only, so the read-out must select over the slots
instead of indexing them.  ScratchSize must be 0 for both kernels.  NumVgprs, the number of VALU instructions, of DPP moves and
of separate f64 multiplications (the products the tree's additions must not fuse with) are printed for DESIGN.md section 3
(pytest -s), not asserted."""
import re
import subprocess

import pytest

from tests.test_generator_isa import CSRC, ROOT, basic_blocks, find_hipcc

SRC = ROOT + "/tests/team_series/series_isa_probe.hip"


def test_the_spread_series_of_128_stays_in_registers(tmp_path):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    out = tmp_path / "series_isa_probe.s"
    # -ffp-contract=fast: what the run-time compiler is told (csrc/rtc.cpp)
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", "-ffp-contract=fast", f"-I{CSRC}", SRC, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    asm = out.read_text()
    for lanes in (16, 4):
        kernel = f"k_team_series_probe_{lanes}"
        ops = [op for b in basic_blocks(asm, kernel) for op in b]
        valu = [op for op in ops if op.startswith("v_")]
        mul = [op for op in ops if op.startswith("v_mul_f64")]
        tail = asm.split(f"\n{kernel}:", 1)[1]
        dpp = re.findall(r"row_shr:\d+", tail.split(".end_amdhsa_kernel", 1)[0])
        scratch, vgprs, occ = (re.search(rf"; {key}: (\d+)", tail) for key in ("ScratchSize", "NumVgprs", "Occupancy"))
        print(f"Series<128, {lanes}> fill + lag<1> + lag<2> + 2 zips + autocovariance<0|1|2> + at(t): {len(valu)} VALU instructions in the "
              f"kernel, {len(dpp)} row_shr moves, {len(mul)} v_mul_f64, NumVgprs {vgprs and vgprs.group(1)}, occupancy {occ and occ.group(1)}, "
              f"ScratchSize {scratch and scratch.group(1)}")
        assert scratch and int(scratch.group(1)) == 0, f"Series<128, {lanes}> leaves the registers"
