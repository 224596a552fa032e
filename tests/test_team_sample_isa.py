"""sabc::Sample<128, W> stays in registers (CPU only: hipcc cross-compiles for gfx950 without a GPU).

tests/team_sample/team_sort_probe.hip fills a sample of 128 doubles over a team of 16 lanes (8 slots per lane) and of 4 lanes
(32 slots per lane), sorts it and reads ONE quantile whose probability is a kernel argument: the rank is known at run time
only, so the read-out must select over the slots instead of indexing them.  ScratchSize must be 0 for both kernels.  NumVgprs
and the number of VALU instructions are printed for DESIGN.md section 3 (pytest -s), not asserted."""
import re
import subprocess

import pytest

from tests.test_generator_isa import CSRC, ROOT, basic_blocks, find_hipcc

SRC = ROOT + "/tests/team_sample/team_sort_probe.hip"


def test_the_spread_sample_of_128_stays_in_registers(tmp_path):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    out = tmp_path / "team_sort_probe.s"
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", f"-I{CSRC}", SRC, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    asm = out.read_text()
    for lanes in (16, 4):
        kernel = f"k_team_sort_probe_{lanes}"
        ops = [op for b in basic_blocks(asm, kernel) for op in b]
        valu = [op for op in ops if op.startswith("v_")]
        tail = asm.split(f"\n{kernel}:", 1)[1]
        scratch, vgprs, occ = (re.search(rf"; {key}: (\d+)", tail) for key in ("ScratchSize", "NumVgprs", "Occupancy"))
        print(f"Sample<128, {lanes}> fill + sort + quantile: {len(valu)} VALU instructions in the kernel, NumVgprs {vgprs and vgprs.group(1)}, "
              f"occupancy {occ and occ.group(1)}, ScratchSize {scratch and scratch.group(1)}")
        assert scratch and int(scratch.group(1)) == 0, f"Sample<128, {lanes}> leaves the registers"
