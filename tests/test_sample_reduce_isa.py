"""The reductions of sabc::Sample<128, W> leave the sample in registers (CPU only: hipcc cross-compiles for gfx950 without a GPU).

tests/sample_reduce/reduce_isa_probe.hip fills a sample of 128 doubles over a team of 16 lanes (8 slots per lane) and of 4 lanes
(32 slots per lane), sorts it and takes sum(), wasserstein1 and ks against an observed sample in memory.  ScratchSize must be 0
for both kernels.  NumVgprs and the number of VALU instructions are printed for DESIGN.md section 3 (pytest -s), next to those of
fill + sort + one quantile (tests/test_team_sample_isa.py), not asserted."""
import re
import subprocess

import pytest

from tests.test_generator_isa import CSRC, ROOT, basic_blocks, find_hipcc

SRC = ROOT + "/tests/sample_reduce/reduce_isa_probe.hip"


def test_the_reductions_of_a_spread_sample_of_128_stay_in_registers(tmp_path):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    out = tmp_path / "reduce_isa_probe.s"
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", f"-I{CSRC}", SRC, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    asm = out.read_text()
    for lanes in (16, 4):
        kernel = f"k_reduce_probe_{lanes}"
        ops = [op for b in basic_blocks(asm, kernel) for op in b]
        valu = [op for op in ops if op.startswith("v_")]
        adds = [op for op in valu if op.startswith("v_add_f64")]
        loads = [op for op in ops if op.startswith(("global_load", "flat_load"))]
        tail = asm.split(f"\n{kernel}:", 1)[1]
        scratch, vgprs, occ = (re.search(rf"; {key}: (\d+)", tail) for key in ("ScratchSize", "NumVgprs", "Occupancy"))
        print(f"Sample<128, {lanes}> fill + sort + sum + wasserstein1 + ks: {len(valu)} VALU instructions in the kernel ({len(adds)} v_add_f64), "
              f"{len(loads)} vector loads, NumVgprs {vgprs and vgprs.group(1)}, occupancy {occ and occ.group(1)}, "
              f"ScratchSize {scratch and scratch.group(1)}")
        assert scratch and int(scratch.group(1)) == 0, f"the reductions of Sample<128, {lanes}> leave the registers"
