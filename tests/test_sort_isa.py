"""The unrolled sorting network stays in registers (CPU only: hipcc cross-compiles for gfx950 without a GPU).

tests/sort_isa/sort32_probe.hip fills double x[32] from a counter, calls the template form of sabc::sort_ascending
(csrc/sort_network.hpp) and stores the array.  With every index a compile-time constant the 32 doubles are 64 vector
registers and the 191 comparators of Batcher's odd-even merge sort straight-line code: the kernel's ScratchSize must be 0.
NumVgprs and the number of VALU instructions are printed for DESIGN.md section 3 (pytest -s), not asserted."""
import re
import subprocess

import pytest

from tests.test_generator_isa import CSRC, ROOT, basic_blocks, find_hipcc

SRC = ROOT + "/tests/sort_isa/sort32_probe.hip"
KERNEL = "k_sort32_probe"


def test_the_unrolled_network_of_32_stays_in_registers(tmp_path):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    out = tmp_path / "sort32_probe.s"
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", f"-I{CSRC}", SRC, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    asm = out.read_text()
    ops = [op for b in basic_blocks(asm, KERNEL) for op in b]
    valu = [op for op in ops if op.startswith("v_")]
    tail = asm.split(f"\n{KERNEL}:", 1)[1]
    scratch, vgprs, occ = (re.search(rf"; {key}: (\d+)", tail) for key in ("ScratchSize", "NumVgprs", "Occupancy"))
    print(f"sort_ascending(double (&)[32]): {len(valu)} VALU instructions in the kernel (fill and stores included), "
          f"NumVgprs {vgprs and vgprs.group(1)}, occupancy {occ and occ.group(1)}, ScratchSize {scratch and scratch.group(1)}")
    assert scratch and int(scratch.group(1)) == 0, "the unrolled network of 32 doubles leaves the registers"
