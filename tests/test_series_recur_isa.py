"""sabc::Series<128, W>::recur stays in registers and moves the state with DPP alone (CPU only: hipcc cross-compiles for gfx950
without a GPU).

tests/series_recur/recur_isa_probe.hip fills a series of 128 doubles over a team of 16 lanes (8 slots per lane, 16 phases) and of
4 lanes (32 slots per lane, 4 phases) from kernel arguments -- fill(g) involves no generator and so no LDS tables --, runs
cumsum(), the AR(2) recurrence with a Carry<2>, then sum().  For both kernels: ScratchSize 0, no LDS memory (a group segment of 0
bytes), no s_barrier and no ds_ instruction from the relay -- none at all in the quad; in the row of 16 exactly the four
ds_swizzle_b32 that sum()'s butterfly has always issued for the lane distances 4 and 8 (csrc/team_sample.hpp, team_add: a
cross-lane move, no memory), which is what sum() alone compiles to.  The compiler gives the quad's 32 slots per lane ScratchSize 0
as well (checked here, before any GPU run), so it is asserted for both.  NumVgprs, the number of VALU instructions and of DPP
moves are printed for DESIGN.md section 3 (pytest -s), not asserted."""
import re
import subprocess

import pytest

from tests.test_generator_isa import CSRC, ROOT, basic_blocks, find_hipcc

SRC = ROOT + "/tests/series_recur/recur_isa_probe.hip"


def test_the_relay_of_128_stays_in_registers_and_uses_no_lds(tmp_path):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    out = tmp_path / "recur_isa_probe.s"
    # -ffp-contract=fast: what the run-time compiler is told (csrc/rtc.cpp)
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", "-ffp-contract=fast", f"-I{CSRC}", SRC, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    asm = out.read_text()
    for lanes in (16, 4):
        kernel = f"k_series_recur_probe_{lanes}"
        ops = [op for b in basic_blocks(asm, kernel) for op in b]
        valu = [op for op in ops if op.startswith("v_")]
        fma = [op for op in ops if op.startswith(("v_fma_f64", "v_fmac_f64"))]
        add = [op for op in ops if op.startswith("v_add_f64")]
        lds = [op for op in ops if op.startswith("ds_")]
        barriers = [op for op in ops if op.startswith("s_barrier")]
        tail = asm.split(f"\n{kernel}:", 1)[1]
        body = tail.split(".end_amdhsa_kernel", 1)[0]
        dpp = re.findall(r"quad_perm:\[\d,\d,\d,\d\]|row_newbcast:\d+|row_share:\d+", body)
        scratch, vgprs, occ = (re.search(rf"; {key}: (\d+)", tail) for key in ("ScratchSize", "NumVgprs", "Occupancy"))
        print(f"Series<128, {lanes}> fill + cumsum + recur<Carry<2>> (AR(2)) + sum: {len(valu)} VALU instructions in the kernel, {len(fma)} "
              f"f64 fmas, {len(add)} v_add_f64, {len(dpp)} DPP broadcasts, {len(lds)} ds_ instructions, {len(barriers)} s_barrier, NumVgprs "
              f"{vgprs and vgprs.group(1)}, occupancy {occ and occ.group(1)}, ScratchSize {scratch and scratch.group(1)}")
        assert scratch and int(scratch.group(1)) == 0, f"Series<128, {lanes}>::recur leaves the registers"
        # sum()'s butterfly over a row of 16 pairs the lanes at distances 4 and 8 with ds_swizzle (teamsort::team_add: one per 32-bit
        # half, four in all; a cross-lane move that touches no LDS memory), a quad needs none: the relay adds no ds_ instruction
        swizzles = [op for op in lds if op.startswith("ds_swizzle_b32")]
        assert len(swizzles) == (4 if lanes == 16 else 0) and len(lds) == len(swizzles), f"Series<128, {lanes}>::recur uses LDS: {sorted(set(lds))}"
        lds_bytes = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", tail)
        assert lds_bytes and int(lds_bytes.group(1)) == 0, f"Series<128, {lanes}>::recur allocates LDS memory"
        assert not barriers, f"Series<128, {lanes}>::recur waits at a barrier"
        assert dpp, "the state is handed on by DPP moves"
