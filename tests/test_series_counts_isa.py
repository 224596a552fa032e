"""sabc::Series<128, W>::map_poisson draws lane-locally (CPU only: hipcc cross-compiles for gfx950 without a GPU).

tests/series_counts/counts_isa_probe.hip fills a series of 128 doubles over a team of 16 lanes (8 slots per lane) and of 4 lanes
(32 slots per lane) from kernel arguments and sums it, once with map_poisson in between and once without.  The draw of time t is
a pure function of (t, lambda_t) that the lane holding t computes alone, so the map adds NO s_barrier, NO DPP move and NO
ds_swizzle to the kernel without it (whose sum() has the butterfly's own).  NumVgprs, ScratchSize, occupancy, the number of
instructions and the text size are printed for DESIGN.md section 3 (pytest -s), not asserted."""
import re
import subprocess

import pytest

from tests.test_generator_isa import CSRC, ROOT, basic_blocks, find_hipcc

SRC = ROOT + "/tests/series_counts/counts_isa_probe.hip"
DPP = r"quad_perm:\[\d,\d,\d,\d\]|row_newbcast:\d+|row_share:\d+|row_shr:\d+|row_shl:\d+|row_ror:\d+|row_bcast:\d+|row_mirror|row_half_mirror|wave_\w+:\d+"


def cross_lane(asm, kernel):
    ops = [op for b in basic_blocks(asm, kernel) for op in b]
    body = asm.split(f"\n{kernel}:", 1)[1].split(".end_amdhsa_kernel", 1)[0]
    return dict(barriers=len([op for op in ops if op.startswith("s_barrier")]), dpp=len(re.findall(DPP, body)),
                swizzles=len([op for op in ops if op.startswith("ds_swizzle")]), instructions=len(ops))


def test_map_poisson_adds_no_cross_lane_operation(tmp_path):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    out = tmp_path / "counts_isa_probe.s"
    # -ffp-contract=fast: what the run-time compiler is told (csrc/rtc.cpp)
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", "-ffp-contract=fast", f"-I{CSRC}", SRC, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    asm = out.read_text()
    sizes = {k: int(v) for k, v in re.findall(r"\n(k_series_counts_\w+):.*?; codeLenInByte = (\d+)", asm, re.S)}
    for lanes in (16, 4):
        with_map, without = (cross_lane(asm, f"k_series_counts_{kind}_{lanes}") for kind in ("probe", "base"))
        tail = asm.split(f"\nk_series_counts_probe_{lanes}:", 1)[1]
        scratch, vgprs, occ = (re.search(rf"; {key}: (\d+)", tail) for key in ("ScratchSize", "NumVgprs", "Occupancy"))
        print(f"Series<128, {lanes}> fill + map_poisson + sum: {with_map['instructions']} instructions ({without['instructions']} without the map), "
              f"text {sizes.get(f'k_series_counts_probe_{lanes}', 'n/a')} bytes ({sizes.get(f'k_series_counts_base_{lanes}', 'n/a')} without), "
              f"NumVgprs {vgprs and vgprs.group(1)}, occupancy {occ and occ.group(1)}, ScratchSize {scratch and scratch.group(1)}; "
              f"s_barrier {with_map['barriers']}, DPP moves {with_map['dpp']}, ds_swizzle {with_map['swizzles']}")
        assert with_map["instructions"] > without["instructions"] + 100, "the draw is in the kernel"
        assert with_map["barriers"] == without["barriers"] == 1, f"Series<128, {lanes}>::map_poisson waits at a barrier"
        assert with_map["dpp"] == without["dpp"], f"Series<128, {lanes}>::map_poisson moves values between lanes (DPP)"
        assert with_map["swizzles"] == without["swizzles"], f"Series<128, {lanes}>::map_poisson moves values between lanes (ds_swizzle)"
