"""Instruction count of the binary32 generator's hot loop (CPU only: hipcc cross-compiles for gfx950 without a GPU): the twin
of tests/test_generator_isa.py for NormalStream::for_quads_f32 with a lane per particle, two Philox4x32-10 blocks and eight
normals per trip (tests/generator_isa/for_quads_f32_sum.hip).

Done means at most 216 VALU instructions per trip, 27 per normal: the f64 loop's 43.5 less the 16.5 that half a Philox block
per pair saves by itself.  The loop stands at 208 (26 per normal): 64 of Philox, 48 packed (v_pk_fma_f32 / v_pk_mul_f32 /
v_pk_add_f32, each working on both pairs of a block), 28 of the two correctly rounded square roots' fix-ups, the rest integer
work on the table indices and exponents; no conversion from the f64 tables (the loop reads their binary32 copies in LDS).  No
hardware transcendental but the square root's seed, no scratch."""
import re
import subprocess

import pytest

from tests.test_generator_isa import CSRC, ROOT, basic_blocks, find_hipcc

SRC = ROOT + "/tests/generator_isa/for_quads_f32_sum.hip"
KERNEL = "k_for_quads_f32_sum"
MAX_VALU_PER_TRIP = 208
DONE_VALU_PER_TRIP = 216
FORBIDDEN = ("v_log_f32", "v_sin_f32", "v_cos_f32", "v_rcp_f32", "v_rsq_f32")


def test_for_quads_f32_loop_instruction_count(tmp_path):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    out = tmp_path / "for_quads_f32_sum.s"
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", f"-I{CSRC}", SRC, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    asm = out.read_text()
    blocks = basic_blocks(asm, KERNEL)
    loop = max(blocks, key=lambda b: sum(op == "v_mad_u64_u32" for op in b))
    n_mad = sum(op == "v_mad_u64_u32" for op in loop)
    valu = [op for op in loop if op.startswith("v_")]
    packed = [op for op in valu if op.startswith("v_pk_")]
    tail = asm.split(f"\n{KERNEL}:", 1)[1]
    scratch, vgprs, occ = (re.search(rf"; {key}: (\d+)", tail) for key in ("ScratchSize", "NumVgprs", "Occupancy"))
    print(f"for_quads_f32 trip of two blocks = {len(valu)} VALU ({len(valu) / 8:g} per normal), {len(packed)} packed "
          f"({sum(op == 'v_pk_fma_f32' for op in loop)} v_pk_fma_f32), {n_mad} v_mad_u64_u32, "
          f"{sum(op.startswith('v_cvt_f32_f64') for op in loop)} v_cvt_f32_f64, {sum(op.startswith('ds_read') for op in loop)} LDS reads; "
          f"NumVgprs {vgprs and vgprs.group(1)}, occupancy {occ and occ.group(1)}, ScratchSize {scratch and scratch.group(1)}")
    assert 30 <= n_mad <= 40, f"not the two-block loop: {n_mad} v_mad_u64_u32 in its largest block"
    assert MAX_VALU_PER_TRIP <= DONE_VALU_PER_TRIP
    assert len(valu) <= MAX_VALU_PER_TRIP, f"{len(valu)} VALU instructions per trip of two blocks (limit {MAX_VALU_PER_TRIP})"
    assert any(op == "v_pk_fma_f32" for op in loop), "no v_pk_fma_f32 in the loop: the two pairs of a block do not run packed"
    assert scratch and int(scratch.group(1)) == 0, "the loop spills to scratch"
    kernel_ops = [op for b in blocks for op in b]
    bad = sorted({op for op in kernel_ops if op.startswith(FORBIDDEN)})
    assert not bad, f"hardware transcendentals in the kernel: {bad}"
    assert sum(op.startswith("v_sqrt_f32") for op in loop) == 4, "one seed per radius: four v_sqrt_f32 per trip"
