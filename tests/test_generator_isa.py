"""Instruction count of the generator's hot loop (CPU only: hipcc cross-compiles for gfx950 without a GPU).

The update kernels sit at the VALU issue ceiling: their time is the number of VALU instructions
they issue, and nine tenths of those come from one loop -- NormalStream::for_pairs with a lane per particle, two
Philox4x32-10 blocks + Box-Muller pairs per trip.  This test compiles that loop on its own
(tests/generator_isa/for_pairs_sum.hip) and holds the count per trip: 174 VALU instructions (87 per pair; 188 before the
wave-uniform half of Philox rounds 1-2 moved to the scalar unit and the loop's two f64 / u32 literals into registers),
the uniform products on the SALU (s_mul_hi_u32, no v_mul_lo_u32 / v_mul_hi_u32), no scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simulatedannealingabc.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "generator_isa", "for_pairs_sum.hip")
MAX_VALU_PER_TRIP = 174


def find_hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand) and os.access(cand, os.X_OK):
            return cand
    return None


def basic_blocks(asm, kernel):
    """The instruction lines of `kernel`, split at labels."""
    body = asm.split(f"\n{kernel}:", 1)[1].split(".end_amdhsa_kernel", 1)[0]
    blocks, cur = [], []
    for line in body.splitlines():
        s = line.split(";", 1)[0].strip()
        if not s or s.startswith("."):
            if re.match(r"^\.?[A-Za-z_][\w.$]*:$", s):
                blocks.append(cur)
                cur = []
            continue
        if s.endswith(":"):
            blocks.append(cur)
            cur = []
            continue
        cur.append(s.split()[0])
    blocks.append(cur)
    return [b for b in blocks if b]


def test_for_pairs_loop_instruction_count(tmp_path):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    version = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.strip().splitlines()
    out = tmp_path / "for_pairs_sum.s"
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", f"-I{CSRC}", SRC, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    asm = out.read_text()
    blocks = basic_blocks(asm, "k_for_pairs_sum")
    loop = max(blocks, key=lambda b: sum(op == "v_mad_u64_u32" for op in b))
    n_mad = sum(op == "v_mad_u64_u32" for op in loop)
    valu = [op for op in loop if op.startswith("v_")]
    salu = [op for op in loop if op.startswith("s_")]
    scratch = re.search(r"; ScratchSize: (\d+)", asm.split("\nk_for_pairs_sum:", 1)[1])
    vgprs = re.search(r"; NumVgprs: (\d+)", asm.split("\nk_for_pairs_sum:", 1)[1])
    occ = re.search(r"; Occupancy: (\d+)", asm.split("\nk_for_pairs_sum:", 1)[1])
    print(f"{' | '.join(version[:2])}: for_pairs trip of two pairs = {len(valu)} VALU ({len(valu) / 2:g} per pair), "
          f"{len(salu)} SALU, {n_mad} v_mad_u64_u32, {sum(op == 'v_bitop3_b32' for op in loop)} v_bitop3_b32, "
          f"{sum(op == 'v_and_or_b32' for op in loop)} v_and_or_b32; NumVgprs {vgprs and vgprs.group(1)}, "
          f"occupancy {occ and occ.group(1)}, ScratchSize {scratch and scratch.group(1)}")
    # two blocks per trip, 10 rounds of two products each; the wave-uniform ones are not v_mad: between 30 and 40
    assert 30 <= n_mad <= 40, f"not the two-pair loop: {n_mad} v_mad_u64_u32 in its largest block"
    assert len(valu) <= MAX_VALU_PER_TRIP, f"{len(valu)} VALU instructions per trip of two pairs (limit {MAX_VALU_PER_TRIP})"
    assert not [op for op in loop if op in ("v_mul_lo_u32", "v_mul_hi_u32")], "a wave-uniform Philox product on the VALU"
    assert any(op == "s_mul_hi_u32" for op in loop), "no s_mul_hi_u32 in the loop: round 2's uniform product is not on the SALU"
    assert scratch and int(scratch.group(1)) == 0, "the loop spills to scratch"
