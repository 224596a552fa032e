"""sabc::SampleF32<128, W> stays in registers and takes fewer of them, and fewer instructions, than sabc::Sample<128, W> (CPU only:
hipcc cross-compiles for gfx950 without a GPU).

tests/team_sample_f32/team_sort_probe_f32.hip fills a sample of 128 binary32 values over a team of 16 lanes (8 slots per lane)
and of 4 lanes (32 slots per lane), sorts it and reads ONE quantile whose probability is a kernel argument.  ScratchSize must be
0 for both kernels, and each must have strictly fewer NumVgprs and strictly fewer VALU instructions than the same kernel of
tests/team_sample/team_sort_probe.hip, the f64 form, compiled here with the same flags: a slot is one register instead of two
and a cross-lane exchange moves one word instead of two.  The counts are printed for DESIGN.md section 3 (pytest -s); nothing
else about the instructions is asserted."""
import re
import subprocess

import pytest

from tests.test_generator_isa import CSRC, ROOT, basic_blocks, find_hipcc

F32 = ROOT + "/tests/team_sample_f32/team_sort_probe_f32.hip"
F64 = ROOT + "/tests/team_sample/team_sort_probe.hip"


def figures(asm, kernel):
    ops = [op for b in basic_blocks(asm, kernel) for op in b]
    tail = asm.split(f"\n{kernel}:", 1)[1]
    scratch, vgprs, occ = (int(re.search(rf"; {key}: (\d+)", tail).group(1)) for key in ("ScratchSize", "NumVgprs", "Occupancy"))
    return dict(valu=sum(op.startswith("v_") for op in ops), dpp=sum("_dpp" in op for op in ops),
                swizzle=sum(op.startswith("ds_swizzle") for op in ops), scratch=scratch, vgprs=vgprs, occupancy=occ)


def test_the_binary32_sample_of_128_needs_fewer_registers_and_instructions_than_the_f64_one(tmp_path):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    asm = {}
    for name, src in (("f32", F32), ("f64", F64)):
        out = tmp_path / f"{name}.s"
        cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", f"-I{CSRC}", src, "-o", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        asm[name] = out.read_text()
    for lanes in (16, 4):
        f32, f64 = figures(asm["f32"], f"k_team_sort_probe_f32_{lanes}"), figures(asm["f64"], f"k_team_sort_probe_{lanes}")
        for name, f in (("SampleF32", f32), ("Sample", f64)):
            print(f"{name}<128, {lanes}> fill + sort + quantile: {f['valu']} VALU instructions ({f['dpp']} with a DPP operand), "
                  f"{f['swizzle']} ds_swizzle, NumVgprs {f['vgprs']}, occupancy {f['occupancy']}, ScratchSize {f['scratch']}")
        assert f32["scratch"] == 0, f"SampleF32<128, {lanes}> leaves the registers"
        assert f32["vgprs"] < f64["vgprs"], (lanes, f32, f64)
        assert f32["valu"] < f64["valu"], (lanes, f32, f64)
