"""Registers and scratch of every way a NormalStream is shared (CPU only: hipcc cross-compiles for gfx950 without a GPU).

tests/generator_isa/team_draws_probe.hip calls every public draw member -- for_pairs and for_quads_f32 with run-time trip counts,
pair, uniform_pair, quad_f32, uniform_quad_f32, next and poisson -- from one kernel per coop: a lane per particle (0), a quad and a
row of 16 lanes per particle (4, 16), and the plain loops (kCoopPlainLoop).  The team loops keep four blocks per lane in
registers -- eight doubles or sixteen floats -- next to the simulator's own state; this test holds that none of the four kernels
spills and that none grows: the private segment is 0 bytes and NumVgprs is what the header gave when the f64 and f32 team loops
were merged into one text over the element type (measured on the commit before the merge with the same command; the merge compiled
to the same instructions, profiles/team_draws_refactor_code_objects.txt).  It reads the kernel descriptor and the figures the
compiler prints behind it, no instruction."""
import os
import re
import subprocess

import pytest

from tests.test_generator_isa import CSRC, ROOT, find_hipcc

SRC = os.path.join(ROOT, "tests", "generator_isa", "team_draws_probe.hip")
NUM_VGPRS = {"0": 130, "4": 120, "16": 98, "n1": 130}          # by COOP as the mangled name has it (n1: kCoopPlainLoop = -1)


def test_no_team_draws_kernel_spills_or_grows(tmp_path):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    out = tmp_path / "team_draws_probe.s"
    cmd = [hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", f"-I{CSRC}", SRC, "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    asm = out.read_text()
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(_Z12k_team_drawsILi(\w+)EE\w+)$", asm, re.M)
    assert sorted(coop for _, coop in kernels) == sorted(NUM_VGPRS), kernels
    for name, coop in kernels:
        # the descriptor, and behind .end_amdhsa_kernel the figures of this kernel (up to the next kernel's text)
        descriptor, behind = asm.split(f".amdhsa_kernel {name}\n", 1)[1].split(".end_amdhsa_kernel", 1)
        private = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", descriptor).group(1))
        vgprs = int(re.search(r"; NumVgprs: (\d+)", behind).group(1))
        print(f"k_team_draws<{coop.replace('n', '-')}>: NumVgprs {vgprs}, private segment {private} bytes")
        assert private == 0, f"k_team_draws<{coop}> spills: a private segment of {private} bytes"
        assert vgprs == NUM_VGPRS[coop], f"k_team_draws<{coop}>: NumVgprs {vgprs}, was {NUM_VGPRS[coop]}"
