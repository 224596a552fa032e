"""Device assembly of the run-time compiled unit of a shipped simulator source, without a device and without hipRTC: the unit
text is composed the way rtc_compile (csrc/rtc.cpp) composes it -- the two headers, the data preamble, the source, the tail
that defines Sim<SABC_MODEL_USER> -- from the files of ONE tree, the kernels of the table (rtc_kernel_names: 16 for a narrow
source) are instantiated by taking their addresses, and hipcc compiles it with the run-time compiler's options.  Two trees
(a checkout of the parent commit and this one) give two files for tools/kernel_isa_diff.py: the question "are the update
kernels still the same kernels" answered instruction by instruction.
usage: python tools/rtc_unit_isa.py --tree DIR --source sir|sir_series|normal_moments --out unit.s"""
import argparse
import os
import re
import subprocess
import sys

SHIPPED = {"sir": (2, 3, "#define SIR_N_STATS 3\n"), "sir_series": (2, 1, ""), "normal_moments": (2, 2, "")}
MODEL_USER = 5
TEAM_LANES = (1, 4, 16)


def kernel_names(d, s):
    """rtc.cpp's kernel_table for a narrow source with the one-launch kernels."""
    mds = f"{MODEL_USER}, {d}, {s}"
    names = [f"sabc::k_prior_simulate<{mds}>"] + [f"sabc::k_update<{mds}, {p}>" for p in range(3)]
    names += [f"sabc::k_simulate_batch<{mds}>", f"sabc::k_stats<{d}, {s}>", f"sabc::k_prior_op_t<{d}>"]
    for lanes in TEAM_LANES:
        names += [f"sabc::k_update_persistent<{mds}, {p}" + (f", {lanes}" if lanes > 1 else "") + ">" for p in range(3)]
    return names


def raw_string(text, name):
    m = re.search(r"const char %s\[\] = R\"SABC\((.*?)\)SABC\";" % name, text, re.S)
    if not m:
        sys.exit(f"{name} not found in rtc.cpp")
    return m.group(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="root of a checkout")
    ap.add_argument("--source", required=True, choices=sorted(SHIPPED))
    ap.add_argument("--out", required=True)
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "hipcc"))
    a = ap.parse_args()
    pkg = os.path.join(a.tree, "simulatedannealingabc.jl_amd")
    csrc = os.path.join(pkg, "csrc")
    rtc = open(os.path.join(csrc, "rtc.cpp"), encoding="utf-8").read()
    d, s, head = SHIPPED[a.source]
    user = head + open(os.path.join(pkg, "device_sources", a.source + ".hip"), encoding="utf-8").read()
    unit = '#include "update_kernel.hpp"\n#include "persistent_kernel.hpp"\n' + raw_string(rtc, "kDataPreamble")
    unit += '#line 1 "f_dist.hip"\n' + user + raw_string(rtc, "kUserSimTail")
    unit += "\nvoid *sabc_unit_kernels[] = {\n" + "".join(f"  (void *)&{n},\n" for n in kernel_names(d, s)) + "};\n"
    src = a.out + ".hip"
    with open(src, "w", encoding="utf-8") as f:
        f.write(unit)
    # (the launch geometry the library forwards as -D options is the headers' own defaults: nothing to add here)
    cmd =[a.hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", "-ffp-contract=fast", f"-I{csrc}",
           src, "-o", a.out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stdout + r.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
