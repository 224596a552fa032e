"""What sabc::sort_ascending costs a simulator from source (csrc/sort_network.hpp), next to the built-in g-and-k model, whose
kernel (k_update_gk) sorts 128 draws across a row of lanes: us per population update, the models alternating inside this
process on one box.

  update    GandKQuantiles with four quantiles at n_draws = 32 (the unrolled network) and 128 (the loop form) and the built-in
            GandK at 128 draws and four ranks; RandomWalk; n = 1e6 on the launch chain and n = 1000 in one launch (the engine's
            own choice of lanes); a warm-up region, then --regions regions of --updates updates per model
  code      NumVgprs and ScratchSize of the update kernels the run-time compiler makes of the two source models (the compiler
            stage alone, no device), and of the bare unrolled network of 32 (tests/sort_isa/sort32_probe.hip)

No threshold.  In the one-launch form every lane of a team sorts the whole sample; a cooperative sort -- the lanes of a team
holding n / W values each -- is not built, and the gap to the built-in model at 128 draws is its price.

    python tools/sort_network_ab.py --out profiles/sort_network.txt
"""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROBS = (0.125, 0.375, 0.625, 0.875)                   # the ranks (16, 48, 80, 112) of 128 the built-in model is run with, as probabilities
OBS = (1.9, 2.7, 3.6, 6.4)
BOX = [(0.0, 10.0)] * 4                                # tests/cases.py: gk_cfg4


def source_models(S):
    return {f"source{n}": S.GandKQuantiles(PROBS, OBS, n_draws=n, c=0.8) for n in (32, 128)}


def code_figures(S, say):
    """registers and scratch of the update kernels, from the code objects of the compiler stage"""
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    filt = shutil.which("c++filt")
    with tempfile.TemporaryDirectory() as tmp:
        for tag, model in source_models(S).items():
            path = os.path.join(tmp, tag + ".co")
            os.environ["SABC_RTC_CODE_OUT"] = path
            try:
                model.compile_check()
            finally:
                os.environ.pop("SABC_RTC_CODE_OUT", None)
            notes = subprocess.run([readelf, "--notes", path], check=True, capture_output=True, text=True).stdout
            for k in notes.split("- .agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S+)", k).group(1)
                if filt:
                    name = subprocess.run([filt, name], capture_output=True, text=True).stdout.strip()
                name = re.sub(r"^void sabc::|\(.*$", "", name)
                if not name.startswith("k_update"):
                    continue
                fig = {key: int(re.search(rf"\.{key}:\s+(\d+)", k).group(1)) for key in ("vgpr_count", "private_segment_fixed_size")}
                say(f"code: {tag:10s} {name:44s} NumVgprs {fig['vgpr_count']:4d}  ScratchSize {fig['private_segment_fixed_size']:5d}")
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if os.path.exists(hipcc):
            asm_path = os.path.join(tmp, "sort32_probe.s")
            subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17",
                            "-I" + os.path.join(ROOT, "simulatedannealingabc.jl_amd", "csrc"),
                            os.path.join(ROOT, "tests", "sort_isa", "sort32_probe.hip"), "-o", asm_path], check=True, capture_output=True)
            asm = open(asm_path, encoding="utf-8").read().split("\nk_sort32_probe:", 1)[1]
            body = asm.split(".end_amdhsa_kernel", 1)[0]
            valu = len(re.findall(r"^\s+v_\w+", body, re.M))
            fig = {k: int(re.search(rf"; {k}: (\d+)", asm).group(1)) for k in ("NumVgprs", "ScratchSize", "Occupancy")}
            say(f"code: bare network of 32 doubles (k_sort32_probe): {valu} VALU instructions, fill and stores included; NumVgprs {fig['NumVgprs']}, "
                f"ScratchSize {fig['ScratchSize']}, occupancy {fig['Occupancy']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sort_network.txt"))
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20241220)
    ap.add_argument("--code-only", action="store_true", help="the compiler stage's figures alone: needs no device")
    args = ap.parse_args()
    import sabc_amd as S
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# tools/sort_network_ab.py: the models alternating in one process, {args.regions} regions of {args.updates} updates each")
    code_figures(S, say)
    if not args.code_only:
        prior = S.product_distribution([S.Uniform(lo, hi) for lo, hi in BOX])
        for n, persistent in ((1_000_000, "0"), (1000, "1")):
            os.environ["SABC_PERSISTENT"] = persistent        # read when the handle is created
            os.environ.pop("SABC_PERSISTENT_LANES", None)
            models = dict(builtin128=S.GandK(n_draws=128, c=0.8, ranks=(16, 48, 80, 112), obs=OBS), **source_models(S))
            handles = {k: S.SabcHandle(n_particles=n, model=m, prior=prior, seed=args.seed, algorithm=S._lib.ALG_MULTI_EPS)
                       for k, m in models.items()}
            for h in handles.values():
                h.initialize(n)
                h.update(n_simulation=args.updates * n, proposal=S.RandomWalk(n_para=4))     # warm-up: as long as a timed region
            times = {k: [] for k in handles}
            for _ in range(args.regions):
                for k, h in handles.items():
                    t0 = time.perf_counter()
                    h.update(n_simulation=args.updates * n, proposal=S.RandomWalk(n_para=4))
                    times[k].append((time.perf_counter() - t0) / args.updates * 1e6)
            med = {k: statistics.median(v) for k, v in times.items()}
            for k, h in handles.items():
                # (the built-in g-and-k model has no one-launch form: its kernel runs on the launch chain at every n)
                form = f"one launch ({h.persistent_lanes} lanes)" if h.persistent_lanes else "launch chain"
                say(f"update: n={n:8d} {form:22s} {k:10s} {med[k]:10.2f} us/update (spread {max(times[k]) - min(times[k]):8.2f})  "
                    f"/ builtin128 = {med[k] / med['builtin128']:.2f}   regions: " + " ".join(f"{x:.2f}" for x in times[k]))
            for h in handles.values():
                h.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
