"""What a binary32 sample buys the cooperative form (csrc/team_sample_f32.hpp): GandKSample and GandKSampleF32 at 128 draws with each
of their distances and team_lanes = 4 and 16 -- the same model, the f64 sample on two normals per Philox block against the
binary32 sample on four --; us per population update, the models alternating inside this process on one box.

  update    RandomWalk; n = 1e6 on the launch chain and n = 1000 in one launch (the engine's own choice of lanes, where
            team_lanes 4 and 16 are one unit); a warm-up region, then --regions regions of --updates updates per model, medians.
  code      NumVgprs and ScratchSize of the six k_update_team code objects (two widths, three proposals) of both models, with
            each distance, from the compiler stage (no device).

No speed-up is fixed in advance.  The expectations each row confirms or refutes: no scratch on a quad at 128 draws; fewer us
per update with the binary32 sample in every row.

    python tools/team_sample_f32_ab.py --out profiles/team_sample_f32.txt
    python tools/team_sample_f32_ab.py --code-only        (needs no device)
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DRAWS = 128
BOX = [(0.0, 10.0)] * 4                                # tests/cases.py: gk_cfg4
TEAMS = (4, 16)
DISTANCES = ("wasserstein", "ks")


def observed_sample(seed):
    z = np.random.default_rng(seed).normal(size=DRAWS)
    return np.sort(3.0 + 1.0 * (1.0 + 0.8 * np.tanh(2.0 * z / 2.0)) * (1.0 + z * z) ** 0.5 * z)


def models(S, y, distances=DISTANCES):
    """f64 and f32 side by side, so that the two of a row run next to each other in every region"""
    out = {}
    for team in TEAMS:
        for d in distances:
            out[f"{d}_team{team}_f64"] = S.GandKSample(y, distance=d, c=0.8, team_lanes=team)
            out[f"{d}_team{team}_f32"] = S.GandKSampleF32(y, distance=d, c=0.8, team_lanes=team)
    return out


def code_figures(S, y, say):
    """registers and scratch of k_update_team, from the compiler stage alone; both widths are in every team-aware unit"""
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    filt = shutil.which("c++filt")
    os.environ["SABC_RTC_CACHE"] = "0"
    with tempfile.TemporaryDirectory() as tmp:
        units = [(f"{d}_{kind}", cls(y, distance=d, c=0.8, team_lanes=16))
                 for d in DISTANCES for kind, cls in (("f64", S.GandKSample), ("f32", S.GandKSampleF32))]
        for name, model in units:
            path = os.path.join(tmp, name + ".co")
            os.environ["SABC_RTC_CODE_OUT"] = path
            t0 = time.perf_counter()
            try:
                model.compile_check()
            finally:
                os.environ.pop("SABC_RTC_CODE_OUT", None)
            say(f"code: {name:16s} {DRAWS} draws; the compiler stage (with the one-launch kernels): {time.perf_counter() - t0:6.1f} s")
            notes = subprocess.run([readelf, "--notes", path], check=True, capture_output=True, text=True).stdout
            for k in notes.split("- .agpr_count")[1:]:
                kernel = re.search(r"\.name:\s+(\S+)", k).group(1)
                if filt:
                    kernel = subprocess.run([filt, kernel], capture_output=True, text=True).stdout.strip()
                kernel = re.sub(r"^void sabc::|\(.*$", "", kernel)
                if not kernel.startswith("k_update_team"):
                    continue
                fig = {key: int(re.search(rf"\.{key}:\s+(\d+)", k).group(1)) for key in ("vgpr_count", "private_segment_fixed_size")}
                quad = name.endswith("f32") and kernel.endswith(", 4>")
                verdict = "" if not quad else ("   no scratch on a quad: confirmed" if fig["private_segment_fixed_size"] == 0 else "   no scratch on a quad: refuted")
                say(f"code: {name:16s} {kernel:44s} NumVgprs {fig['vgpr_count']:4d}  ScratchSize {fig['private_segment_fixed_size']:5d}{verdict}")
    os.environ.pop("SABC_RTC_CACHE", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "team_sample_f32.txt"))
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20241220)
    ap.add_argument("--code-only", action="store_true", help="the compiler stage's figures alone: needs no device")
    ap.add_argument("--no-code", action="store_true", help="the timed updates alone")
    args = ap.parse_args()
    import sabc_amd as S
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# tools/team_sample_f32_ab.py: {DRAWS} draws, GandKSample (f64) and GandKSampleF32 (f32) alternating in one process, medians of "
        f"{args.regions} regions of {args.updates} updates each")
    y = observed_sample(args.seed)
    if not args.no_code:
        code_figures(S, y, say)
    if not args.code_only:
        prior = S.product_distribution([S.Uniform(lo, hi) for lo, hi in BOX])
        for n, persistent in ((1_000_000, "0"), (1000, "1")):
            os.environ["SABC_PERSISTENT"] = persistent        # read when the handle is created
            os.environ.pop("SABC_PERSISTENT_LANES", None)
            handles = {}
            for k, m in models(S, y).items():
                t0 = time.perf_counter()
                handles[k] = S.SabcHandle(n_particles=n, model=m, prior=prior, seed=args.seed, algorithm=S._lib.ALG_MULTI_EPS)
                say(f"handle: n={n:8d} {k:24s} created in {time.perf_counter() - t0:6.1f} s (the run-time compiler, "
                    f"{'with' if persistent == '1' else 'without'} the one-launch kernels)")
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
                form = f"one launch ({h.persistent_lanes} lanes)" if h.persistent_lanes else f"launch chain ({h.chain_team_lanes or 1} lanes)"
                base = med[k[:-3] + "f64"]
                verdict = "" if k.endswith("f64") else ("   fewer us: confirmed" if med[k] < base else "   fewer us: refuted")
                say(f"update: n={n:8d} {form:24s} {k:24s} {med[k]:10.2f} us/update (spread {max(times[k]) - min(times[k]):8.2f})  "
                    f"/ f64 at the same lanes = {med[k] / base:6.2f}{verdict}   regions: " + " ".join(f"{x:.2f}" for x in times[k]))
            for h in handles.values():
                h.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
