"""What sabc::Sample buys a simulator from source (csrc/team_sample.hpp): GandKQuantiles through its team-aware form, a team of
lanes drawing and sorting one particle's sample, next to its lane form and to the built-in g-and-k model; us per population
update, the models alternating inside this process on one box.

  update    the built-in GandK at 128 draws and four ranks; GandKQuantiles with four quantiles at 128 draws with team_lanes =
            None, 4 and 16, and at 32 draws with team_lanes = None and 4; RandomWalk; n = 1e6 on the launch chain and n = 1000
            in one launch (the engine's own choice of lanes); a warm-up region, then --regions regions of --updates updates
            per model.  The control step's share: the engine's profile of the reduce + control launches at n = 1e6.
  code      NumVgprs and ScratchSize of k_update_team for both widths and of k_update, from the code objects of the compiler
            stage (no device), and the compiler's time for a team-aware unit against a plain one.

No threshold is built in; the acceptance is read off the table: at 128 draws team_lanes = 16 beats team_lanes = None at both
sizes.

    python tools/team_sample_ab.py --out profiles/team_sample.txt
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
FORMS = ((128, None), (128, 4), (128, 16), (32, None), (32, 4))


def tag(n_draws, team):
    return f"source{n_draws}" + ("" if team is None else f"_team{team}")


def source_models(S):
    return {tag(n, t): S.GandKQuantiles(PROBS, OBS, n_draws=n, c=0.8, team_lanes=t) for n, t in FORMS}


def code_figures(S, say):
    """registers and scratch of the update kernels and the compiler's time, from the compiler stage alone"""
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    filt = shutil.which("c++filt")
    os.environ["SABC_RTC_CACHE"] = "0"
    with tempfile.TemporaryDirectory() as tmp:
        for name, model in source_models(S).items():
            if name.endswith("_team4") and name.startswith("source128"):
                continue                                   # (the unit of source128_team16: both widths are in every team-aware unit)
            path = os.path.join(tmp, name + ".co")
            os.environ["SABC_RTC_CODE_OUT"] = path
            t0 = time.perf_counter()
            try:
                model.compile_check()
            finally:
                os.environ.pop("SABC_RTC_CODE_OUT", None)
            say(f"code: {name:18s} the compiler stage (with the one-launch kernels): {time.perf_counter() - t0:6.1f} s")
            notes = subprocess.run([readelf, "--notes", path], check=True, capture_output=True, text=True).stdout
            for k in notes.split("- .agpr_count")[1:]:
                kernel = re.search(r"\.name:\s+(\S+)", k).group(1)
                if filt:
                    kernel = subprocess.run([filt, kernel], capture_output=True, text=True).stdout.strip()
                kernel = re.sub(r"^void sabc::|\(.*$", "", kernel)
                if not (kernel.startswith("k_update_team") or kernel.startswith("k_update<") or kernel.startswith("k_simulate_batch_team")):
                    continue
                fig = {key: int(re.search(rf"\.{key}:\s+(\d+)", k).group(1)) for key in ("vgpr_count", "private_segment_fixed_size")}
                say(f"code: {name:18s} {kernel:44s} NumVgprs {fig['vgpr_count']:4d}  ScratchSize {fig['private_segment_fixed_size']:5d}")
    os.environ.pop("SABC_RTC_CACHE", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "team_sample.txt"))
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

    say(f"# tools/team_sample_ab.py: the models alternating in one process, {args.regions} regions of {args.updates} updates each")
    if not args.no_code:
        code_figures(S, say)
    if not args.code_only:
        prior = S.product_distribution([S.Uniform(lo, hi) for lo, hi in BOX])
        for n, persistent in ((1_000_000, "0"), (1000, "1")):
            os.environ["SABC_PERSISTENT"] = persistent        # read when the handle is created
            os.environ.pop("SABC_PERSISTENT_LANES", None)
            models = dict(builtin128=S.GandK(n_draws=128, c=0.8, ranks=(16, 48, 80, 112), obs=OBS), **source_models(S))
            handles = {}
            for k, m in models.items():
                t0 = time.perf_counter()
                handles[k] = S.SabcHandle(n_particles=n, model=m, prior=prior, seed=args.seed, algorithm=S._lib.ALG_MULTI_EPS)
                say(f"handle: n={n:8d} {k:18s} created in {time.perf_counter() - t0:6.1f} s (a simulator from source: the run-time compiler, "
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
                # (the built-in g-and-k model has no one-launch form: its kernel runs on the launch chain at every n)
                form = f"one launch ({h.persistent_lanes} lanes)" if h.persistent_lanes else f"launch chain ({h.chain_team_lanes or 1} lanes)"
                say(f"update: n={n:8d} {form:24s} {k:18s} {med[k]:10.2f} us/update (spread {max(times[k]) - min(times[k]):8.2f})  "
                    f"/ builtin128 = {med[k] / med['builtin128']:6.2f}   regions: " + " ".join(f"{x:.2f}" for x in times[k]))
            if persistent == "0":                             # the reduce + control launches with the rows k_update_team writes
                for k in ("source128", "source128_team16"):
                    h = handles[k]
                    h.profile_enable(2)
                    h.update(n_simulation=args.updates * n, proposal=S.RandomWalk(n_para=4))
                    ms, launches = h.profile_get(S._lib.KERNEL_REDUCE)
                    ms_u, launches_u = h.profile_get(S._lib.KERNEL_UPDATE)
                    say(f"control: n={n:8d} {k:18s} reduce + control {1e3 * ms / max(launches, 1):8.2f} us per launch ({launches} launches), "
                        f"update kernel {1e3 * ms_u / max(launches_u, 1):10.2f} us per launch ({launches_u} launches)")
                    h.profile_enable(0)
            for h in handles.values():
                h.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
