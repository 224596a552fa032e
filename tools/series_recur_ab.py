"""What sabc::Series::recur costs or buys a simulator from source (csrc/team_series.hpp): GARCH11 at n_obs = 100 and n_lags = 2
through its plain form (team_lanes = None: a private array per lane, the plain loop) and with 4 and 16 lanes per particle, where
the recurrence is relayed from lane to lane -- every lane issues all N steps -- and only the draws, the summaries and the
registers are divided; us per population update, the forms alternating inside this process on one box.  The comparison is the
plain form measured in the same run, and the run's own spread is printed beside every figure.

  update    GARCH11(n_obs=100) with team_lanes = None, 4 and 16; RandomWalk; n = 1e6 on the launch chain and n = 1000 in one
            launch (the engine's own choice of lanes; plain against team-aware); a warm-up region, then --regions regions of
            --updates updates per form.  On the launch chain two clocks per region: the device's (HIP events around every launch
            of the update kernel, SabcHandle.profile_enable(3) -- the figure compared) and the host's around the whole region.
            The one-launch form is timed by the host's clock alone: a handle that brackets every kernel with events takes the
            launch chain (csrc/hip_backend.hip), so events would measure another form.
  code      NumVgprs and ScratchSize of k_update_team for both widths and of k_update, from the code objects of the compiler
            stage (no device), and the compiler's time for a team-aware unit against a plain one.

No threshold is built in and nothing was promised: the recurrence itself is not parallel.  The default stays team_lanes = None.
Not measured here: a hand-written streaming loop without arrays (draw, step, accumulate), which the plain form is not.

    python tools/series_recur_ab.py --out profiles/series_recur.txt
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

N_OBS, N_LAGS, SIGMA2_0 = 100, 2, 1.0
SUMMARIES_OBS = (1.3, 4.1, 1.0, 0.7)                   # of the size of the model's own at theta = (0.2, 0.15, 0.7)
BOX = [(0.05, 1.0), (0.0, 0.5), (0.0, 0.9)]
FORMS = (None, 4, 16)
KERNEL_UPDATE = 0                                      # include/sabc_hip.h: SABC_KERNEL_UPDATE


def tag(team):
    return "plain" if team is None else f"team{team}"


def models(S, forms=FORMS):
    return {tag(t): S.GARCH11(SUMMARIES_OBS, n_obs=N_OBS, n_lags=N_LAGS, sigma2_0=SIGMA2_0, team_lanes=t) for t in forms}


def code_figures(S, say):
    """registers and scratch of the update kernels and the compiler's time, from the compiler stage alone"""
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    filt = shutil.which("c++filt")
    os.environ["SABC_RTC_CACHE"] = "0"
    with tempfile.TemporaryDirectory() as tmp:
        for name, model in models(S, (None, 16)).items():  # (the unit of team16 holds both widths)
            path = os.path.join(tmp, name + ".co")
            os.environ["SABC_RTC_CODE_OUT"] = path
            t0 = time.perf_counter()
            try:
                model.compile_check()
            finally:
                os.environ.pop("SABC_RTC_CODE_OUT", None)
            say(f"code: {name:8s} the compiler stage (with the one-launch kernels): {time.perf_counter() - t0:6.1f} s")
            notes = subprocess.run([readelf, "--notes", path], check=True, capture_output=True, text=True).stdout
            for k in notes.split("- .agpr_count")[1:]:
                kernel = re.search(r"\.name:\s+(\S+)", k).group(1)
                if filt:
                    kernel = subprocess.run([filt, kernel], capture_output=True, text=True).stdout.strip()
                kernel = re.sub(r"^void sabc::|\(.*$", "", kernel)
                if not (kernel.startswith("k_update_team") or kernel.startswith("k_update<") or kernel.startswith("k_simulate_batch_team")):
                    continue
                fig = {key: int(re.search(rf"\.{key}:\s+(\d+)", k).group(1)) for key in ("vgpr_count", "private_segment_fixed_size")}
                say(f"code: {name:8s} {kernel:44s} NumVgprs {fig['vgpr_count']:4d}  ScratchSize {fig['private_segment_fixed_size']:5d}")
    os.environ.pop("SABC_RTC_CACHE", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "series_recur.txt"))
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

    say(f"# tools/series_recur_ab.py: GARCH11(n_obs={N_OBS}, n_lags={N_LAGS}), its forms alternating in one process, {args.regions} regions of "
        f"{args.updates} updates each")
    if not args.no_code:
        code_figures(S, say)
    if args.code_only:
        say("update: not measured (--code-only: no device was used)")
    else:
        prior = S.product_distribution([S.Uniform(lo, hi) for lo, hi in BOX])
        # n = 1e6 on the launch chain: None, 4 and 16 lanes per particle; n = 1000 in one launch: plain against team-aware
        for n, persistent, forms in ((1_000_000, "0", FORMS), (1000, "1", (None, 16))):
            os.environ["SABC_PERSISTENT"] = persistent        # read when the handle is created
            os.environ.pop("SABC_PERSISTENT_LANES", None)
            handles = {}
            for k, m in models(S, forms).items():
                t0 = time.perf_counter()
                handles[k] = S.SabcHandle(n_particles=n, model=m, prior=prior, seed=args.seed, algorithm=S._lib.ALG_MULTI_EPS)
                say(f"handle: n={n:8d} {k:8s} created in {time.perf_counter() - t0:6.1f} s (the run-time compiler, "
                    f"{'with' if persistent == '1' else 'without'} the one-launch kernels)")
            for h in handles.values():
                h.initialize(n)
                if persistent == "0":
                    h.profile_enable(3)                    # HIP events around every launch of the update kernel
                h.update(n_simulation=args.updates * n, proposal=S.RandomWalk(n_para=3))     # warm-up: as long as a timed region
            host = {k: [] for k in handles}
            device = {k: [] for k in handles}
            for _ in range(args.regions):
                for k, h in handles.items():
                    ms0, c0 = h.profile_get(KERNEL_UPDATE)
                    t0 = time.perf_counter()
                    h.update(n_simulation=args.updates * n, proposal=S.RandomWalk(n_para=3))
                    host[k].append((time.perf_counter() - t0) / args.updates * 1e6)
                    ms1, c1 = h.profile_get(KERNEL_UPDATE)
                    # per population update: a launch of the chain is one update; the one-launch form runs the region's updates in
                    # however many launches it takes
                    device[k].append((ms1 - ms0) * 1e3 / args.updates if c1 > c0 else float("nan"))
            for clock, times in (("device events", device), ("host clock", host)) if persistent == "0" else (("host clock", host),):
                med = {k: statistics.median(v) for k, v in times.items()}
                for k, h in handles.items():
                    form = f"one launch ({h.persistent_lanes} lanes)" if h.persistent_lanes else f"launch chain ({h.chain_team_lanes or 1} lanes)"
                    say(f"update: n={n:8d} {form:24s} {k:8s} {clock:13s} {med[k]:10.2f} us/update (spread {max(times[k]) - min(times[k]):8.2f})  "
                        f"/ plain = {med[k] / med['plain']:6.2f}   regions: " + " ".join(f"{x:.2f}" for x in times[k]))
            for h in handles.values():
                h.close()
        say("not measured: a hand-written streaming loop without arrays; the one-launch form with SABC_PERSISTENT_LANES forced to 1 and 4")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
