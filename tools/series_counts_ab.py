"""What count draws keyed by the time step cost or buy a simulator from source (sabc::CountDraws, csrc/device_rng.hpp;
Series::map_poisson, csrc/team_series.hpp): Ricker at N = burn_in + n_obs = 100 time steps and n_lags = 5 through its plain form
(team_lanes = None: a private array per lane, every lane all 100 draws) and with 4 and 16 lanes per particle, where a lane draws
the counts of the times it holds -- the normals, the counts and the summaries are divided, the latent recurrence is relayed and
is not --; us per population update, the forms alternating inside this process on one box.  The comparison is the plain form
measured in the same run, and the run's own spread is printed beside every figure.

  update    Ricker(n_obs=50, burn_in=50, n_lags=5) with team_lanes = None, 4 and 16; RandomWalk; n = 1e6 on the launch chain and
            n = 1000 in one launch (the engine's own choice of lanes; plain against team-aware); a warm-up region, then --regions
            regions of --updates updates per form.  On the launch chain two clocks per region: the device's (HIP events around
            every launch of the update kernel, SabcHandle.profile_enable(3) -- the figure compared) and the host's around the
            whole region.  The one-launch form is timed by the host's clock alone: a handle that brackets every kernel with events
            takes the launch chain (csrc/hip_backend.hip), so events would measure another form.
  code      NumVgprs, ScratchSize and the text size of k_update_team for both widths and of k_update, from the code objects of
            the compiler stage (no device), and the compiler's time for a team-aware unit against a plain one; the same for the
            team-aware unit with map_poisson spelled through map (a copy of the draw per slot: before the slot loop was rolled).

No threshold is built in and nothing was promised.  The default stays team_lanes = None.
Not measured here: a hand-written streaming Ricker without arrays (draw, step, count, accumulate), which the plain form is not.

    python tools/series_counts_ab.py --out profiles/series_counts.txt
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

N_OBS, BURN_IN, N_LAGS, N0 = 50, 50, 5, 1.0
SUMMARIES_OBS = (40.0, 25.0, 4000.0, -600.0, -300.0, 1200.0, -400.0, -200.0)      # of the size of the model's own at theta = (3.8, 0.3, 10)
BOX = [(2.0, 4.5), (0.05, 0.6), (4.0, 16.0)]
FORMS = (None, 4, 16)
KERNEL_UPDATE = 0                                      # include/sabc_hip.h: SABC_KERNEL_UPDATE


def tag(team):
    return "plain" if team is None else f"team{team}"


def models(S, forms=FORMS):
    return {tag(t): S.Ricker(SUMMARIES_OBS, n_obs=N_OBS, burn_in=BURN_IN, n_lags=N_LAGS, n0=N0, team_lanes=t) for t in forms}


def unrolled(S, model):
    """the team-aware model with map_poisson spelled through map: a copy of the draw per slot, what map_poisson's rolled loop replaced"""
    rolled = "y.map_poisson(rng, phi);"
    plain = ("{ const sabc::CountDraws cd = rng.reserve_counts(RICKER_N); "
             "y.map([&](const int t, const double v) { return (double)cd.poisson(t, sabc::series::rounded_product(phi, v)); }); }")
    assert model.source.count(rolled) == 1
    return S.DeviceSource(model.source.replace(rolled, plain), 3, model.n_stats, model.params, data=model.data, n_outputs=model.n_outputs,
                          team_lanes=model.team_lanes)


def code_figures(S, say):
    """registers, scratch and text size of the update kernels and the compiler's time, from the compiler stage alone: the kernel
    descriptors and the symbol table as llvm-objdump prints them"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    objdump = next((p for p in (os.path.join(rocm, "llvm", "bin", "llvm-objdump"), os.path.join(rocm, "lib", "llvm", "bin", "llvm-objdump"))
                    if os.path.exists(p)), None) or shutil.which("llvm-objdump")
    filt = shutil.which("c++filt")
    os.environ["SABC_RTC_CACHE"] = "0"
    with tempfile.TemporaryDirectory() as tmp:
        units = models(S, (None, 16))                      # (the unit of team16 holds both widths)
        units["team16-unrolled"] = unrolled(S, units["team16"])    # BEFORE the slot loop was rolled: the draw through map
        for name, model in units.items():
            path = os.path.join(tmp, name + ".co")
            os.environ["SABC_RTC_CODE_OUT"] = path
            t0 = time.perf_counter()
            try:
                model.compile_check()
            finally:
                os.environ.pop("SABC_RTC_CODE_OUT", None)
            say(f"code: {name:15s} the compiler stage (with the one-launch kernels): {time.perf_counter() - t0:6.1f} s")
            if objdump is None:
                say(f"code: {name:15s} no llvm-objdump here: registers, scratch and text size not read")
                continue
            symbols = subprocess.run([objdump, "-t", path], check=True, capture_output=True, text=True).stdout
            sizes = {m.group(2): int(m.group(1), 16) for m in re.finditer(r"F \.text\s+([0-9a-f]+)\s+(?:\.\w+\s+)?(\S+)", symbols)}
            descriptors = subprocess.run([objdump, "-d", "--section=.rodata", path], check=True, capture_output=True, text=True).stdout
            for k in descriptors.split(".amdhsa_kernel ")[1:]:
                mangled = k.split()[0]
                kernel = subprocess.run([filt, mangled], capture_output=True, text=True).stdout.strip() if filt else mangled
                kernel = re.sub(r"^void sabc::|\(.*$", "", kernel)
                if not (kernel.startswith("k_update_team") or kernel.startswith("k_update<") or kernel.startswith("k_simulate_batch_team")):
                    continue
                fig = {key: int(re.search(rf"\.amdhsa_{key} (\d+)", k).group(1)) for key in ("next_free_vgpr", "private_segment_fixed_size")}
                say(f"code: {name:15s} {kernel:44s} NumVgprs {fig['next_free_vgpr']:4d}  ScratchSize {fig['private_segment_fixed_size']:5d}  "
                    f"text {sizes.get(mangled, 0):7d} bytes")
    os.environ.pop("SABC_RTC_CACHE", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "series_counts.txt"))
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20241220)
    ap.add_argument("--code-only", action="store_true", help="the compiler stage's figures alone: needs no device")
    ap.add_argument("--no-code", action="store_true", help="the timed updates alone")
    ap.add_argument("--append", action="store_true", help="add to --out (the other half of a run split with --code-only / --no-code)")
    args = ap.parse_args()
    import sabc_amd as S
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# tools/series_counts_ab.py: Ricker(n_obs={N_OBS}, burn_in={BURN_IN}, n_lags={N_LAGS}), its forms alternating in one process, {args.regions} regions of "
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
        say("not measured: a hand-written streaming Ricker without arrays; the one-launch form with SABC_PERSISTENT_LANES forced to 1 and 4")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
