"""What the two-sample distances of sabc::Sample cost (csrc/sample_reduce.hpp): GandKSample with each of its distances at 128
draws, as plain arrays (team_lanes = None) and through sabc::Sample with 4 and 16 lanes per particle, next to GandKQuantiles
with four quantiles at the same shape -- the same draws and the same sort, so the difference is the reductions' --; us per
population update, the models alternating inside this process on one box.

  update    RandomWalk; n = 1e6 on the launch chain and n = 1000 in one launch (the engine's own choice of lanes); a warm-up
            region, then --regions regions of --updates updates per model, medians.

No threshold is built in.  The expectation the table confirms or refutes: at 128 draws the reductions add little to the sort's
28 steps; and which team_lanes pays.

    python tools/sample_distance_ab.py --out profiles/sample_distances.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DRAWS = 128
PROBS = (0.125, 0.375, 0.625, 0.875)
BOX = [(0.0, 10.0)] * 4                                # tests/cases.py: gk_cfg4
TEAMS = (None, 4, 16)


def observed_sample(seed):
    z = np.random.default_rng(seed).normal(size=DRAWS)
    return np.sort(3.0 + 1.0 * (1.0 + 0.8 * np.tanh(2.0 * z / 2.0)) * (1.0 + z * z) ** 0.5 * z)


def tag(kind, team):
    return kind + ("" if team is None else f"_team{team}")


def models(S, y):
    out = {}
    for team in TEAMS:
        out[tag("quantiles", team)] = S.GandKQuantiles(PROBS, np.quantile(y, PROBS), n_draws=DRAWS, c=0.8, team_lanes=team)
        for d in ("wasserstein", "ks"):
            out[tag(d, team)] = S.GandKSample(y, distance=d, c=0.8, team_lanes=team)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_distances.txt"))
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20241220)
    args = ap.parse_args()
    import sabc_amd as S
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# tools/sample_distance_ab.py: {DRAWS} draws, the models alternating in one process, medians of {args.regions} regions of "
        f"{args.updates} updates each")
    y = observed_sample(args.seed)
    prior = S.product_distribution([S.Uniform(lo, hi) for lo, hi in BOX])
    for n, persistent in ((1_000_000, "0"), (1000, "1")):
        os.environ["SABC_PERSISTENT"] = persistent        # read when the handle is created
        os.environ.pop("SABC_PERSISTENT_LANES", None)
        handles = {}
        for k, m in models(S, y).items():
            t0 = time.perf_counter()
            handles[k] = S.SabcHandle(n_particles=n, model=m, prior=prior, seed=args.seed, algorithm=S._lib.ALG_MULTI_EPS)
            say(f"handle: n={n:8d} {k:20s} created in {time.perf_counter() - t0:6.1f} s (the run-time compiler, "
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
            base = med["quantiles" + k[k.find("_team"):] if "_team" in k else "quantiles"]
            say(f"update: n={n:8d} {form:24s} {k:20s} {med[k]:10.2f} us/update (spread {max(times[k]) - min(times[k]):8.2f})  "
                f"/ quantiles at the same lanes = {med[k] / base:6.2f}   regions: " + " ".join(f"{x:.2f}" for x in times[k]))
        for h in handles.values():
            h.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
