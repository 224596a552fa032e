#!/usr/bin/env python3
"""The reference's documentation example on the device: sabc(StochasticSIR(data_obs), prior; n_particles = 5000,
n_simulation = 500_000) (docs/src/example.md:75-198), timed.  One JSON line per row: both distance forms (three statistics,
their sum) under each of the three proposals at n = 5000, and one row at n = 1e6.  Per row: wall time per population update,
the update kernel's own time (sabc_profile_get), the acceptance rate, and which form of the update ran (launches of the
one-launch form and its lanes per particle; 0 = the launch chain).  The host-side counterpart is `python bench.py --config host`
(its "docs SIR" row); profiles/sir_device.jsonl holds both from one box.

    python tools/sir_device.py [--large 1000000] [--large-updates 20]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 20241220


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large", type=int, default=1_000_000, help="particles of the large row (0: none)")
    ap.add_argument("--large-updates", type=int, default=20)
    args = ap.parse_args()
    import torch
    import sabc_amd as S
    from sabc_amd.examples import sir_observation
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: the SABC engine has no CPU path")
    obs = sir_observation((0.3, 0.1), seed=123)
    prior = S.product_distribution([S.Uniform(0.1, 1), S.Uniform(0.05, 0.5)])
    proposals = {"DifferentialEvolution": lambda: S.DifferentialEvolution(n_para=2), "RandomWalk": lambda: S.RandomWalk(n_para=2),
                 "StretchMove": lambda: S.StretchMove()}

    def row(n, n_simulation, n_stats, prop):
        model = S.StochasticSIR(obs, n_stats=n_stats)
        t_create = time.perf_counter()
        h = S.SabcHandle(n_particles=n, model=model, prior=prior, seed=SEED)      # compiles the source (or finds it cached)
        t_create = time.perf_counter() - t_create
        h.initialize(n_simulation)
        torch.cuda.synchronize()
        updates = (n_simulation - n) // n
        h.profile_enable(1)
        acc0 = h.counters["n_accept"]
        t0 = time.perf_counter()
        h.update(n_simulation=updates * n, proposal=proposals[prop]())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        kern_ms, launches = h.profile_get(S._lib.KERNEL_UPDATE)
        c = h.counters
        theta = h.get_population()[0]
        out = {"model": "docs SIR (Gillespie) on the device", "n_particles": n, "n_simulation": n_simulation, "n_stats": n_stats,
               "proposal": prop, "updates": c["n_population_updates"], "per_update_us": dt / updates * 1e6,
               "update_kernel_us_per_update": kern_ms * 1e3 / updates, "update_kernel_launches_timed": launches,
               "acceptance_rate": (c["n_accept"] - acc0) / (updates * n), "n_resampling": c["n_resampling"],
               "persistent_launches": h.persistent_launches, "persistent_lanes": h.persistent_lanes,
               "particle_sims_per_s": updates * n / dt, "handle_create_s": t_create,
               "posterior_mean": [float(theta[0].mean()), float(theta[1].mean())], "data_obs": obs}
        h.close()
        print(json.dumps(out), flush=True)

    for n_stats in (3, 1):
        for prop in proposals:
            row(5000, 500_000, n_stats, prop)
    if args.large:
        row(args.large, (args.large_updates + 1) * args.large, 3, "DifferentialEvolution")


if __name__ == "__main__":
    main()
