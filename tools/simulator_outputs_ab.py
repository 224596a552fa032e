#!/usr/bin/env python3
"""What the forward run of device-coded simulators (sabc::emit, sabc_op_simulate_outputs) costs the paths it shares a kernel
with, and what it delivers.  One JSON line per figure, for the package of ONE tree -- run it on a checkout of the parent commit
and on this one, alternating, on one box, and compare the branch's median with the parent's own spread:

  host_prior   k_simulate_batch also serves the host-prior path: a scipy prior next to StochasticSIR, n = 5000, RandomWalk,
               20 population updates; microseconds per update.
  forward      (a tree that has simulate_outputs) StochasticSIRSeries with 32 observation times, m = 1e6 rows through
               SabcHandle.simulate_outputs on the predictive stream, host arrays in and out: simulations/s and output bytes/s.

    python tools/simulator_outputs_ab.py --tree . [--what host_prior,forward] [--label branch]"""
import argparse
import json
import os
import sys
import time

SEED = 20241220


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--what", default="host_prior,forward")
    ap.add_argument("--label", default="")
    ap.add_argument("--rows", type=int, default=1_000_000)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch
    import sabc_amd as S
    from sabc_amd.examples import sir_observation, sir_series_observation
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: the SABC engine has no CPU path")
    what = args.what.split(",")

    if "host_prior" in what:
        from scipy import stats
        n, updates = 5000, 20
        model = S.StochasticSIR(sir_observation((0.3, 0.1), seed=123))
        prior = [stats.uniform(0.1, 0.9), stats.uniform(0.05, 0.45)]
        res = S.initialization(model, prior, n_particles=n, n_simulation=n, seed=SEED)
        prior = res._prior
        S.update_population_(res, model, prior, n_simulation=2 * n, proposal=S.RandomWalk(n_para=2), show_progressbar=False,
                             show_checkpoint=float("inf"))                           # warm: every kernel has run once
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.update_population_(res, model, prior, n_simulation=updates * n, proposal=S.RandomWalk(n_para=2), show_progressbar=False,
                             show_checkpoint=float("inf"))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"what": "host_prior", "label": args.label, "n_particles": n, "updates": updates,
                          "per_update_us": dt / updates * 1e6, "n_accept": res.state.n_accept}), flush=True)
        res._handle.close()

    if "forward" in what and hasattr(S, "simulate_outputs"):
        t_obs, I_obs = sir_series_observation((0.3, 0.1), seed=123)                 # 32 observation times
        model = S.StochasticSIRSeries(t_obs, I_obs)
        h = S.SabcHandle(n_particles=256, model=model, prior=S.product_distribution([S.Uniform(0.1, 1), S.Uniform(0.05, 0.5)]),
                         seed=SEED)
        rng = np.random.default_rng(1)
        m = args.rows
        theta = np.stack([rng.uniform(0.1, 1.0, m), rng.uniform(0.05, 0.5, m)])
        h.simulate_outputs(theta[:, :4096], 0, 0, stream="predict")                  # warm
        best = None
        for rep in range(3):
            t0 = time.perf_counter()
            rho, out = h.simulate_outputs(theta, 0, rep, stream="predict")
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        print(json.dumps({"what": "forward", "label": args.label, "rows": m, "n_out": int(out.shape[0]), "seconds_best_of_3": best,
                          "simulations_per_s": m / best, "output_bytes_per_s": out.nbytes / best,
                          "nan_outputs": int(np.isnan(out).sum())}), flush=True)
        h.close()


if __name__ == "__main__":
    main()
