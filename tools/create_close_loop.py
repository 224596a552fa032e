"""20 cycles of create, initialize, one update and close at n = 1000 (the one-launch form): what a handle's set-up and
tear-down cost.  Run from the root of the tree to measure; prints one JSON line (milliseconds, medians over the cycles)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.getcwd())
import sabc_amd as S
from tests.cases import hip_model_prior, hip_proposal
model, prior = hip_model_prior(S, "gauss1_cfg2")
create, close, cycle = [], [], []
for rep in range(20):
    t0 = time.perf_counter()
    h = S.SabcHandle(n_particles=1000, model=model, prior=prior, seed=7); t1 = time.perf_counter()
    h.initialize(1000)
    h.update(n_simulation=100 * 1000, proposal=hip_proposal(S, "rw", 1)); t2 = time.perf_counter()
    h.close(); t3 = time.perf_counter()
    create.append(t1 - t0); close.append(t3 - t2); cycle.append(t3 - t0)
ms = lambda v: round(1e3 * v, 4)
print(json.dumps(dict(cycles=len(cycle), loop_ms=ms(sum(cycle)), cycle_ms=ms(statistics.median(cycle)),
                      create_ms=ms(statistics.median(create)), close_ms=ms(statistics.median(close)))))
