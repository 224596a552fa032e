"""What the data pointer of a simulator from source costs (sabc_set_device_data, sabc::data_at) against the form the library
offered before it: the same simulator with its observations baked into the source as a __constant__ array.

The simulator is a pointwise distance over a series, rho = mean_j |y_sim(j) - y_obs(j)| with y_sim(j) = theta + z_j, one normal
per point.  For T = 16 and T = 1024, on the launch chain (n = 1 000 000) and in the one-launch form (n = 1000): RandomWalk, a
warm-up as long as a region, then five timed regions of --updates population updates per form, the two forms alternating inside this process.
Reported: us per update (median of the five regions) and the spread (max - min) of each form's own regions; the data form
passes where its median lies within the baked form's spread of the baked form's median.

Also, without a threshold, what a change of data set costs: set_data + the next update on the same handle, against a new
handle on a new baked source (compile included) + its initialisation and first update.

    python tools/device_data_ab.py --out profiles/device_data_ab.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

BODY = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const double mu = theta[0];
  double acc = 0.0;
  int j = 0;
  rng.for_pairs(T_LEN / 2, [&](const double z0, const double z1) {
    acc += fabs(mu + z0 - OBS(j));
    acc += fabs(mu + z1 - OBS(j + 1));
    j += 2;
  });
  rho[0] = acc / (double)T_LEN;
}
"""


def baked_source(obs, tag=""):
    arr = "__constant__ double kObs[%d] = {%s};\n" % (len(obs), ", ".join(repr(float(v)) for v in obs))
    return f"// {tag}\n#define T_LEN {len(obs)}\n{arr}#define OBS(j) kObs[j]\n" + BODY


def data_source(T):
    return f"#define T_LEN {T}\n#define OBS(j) sabc::data_at(j)\n" + BODY


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_data_ab.txt"))
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20241220)
    args = ap.parse_args()
    import sabc_amd as S
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# tools/device_data_ab.py: {args.regions} regions of {args.updates} updates per form, forms alternating, RandomWalk")
    say("# T  n  form  us/update baked (median, spread)  us/update data (median, spread)  data - baked  within the baked spread")
    rng = np.random.default_rng(args.seed)
    prior = S.Normal(0.0, 2.0)
    peak = S.op_rng_peak()                                    # normals/s of the bare Philox + Box-Muller loop, this device, now
    for T in (16, 1024):
        obs = rng.normal(1.0, 1.0, T)
        for n, persistent in ((1_000_000, "0"), (1000, "1")):
            os.environ["SABC_PERSISTENT"] = persistent        # read when the handle is created
            os.environ["SABC_PERSISTENT_MAX"] = "65536"
            models = dict(baked=S.DeviceSource(baked_source(obs), 1, 1), data=S.DeviceSource(data_source(T), 1, 1, data=obs))
            handles = {k: S.SabcHandle(n_particles=n, model=m, prior=prior, seed=args.seed) for k, m in models.items()}
            for h in handles.values():
                h.initialize(n)
                h.update(n_simulation=args.updates * n, proposal=S.RandomWalk(n_para=1))   # warm-up: as long as a timed region
            times = dict(baked=[], data=[])
            for _ in range(args.regions):
                for k, h in handles.items():
                    t0 = time.perf_counter()
                    h.update(n_simulation=args.updates * n, proposal=S.RandomWalk(n_para=1))
                    times[k].append((time.perf_counter() - t0) / args.updates * 1e6)
            same = all(np.array_equal(a, b) for a, b in zip(handles["baked"].get_population(), handles["data"].get_population()))
            form = "launch chain" if persistent == "0" else f"one launch ({handles['data'].persistent_lanes} lanes)"
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = {k: max(v) - min(v) for k, v in times.items()}
            ok = abs(med["data"] - med["baked"]) <= spread["baked"]
            say(f"T={T:5d} n={n:8d} {form:22s} baked {med['baked']:10.2f} ({spread['baked']:8.2f})  data {med['data']:10.2f} "
                f"({spread['data']:8.2f})  diff {med['data'] - med['baked']:+9.2f}  {'PASS' if ok else 'GAP'}  same particles: {same}")
            if persistent == "0":                             # the launch chain draws n T normals per update
                say(f"    normals drawn: {n * T / (med['data'] * 1e-6):.3g} per second (data form; the bare generator on this device, "
                    f"sabc_op_rng_peak: {peak:.3g})")
            say("    regions baked: " + " ".join(f"{x:.2f}" for x in times["baked"]) + " | data: " + " ".join(f"{x:.2f}" for x in times["data"]))
            if n == 1000:                                     # what a change of data set costs
                h = handles["data"]
                swap = []
                for r in range(5):
                    new = rng.normal(1.0, 1.0, T)
                    t0 = time.perf_counter()
                    h.set_data(new)
                    h.update(n_simulation=n, proposal=S.RandomWalk(n_para=1))
                    swap.append((time.perf_counter() - t0) * 1e3)
                fresh = []
                for r in range(2):
                    new = rng.normal(1.0, 1.0, T)
                    t0 = time.perf_counter()
                    g = S.SabcHandle(n_particles=n, model=S.DeviceSource(baked_source(new, f"data set {r}"), 1, 1), prior=prior, seed=args.seed)
                    g.initialize(n)
                    g.update(n_simulation=n, proposal=S.RandomWalk(n_para=1))
                    fresh.append((time.perf_counter() - t0) * 1e3)
                    g.close()
                say(f"    new data set, T={T}: set_data + one update {statistics.median(swap):.3f} ms (median of 5) | new handle on a new "
                    f"baked source, compile + initialize + one update: " + ", ".join(f"{x:.0f} ms" for x in fresh))
            for h in handles.values():
                h.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
