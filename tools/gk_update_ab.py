#!/usr/bin/env python3
"""Same-session A/B of library variants on the g-and-k update kernel (k_update_gk), both of its networks, all three proposals:
equal bits first, then kernel time against the first variant's own spread.

  python tools/gk_update_ab.py ab --libs parent=PATH,all=PATH[,name=PATH ...] --rounds 3 --out DIR [--bits parent,all]

Network 3 (k_update_gk<P, true>) is BASELINE config 4 as bench.py --config cfg4 runs it (tests/cases.py: gk_cfg4), network 2
(k_update_gk<P, false>) the gk_c09 case (ranks 10, 40, 60, 95); n = 1e6 and n = 647 (the population of
tests/test_gpu_gk_order_statistics.py: a third wave of 7 particles, a fourth without any, half batches of 323 and 324).
Every variant runs in a fresh child process per round, one after the other, in the order given: parent, branch, parent, ...
A child times the update kernel the way bench.py --full does (HIP events on every second launch, sabc_profile_enable level 1;
W warm-up and K timed updates after a pre-heat, the median of R such regions) and, in the first round, writes what a caller
holds after the timed path -- population, u, rho, eps, counters, history -- for the variants named by --bits; the driver
compares them with np.array_equal (every particle, nothing sampled) and keeps their SHA-256.
The rule per case: the first variant's median over the rounds is the figure to hold, the largest gap between two of its own
rounds the margin; another variant passes if its median is not above the sum.  A child that fails ends the session."""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NETWORKS = {3: "gk_cfg4", 2: "gk_c09"}
PROPOSALS = ("rw", "de", "stretch")
SIZES = (1_000_000, 647)
SEED = 20241220


def child(args):
    import numpy as np
    import sabc_amd as S
    from tests import cases
    S._lib.LIB_PATH = os.path.abspath(args.lib)
    import torch
    assert S.lib().sabc_device_count() > 0, "no HIP device"
    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < 1.0:                     # the device's clocks ramp over the first ~100 ms of load
        S.op_rng_peak(n_lanes=1_000_000, pairs_per_lane=50, repeats=20, device=0)
    out = {}
    for net, name in NETWORKS.items():
        model, prior = cases.hip_model_prior(S, name)
        assert all(r % 16 == 0 for r in model.params[2:6]) == (net == 3), model.params
        for prop in PROPOSALS:
            proposal = cases.hip_proposal(S, prop, len(prior))
            for n in SIZES:
                h = S.SabcHandle(n_particles=n, model=model, prior=prior, seed=SEED)
                regions = []
                for _ in range(args.repeats if n == SIZES[0] else 1):
                    h.initialize(n)
                    h.update(n_simulation=args.warmup * n, proposal=proposal)
                    h.profile_enable(1)
                    torch.cuda.synchronize()
                    h.update(n_simulation=args.steps * n, proposal=proposal)
                    torch.cuda.synchronize()
                    ms, launches = h.profile_get(S._lib.KERNEL_UPDATE)
                    h.profile_enable(0)
                    regions.append(ms / launches * 1e3 if launches else None)
                key = f"net{net}_{prop}_n{n}"
                out[key] = {"kernel_us_regions": regions, "persistent_launches": h.persistent_launches,
                            "n_accept": h.counters["n_accept"], "n_resampling": h.counters["n_resampling"]}
                if args.dump:
                    th, uu, rr = h.get_population()
                    eps_h, u_h, rho_h = h.history
                    c = h.counters
                    arrays = {"population": th, "u": uu, "rho": rr, "eps": h.eps, "eps_history": eps_h, "u_history": u_h,
                              "rho_history": rho_h, "counters": np.array([c[k] for k in sorted(c)], dtype=np.int64)}
                    os.makedirs(os.path.join(args.dump, key), exist_ok=True)
                    for a_name, a in arrays.items():
                        np.save(os.path.join(args.dump, key, a_name + ".npy"), np.ascontiguousarray(a))
                h.close()
    with open(args.out, "w") as f:
        json.dump(out, f)
    return 0


def compare_bits(dirs, report):
    import numpy as np
    (name_a, dir_a), (name_b, dir_b) = dirs
    equal = True
    for key in sorted(os.listdir(dir_a)):
        for fn in sorted(os.listdir(os.path.join(dir_a, key))):
            a, b = np.load(os.path.join(dir_a, key, fn)), np.load(os.path.join(dir_b, key, fn))
            same = a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
            equal = equal and same
            sha = hashlib.sha256(a.tobytes()).hexdigest()[:16], hashlib.sha256(b.tobytes()).hexdigest()[:16]
            report.append(f"{key:24s} {fn:16s} {str(a.shape):14s} {name_a} {sha[0]} {name_b} {sha[1]} {'EQUAL' if same else 'DIFFERENT'}")
    return equal


def ab(args):
    libs = [tuple(s.split("=", 1)) for s in args.libs.split(",")]
    bits = args.bits.split(",") if args.bits else []
    os.makedirs(args.out, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="gk_ab_")
    figures = {}                                                   # (case, lib) -> one figure per round
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(os.path.join(args.out, "gk_update_ab.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")

    say(f"libs {[n for n, _ in libs]}, rounds {args.rounds}, warm-up {args.warmup}, steps {args.steps}, regions per child {args.repeats}")
    try:
        for rnd in range(args.rounds):
            for name, path in libs:
                res = os.path.join(tmp, f"{name}_{rnd}.json")
                cmd = [sys.executable, os.path.abspath(__file__), "child", "--lib", path, "--out", res, "--steps", str(args.steps),
                       "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
                if rnd == 0 and name in bits:
                    cmd += ["--dump", os.path.join(tmp, "dump_" + name)]
                r = subprocess.run(cmd, timeout=args.child_timeout)
                if r.returncode:
                    say(f"child {name} round {rnd} ended with status {r.returncode}: the session stops here")
                    return 2
                with open(res) as f:
                    for case, v in json.load(f).items():
                        assert v["persistent_launches"] == 0, (case, v)     # k_update_gk, not a one-launch form
                        if v["kernel_us_regions"][0] is not None and case.endswith(f"_n{SIZES[0]}"):
                            figures.setdefault((case, name), []).append(statistics.median(v["kernel_us_regions"]))
                        if rnd == 0:
                            say(f"round 0 {name:12s} {case:22s} n_accept {v['n_accept']} n_resampling {v['n_resampling']} "
                                f"regions {' '.join('%.1f' % x for x in v['kernel_us_regions'] if x is not None)}")
            if rnd == 0 and len(bits) == 2:
                report = []
                equal = compare_bits([(b, os.path.join(tmp, "dump_" + b)) for b in bits], report)
                for s in report:
                    say(s)
                say(f"bits {bits[0]} vs {bits[1]}: {'ALL EQUAL' if equal else 'DIFFERENT'}")
                if not equal:
                    return 3
        ok = True
        base = libs[0][0]
        say(f"kernel us per timed launch of k_update_gk at n = {SIZES[0]}: one figure per round (median of the child's regions)")
        for case in sorted({c for c, _ in figures}):
            p = figures[(case, base)]
            hold, margin = statistics.median(p), max(p) - min(p)
            say(f"{case:22s} {base:12s} {' '.join('%.1f' % x for x in p)} | median {hold:.1f} margin {margin:.1f} ({100 * margin / hold:.1f} %)"
                f" -> bound {hold + margin:.1f}")
            for name, _ in libs[1:]:
                v = figures[(case, name)]
                passed = statistics.median(v) <= hold + margin
                ok = ok and passed
                say(f"{'':22s} {name:12s} {' '.join('%.1f' % x for x in v)} | median {statistics.median(v):.1f} {'pass' if passed else 'SLOWER'}")
        say("all variants within the bound" if ok else "a variant is above the bound")
        return 0 if ok else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("ab", "child"):
        p = sub.add_parser(name)
        p.add_argument("--steps", type=int, default=50)            # bench.py's defaults
        p.add_argument("--warmup", type=int, default=5)
        p.add_argument("--repeats", type=int, default=3)
        p.add_argument("--out", required=True)
    sub.choices["ab"].add_argument("--libs", required=True)
    sub.choices["ab"].add_argument("--rounds", type=int, default=3)
    sub.choices["ab"].add_argument("--bits", default="")
    sub.choices["ab"].add_argument("--child-timeout", type=float, default=240.0)
    sub.choices["child"].add_argument("--lib", required=True)
    sub.choices["child"].add_argument("--dump", default=None)
    args = ap.parse_args()
    return child(args) if args.cmd == "child" else ab(args)


if __name__ == "__main__":
    sys.exit(main())
