"""A time series of 48 points as 48 statistics (the model of tools/many_stats_probe.py): particle simulations per second and
microseconds per population update, with f_dist as HIP source (the wide kernels, SABC_MAX_SOURCE_STATS = 64) and as a batched
NumPy host callback.  --compile: the hipRTC compile time (compiler stage only, no device) of the (16, 16), (3, 48) and (16, 64)
shapes.

    python tools/source_many_stats.py [--n 100000 1000000] [--compile] [--device-only]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sabc_amd as S  # noqa: E402

d, s = 3, 48
t = np.linspace(0.0, 4.0, s)
obs = 2.0 * np.exp(-0.6 * t) + 0.3
NOISE = 0.05


def carray(name, vals):
    return f"__constant__ double {name}[{len(vals)}] = {{" + ", ".join(repr(float(v)) for v in vals) + "};\n"


SRC = carray("kT", t) + carray("kObs", obs) + r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  for (int j = 0; j < 48; j += 2) {
    double z0, z1;
    rng.pair(z0, z1);
    rho[j] = fabs(theta[0] * exp(-theta[1] * kT[j]) + theta[2] + p[0] * z0 - kObs[j]);
    rho[j + 1] = fabs(theta[0] * exp(-theta[1] * kT[j + 1]) + theta[2] + p[0] * z1 - kObs[j + 1]);
  }
}
"""
rng = np.random.default_rng(1)


def f_host(theta):
    return np.abs(theta[:, :1] * np.exp(-theta[:, 1:2] * t) + theta[:, 2:3] + NOISE * rng.standard_normal((len(theta), s)) - obs)


def prior():
    return S.product_distribution([S.Uniform(0.5, 4.0), S.Uniform(0.05, 2.0), S.Normal(0.0, 1.0)])


def measure(model, n, warm, k):
    h = S.SabcHandle(n_particles=n, model=model, prior=prior(), seed=5, algorithm=S._lib.ALG_MULTI_EPS)
    h.initialize(n)
    h.update(n_simulation=warm * n, proposal=S.RandomWalk(n_para=d))
    t0 = time.perf_counter()
    h.update(n_simulation=k * n, proposal=S.RandomWalk(n_para=d))
    dt = time.perf_counter() - t0
    c = h.counters
    h.close()
    return dt / k * 1e6, n * k / dt, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--compile", action="store_true")
    ap.add_argument("--device-only", action="store_true", help="skip the host callback (a profiler run of the device kernels)")
    a = ap.parse_args()
    if a.compile:
        shape_src = carray("kTarget", [0.1 * j for j in range(64)]) + r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const int d = (int)p[0], s = (int)p[1];
  for (int j = 0; j < s; ++j) rho[j] = fabs(theta[j % d] + 0.4 * rng.next() - kTarget[j]);
}
"""
        for dd, ss in ((16, 16), (3, 48), (16, 64)):
            t0 = time.perf_counter()
            S.DeviceSource(shape_src, dd, ss, [dd, ss]).compile_check()
            print(f"compile (d, s) = ({dd}, {ss}): {time.perf_counter() - t0:.1f} s", flush=True)
    for n in a.n:
        us, rate, c = measure(S.DeviceSource(SRC, d, s, [NOISE]), n, 5, 40 if n <= 100_000 else 20)
        print(f"device source  n = {n:>8}: {us:9.1f} us per update, {rate:.3e} particle-simulations/s  (accept {c['n_accept']})", flush=True)
        if a.device_only:
            continue
        k = 10 if n <= 100_000 else 3
        us, rate, c = measure(S.HostDistance(f_host, n_stats=s, n_para=d, univariate=False, batched=True), n, 1, k)
        print(f"host callback  n = {n:>8}: {us:9.1f} us per update, {rate:.3e} particle-simulations/s  (accept {c['n_accept']})", flush=True)


if __name__ == "__main__":
    main()
