"""Simulators from HIP source with more than 16 summary statistics (SABC_MAX_SOURCE_STATS = 64): the wide form of the
per-particle kernels (csrc/update_kernel.hpp: k_update_wide and its companions).  The reference's f_dist may return any number
of distances (SimulatedAnnealingABC.jl:163-167,181); one per time point of an observed series is the common case.

CPU: the compiler stage at the new shapes, the limit, and the code object of the wide update kernel (no scratch).
GPU: against the oracle's host-callback model driven by a Python restatement of the same arithmetic with the same Philox
blocks (O.normal_pair), as tests/test_user_simulator.py does for the narrow shapes."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.cases import SEED, hip_proposal, oracle_proposal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- a time series of 48 points: y_t = a + b x_t + c x_t^2 + sigma z_t, one distance |y_t - obs_t| per point ----
# The observations travel in the source (a __constant__ array): the 32 model parameters could not hold them.
T = 48
X = [t / (T - 1) - 0.5 for t in range(T)]
TRUTH, SIGMA = (0.6, -0.8, 1.5), 0.3
OBS = [float(v) for v in TRUTH[0] + TRUTH[1] * np.array(X) + TRUTH[2] * np.array(X) ** 2
       + SIGMA * np.random.default_rng(7).normal(size=T)]


def _carray(name, vals):
    return f"__constant__ double {name}[{len(vals)}] = {{" + ", ".join(repr(float(v)) for v in vals) + "};\n"


SERIES_SRC = _carray("kX", X) + _carray("kObs", OBS) + r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  for (int t = 0; t < 48; t += 2) {
    double z0, z1;
    rng.pair(z0, z1);
    rho[t] = fabs(theta[0] + theta[1] * kX[t] + theta[2] * kX[t] * kX[t] + p[0] * z0 - kObs[t]);
    rho[t + 1] = fabs(theta[0] + theta[1] * kX[t + 1] + theta[2] * kX[t + 1] * kX[t + 1] + p[0] * z1 - kObs[t + 1]);
  }
}
"""


def series_f(O, pid, it, θ):
    th = np.atleast_1d(θ)
    out = np.empty(T)
    for b in range(T // 2):
        z = O.normal_pair(SEED, pid, O.PURPOSE_SIM, it, b)
        for q in range(2):
            t = 2 * b + q
            out[t] = abs(th[0] + th[1] * X[t] + th[2] * X[t] * X[t] + SIGMA * z[q] - OBS[t])
    return out


# ---- any (d, s): distance j from parameters j % d and (j + 1) % d, targets in the source ----
WIDE_TARGETS = [0.3 * ((j % 5) - 2) for j in range(64)]
SHAPE_SRC = _carray("kTarget", WIDE_TARGETS) + r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const int d = (int)p[0], s = (int)p[1];
  for (int j = 0; j < s; ++j) {
    const double z = rng.next();
    rho[j] = fabs(theta[j % d] + 0.5 * theta[(j + 1) % d] + p[2] * z - kTarget[j]);
  }
}
"""


def shape_f(O, d, s):
    def f(θ, pid, it):
        th = np.atleast_1d(θ)
        return tuple(abs(th[j % d] + 0.5 * th[(j + 1) % d] + 0.4 * O.normal_pair(SEED, pid, O.PURPOSE_SIM, it, j // 2)[j % 2]
                         - WIDE_TARGETS[j]) for j in range(s))
    return f


TOL = {"rw": 1e-8, "stretch": 1e-6, "de": 1e-5}


# ---------------------------------------------------------------- CPU
def test_the_limit_is_the_header_value(S):
    text = open(os.path.join(ROOT, "include", "sabc_hip.h")).read()
    assert int(re.search(r"#define SABC_MAX_SOURCE_STATS (\d+)", text).group(1)) == S._lib.MAX_SOURCE_STATS == 64


@pytest.mark.parametrize("d,s", [(1, 17), (3, 48), (16, 64)])
def test_wide_shapes_compile_without_a_device(S, d, s):
    assert S.DeviceSource(SHAPE_SRC, d, s, [d, s, 0.4]).compile_check()


def test_more_than_64_statistics_are_refused(S):
    with pytest.raises(S.SABCError):
        S.DeviceSource(SHAPE_SRC, 3, 65, [3, 65, 0.4]).compile_check()


def test_the_wide_update_kernel_uses_no_scratch(S, tmp_path, monkeypatch):
    """The distances of a particle live in LDS, its transforms in registers: the code object's metadata of k_update_wide at
    (3, 48) shows no private segment."""
    path = tmp_path / "series.co"
    monkeypatch.setenv("SABC_RTC_CODE_OUT", str(path))
    assert S.DeviceSource(SERIES_SRC, 3, T, [SIGMA]).compile_check()
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    notes = subprocess.run([readelf, "--notes", str(path)], check=True, capture_output=True, text=True).stdout
    kernels = re.split(r"\n\s*- \.", notes)
    found = 0
    for k in kernels:
        name = re.search(r"\.name:\s+(\S+)", k)
        if not name or "k_update_wide" not in name.group(1):
            continue
        found += 1
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", k).group(1)) == 0, name.group(1)
        assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", k).group(1)) <= 64 * 1024
    assert found == 3                                       # RandomWalk, DifferentialEvolution, StretchMove


# ---------------------------------------------------------------- GPU
def oracle_run(O, d, s, f, n, k, alg, prop, prior, resample=None):
    cfg = O.make_config(n_particles=n, n_para=d, n_stats=s, model_id=O.MODEL_HOST, model_params=[], seed=SEED,
                        prior=prior, host_fn=O.host_simulator(f, d, s),
                        algorithm=O.ALG_MULTI_EPS if alg == "multi_eps" else O.ALG_SINGLE_EPS)
    run = O.OracleRun(cfg)
    run.initialize((k + 1) * n)
    run.update(O.make_update_args(n_simulation=k * n, proposal=oracle_proposal(O, prop, d), n_para=d, n_particles=n,
                                  resample=resample or n // 4))
    return run


def assert_same_run(res, run, n, prop):
    c = run.counters
    assert (res.state.n_accept, res.state.n_resampling) == (c["n_accept"], c["n_resampling"])
    assert res.state.n_resampling >= 2
    tol = TOL[prop]
    np.testing.assert_allclose(res.population.reshape(n, -1).T, run.theta, rtol=tol, atol=tol * 1e-3)
    np.testing.assert_allclose(res.ρ.T, run.rho, rtol=tol, atol=tol * 1e-3)
    np.testing.assert_allclose(res.state.ϵ, run.eps, rtol=tol)
    e, _, _ = run.history
    np.testing.assert_allclose(np.array(res.state.ϵ_history), e, rtol=tol)


SERIES_PRIOR = [(0, 0.0, 1.0), (0, 0.0, 1.0), (0, 0.0, 2.0)]       # Normal(mu, sigma) x 3


def series_prior(S):
    return S.product_distribution([S.Normal(0.0, 1.0), S.Normal(0.0, 1.0), S.Normal(0.0, 2.0)])


@pytest.mark.gpu
@pytest.mark.parametrize("alg,prop", [("multi_eps", "rw"), ("single_eps", "de"), ("multi_eps", "stretch")])
def test_a_time_series_of_48_points_against_the_oracle(S, O, gpu, alg, prop):
    n, k, d = 1500, 5, 3
    res = S.sabc(S.DeviceSource(SERIES_SRC, d, T, [SIGMA]), series_prior(S), n_particles=n, n_simulation=(k + 1) * n,
                 proposal=hip_proposal(S, prop, d), resample=n // 4, algorithm=alg, seed=SEED)
    prior = [(O.PRIOR_NORMAL, a, b) for _, a, b in SERIES_PRIOR]
    run = oracle_run(O, d, T, lambda θ, pid, it: tuple(series_f(O, pid, it, θ)), n, k, alg, prop, prior)
    assert_same_run(res, run, n, prop)


@pytest.mark.gpu
@pytest.mark.parametrize("d,s,n,k,resample", [(16, 64, 1000, 6, 125), (5, 17, 1500, 5, 375)])
def test_the_largest_and_the_boundary_shape_against_the_oracle(S, O, gpu, d, s, n, k, resample):
    prior = S.product_distribution([S.Normal(0.0, 1.0)] * d)
    res = S.sabc(S.DeviceSource(SHAPE_SRC, d, s, [d, s, 0.4]), prior, n_particles=n, n_simulation=(k + 1) * n,
                 proposal=S.RandomWalk(n_para=d), resample=resample, algorithm="multi_eps", seed=SEED)
    run = oracle_run(O, d, s, shape_f(O, d, s), n, k, "multi_eps", "rw", [(O.PRIOR_NORMAL, 0.0, 1.0)] * d, resample)
    assert_same_run(res, run, n, "rw")


@pytest.mark.gpu
def test_a_small_population_takes_the_launch_chain(S, O, gpu, monkeypatch):
    """n = 1000 runs in one launch per call at s <= 16; the wide form has no such launch and must never try it."""
    monkeypatch.setenv("SABC_PERSISTENT", "1")
    n, k, d = 1000, 5, 3
    h = S.SabcHandle(n_particles=n, model=S.DeviceSource(SERIES_SRC, d, T, [SIGMA]), prior=series_prior(S), seed=SEED,
                     algorithm=S._lib.ALG_MULTI_EPS)
    h.initialize((k + 1) * n)
    h.update(n_simulation=k * n, proposal=S.RandomWalk(n_para=d), resample=n // 4)
    counters, eps, (theta, _, rho), launches = dict(h.counters), h.eps.copy(), h.get_population(), h.persistent_launches
    h.close()
    prior = [(O.PRIOR_NORMAL, a, b) for _, a, b in SERIES_PRIOR]
    run = oracle_run(O, d, T, lambda θ, pid, it: tuple(series_f(O, pid, it, θ)), n, k, "multi_eps", "rw", prior)
    assert launches == 0
    c = run.counters
    assert (counters["n_accept"], counters["n_resampling"]) == (c["n_accept"], c["n_resampling"]) and c["n_resampling"] >= 2
    np.testing.assert_allclose(theta, run.theta, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(rho, run.rho, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(eps, run.eps, rtol=1e-8)


@pytest.mark.gpu
def test_simulate_at_48_statistics_matches_numpy(S, O, gpu):
    d, m, pid0, it = 3, 300, 1234, 7
    h = S.SabcHandle(n_particles=256, model=S.DeviceSource(SERIES_SRC, d, T, [SIGMA]), prior=series_prior(S), seed=SEED)
    theta = np.random.default_rng(1).normal(size=(d, m))
    rho = h.simulate(theta, pid0, it)
    h.close()
    want = np.stack([series_f(O, pid0 + i, it, theta[:, i]) for i in range(m)], axis=1)
    assert rho.shape == (T, m)
    np.testing.assert_allclose(rho, want, rtol=1e-9, atol=1e-12)


@pytest.mark.gpu
def test_a_host_prior_next_to_a_wide_source_simulator(S, gpu):
    """The same prior once as data and once as host callbacks that return the device's own draws: the same run."""
    from scipy import stats
    n, k, d = 600, 5, 3
    model = S.DeviceSource(SERIES_SRC, d, T, [SIGMA])
    kw = dict(n_particles=n, n_simulation=(k + 1) * n, proposal=S.RandomWalk(n_para=d), resample=n // 4, seed=SEED,
              algorithm="multi_eps")
    ref = S.sabc(model, series_prior(S), **kw)
    helper = S.SabcHandle(n_particles=256, model=model, prior=series_prior(S), seed=SEED)

    def sample(ids):
        th, _ = helper.prior(int(ids[0]), len(ids))
        return th.T

    def logpdf(th):
        return sum(stats.norm(a, b).logpdf(th[:, i]) for i, (_, a, b) in enumerate(SERIES_PRIOR))
    res = S.sabc(model, S.HostPrior(sample, logpdf, d), **kw)
    helper.close()
    assert (res.state.n_accept, res.state.n_resampling) == (ref.state.n_accept, ref.state.n_resampling)
    assert ref.state.n_resampling >= 1
    np.testing.assert_allclose(res.population, ref.population, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(res.state.ϵ, ref.state.ϵ, rtol=1e-9)
