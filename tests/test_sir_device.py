"""StochasticSIR -- the stochastic SIR epidemic of the reference's documentation (docs/src/example.md:75-198) as HIP source
on the device generator's event draws (device_sources/sir.hip, NormalStream::while_events) -- and a chain-binomial model on its
count draws.  Against the oracle's host-callback model driving the Python restatement (tests/discrete_draws_ref.py) with the
same Philox blocks; the one-launch forms (a lane, a quad, a row of lanes per particle) against the launch chain; and the
documentation's call end to end."""
import numpy as np
import pytest

from tests.cases import SEED, hip_proposal, oracle_proposal
from tests.discrete_draws_ref import sir_distances
from tests.test_discrete_draws import CHAIN_BINOMIAL_PARAMS, CHAIN_BINOMIAL_SRC, chain_binomial_f

pytestmark = pytest.mark.gpu

PRIOR = [(0.1, 1.0), (0.05, 0.5)]                       # the documentation's: Uniform(0.1, 1) x Uniform(0.05, 0.5)
TOL = {"rw": 1e-9, "de": 1e-6}                          # tests/test_user_simulator.py


def docs_prior(S):
    return S.product_distribution([S.Uniform(*PRIOR[0]), S.Uniform(*PRIOR[1])])


# ---- against the oracle: S0 = 29 (about 30 events per simulation) ----
SMALL = {40.0: dict(S0=29, I0=1, R0=0, t_max=40.0, obs=(22.0, 9.0, 12.0)),
         3.0: dict(S0=29, I0=1, R0=0, t_max=3.0, obs=(1.0, 2.0, 1.5))}      # t_max = 3: most runs leave through t < t_max


@pytest.mark.parametrize("n_stats,alg,prop,t_max", [(3, "multi_eps", "rw", 40.0), (1, "single_eps", "de", 40.0),
                                                    (3, "multi_eps", "rw", 3.0)])
def test_sir_against_the_oracle(S, O, gpu, n_stats, alg, prop, t_max):
    n, k = 1024, 6
    case = SMALL[t_max]
    model = S.StochasticSIR(case["obs"], S0=case["S0"], I0=case["I0"], R0=case["R0"], t_max=t_max, n_stats=n_stats)
    res = S.sabc(model, docs_prior(S), n_particles=n, n_simulation=(k + 1) * n, proposal=hip_proposal(S, prop, 2),
                 resample=n // 2, algorithm=alg, seed=SEED)
    params = model.params

    def f(θ, pid, it):
        return sir_distances(O, SEED, pid, it, θ, params, n_stats)

    cfg = O.make_config(n_particles=n, n_para=2, n_stats=n_stats, model_id=O.MODEL_HOST, model_params=[], seed=SEED,
                        prior=[(O.PRIOR_UNIFORM, *PRIOR[0]), (O.PRIOR_UNIFORM, *PRIOR[1])], host_fn=O.host_simulator(f, 2, n_stats),
                        algorithm=O.ALG_MULTI_EPS if alg == "multi_eps" else O.ALG_SINGLE_EPS)
    run = O.OracleRun(cfg)
    run.initialize((k + 1) * n)
    run.update(O.make_update_args(n_simulation=k * n, proposal=oracle_proposal(O, prop, 2), n_para=2, n_particles=n, resample=n // 2))
    c = run.counters
    assert (res.state.n_accept, res.state.n_resampling, res.state.n_population_updates) == \
        (c["n_accept"], c["n_resampling"], c["n_population_updates"])
    assert res.state.n_accept > n // 4
    tol = TOL[prop]
    np.testing.assert_allclose(res.population.T, run.theta, rtol=tol, atol=tol * 1e-3)
    np.testing.assert_allclose(res.ρ.T, run.rho, rtol=tol, atol=tol * 1e-3)
    np.testing.assert_allclose(res.state.ϵ, run.eps, rtol=tol)


# ---- the one-launch forms against the launch chain ----
def run_forms(S, monkeypatch, model, prior, d, alg, prop, n, k, lanes):
    """lanes = 0: the launch chain | 1, 4, 16: one launch per stretch between two resamples, that many lanes per particle"""
    monkeypatch.setenv("SABC_PERSISTENT", "1" if lanes else "0")
    monkeypatch.setenv("SABC_PERSISTENT_MAX", "65536")
    if lanes:
        monkeypatch.setenv("SABC_PERSISTENT_LANES", str(lanes))
    else:
        monkeypatch.delenv("SABC_PERSISTENT_LANES", raising=False)
    h = S.SabcHandle(n_particles=n, model=model, prior=prior, seed=SEED,
                     algorithm=S._lib.ALG_MULTI_EPS if alg == "multi_eps" else S._lib.ALG_SINGLE_EPS)
    h.initialize((k + 1) * n)
    h.update(n_simulation=k * n, proposal=hip_proposal(S, prop, d), resample=n // 2)
    out = dict(zip(("theta", "u", "rho"), h.get_population()), eps=h.eps.copy(), counters=dict(h.counters), lanes=h.persistent_lanes)
    h.close()
    return out


def assert_same_forms(a, b, prop, lanes):
    assert a["counters"] == b["counters"] and a["counters"]["n_resampling"] >= 3          # (the first is the initial one)
    assert (a["lanes"], b["lanes"]) == (0, lanes)
    tol = 1e-10 if prop == "rw" else 1e-6                  # tests/test_persistent.py
    for key in ("theta", "u", "rho", "eps"):
        np.testing.assert_allclose(b[key], a[key], rtol=tol, atol=tol * 1e-2)


FORMS = [(1000, 16), (3000, 4), (20_000, 1)]


@pytest.mark.parametrize("n,lanes", FORMS)
@pytest.mark.parametrize("n_stats,alg,prop", [(3, "multi_eps", "rw"), (1, "single_eps", "de")])
def test_sir_one_launch_equals_the_launch_chain(S, gpu, monkeypatch, n_stats, alg, prop, n, lanes):
    """The documentation's S0 = 99: up to 199 events per simulation, whose number differs from particle to particle (and, in a
    team, ends anywhere inside a group of 4 | 16 events)."""
    model = S.StochasticSIR((77.0, 30.0, 38.0), n_stats=n_stats)
    a = run_forms(S, monkeypatch, model, docs_prior(S), 2, alg, prop, n, 8, 0)
    b = run_forms(S, monkeypatch, model, docs_prior(S), 2, alg, prop, n, 8, lanes)
    assert_same_forms(a, b, prop, lanes)


def chain_binomial_prior(S):
    return S.product_distribution([S.Uniform(0.0005, 0.01), S.Uniform(0.1, 1.0)])


@pytest.mark.parametrize("n,lanes", FORMS)
def test_chain_binomial_one_launch_equals_the_launch_chain(S, gpu, monkeypatch, n, lanes):
    """binomial() per generation and poisson() observation noise inside teams: the count draws go through uniform_pair, a
    group of W blocks at a time, with a number of rejection trials that differs from particle to particle."""
    model = S.DeviceSource(CHAIN_BINOMIAL_SRC, 2, 2, CHAIN_BINOMIAL_PARAMS)
    a = run_forms(S, monkeypatch, model, chain_binomial_prior(S), 2, "multi_eps", "rw", n, 8, 0)
    b = run_forms(S, monkeypatch, model, chain_binomial_prior(S), 2, "multi_eps", "rw", n, 8, lanes)
    assert_same_forms(a, b, "rw", lanes)


def test_chain_binomial_simulations_equal_the_restatement(S, O, gpu):
    m, pid0, it = 200, 31, 4
    rng = np.random.default_rng(8)
    theta = np.stack([rng.uniform(0.0005, 0.01, m), rng.uniform(0.1, 1.0, m)])
    h = S.SabcHandle(n_particles=256, model=S.DeviceSource(CHAIN_BINOMIAL_SRC, 2, 2, CHAIN_BINOMIAL_PARAMS),
                     prior=chain_binomial_prior(S), seed=SEED)
    rho = h.simulate(theta, pid0, it)
    h.close()
    want = np.array([chain_binomial_f(O, pid0 + i, it, theta[:, i]) for i in range(m)]).T
    np.testing.assert_array_equal(rho, want)
    assert len(np.unique(want[0])) > 20                    # epidemics that took off and epidemics that did not


# ---- the documentation's call ----
def test_the_documentation_s_run_moves_to_the_truth(S, gpu):
    """sabc(f_dist_multi_stats, prior, data_obs; n_simulation = 500_000, n_particles = 5000) with an observation simulated at
    theta = (0.3, 0.1) the way the documentation does (one Gillespie run, its seed 123): the point of the posterior means lies
    within half the distance from the point of the prior means, (0.55, 0.275), to the truth -- 0.153.  A sanity check of the
    whole path, not a measurement: one realisation speaks for its own theta.  Measured: this observation (98 infected, peak 43
    at t = 26.1 -- the final size of beta / gamma = 4) gives means (0.429, 0.110), 0.130 from the truth (beta alone is 0.129 off,
    just beyond HALF OF ITS OWN prior-to-truth distance, 0.125); the first realisation with the final size the truth predicts
    (seed 24: 94 infected, peak 39 at t = 22.8, an early peak) gives (0.455, 0.145), 0.161 from the truth: outside."""
    from sabc_amd.examples import sir_observation
    truth = np.array([0.3, 0.1])
    obs = sir_observation(truth, seed=123)
    assert obs["total_infected"] > 50                      # an epidemic that took off
    res = S.sabc(S.StochasticSIR(obs), docs_prior(S), n_particles=5000, n_simulation=500_000, seed=SEED)
    mean = res.population.mean(axis=0)
    prior_mean = np.array([0.5 * (a + b) for a, b in PRIOR])
    print("posterior mean", mean, "observation", obs, "distance", np.linalg.norm(mean - truth), "of", np.linalg.norm(prior_mean - truth))
    assert res.state.n_simulation <= 500_000 and res.state.n_population_updates == 99
    assert np.linalg.norm(mean - truth) < 0.5 * np.linalg.norm(prior_mean - truth), (mean, truth)
