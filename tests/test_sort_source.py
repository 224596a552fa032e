"""Order statistics for simulators from source (csrc/sort_network.hpp: sabc::sort_ascending, order_statistic, quantile) and the
model shipped on them, GandKQuantiles (device_sources/gk_quantiles.hip).

CPU: the compiler stage of a source that calls every new function and of the shipped model (hipRTC needs no device), and the
model class' checks.  GPU: the forward run of a probe that emits a sample unsorted and sorted -- the sorted half IS np.sort
of the unsorted half, bit for bit, at the sizes where a network goes wrong (1, non-powers of two on both sides of a power, the
unrolled | loop boundary 32 | 33) --, population runs of the model against the oracle driving a Python transcription with the
same Philox blocks in all four kernel forms, and the posterior-predictive shape.

GPU time on an MI355X: 29 s for the 16 GPU tests, most of it the run-time compiler -- 1.0 to 1.2 s per probe source (eleven
of them, compiled without the one-launch kernels a forward run never launches: with them 4.7 to 6.7 s each) and 12.7 s for
the model's sixteen kernels; the runs themselves and the oracle's transcription (n = 1000 and n = 3000, once each, shared)
are 0.3 to 2 s."""
import numpy as np
import pytest

from tests.cases import SEED, oracle_proposal

# every function the header adds, in one simulator: both forms of the sort for double and float, the rank and the quantile
EVERY_CALL_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  double x[6], y[40];
  float xf[6], yf[40];
  double z0, z1;
  for (int i = 0; i < 40; i += 2) {
    rng.pair(z0, z1);
    y[i] = theta[0] + z0;
    y[i + 1] = theta[0] + z1;
    yf[i] = (float)z0;
    yf[i + 1] = (float)z1;
  }
  for (int i = 0; i < 6; ++i) { x[i] = y[i]; xf[i] = yf[i]; }
  sabc::sort_ascending(x);                   // template form, unrolled
  sabc::sort_ascending(y);                   // template form above 32 elements: the loop form
  sabc::sort_ascending(y, (int)p[0]);        // loop form, n at run time
  sabc::sort_ascending(xf);
  sabc::sort_ascending(yf);
  sabc::sort_ascending(yf, (int)p[0]);
  rho[0] = fabs(sabc::order_statistic(x, 6, 3) - p[1]) + fabs((double)xf[2] + (double)yf[7]);
  rho[1] = fabs(sabc::quantile(y, 40, 0.25) - p[1]);
}
"""

# A sample of PROBE_N draws through for_pairs (an odd last draw through pair()), emitted as it was drawn (outputs 0..N-1) and
# sorted (N..2N-1).  PROBE_LOOP: the loop form with n read from params at run time; else the template form.
PROBE_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  constexpr int N = PROBE_N;
  double x[N];
  int at = 0;
  rng.for_pairs(N >> 1, [&](const double z0, const double z1) {
    x[at] = theta[0] + theta[1] * z0;
    x[at + 1] = theta[0] + theta[1] * z1;
    at += 2;
  });
  if (N & 1) {
    double z0, z1;
    rng.pair(z0, z1);
    x[N - 1] = theta[0] + theta[1] * z0;
  }
  for (int i = 0; i < N; ++i) sabc::emit(rng, i, x[i]);
#if PROBE_LOOP
  sabc::sort_ascending(&x[0], (int)p[0]);
#else
  sabc::sort_ascending(x);
#endif
  for (int i = 0; i < N; ++i) sabc::emit(rng, N + i, x[i]);
  rho[0] = fabs(x[0]);
}
"""

# Eight draws with a NaN and duplicates planted by construction: outputs 0..7 as planted, 8..15 sorted by the template form,
# 16..23 by the loop form.  (Copies of one draw are equal bits whatever the draw is.)
PLANTED_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  double x[8], y[8];
  int at = 0;
  rng.for_pairs(4, [&](const double z0, const double z1) {
    x[at] = theta[0] + theta[1] * z0;
    x[at + 1] = theta[0] + theta[1] * z1;
    at += 2;
  });
  x[1] = __builtin_nan("");
  x[3] = x[0];
  x[5] = x[0];
  x[6] = x[2];
  for (int i = 0; i < 8; ++i) { y[i] = x[i]; sabc::emit(rng, i, x[i]); }
  sabc::sort_ascending(x);
  sabc::sort_ascending(&y[0], (int)p[0]);
  for (int i = 0; i < 8; ++i) { sabc::emit(rng, 8 + i, x[i]); sabc::emit(rng, 16 + i, y[i]); }
  rho[0] = fabs(x[0]);
}
"""


def probe(S, n, loop):
    return S.DeviceSource(f"#define PROBE_N {n}\n#define PROBE_LOOP {int(loop)}\n" + PROBE_SRC, 2, 1, [n], n_outputs=2 * n)


def probe_theta():
    rng = np.random.default_rng(SEED)
    return np.column_stack([rng.normal(0.0, 3.0, 256), rng.uniform(0.1, 4.0, 256)])


# ---- CPU ----

def test_a_source_that_calls_every_new_function_compiles(S):
    assert S.DeviceSource(EVERY_CALL_SRC, 1, 2, [40, 0.5]).compile_check()


def test_gk_quantiles_compiles(S):
    # 33 draws: the loop form and the odd last draw (the GPU tests below run the unrolled network of 32; one compilation here,
    # each is the unit's sixteen kernels)
    assert S.GandKQuantiles((0.25, 0.5, 0.75), (1.0, 2.0, 3.0), n_draws=33).compile_check()


def test_gk_quantiles_checks_its_arguments(S):
    with pytest.raises(ValueError, match="same number"):
        S.GandKQuantiles((0.25, 0.5, 0.75), (1.0, 2.0))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        S.GandKQuantiles((0.25, 1.5), (1.0, 2.0))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        S.GandKQuantiles((-0.1, 0.5), (1.0, 2.0))
    with pytest.raises(ValueError, match="1 to 16"):
        S.GandKQuantiles(np.linspace(0.0, 1.0, 17), np.zeros(17))
    with pytest.raises(ValueError, match="1 to 16"):
        S.GandKQuantiles((), ())
    for n_draws in (1, 0, -3, 2.5, True):
        with pytest.raises(ValueError, match="n_draws"):
            S.GandKQuantiles((0.5,), (1.0,), n_draws=n_draws)
    model = S.GandKQuantiles((0.25, 0.5, 0.75), (1.0, 2.0, 3.0), n_draws=32, c=0.7)
    assert (model.n_stats, model.n_para, model.params, model.n_outputs_for()) == (3, (4,), [32.0, 0.7], 32)
    assert model.source.startswith("#define GKQ_N_DRAWS 32\n#define GKQ_N_STATS 3\n")
    # data that arrive later pass the same checks: validate_data is what sabc(..., probs=, q_obs=) and set_data call
    seg = lambda *a: [np.asarray(x, dtype=np.float64) for x in a]
    model.validate_data(seg((0.1, 0.2, 0.9), (0.0, 1.0, 5.0)))
    with pytest.raises(ValueError, match="same number"):
        model.validate_data(seg((0.1, 0.2, 0.9), (0.0, 1.0)))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        model.validate_data(seg((0.1, 0.2, 1.0 + 1e-12), (0.0, 1.0, 5.0)))
    with pytest.raises(ValueError, match="3 quantiles"):                       # rho has n_stats slots: the source writes no other number
        model.validate_data(seg((0.1, 0.2), (0.0, 1.0)))
    with pytest.raises(ValueError):
        model.bind_data((), dict(probs=(0.1, 0.2, 0.3), q_obs=(1.0, 2.0)))


def test_from_observations_reproduces_np_quantile(S):
    y = np.random.default_rng(SEED).normal(3.0, 2.0, 57)
    model = S.GandKQuantiles.from_observations(y)
    octiles = np.arange(1, 8) / 8
    np.testing.assert_array_equal(model.data[0], octiles)
    np.testing.assert_array_equal(model.data[1], np.quantile(y, octiles))
    assert (model.n_draws, model.n_stats, model.c) == (57, 7, 0.8)
    model = S.GandKQuantiles.from_observations(y, probs=(0.1, 0.9), n_draws=16, c=0.5)
    np.testing.assert_array_equal(model.data[1], np.quantile(y, (0.1, 0.9)))
    assert (model.n_draws, model.n_stats, model.c) == (16, 2, 0.5)


# ---- GPU: the forward run ----

@pytest.mark.gpu
@pytest.mark.parametrize("n,loop", [(1, False), (2, False), (3, False), (5, False), (8, False), (17, False), (32, False),
                                    (33, True), (100, True), (257, True)])
def test_the_sorted_half_is_np_sort_of_the_unsorted_half(S, gpu, monkeypatch, n, loop):
    monkeypatch.setenv("SABC_PERSISTENT", "0")      # a forward run is a lane per simulation: the unit without its one-launch kernels, 7 of 16
    out = S.simulate_outputs(probe(S, n, loop), probe_theta(), seed=SEED)
    assert out.shape == (256, 1, 2 * n)
    drawn, ordered = out[:, 0, :n], out[:, 0, n:]
    assert np.isfinite(drawn).all() and (n < 2 or (np.diff(drawn, axis=1) < 0).any())      # a sample, not an ascending ramp
    np.testing.assert_array_equal(ordered, np.sort(drawn, axis=1))


@pytest.mark.gpu
def test_a_planted_nan_and_duplicates(S, gpu, monkeypatch):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    out = S.simulate_outputs(S.DeviceSource(PLANTED_SRC, 2, 1, [8], n_outputs=24), probe_theta(), seed=SEED)[:, 0, :]
    planted = out[:, :8]
    assert np.isnan(planted[:, 1]).all() and np.isfinite(np.delete(planted, 1, axis=1)).all()
    assert (planted[:, 3] == planted[:, 0]).all() and (planted[:, 5] == planted[:, 0]).all() and (planted[:, 6] == planted[:, 2]).all()
    expect = np.sort(np.where(np.isnan(planted), np.inf, planted), axis=1)      # the NaN enters as +inf and comes out last
    np.testing.assert_array_equal(out[:, 8:16], expect)
    np.testing.assert_array_equal(out[:, 16:24], expect)
    assert (expect[:, 7] == np.inf).all()


# ---- GPU: population runs against the oracle ----
GK_PROBS, GK_DRAWS, GK_C, GK_UPDATES = (0.25, 0.5, 0.75), 32, 0.8, 6
# a box inside which no draw overflows: |z| <= 8.57 (the f64 normals' reach), so (1 + z^2)^k <= 74.5^1.5 = 643 and
# |x| <= 6 + 3 * 1.8 * 643 * 8.57
GK_BOX = [(1.0, 6.0), (0.2, 3.0), (-1.0, 3.0), (0.0, 1.5)]


def gk_q_obs():
    z = np.random.default_rng(SEED).normal(size=400)
    x = 3.0 + 1.0 * (1.0 + GK_C * np.tanh(2.0 * z / 2.0)) * (1.0 + z * z) ** 0.5 * z
    return np.quantile(x, GK_PROBS)


def quantile_type7(x, p):
    h = (len(x) - 1) * p
    i = int(np.floor(h))
    return float(x[-1]) if i >= len(x) - 1 else float(x[i] + (h - i) * (x[i + 1] - x[i]))


def gk_quantiles_f(O, q_obs, seen):
    """device_sources/gk_quantiles.hip over the oracle's Philox blocks; every distance it returns is also noted in `seen`"""
    def f(θ, pid, it):
        A, B, g, k = (float(t) for t in θ)
        z = np.array([O.normal_pair(SEED, pid, O.PURPOSE_SIM, it, b) for b in range(GK_DRAWS // 2)]).reshape(-1)
        x = np.sort(A + B * (1.0 + GK_C * np.tanh(g * z / 2.0)) * np.exp(k * np.log1p(z * z)) * z)
        rho = tuple(abs(quantile_type7(x, p) - q) for p, q in zip(GK_PROBS, q_obs))
        seen.extend(rho)
        return rho
    return f


def oracle_gk_run(O, n):
    seen = []
    cfg = O.make_config(n_particles=n, n_para=4, n_stats=3, model_id=O.MODEL_HOST, model_params=[], seed=SEED,
                        prior=[(O.PRIOR_UNIFORM, lo, hi) for lo, hi in GK_BOX], host_fn=O.host_simulator(gk_quantiles_f(O, gk_q_obs(), seen), 4, 3),
                        algorithm=O.ALG_MULTI_EPS)
    run = O.OracleRun(cfg)
    run.initialize((GK_UPDATES + 1) * n)
    run.update(O.make_update_args(n_simulation=GK_UPDATES * n, proposal=oracle_proposal(O, "rw", 4), n_para=4, n_particles=n, resample=n // 2))
    # copies: the arrays are read once and shared by the tests below, which leave them unchanged
    return dict(counters=dict(run.counters), theta=np.array(run.theta), rho=np.array(run.rho), eps=np.array(run.eps), seen=np.array(seen))


@pytest.fixture(scope="module")
def oracle_small(O):
    return oracle_gk_run(O, 1000)


@pytest.fixture(scope="module")
def oracle_chain(O):
    return oracle_gk_run(O, 3000)


def device_gk_run(S, n):
    prior = S.product_distribution([S.Uniform(lo, hi) for lo, hi in GK_BOX])
    model = S.GandKQuantiles(GK_PROBS, gk_q_obs(), n_draws=GK_DRAWS, c=GK_C)
    return S.sabc(model, prior, n_particles=n, n_simulation=(GK_UPDATES + 1) * n, proposal=S.RandomWalk(n_para=4), resample=n // 2,
                  algorithm="multi_eps", seed=SEED)


def assert_matches_the_oracle(res, ref):
    # the transcription first: inside the box every distance is finite, so no particle has to be excluded anywhere
    assert len(ref["seen"]) >= 3 * len(res.population) and np.isfinite(ref["seen"]).all()
    assert not (res.ρ == 1e30).any() and not any((np.asarray(r) == 1e30).any() for r in res.state.ρ_history)
    c = ref["counters"]
    assert (res.state.n_accept, res.state.n_resampling) == (c["n_accept"], c["n_resampling"])
    np.testing.assert_allclose(res.population.T, ref["theta"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(res.ρ.T, ref["rho"], rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(res.state.ϵ, ref["eps"], rtol=1e-9)


SMALL_ACCEPTS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_gk_quantiles_in_one_launch_against_the_oracle(S, gpu, monkeypatch, oracle_small, lanes):
    """n = 1000: the one-launch form with a lane, a quad and a row of 16 lanes per particle.  Every lane of a team sorts the
    whole sample; a sorted array is unique, so the three runs are the oracle's run and each other's."""
    monkeypatch.setenv("SABC_PERSISTENT", "1")
    monkeypatch.setenv("SABC_PERSISTENT_LANES", str(lanes))
    res = device_gk_run(S, 1000)
    assert res._handle.persistent_lanes == lanes
    assert_matches_the_oracle(res, oracle_small)
    SMALL_ACCEPTS[lanes] = res.state.n_accept
    assert len(set(SMALL_ACCEPTS.values())) == 1, SMALL_ACCEPTS


@pytest.mark.gpu
def test_gk_quantiles_on_the_launch_chain_against_the_oracle(S, gpu, monkeypatch, oracle_chain):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_gk_run(S, 3000)
    assert res._handle.persistent_lanes == 0
    assert_matches_the_oracle(res, oracle_chain)


@pytest.mark.gpu
def test_posterior_predictive_is_the_sorted_sample(S, gpu):
    n = 500
    res = device_gk_run(S, n)
    pp = S.posterior_predictive(res, n_rep=2)
    assert pp.shape == (n, 2, GK_DRAWS)
    assert np.isfinite(pp).all() and (np.diff(pp, axis=2) >= 0).all()
    assert len(np.unique(pp[:, 0, :])) > n                                   # samples, not one constant
