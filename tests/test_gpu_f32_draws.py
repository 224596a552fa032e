"""The binary32 draws on the device (csrc/device_rng.hpp, namespace f32) against their NumPy restatement
(tests/elementary_f32_ref.py): bit for bit from the stand-alone operator and through a simulator compiled at run time, the
stream's position after them in every kernel form a source simulator runs in, and the shipped LotkaVolterraF32 against the
oracle over its restatement.  The oracle side of each parity case is computed once and shared across the parameters."""
import math

import numpy as np
import pytest

from tests import elementary_f32_ref as E
from tests.cases import SEED
from tests.test_f32_draws import LV_OBS, POSITION_SRC, POSITION_TARGET, PROBE_SRC, position_f, probe_ref

pytestmark = pytest.mark.gpu

LV_HI = (2.0, 0.1, 2.0)


@pytest.mark.parametrize("purpose", [1, 6])
@pytest.mark.parametrize("pid0,it,k", [(77, 3, 0), ((1 << 33) + 12345, 900, 7)])
def test_normal_quads_equal_the_restatement_bit_for_bit(S, gpu, pid0, it, k, purpose):
    m = 4096
    got = S.op_normal_quads_f32(SEED, pid0, m, purpose=purpose, it=it, k=k)
    want = E.box_muller_quad(E.philox_blocks(SEED, pid0 + np.arange(m, dtype=np.uint64), purpose, it, k))
    assert got.shape == want.shape == (m, 4) and got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.abs(got).max() > 3.0


def test_draws_through_a_run_time_compiled_simulator_equal_the_restatement(S, O, gpu):
    """8 x quad_f32, 4 x uniform_quad_f32, a for_quads_f32 of 5 blocks (the binary32 tables in LDS, filled by the loop), then
    pair(): block 17 of the stream, its f64 bits intact.  Pins the run-time compiler's defaults too (the correctly rounded sqrt)."""
    m, pid0, it = 300, (1 << 33) + 99, 11
    h = S.SabcHandle(n_particles=256, model=S.DeviceSource(PROBE_SRC, 1, 64, []), prior=S.Uniform(0.0, 1.0), seed=SEED)
    got = h.simulate(np.zeros((1, m)), pid0, it)
    h.close()
    want = np.array([probe_ref(O, pid0 + i, it) for i in range(m)]).T
    assert got.shape == want.shape == (64, m)
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.all((got[32:48] > 0.0) & (got[32:48] < 1.0)) and np.all(got[55:] == 0.0)


# ---------------------------------------------------------------- the stream's position, kernel form by kernel form
_POSITION_RUNS = {}


def position_oracle(O, n, k, proposal):
    key = (n, k, proposal)
    if key not in _POSITION_RUNS:
        cfg = O.make_config(n_particles=n, n_para=1, n_stats=4, model_id=O.MODEL_HOST, model_params=[], seed=SEED,
                            prior=[(O.PRIOR_UNIFORM, 0.0, 70.0)], algorithm=O.ALG_MULTI_EPS,
                            host_fn=O.host_simulator(lambda th, pid, it: position_f(O, pid, it, th), 1, 4))
        run = O.OracleRun(cfg)
        run.initialize((k + 1) * n)
        prop = (O.PROP_RANDOMWALK, 0.8, 0.0) if proposal == "rw" else (O.PROP_DIFFEVO, None, 1e-5)
        run.update(O.make_update_args(n_simulation=k * n, proposal=prop, n_para=1, n_particles=n, resample=10 ** 9))
        _POSITION_RUNS[key] = run
    return _POSITION_RUNS[key]


def position_model(S):
    return S.DeviceSource(POSITION_SRC, 1, 4, [POSITION_TARGET])


def device_position_run(S, n, k, proposal, prior=None):
    h = S.SabcHandle(n_particles=n, model=position_model(S), prior=S.Uniform(0.0, 70.0) if prior is None else prior, seed=SEED,
                     algorithm=S._lib.ALG_MULTI_EPS)
    try:
        h.initialize((k + 1) * n)
        h.update(n_simulation=k * n, proposal=proposal, resample=10 ** 9)
        return dict(h.counters), h.get_population(), h.persistent_lanes
    finally:
        h.close()


@pytest.mark.parametrize("lanes", [0, 1, 4, 16])
def test_for_quads_f32_leaves_the_stream_at_its_block_count(S, O, gpu, monkeypatch, lanes):
    """lanes = 0: the launch chain; 1, 4, 16: one launch per call with a lane, a quad, a row of lanes per particle.  The quad
    and the pair drawn after the loop are those of blocks n and n + 1 wherever in a group of the team the loop ended."""
    n, k = 512, 3
    monkeypatch.setenv("SABC_PERSISTENT", "0" if lanes == 0 else "1")
    if lanes:
        monkeypatch.setenv("SABC_PERSISTENT_LANES", str(lanes))
    counters, (theta, _, rho), ran = device_position_run(S, n, k, S.RandomWalk(n_para=1))
    run = position_oracle(O, n, k, "rw")
    assert ran == lanes
    assert counters["n_accept"] == run.counters["n_accept"] > 0
    trips = set((1 + np.floor(theta[0])).astype(int))
    # whole groups of 4 W and every length of tail, for teams of 4 and of 16 (70 = 4 x 16 + 6 is the longest loop)
    assert trips >= {1, 4, 5, 16, 17, 23, 64, 65, 70}, sorted(trips)
    np.testing.assert_allclose(theta, run.theta, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(rho, run.rho, rtol=1e-9, atol=1e-12)


def test_a_host_prior_between_the_propose_and_accept_kernels(S, gpu, monkeypatch):
    """With a HostPrior k_simulate_batch sits between the two: the same run as with the prior as data."""
    from scipy import stats
    n, k = 512, 2
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    ref_counters, (ref_theta, _, ref_rho), _ = device_position_run(S, n, k, S.RandomWalk(n_para=1))
    helper = S.SabcHandle(n_particles=256, model=position_model(S), prior=S.Uniform(0.0, 70.0), seed=SEED)

    def sample(ids):
        return helper.prior(int(ids[0]), len(ids))[0].T
    try:
        prior = S.HostPrior(sample, lambda th: stats.uniform(0.0, 70.0).logpdf(th[:, 0]), 1)
        counters, (theta, _, rho), _ = device_position_run(S, n, k, S.RandomWalk(n_para=1), prior=prior)
    finally:
        helper.close()
    assert counters["n_accept"] == ref_counters["n_accept"] > 0
    np.testing.assert_allclose(theta, ref_theta, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(rho, ref_rho, rtol=1e-9, atol=1e-12)


def test_differential_evolution_on_the_launch_chain(S, O, gpu, monkeypatch):
    n, k = 512, 2
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    counters, (theta, _, rho), ran = device_position_run(S, n, k, S.DifferentialEvolution(n_para=1))
    run = position_oracle(O, n, k, "de")
    assert ran == 0
    assert counters["n_accept"] == run.counters["n_accept"] > 0
    np.testing.assert_allclose(theta, run.theta, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(rho, run.rho, rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------- LotkaVolterraF32
def lv_params(n_steps=256):
    return [n_steps, 0.05, 0.1, 50.0, 50.0, *LV_OBS]


LV_PARITY_STEPS = 63          # odd: 31 blocks by for_quads_f32 and half of a 32nd by quad_f32


def lv_host_fn(O, n):
    """The restatement as the oracle's host simulator.  The oracle asks particle by particle; the normals do not depend on
    theta, so those of a whole iteration are restated at once, the first time one of them is asked for."""
    normals = {}
    n_blocks = (LV_PARITY_STEPS + 1) // 2

    def f(theta, pid, it):
        if it not in normals:
            w = E.philox_blocks(SEED, np.arange(n, dtype=np.uint64)[:, None], 1, it, np.arange(n_blocks)[None, :])
            normals[it] = E.box_muller_quad(w.reshape(-1, 4)).reshape(n, n_blocks, 4)
        return E.lv_f32_one(theta, lv_params(LV_PARITY_STEPS), normals[it][pid])
    return O.host_simulator(f, 3, 4)


def test_lotka_volterra_f32_runs_like_the_oracle_over_its_restatement(S, O, gpu):
    n, k = 1000, 5
    fn = lv_host_fn(O, n)
    cfg = O.make_config(n_particles=n, n_para=3, n_stats=4, model_id=O.MODEL_HOST, model_params=[], seed=SEED,
                        prior=[(O.PRIOR_UNIFORM, 0.0, hi) for hi in LV_HI], algorithm=O.ALG_MULTI_EPS, host_fn=fn)
    run = O.OracleRun(cfg)
    run.initialize((k + 1) * n)
    run.update(O.make_update_args(n_simulation=k * n, proposal=(O.PROP_RANDOMWALK, 0.8, 0.0), n_para=3, n_particles=n,
                                  resample=10 ** 9))
    h = S.SabcHandle(n_particles=n, model=S.LotkaVolterraF32(n_steps=LV_PARITY_STEPS, obs=LV_OBS), seed=SEED,
                     algorithm=S._lib.ALG_MULTI_EPS, prior=S.product_distribution([S.Uniform(0.0, hi) for hi in LV_HI]))
    try:
        h.initialize((k + 1) * n)
        h.update(n_simulation=k * n, proposal=S.RandomWalk(n_para=3), resample=10 ** 9)
        counters, (theta, _, rho) = dict(h.counters), h.get_population()
    finally:
        h.close()
    assert counters["n_accept"] == run.counters["n_accept"] > 0
    np.testing.assert_allclose(theta, run.theta, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(rho, run.rho, rtol=1e-9, atol=1e-12)


def test_lotka_volterra_f32_emits_its_paths(S, gpu):
    n = 1000
    model = S.LotkaVolterraF32(obs=LV_OBS)
    prior = S.product_distribution([S.Uniform(0.0, hi) for hi in LV_HI])
    res = S.initialization(model, prior, n_particles=n, n_simulation=n, seed=SEED, algorithm="multi_eps")
    try:
        pp = S.posterior_predictive(res, n_rep=2)
        assert pp.shape == (n, 2, 512) and not np.any(np.isnan(pp))
        assert not np.array_equal(pp[:, 0], pp[:, 1])
        theta = np.ascontiguousarray(res.population.T)[:, :200]
        rho, out = res._handle.simulate_outputs(theta, 40, 3, stream="update")
        np.testing.assert_array_equal(rho, res._handle.simulate(theta, 40, 3))
        want_rho, want_out = E.lv_f32(theta, lv_params(), SEED, 40 + np.arange(200), 3, paths=True)
        np.testing.assert_array_equal(out, want_out)                            # the paths are binary32 values: equal or not
        np.testing.assert_allclose(rho, want_rho, rtol=1e-12, atol=0.0)
    finally:
        res._handle.close()


def test_rng_peak_f32_returns_a_rate(S, gpu):
    for args in ((1, 1, 1), (4096, 8, 2)):
        rate = S.op_rng_peak_f32(*args)
        assert math.isfinite(rate) and rate > 0.0
