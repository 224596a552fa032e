"""Outputs of device-coded simulators on the GPU: what a source hands to sabc::emit comes back from the forward run
(sabc_op_simulate_outputs, SabcHandle.simulate_outputs, simulate_outputs, posterior_predictive) value for value -- against its
own inputs, against the oracle's Philox blocks, against the Python restatements of the shipped simulators -- on the update's
stream and on the predictive one; the distances of the call are those of SabcHandle.simulate; what is never emitted is NaN;
large calls run in chunks; and a forward run changes nothing of the handle it runs on."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.cases import SEED
from tests.discrete_draws_ref import Stream, sir_statistics

pytestmark = pytest.mark.gpu

PURPOSE_PREDICT = 6                                    # csrc/device_rng.hpp; the oracle takes the purpose as an argument
PRIOR = [(0.1, 1.0), (0.05, 0.5)]                      # the documentation's box of the SIR example
SMALL = dict(S0=29, I0=1, R0=0, t_max=40.0)            # tests/test_sir_device.py: about 30 events per simulation

PROBE = """
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  double u0, u1, z0, z1;
  rng.uniform_pair(u0, u1);                            // block 0
  rng.pair(z0, z1);                                    // block 1
  rho[0] = fabs(theta[0] + 0.1 * z0);
  rho[1] = fabs(theta[1] + 0.1 * z1) + u0;
  sabc::emit(rng, 0, theta[0]);
  sabc::emit(rng, 1, p[1]);
  sabc::emit(rng, 2, sabc::data_at(2));
  sabc::emit(rng, 3, u0);
  sabc::emit(rng, 4, u1);
  sabc::emit(rng, 5, z0);
  sabc::emit(rng, -1, 99.0);                           // outside [0, n_outputs): ignored
  sabc::emit(rng, sabc::n_outputs(rng), 99.0);
}
"""
PROBE_PARAMS, PROBE_DATA = [0.25, -7.5, 3.0], [10.0, 11.0, 12.5, 13.0]

WIDE = """
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  double first = 0.0;
  for (int j = 0; j < 48; j += 2) {
    double z0, z1;
    rng.pair(z0, z1);
    rho[j] = fabs(theta[0] + 0.3 * z0);
    rho[j + 1] = fabs(theta[1] + 0.3 * z1);
    if (j == 0) first = z0;
  }
  sabc::emit(rng, 0, theta[1]);
  sabc::emit(rng, 1, first);
  if (sabc::emitting(rng)) sabc::emit(rng, 2, (double)sabc::n_outputs(rng));
}
"""

RAMP = """
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  rho[0] = fabs(theta[0]);
  for (int i = 0; i < 512; ++i) sabc::emit(rng, i, 1000.0 * theta[0] + (double)i);
}
"""


def box(S):
    return S.product_distribution([S.Uniform(*PRIOR[0]), S.Uniform(*PRIOR[1])])


def box_draws(m, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(*PRIOR[0], m), rng.uniform(*PRIOR[1], m)])           # [d][m]


@pytest.fixture(scope="module")
def probe(S, gpu):
    model = S.DeviceSource(PROBE, 2, 2, PROBE_PARAMS, data=PROBE_DATA, n_outputs=6)
    h = S.SabcHandle(n_particles=256, model=model, prior=box(S), seed=SEED)
    yield h
    h.close()


@pytest.fixture(scope="module")
def probe_run(probe):
    """theta, and (rho, out) of the probe at m = 300, pid0 = 31, it = 4 on the update's stream: computed once."""
    theta = box_draws(300, 1)
    return theta, probe.simulate_outputs(theta, 31, 4, stream="update")


@pytest.mark.parametrize("stream,purpose", [("update", 1), ("predict", PURPOSE_PREDICT)])
def test_probe_outputs_are_its_inputs_and_its_draws(S, O, probe, probe_run, stream, purpose):
    m, pid0, it = 300, 31, 4
    theta, (rho_u, out_u) = probe_run
    rho, out = (rho_u, out_u) if stream == "update" else probe.simulate_outputs(theta, pid0, it, stream=stream)
    assert out.shape == (6, m) and rho.shape == (2, m)
    np.testing.assert_array_equal(out[0], theta[0])
    np.testing.assert_array_equal(out[1], np.full(m, PROBE_PARAMS[1]))
    np.testing.assert_array_equal(out[2], np.full(m, PROBE_DATA[2]))
    blocks = [O.stream_block(SEED, pid0 + i, purpose, it, 0) for i in range(m)]
    np.testing.assert_array_equal(out[3], [O.u52(w[0], w[1]) for w in blocks])
    np.testing.assert_array_equal(out[4], [O.u52(w[2], w[3]) for w in blocks])
    z = S.op_normal_pairs(SEED, pid0, m, purpose=purpose, it=it, k=1)[:, 0]
    np.testing.assert_allclose(out[5], z, rtol=1e-13, atol=0)
    if stream == "predict":                            # ... and no draw of the update's stream
        assert not np.any(out[3] == out_u[3]) and not np.any(out[4] == out_u[4]) and not np.any(out[5] == out_u[5])
        assert not np.any(rho == rho_u)


@pytest.mark.parametrize("kind", ["narrow", "wide"])
def test_distances_of_the_call_are_those_of_simulate(S, gpu, probe, kind):
    m, pid0, it = 130, 7, 2
    theta = box_draws(m, 2)
    if kind == "narrow":
        h = probe
    else:
        h = S.SabcHandle(n_particles=256, model=S.DeviceSource(WIDE, 2, 48, n_outputs=3), prior=box(S), seed=SEED)
    try:
        want = h.simulate(theta, pid0, it)
        rho, out = h.simulate_outputs(theta, pid0, it, stream="update")
        rho0, none = h.simulate_outputs(theta, pid0, it, n_out=0, stream="update")     # n_out = 0: sabc_op_simulate
    finally:
        if kind == "wide":
            h.close()
    np.testing.assert_allclose(rho, want, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(rho0, want, rtol=1e-13, atol=1e-15)
    assert none.shape == (0, m) and not np.any(np.isnan(out))
    if kind == "wide":
        np.testing.assert_array_equal(out[0], theta[1])
        np.testing.assert_array_equal(out[2], np.full(m, 3.0))
        z = S.op_normal_pairs(SEED, pid0, m, purpose=1, it=it, k=0)[:, 0]
        np.testing.assert_allclose(out[1], z, rtol=1e-13, atol=0)


def test_never_emitted_is_nan_and_fewer_outputs_are_legal(probe, probe_run):
    theta, (rho6, out6) = probe_run
    rho8, out8 = probe.simulate_outputs(theta, 31, 4, n_out=8, stream="update")
    rho4, out4 = probe.simulate_outputs(theta, 31, 4, n_out=4, stream="update")
    assert out8.shape == (8, 300) and np.all(np.isnan(out8[6:]))
    np.testing.assert_array_equal(out8[:6], out6)
    assert out4.shape == (4, 300) and out4.tobytes() == out6[:4].tobytes()
    assert rho8.tobytes() == rho6.tobytes() and rho4.tobytes() == rho6.tobytes()
    assert not np.any(out6 == 99.0)                    # the two emits outside [0, n_outputs) went nowhere


def test_bad_arguments_are_refused_with_a_reason(S, gpu, probe):
    theta = box_draws(5, 3)
    with pytest.raises(S.SABCError, match="n_out must not be negative") as e:
        probe.simulate_outputs(theta, 0, 0, n_out=-1)
    assert e.value.code == -8
    with pytest.raises(ValueError, match="stream"):
        probe.simulate_outputs(theta, 0, 0, stream="prior")
    rho, out = np.empty((2, 5)), np.empty((6, 5))
    dp = C.POINTER(C.c_double)
    rc = probe._L.sabc_op_simulate_outputs(probe._h, theta.ctypes.data_as(dp), 5, 0, 0, 2, 6, rho.ctypes.data_as(dp), out.ctypes.data_as(dp))
    assert rc == -8 and b"stream" in probe._L.sabc_last_error(probe._h)
    g = S.SabcHandle(n_particles=256, model=S.GaussianIID(n_obs=10), prior=S.Normal(0.0, 1.0), seed=SEED)
    try:
        with pytest.raises(S.SABCError, match="SABC_MODEL_USER"):
            g.simulate_outputs(np.zeros((1, 5)), 0, 0, n_out=2)
        with pytest.raises(TypeError, match="declares none"):
            g.simulate_outputs(np.zeros((1, 5)), 0, 0)
        rho1, _ = g.simulate_outputs(np.zeros((1, 5)), 3, 1, n_out=0)          # a built-in model, no outputs: sabc_op_simulate
        np.testing.assert_array_equal(rho1, g.simulate(np.zeros((1, 5)), 3, 1))
    finally:
        g.close()


# ---- the shipped sources ----
@pytest.fixture(scope="module")
def sir_case(O):
    """m = 200 draws of the documentation's box and the restatement's (total, peak, t_peak) for pid 31.., it = 4: once."""
    m, pid0, it = 200, 31, 4
    theta = box_draws(m, 4)
    want = np.array([sir_statistics(Stream(O, SEED, pid0 + i, it), theta[0, i], theta[1, i], SMALL["S0"], SMALL["I0"], SMALL["R0"],
                                    SMALL["t_max"]) for i in range(m)]).T
    return theta, pid0, it, want


def test_sir_outputs_equal_the_restatement(S, gpu, sir_case):
    theta, pid0, it, want = sir_case
    assert len(np.unique(want[0])) > 20                # epidemics that take off and epidemics that die out
    model = S.StochasticSIR((22.0, 9.0, 12.0), **SMALL)
    h = S.SabcHandle(n_particles=256, model=model, prior=box(S), seed=SEED)
    try:
        rho, out = h.simulate_outputs(theta, pid0, it, stream="update")
        assert h.n_outputs == 3 and model.output_names == ("total_infected", "peak_infected", "t_peak")
    finally:
        h.close()
    np.testing.assert_array_equal(out[:2], want[:2])
    # t_peak: a sum of at most 59 terms e / rate, e within 2 ulp of the restatement's math.log: <= 1e-13, times ten
    np.testing.assert_allclose(out[2], want[2], rtol=1e-12, atol=0)
    np.testing.assert_allclose(rho, (out - np.array([[22.0], [9.0], [12.0]])) ** 2, rtol=1e-13, atol=0)


def sir_series_curve(rng, beta, gamma, S0, I0, R0, t_max, t_obs):
    """device_sources/sir_series.hip's I(t_k) (after examples.sir_series_observation), event j = block j of the stream."""
    N = float(S0 + I0 + R0)
    st = dict(S=S0, I=I0, t=0.0, k=0)
    out = np.full(len(t_obs), np.nan)

    def event(e, u):
        infection_rate = beta * st["S"] * st["I"] / N
        recovery_rate = gamma * st["I"]
        total_rate = infection_rate + recovery_rate
        if not total_rate > 0.0:
            return False
        st["t"] += e / total_rate
        while st["k"] < len(t_obs) and t_obs[st["k"]] < st["t"]:
            out[st["k"]] = st["I"]
            st["k"] += 1
        if u < infection_rate / total_rate:
            st["S"] -= 1
            st["I"] += 1
        else:
            st["I"] -= 1
        return st["t"] < t_max and st["I"] > 0

    if st["t"] < t_max and st["I"] > 0:
        rng.while_events(2 * S0 + I0, event)
    out[st["k"]:] = st["I"]
    return out


def test_sir_series_outputs_equal_the_restatement_and_give_the_distance(S, O, gpu):
    m, pid0, it = 150, 31, 4
    t_obs = np.arange(0.0, 40.0, 5.0)                  # 0, 5, ..., 35
    I_obs = np.array([1.0, 3.0, 6.0, 9.0, 7.0, 4.0, 2.0, 1.0])
    theta = box_draws(m, 5)
    model = S.StochasticSIRSeries(t_obs, I_obs, **SMALL)
    h = S.SabcHandle(n_particles=256, model=model, prior=box(S), seed=SEED)
    try:
        assert h.n_outputs == 8
        rho, out = h.simulate_outputs(theta, pid0, it, stream="update")
    finally:
        h.close()
    want = np.array([sir_series_curve(Stream(O, SEED, pid0 + i, it), theta[0, i], theta[1, i], SMALL["S0"], SMALL["I0"], SMALL["R0"],
                                      SMALL["t_max"], t_obs) for i in range(m)]).T
    assert out.shape == (8, m) and np.array_equal(out, np.round(out))
    np.testing.assert_array_equal(out, want)
    assert len(np.unique(out[-1])) > 3                 # not one curve 150 times
    np.testing.assert_allclose(rho[0], np.mean(np.abs(out - I_obs[:, None]), axis=0), rtol=1e-13, atol=0)


def test_normal_moments_outputs_give_the_distance(S, gpu):
    m, n_obs = 150, 11                                 # odd: the lone last draw is output 10
    y_obs = np.random.default_rng(6).normal(0.0, 1.0, n_obs)
    rng = np.random.default_rng(7)
    theta = np.stack([rng.uniform(2.0, 3.0, m), rng.uniform(0.5, 1.5, m)])
    h = S.SabcHandle(n_particles=256, model=S.NormalMoments(y_obs), prior=box(S), seed=SEED)
    try:
        assert h.n_outputs == n_obs
        rho, y = h.simulate_outputs(theta, 5, 3, stream="update")
        z = np.concatenate([S.op_normal_pairs(SEED, 5, m, purpose=1, it=3, k=b) for b in range(6)], axis=1).T[:n_obs]
    finally:
        h.close()
    assert y.shape == (n_obs, m) and not np.any(np.isnan(y))
    np.testing.assert_allclose(y, theta[0] + theta[1] * z, rtol=1e-12, atol=0)        # the draws, in stream order
    o1 = o2 = 0.0
    for v in y_obs:
        o1, o2 = o1 + v, o2 + v * v
    s1, s2 = np.zeros(m), np.zeros(m)
    for j in range(n_obs):
        s1, s2 = s1 + y[j], s2 + y[j] * y[j]
    np.testing.assert_allclose(rho[0], np.abs(o1 / n_obs - s1 / n_obs), rtol=1e-12, atol=0)
    np.testing.assert_allclose(rho[1], np.abs(o2 - s2), rtol=1e-12, atol=0)


def test_a_large_call_runs_in_chunks(S, gpu):
    m = 40_001                                         # x 512 outputs = 164 MB: two launches of at most 128 MB
    theta = (np.arange(m, dtype=np.float64) % 1000.0).reshape(1, m)
    h = S.SabcHandle(n_particles=256, model=S.DeviceSource(RAMP, 1, 1, n_outputs=512), prior=S.Uniform(0.0, 1000.0), seed=SEED)
    live0, live1 = (C.c_int64 * 2)(), (C.c_int64 * 2)()
    try:
        S.lib().sabc_debug_live_bytes(live0)
        rho, out = h.simulate_outputs(theta, 0, 0, stream="predict")
        S.lib().sabc_debug_live_bytes(live1)
    finally:
        h.close()
    assert list(live0) == list(live1)
    assert out.shape == (512, m)
    np.testing.assert_array_equal(out, 1000.0 * theta + np.arange(512.0)[:, None])
    np.testing.assert_array_equal(rho, theta)


def test_a_forward_run_changes_nothing(S, gpu):
    n = 1001
    model = S.StochasticSIR((77.0, 30.0, 38.0))

    def run(predict):
        res = S.initialization(model, box(S), n_particles=n, n_simulation=n, seed=SEED)
        pp = [S.posterior_predictive(res, n_rep=2)] if predict else []
        S.update_population_(res, model, box(S), n_simulation=3 * n, proposal=S.DifferentialEvolution(n_para=2), resample=n // 2,
                             show_progressbar=False)
        if predict:
            pp.append(S.posterior_predictive(res, n_rep=2, return_distances=True))
        return res, pp

    (a, _), (b, pp) = run(False), run(True)
    try:
        for x, y in ((a.population, b.population), (a.u, b.u), (a.ρ, b.ρ), (a.state.ϵ, b.state.ϵ)):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
        sa, sb = a.state, b.state
        assert (sa.n_simulation, sa.n_accept, sa.n_resampling, sa.n_population_updates) == \
            (sb.n_simulation, sb.n_accept, sb.n_resampling, sb.n_population_updates)
        assert sa.n_population_updates == 3 and sa.n_accept > 0
        for ha, hb in ((sa.ϵ_history, sb.ϵ_history), (sa.u_history, sb.u_history), (sa.ρ_history, sb.ρ_history)):
            assert len(ha) == len(hb) > 0 and all(p.tobytes() == q.tobytes() for p, q in zip(ha, hb))
        before, (after, dist) = pp
        assert before.shape == after.shape == (n, 2, 3) and dist.shape == (n, 2, 3)
        assert not np.any(np.isnan(after))
        for j in range(2):
            rho, out = b._handle.simulate_outputs(b.population.T, 0, j, stream="predict")
            np.testing.assert_array_equal(after[:, j, :], out.T)
            np.testing.assert_array_equal(dist[:, j, :], rho.T)
        assert not np.array_equal(after[:, 0, :], after[:, 1, :])     # two replicates, two streams
    finally:
        a._handle.close()
        b._handle.close()


def test_shipped_models_observe_themselves(S, O, gpu):
    theta = (0.45, 0.12)
    got = S.StochasticSIR.observe(theta, seed=SEED, **SMALL)
    want = sir_statistics(Stream(O, SEED, 0, 0, purpose=PURPOSE_PREDICT), theta[0], theta[1], SMALL["S0"], SMALL["I0"], SMALL["R0"],
                          SMALL["t_max"])
    assert list(got) == ["total_infected", "peak_infected", "t_peak"]
    assert (got["total_infected"], got["peak_infected"]) == want[:2]
    assert math.isclose(got["t_peak"], want[2], rel_tol=1e-12)
    t_obs, I_obs = S.StochasticSIRSeries.observe(theta, np.arange(0.0, 40.0, 5.0), seed=SEED, **SMALL)
    curve = sir_series_curve(Stream(O, SEED, 0, 0, purpose=PURPOSE_PREDICT), theta[0], theta[1], SMALL["S0"], SMALL["I0"],
                             SMALL["R0"], SMALL["t_max"], t_obs)
    np.testing.assert_array_equal(I_obs, curve)
    y = S.NormalMoments.observe((1.5, 0.5), 7, seed=SEED)
    z = np.concatenate([S.op_normal_pairs(SEED, 0, 1, purpose=PURPOSE_PREDICT, it=0, k=b)[0] for b in range(4)])[:7]
    np.testing.assert_allclose(y, 1.5 + 0.5 * z, rtol=1e-12, atol=0)
