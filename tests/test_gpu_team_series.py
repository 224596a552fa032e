"""sabc::Series on the device (csrc/team_series.hpp) and the model shipped on it, MA2 (device_sources/ma2.hip).

The forward run with a team per row: tests/team_series/series_probe.hip emits its series, every reduction and, for each lag
compiled into it, lag<L>(-7.0) whole, two lagged sums of |a - b| and two autocovariances, for 250 rows -- a last wave that is
not full, a last team inside it.  The series is the Python transcription of the stream's normals bit for bit
(tests/elementary_ref.py over the oracle's Philox blocks); lag, sum, lagged_sum and autocovariance are the NumPy restatement's
bits (tests/team_series_ref.py); max and min are exact; the two-pass variance is within 4 (N + 3) 2^-53 of an extended-precision
one.  Sizes: one value, three (lag 2 = N - 1), one block more than a row of lanes, non-powers of two, a full 8 and 32 slots per
lane, the replicated fallback (W = 4, N = 257) and a lane per row; at N = 45 the same bits for 1, 4 and 16 lanes, and with 16
lanes (4 slots per lane) the lags 1, 3, 4, 5, 9, 44 move inside a lane, across exactly one lane, one lane plus a slot, two lanes
plus a slot, and N - 1.  Planted data through fill(g): a NaN and an infinity pass through unchanged into at and lag.
Population runs of MA2 at n_obs = 43 (45 innovations), n_lags = 2 against the oracle driving the Python transcription over the
same Philox blocks: the one-launch form with teams of 1, 4 and 16 lanes, the launch chain with the plain form and with 1, 4 and
16 lanes per particle -- equal accept counts across all of them --, one DifferentialEvolution run; the four forms on the same
thetas and streams, bit for bit; the posterior predictive; and MA2.observe followed by from_observations.

Probes of one size share a compiled unit (both widths are in every team-aware unit, and the width is no part of its key).

GPU time on an MI355X: 53 s for the 27 GPU tests, most of it the run-time compiler -- 1.4 to 7.9 s per probe source (nine of them;
the longest N = 257 on a row of 16, 32 slots per lane and six lags), 9 s for the model's unit with its one-launch kernels and 5 s for
its four forward units; the runs, the transcription of the normals (once per stream, shared) and the oracle's transcriptions are
around a second each."""
import os

import numpy as np
import pytest

from tests import team_series_ref as T
from tests.cases import SEED, hip_proposal, oracle_proposal
from tests.sample_reduce_ref import tree_sum
from tests.test_f32_draws import f64_pair
from tests.test_sort_source import GK_UPDATES, assert_matches_the_oracle
from tests.test_team_series_compile import probe_lags, probe_outputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = open(os.path.join(ROOT, "tests", "team_series", "series_probe.hip")).read()
ROWS = 250
U = 2.0 ** -53
PURPOSE_SIM, PURPOSE_PREDICT = 1, 6                     # csrc/device_rng.hpp

_NORMALS = {}


def stream_normals(O, purpose, it, rows, n):
    """Normals 0 .. n-1 of the streams (SEED, pid = row, purpose, it), transcribed: [rows, n].  Computed once per stream for the
    longest series asked for so far and shared; the callers leave it unchanged."""
    key = (purpose, it, rows)
    blocks = (n + 1) // 2
    if key not in _NORMALS or _NORMALS[key].shape[1] < 2 * blocks:
        _NORMALS[key] = np.array([[z for b in range(blocks) for z in f64_pair(O.stream_block(SEED, pid, purpose, it, b))] for pid in range(rows)])
    return _NORMALS[key][:, :n]


def forward(S, n, lanes, when):
    model = S.DeviceSource(f"#define PROBE_N {n}\n" + PROBE_SRC, 1, 1, [when], n_outputs=probe_outputs(n), team_lanes=lanes)
    out = S.simulate_outputs(model, np.zeros((ROWS, 1)), seed=SEED)
    assert out.shape == (ROWS, 1, probe_outputs(n))
    return out[:, 0, :]


def assert_same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(np.broadcast_to(want, np.shape(got)), dtype=np.float64)
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


def check_probe_outputs(out, x, n, when, finite=True):
    """Everything series_probe.hip emits against the restatement applied to the series x [rows, n]."""
    first = 2 if n > 2 else 0
    index = np.arange(n, dtype=np.float64)
    assert_same_bits(out[:, :n], x)
    r = out[:, n:n + 16]
    assert_same_bits(r[:, 9], x[:, when])
    # map, then zip (where the planted form computes a NaN, inf - inf, its sign and payload are the hardware's: a NaN is a NaN)
    with np.errstate(invalid="ignore"):
        zipped = (x + index) - 2.0 * x
    np.testing.assert_array_equal(out[:, n + 16:2 * n + 16], zipped)
    if finite:
        assert_same_bits(out[:, n + 16:2 * n + 16], zipped)
        assert_same_bits(r[:, 0], tree_sum(x))
        assert_same_bits(r[:, 1], tree_sum(x) / float(n))
        assert_same_bits(r[:, 2], r[:, 1])
        assert_same_bits(r[:, 4], (np.abs(x) + index).max(axis=1))
        assert_same_bits(r[:, 5], (x - index).min(axis=1))
        assert_same_bits(r[:, 6], tree_sum(np.abs(x) + index))
        assert_same_bits(r[:, 7], T.autocovariance(x, 0))
        assert_same_bits(r[:, 8], T.autocovariance(x, 0, 0.25, first))
        if n > 1:
            wide = x.astype(np.longdouble)
            var = ((wide - (wide.sum(axis=1) / n)[:, None]) ** 2).sum(axis=1) / (n - 1)
            err = float(np.abs((r[:, 3].astype(np.longdouble) - var) / var).max())
            print(f"N={n}: relative error of the variance {err:.3e}, bound {4 * (n + 3) * U:.3e}")
            assert err <= 4 * (n + 3) * U
        else:
            assert (r[:, 3] == 0.0).all()
    o = 2 * n + 16
    distance = lambda t, a, b: np.abs(a - b)  # noqa: E731
    for L in probe_lags(n):
        assert_same_bits(out[:, o:o + n], T.lag(x, L, -7.0))
        if finite:
            assert_same_bits(out[:, o + n], T.lagged_sum(x, L, distance))
            assert_same_bits(out[:, o + n + 1], T.lagged_sum(x, L, distance, first))
            assert_same_bits(out[:, o + n + 2], T.autocovariance(x, L))
            assert_same_bits(out[:, o + n + 3], T.autocovariance(x, L, 0.25, first))
        o += n + 4
    assert_same_bits(out[:, o:o + n - first], x[:, first:])
    o += n - first
    assert_same_bits(out[:, o:o + n], x)
    assert o + n == out.shape[1]


BITS_AT_45 = {}


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,n", [(16, 1), (16, 3), (16, 33), (16, 45), (16, 128), (16, 257), (4, 5), (4, 33), (4, 45), (4, 100), (4, 128),
                                     (4, 257), (1, 45)])
def test_the_series_of_a_team_per_row(S, O, gpu, monkeypatch, lanes, n):
    monkeypatch.setenv("SABC_PERSISTENT", "0")      # a forward run never launches the one-launch kernels
    when = (2 * n) // 3
    out = forward(S, n, lanes, when)
    # every output was emitted, and nothing else: what is never emitted reads as NaN (the six spare slots of the block at N)
    assert np.isfinite(np.delete(out, np.s_[n + 10:n + 16], axis=1)).all() and np.isnan(out[:, n + 10:n + 16]).all()
    x = stream_normals(O, PURPOSE_PREDICT, 0, ROWS, n)
    assert len(np.unique(x[:, 0])) == ROWS
    if n == 45:
        assert probe_lags(n) == [1, 3, 4, 5, 9, 44]
    if n == 3:
        assert probe_lags(n) == [1, 2]
    check_probe_outputs(out, x, n, when)
    if n == 45:
        BITS_AT_45[lanes] = np.delete(out, n + 3, axis=1)      # (all but the variance, a sum of products that may fuse)
        first = next(iter(BITS_AT_45.values()))
        for other in BITS_AT_45.values():
            assert_same_bits(other, first)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_a_planted_nan_and_an_infinity_pass_through(S, gpu, monkeypatch, lanes):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    n, when = 12, 5
    planted = np.array([2.5, -1.0, 0.0, -0.0, 7.0, np.nan, 1e300, -1e-300, 3.0, 4.0, np.inf, -np.inf])
    model = S.DeviceSource(f"#define PROBE_N {n}\n#define PROBE_PLANTED 1\n" + PROBE_SRC, 1, 1, [when], data=[planted], n_outputs=probe_outputs(n),
                           team_lanes=lanes)
    out = S.simulate_outputs(model, np.zeros((ROWS, 1)), seed=SEED)[:, 0, :]
    assert probe_lags(n) == [1, 3, 4, 5, 9]
    x = np.tile(planted, (ROWS, 1))
    check_probe_outputs(out, x, n, when, finite=False)          # the series, at(t) for every t and a run-time t, and every lag: bits
    assert np.isnan(out[:, n + 9]).all()                        # at(5) is the NaN
    assert np.isnan(out[:, n]).all()                            # ... and a sum over it is one


# ---- MA2: population runs against the oracle ----
N_OBS, N_LAGS = 43, 2
MA2_BOX = [(-2.0, 2.0), (-1.0, 1.0)]


def ma2_acov_obs():
    e = np.random.default_rng(SEED).normal(size=N_OBS + 2)
    return T.ma2_summaries(T.ma2_series((0.6, 0.2), e), N_LAGS)


def ma2_f(O, acov, seen):
    """device_sources/ma2.hip over the oracle's Philox blocks: ceil(45 / 2) blocks, the odd last innovation the first normal of
    the last one"""
    def f(θ, pid, it):
        e = np.array([O.normal_pair(SEED, pid, O.PURPOSE_SIM, it, b) for b in range((N_OBS + 3) // 2)]).reshape(-1)[:N_OBS + 2]
        rho = tuple(float(v) for v in np.abs(T.ma2_summaries(T.ma2_series(θ, e), N_LAGS) - acov))
        seen.extend(rho)
        return rho
    return f


def oracle_ma2_run(O, n, prop="rw"):
    seen = []
    cfg = O.make_config(n_particles=n, n_para=2, n_stats=N_LAGS + 1, model_id=O.MODEL_HOST, model_params=[], seed=SEED,
                        prior=[(O.PRIOR_UNIFORM, lo, hi) for lo, hi in MA2_BOX],
                        host_fn=O.host_simulator(ma2_f(O, ma2_acov_obs(), seen), 2, N_LAGS + 1), algorithm=O.ALG_MULTI_EPS)
    run = O.OracleRun(cfg)
    run.initialize((GK_UPDATES + 1) * n)
    run.update(O.make_update_args(n_simulation=GK_UPDATES * n, proposal=oracle_proposal(O, prop, 2), n_para=2, n_particles=n, resample=n // 2))
    # copies: the arrays are read once and shared by the tests below, which leave them unchanged
    return dict(counters=dict(run.counters), theta=np.array(run.theta), rho=np.array(run.rho), eps=np.array(run.eps), seen=np.array(seen))


@pytest.fixture(scope="module")
def oracle_small(O):
    return oracle_ma2_run(O, 1000)


@pytest.fixture(scope="module")
def oracle_chain(O):
    return oracle_ma2_run(O, 3000)


def ma2_prior(S):
    return S.product_distribution([S.Uniform(lo, hi) for lo, hi in MA2_BOX])


def device_ma2_run(S, n, team_lanes, prop="rw"):
    model = S.MA2(ma2_acov_obs(), n_obs=N_OBS, n_lags=N_LAGS, team_lanes=team_lanes)
    return S.sabc(model, ma2_prior(S), n_particles=n, n_simulation=(GK_UPDATES + 1) * n, proposal=hip_proposal(S, prop, 2), resample=n // 2,
                  algorithm="multi_eps", seed=SEED)


SMALL_ACCEPTS, CHAIN_ACCEPTS = {}, {}


@pytest.mark.gpu
def test_the_four_forms_of_ma2_give_the_same_bits(S, O, gpu, monkeypatch):
    """The same thetas on the same streams through the plain form and through teams of 1, 4 and 16 lanes: the series are the
    transcription's bits -- the fmas over the transcribed normals --, and the distances the restatement's of the emitted series."""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    acov = ma2_acov_obs()
    rng = np.random.default_rng(SEED)
    theta = np.stack([rng.uniform(lo, hi, ROWS) for lo, hi in MA2_BOX])              # [d][m]
    e = stream_normals(O, PURPOSE_SIM, 3, ROWS, N_OBS + 2)
    want = np.array([T.ma2_series(theta[:, row], e[row]) for row in range(ROWS)])
    seen = {}
    for lanes in (None, 1, 4, 16):
        model = S.MA2(acov, n_obs=N_OBS, n_lags=N_LAGS, team_lanes=lanes)
        h = S.SabcHandle(n_particles=ROWS, model=model, prior=ma2_prior(S), seed=SEED, algorithm=S._lib.ALG_MULTI_EPS)
        try:
            rho, out = h.simulate_outputs(theta, 0, 3)
            rho_again = h.simulate(theta, 0, 3)
        finally:
            h.close()
        y = out.T
        assert_same_bits(y, want)
        assert_same_bits(rho.T, np.abs(T.ma2_summaries(y, N_LAGS) - acov))
        assert_same_bits(rho_again, rho)
        seen[lanes] = (y, rho)
    for lanes in (1, 4, 16):
        assert_same_bits(seen[lanes][0], seen[None][0])
        assert_same_bits(seen[lanes][1], seen[None][1])


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_ma2_in_one_launch_against_the_oracle(S, gpu, monkeypatch, oracle_small, lanes):
    """n = 1000: the one-launch form chooses its own team -- a lane, a quad, a row of 16 lanes per particle -- and the
    team-aware source runs cooperatively with it."""
    monkeypatch.setenv("SABC_PERSISTENT", "1")
    monkeypatch.setenv("SABC_PERSISTENT_LANES", str(lanes))
    res = device_ma2_run(S, 1000, 16)
    assert res._handle.persistent_lanes == lanes and res._handle.chain_team_lanes == 16
    assert_matches_the_oracle(res, oracle_small)
    SMALL_ACCEPTS[lanes] = res.state.n_accept
    assert len(set(SMALL_ACCEPTS.values())) == 1, SMALL_ACCEPTS


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [None, 1, 4, 16])
def test_ma2_on_the_launch_chain_against_the_oracle(S, gpu, monkeypatch, oracle_chain, lanes):
    """n = 3000 is no multiple of the particles a workgroup takes.  None: the plain form, Series<45, 1> in sabc_user_simulate.
    Every form accepts the same number of particles."""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_ma2_run(S, 3000, lanes)
    assert res._handle.persistent_lanes == 0 and res._handle.chain_team_lanes == (lanes or 0)
    assert_matches_the_oracle(res, oracle_chain)
    CHAIN_ACCEPTS[lanes] = res.state.n_accept
    assert len(set(CHAIN_ACCEPTS.values())) == 1, CHAIN_ACCEPTS


@pytest.mark.gpu
def test_differential_evolution_against_the_oracle(S, gpu, monkeypatch, O):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_ma2_run(S, 3000, 16, prop="de")
    assert res._handle.chain_team_lanes == 16
    assert_matches_the_oracle(res, oracle_ma2_run(O, 3000, prop="de"))


@pytest.mark.gpu
def test_posterior_predictive_of_ma2(S, gpu, monkeypatch):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    n = 500
    res = device_ma2_run(S, n, 4)
    pp, dist = S.posterior_predictive(res, n_rep=2, return_distances=True)
    assert pp.shape == (n, 2, N_OBS) and dist.shape == (n, 2, N_LAGS + 1)
    assert np.isfinite(pp).all() and len(np.unique(pp[:, 0, :])) > n         # series, not one constant
    assert_same_bits(dist, np.abs(T.ma2_summaries(pp, N_LAGS) - ma2_acov_obs()))


@pytest.mark.gpu
def test_observe_then_from_observations_round_trips(S, O, gpu, monkeypatch):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    theta = (0.6, 0.2)
    y = S.MA2.observe(theta, n_obs=N_OBS, seed=SEED)
    assert y.shape == (N_OBS,)
    assert_same_bits(y, T.ma2_series(theta, stream_normals(O, PURPOSE_PREDICT, 0, 1, N_OBS + 2)[0]))
    model = S.MA2.from_observations(y, team_lanes=4)
    assert_same_bits(model.data[0], T.ma2_summaries(y, N_LAGS))
    # the model that observed this series finds it again: the same theta on the same stream is at distance +0.0
    h = S.SabcHandle(n_particles=16, model=model, prior=ma2_prior(S), seed=SEED, algorithm=S._lib.ALG_MULTI_EPS)
    try:
        rho, out = h.simulate_outputs(np.array(theta).reshape(2, 1), 0, 0, stream="predict")
    finally:
        h.close()
    assert_same_bits(out[:, 0], y)
    assert_same_bits(rho[:, 0], np.zeros(N_LAGS + 1))
