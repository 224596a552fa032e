"""sabc::Sample on the device (csrc/team_sample.hpp): a team of lanes draws and sorts one particle's sample.

The forward run with a team per row (k_simulate_batch_team): tests/team_sample/sample_probe.hip emits its sample as drawn and
sorted for 250 rows -- a last wave that is not full, a last team inside it --; the sorted half is np.sort of the drawn half
bit for bit, and the drawn half is bit for bit what team_lanes = 1 emits (the stream order of fill_normals does not depend on
the width).  Sizes: one block per team, non-powers of two on both sides of a power, an odd last draw, a number of blocks that
is no multiple of the width, and the replicated fallback (W = 4, N = 257).  A NaN and duplicates planted through fill(g).
Population runs of GandKQuantiles(team_lanes=) against the oracle driving the Python transcription of
tests/test_sort_source.py over the same Philox blocks: the one-launch form with teams of 1, 4 and 16 lanes, the launch chain
(k_update_team) with 1, 4 and 16 lanes per particle and both proposals, one run at 128 draws; and the posterior predictive.

Probes of one size share a compiled unit (both widths are in every team-aware unit, and the width is no part of its key).

GPU time on an MI355X: 65 s for the 24 GPU tests, most of it the run-time compiler -- 1.6 to 4.5 s per probe source (eleven of
them, fifteen kernels each without the one-launch form), 15 s for the model's unit with its one-launch kernels, 5.7 s and 9.8 s
for its launch-chain units at 45 and 128 draws; the runs and the oracle's transcriptions are 0.5 s or less each."""
import os

import numpy as np
import pytest

from tests.cases import SEED, hip_proposal, oracle_proposal
from tests.test_sort_source import GK_BOX, GK_C, GK_PROBS, GK_UPDATES, assert_matches_the_oracle, gk_q_obs, quantile_type7

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = open(os.path.join(ROOT, "tests", "team_sample", "sample_probe.hip")).read()
ROWS = 250


def probe(S, n, lanes, planted=False, data=None):
    head = f"#define PROBE_N {n}\n" + ("#define PROBE_PLANTED 1\n" if planted else "")
    return S.DeviceSource(head + PROBE_SRC, 1, 2, [0.3], data=data, n_outputs=2 * n, team_lanes=lanes)


def forward(S, n, lanes, **kw):
    out = S.simulate_outputs(probe(S, n, lanes, **kw), np.zeros((ROWS, 1)), seed=SEED)
    assert out.shape == (ROWS, 1, 2 * n)
    return out[:, 0, :n], out[:, 0, n:]


DRAWN_BY_ONE_LANE = {}


def drawn_by_one_lane(S, n):
    if n not in DRAWN_BY_ONE_LANE:
        drawn, ordered = forward(S, n, 1)
        np.testing.assert_array_equal(ordered, np.sort(drawn, axis=1))
        DRAWN_BY_ONE_LANE[n] = drawn
    return DRAWN_BY_ONE_LANE[n]


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,n", [(16, 1), (16, 2), (16, 16), (16, 17), (16, 45), (16, 128), (16, 257),
                                     (4, 3), (4, 5), (4, 33), (4, 100), (4, 128), (4, 257)])
def test_a_team_per_row_draws_the_stream_and_sorts_it(S, gpu, monkeypatch, lanes, n):
    monkeypatch.setenv("SABC_PERSISTENT", "0")      # a forward run never launches the one-launch kernels
    drawn, ordered = forward(S, n, lanes)
    assert np.isfinite(drawn).all() and (n < 2 or (np.diff(drawn, axis=1) < 0).any())      # a sample, not an ascending ramp
    np.testing.assert_array_equal(ordered, np.sort(drawn, axis=1))
    np.testing.assert_array_equal(drawn, drawn_by_one_lane(S, n))
    assert len(np.unique(drawn[:, 0])) == ROWS                                              # every row its own stream


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [4, 16])
def test_a_planted_nan_and_duplicates(S, gpu, monkeypatch, lanes):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    planted = np.array([2.5, np.nan, -1.0, 2.5, 7.0, 2.5, -1.0, 0.0])
    drawn, ordered = forward(S, 8, lanes, planted=True, data=[planted])
    entered = np.where(np.isnan(planted), np.inf, planted)             # the NaN enters as +inf (at fill time) and comes out last
    expect = np.sort(entered)
    np.testing.assert_array_equal(drawn, np.tile(entered, (ROWS, 1)))
    np.testing.assert_array_equal(ordered, np.tile(expect, (ROWS, 1)))
    assert expect[7] == np.inf


# ---- population runs against the oracle ----
DRAWS = 45


def gk_f(O, q_obs, seen, n_draws):
    """device_sources/gk_quantiles.hip over the oracle's Philox blocks: ceil(n_draws / 2) blocks, an odd last draw the first
    normal of the last one"""
    def f(θ, pid, it):
        A, B, g, k = (float(t) for t in θ)
        z = np.array([O.normal_pair(SEED, pid, O.PURPOSE_SIM, it, b) for b in range((n_draws + 1) // 2)]).reshape(-1)[:n_draws]
        x = np.sort(A + B * (1.0 + GK_C * np.tanh(g * z / 2.0)) * np.exp(k * np.log1p(z * z)) * z)
        rho = tuple(abs(quantile_type7(x, p) - q) for p, q in zip(GK_PROBS, q_obs))
        seen.extend(rho)
        return rho
    return f


def oracle_gk_run(O, n, n_draws=DRAWS, prop="rw"):
    seen = []
    cfg = O.make_config(n_particles=n, n_para=4, n_stats=3, model_id=O.MODEL_HOST, model_params=[], seed=SEED,
                        prior=[(O.PRIOR_UNIFORM, lo, hi) for lo, hi in GK_BOX],
                        host_fn=O.host_simulator(gk_f(O, gk_q_obs(), seen, n_draws), 4, 3), algorithm=O.ALG_MULTI_EPS)
    run = O.OracleRun(cfg)
    run.initialize((GK_UPDATES + 1) * n)
    run.update(O.make_update_args(n_simulation=GK_UPDATES * n, proposal=oracle_proposal(O, prop, 4), n_para=4, n_particles=n, resample=n // 2))
    return dict(counters=dict(run.counters), theta=np.array(run.theta), rho=np.array(run.rho), eps=np.array(run.eps), seen=np.array(seen))


@pytest.fixture(scope="module")
def oracle_small(O):
    return oracle_gk_run(O, 1000)


@pytest.fixture(scope="module")
def oracle_chain(O):
    return oracle_gk_run(O, 3000)


def device_gk_run(S, n, team_lanes, n_draws=DRAWS, prop="rw"):
    prior = S.product_distribution([S.Uniform(lo, hi) for lo, hi in GK_BOX])
    model = S.GandKQuantiles(GK_PROBS, gk_q_obs(), n_draws=n_draws, c=GK_C, team_lanes=team_lanes)
    return S.sabc(model, prior, n_particles=n, n_simulation=(GK_UPDATES + 1) * n, proposal=hip_proposal(S, prop, 4), resample=n // 2,
                  algorithm="multi_eps", seed=SEED)


SMALL_ACCEPTS, CHAIN_ACCEPTS = {}, {}


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_a_team_aware_model_in_one_launch_against_the_oracle(S, gpu, monkeypatch, oracle_small, lanes):
    """n = 1000, team_lanes = 16: the one-launch form chooses its own team -- a lane, a quad, a row of 16 lanes per particle --
    and the team-aware source runs cooperatively with it."""
    monkeypatch.setenv("SABC_PERSISTENT", "1")
    monkeypatch.setenv("SABC_PERSISTENT_LANES", str(lanes))
    res = device_gk_run(S, 1000, 16)
    assert res._handle.persistent_lanes == lanes and res._handle.chain_team_lanes == 16
    assert_matches_the_oracle(res, oracle_small)
    SMALL_ACCEPTS[lanes] = res.state.n_accept
    assert len(set(SMALL_ACCEPTS.values())) == 1, SMALL_ACCEPTS


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_a_team_per_particle_on_the_launch_chain_against_the_oracle(S, gpu, monkeypatch, oracle_chain, lanes):
    """n = 3000 is no multiple of the particles a workgroup takes: the last workgroup's trips end inside a trip."""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_gk_run(S, 3000, lanes)
    assert res._handle.persistent_lanes == 0 and res._handle.chain_team_lanes == lanes
    assert_matches_the_oracle(res, oracle_chain)
    CHAIN_ACCEPTS[lanes] = res.state.n_accept
    assert len(set(CHAIN_ACCEPTS.values())) == 1, CHAIN_ACCEPTS


@pytest.mark.gpu
def test_differential_evolution_with_a_row_per_particle_against_the_oracle(S, gpu, monkeypatch, O):
    """partners and half batches through PartnerView in k_update_team"""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_gk_run(S, 3000, 16, prop="de")
    assert res._handle.chain_team_lanes == 16
    assert_matches_the_oracle(res, oracle_gk_run(O, 3000, prop="de"))


@pytest.mark.gpu
def test_128_draws_with_a_row_per_particle_against_the_oracle(S, gpu, monkeypatch, O):
    """the headline shape: eight slots per lane, the layout of the built-in g-and-k kernel"""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_gk_run(S, 512, 16, n_draws=128)
    assert res._handle.chain_team_lanes == 16
    assert_matches_the_oracle(res, oracle_gk_run(O, 512, n_draws=128))


@pytest.mark.gpu
def test_posterior_predictive_of_a_team_aware_model(S, gpu, monkeypatch):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    n = 500
    res = device_gk_run(S, n, 16)
    pp = S.posterior_predictive(res, n_rep=2)
    assert pp.shape == (n, 2, DRAWS)
    assert np.isfinite(pp).all() and (np.diff(pp, axis=2) >= 0).all()
    assert len(np.unique(pp[:, 0, :])) > n                                   # samples, not one constant
