"""The reductions and two-sample distances of sabc::Sample on the device (csrc/sample_reduce.hpp, csrc/team_sample.hpp).

The forward run with a team per row: tests/sample_reduce/reduce_probe.hip emits its sample as sorted and as drawn and every
reduction, for 250 rows -- a last wave that is not full, a last team inside it.  After the sort, sum and wasserstein1 are the
NumPy tree of the emitted sample bit for bit (tests/sample_reduce_ref.py), and the same bits for teams of 1, 4 and 16 lanes at
N = 45; before it, sum is within N 2^-53 sum |x| of math.fsum; max and min are exact; the two-pass variance is within
4 (N + 3) 2^-53 of an extended-precision one; ks is the restatement's bits against an observed sample of N and of 7 values.
Sizes: one value, one block more than a row of lanes, non-powers of two, a full 8 and 32 slots per lane, the replicated
fallback (W = 4, N = 257) and a lane per row.  Planted data through fill(g): duplicates, ties with the observed sample and a
NaN that enters as +inf.
Population runs of GandKSample(distance=("wasserstein", "ks")) at 45 draws against the oracle driving a Python transcription
over the same Philox blocks: the one-launch form with teams of 1, 4 and 16 lanes, the launch chain with plain arrays and with
1, 4 and 16 lanes per particle -- equal accept counts across all of them --, one DifferentialEvolution run; the four forms on
the same thetas and streams, bit for bit; and the posterior predictive.

Probes of one size share a compiled unit (both widths are in every team-aware unit, and the width is no part of its key).

GPU time on an MI355X: 58 s for the 23 GPU tests, most of it the run-time compiler -- 1.7 to 6.2 s per probe source (nine of
them), 15 s for the model's unit with its one-launch kernels, 8 s for the four forward units of the model and 6 s for its
launch-chain units; the runs and the oracle's transcriptions are well under a second each."""
import math
import os

import numpy as np
import pytest

from tests import sample_reduce_ref as R
from tests.cases import SEED, hip_proposal, oracle_proposal
from tests.test_sort_source import GK_BOX, GK_C, GK_UPDATES, assert_matches_the_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = open(os.path.join(ROOT, "tests", "sample_reduce", "reduce_probe.hip")).read()
ROWS = 250
U = 2.0 ** -53
SHORT = np.sort(np.random.default_rng(SEED + 1).normal(size=7))


def observed(n):
    return np.sort(np.random.default_rng(SEED + n).normal(size=n))


def forward(S, n, lanes):
    model = S.DeviceSource(f"#define PROBE_N {n}\n" + PROBE_SRC, 1, 1, [0.0], data=[observed(n), SHORT], n_outputs=2 * n + 16, team_lanes=lanes)
    out = S.simulate_outputs(model, np.zeros((ROWS, 1)), seed=SEED)
    assert out.shape == (ROWS, 1, 2 * n + 16)
    return out[:, 0, :n], out[:, 0, n:n + 16], out[:, 0, n + 16:]


BITS_AT_45 = {}


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,n", [(16, 1), (16, 17), (16, 45), (16, 128), (16, 257), (4, 5), (4, 33), (4, 45), (4, 100), (4, 257), (1, 45)])
def test_the_reductions_of_a_team_per_row(S, gpu, monkeypatch, lanes, n):
    monkeypatch.setenv("SABC_PERSISTENT", "0")      # a forward run never launches the one-launch kernels
    x, r, drawn = forward(S, n, lanes)
    y = observed(n)
    assert np.isfinite(x).all() and np.isfinite(r[:, :14]).all() and len(np.unique(x[:, 0])) == ROWS
    np.testing.assert_array_equal(x, np.sort(drawn, axis=1))
    index = np.arange(n, dtype=np.float64)
    # after the sort: the canonical tree over the rank, bit for bit
    np.testing.assert_array_equal(r[:, 1], R.tree_sum(x))
    np.testing.assert_array_equal(r[:, 2], R.wasserstein1(x, y))
    np.testing.assert_array_equal(r[:, 10], R.tree_sum(np.abs(x) + index))
    np.testing.assert_array_equal(r[:, 11], R.tree_sum(x) / float(n))
    np.testing.assert_array_equal(r[:, 5], r[:, 11])
    # before it: the draw layout, any order of summation
    for row in range(ROWS):
        exact, bound = math.fsum(drawn[row]), n * U * math.fsum(np.abs(drawn[row]))
        if row == 0:
            print(f"W={lanes} N={n}: |sum before the sort - fsum| = {abs(r[row, 0] - exact):.3e} in row 0, bound {bound:.3e}")
        assert abs(r[row, 0] - exact) <= bound
    # max and min are order-free
    np.testing.assert_array_equal(r[:, 3], drawn.max(axis=1))
    np.testing.assert_array_equal(r[:, 4], x.min(axis=1))
    np.testing.assert_array_equal(r[:, 12], (np.abs(x) + index).max(axis=1))
    np.testing.assert_array_equal(r[:, 13], (drawn - index).min(axis=1))
    # moments: two passes, against extended precision
    wide = x.astype(np.longdouble)
    mean = wide.sum(axis=1) / n
    if n > 1:
        var = ((wide - mean[:, None]) ** 2).sum(axis=1) / (n - 1)
        err = np.abs((r[:, 6].astype(np.longdouble) - var) / var).max()
        print(f"W={lanes} N={n}: relative error of the variance {float(err):.3e}, bound {4 * (n + 3) * U:.3e}")
        assert err <= 4 * (n + 3) * U
    else:
        assert (r[:, 6] == 0.0).all()
    w2 = ((wide - y.astype(np.longdouble)) ** 2).sum(axis=1) / n
    assert np.abs((r[:, 9].astype(np.longdouble) - w2) / w2).max() <= 4 * (n + 3) * U       # (products may fuse into the adds)
    # Kolmogorov-Smirnov: integers, bit for bit; an observed sample of the same and of another length
    np.testing.assert_array_equal(r[:, 7], R.ks(x, y))
    np.testing.assert_array_equal(r[:, 8], R.ks(x, SHORT))
    if n == 45:
        BITS_AT_45[lanes] = (x, r[:, [1, 2, 5, 7, 8, 10, 11]])
        first = next(iter(BITS_AT_45.values()))
        for other in BITS_AT_45.values():
            np.testing.assert_array_equal(other[0], first[0])
            np.testing.assert_array_equal(other[1], first[1])


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [4, 16])
def test_planted_duplicates_ties_and_a_nan(S, gpu, monkeypatch, lanes):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    n = 8
    planted = np.array([2.5, np.nan, -1.0, 2.5, 7.0, 2.5, -1.0, 0.0])
    obs = np.array([-1.0, -1.0, 0.0, 1.0, 2.5, 2.5, 3.0, 7.0])          # ties with the planted values
    short = np.array([-1.0, 0.0, 0.0, 2.5, 2.5, 6.0, 7.0])
    model = S.DeviceSource(f"#define PROBE_N {n}\n#define PROBE_PLANTED 1\n" + PROBE_SRC, 1, 1, [0.0], data=[planted, obs, short],
                           n_outputs=3 * n + 16, team_lanes=lanes)
    out = S.simulate_outputs(model, np.zeros((ROWS, 1)), seed=SEED)[:, 0, :]
    expect = np.sort(np.where(np.isnan(planted), np.inf, planted))       # the NaN enters as +inf and comes out last
    assert expect[7] == np.inf
    np.testing.assert_array_equal(out[:, :n], np.tile(expect, (ROWS, 1)))
    r = out[:, n:n + 16]
    assert (r[:, 7] == R.ks(expect, obs)).all() and (r[:, 8] == R.ks(expect, short)).all()
    assert (r[:, 1] == np.inf).all() and (r[:, 2] == np.inf).all() and (r[:, 3] == np.inf).all() and (r[:, 4] == -1.0).all()
    np.testing.assert_array_equal(out[:, n + 16:2 * n + 16], np.tile(R.count_less(expect, short), (ROWS, 1)))
    np.testing.assert_array_equal(out[:, 2 * n + 16:], np.tile(R.count_less_equal(expect, short), (ROWS, 1)))
    assert R.count_less(expect, short).tolist() == [0, 0, 1, 3, 3, 3, 6, 7] and R.count_less_equal(expect, short).tolist() == [1, 1, 3, 5, 5, 5, 7, 7]


# ---- population runs against the oracle ----
DRAWS = 45


def gk_y_obs():
    z = np.random.default_rng(SEED).normal(size=DRAWS)
    return np.sort(3.0 + 1.0 * (1.0 + GK_C * np.tanh(2.0 * z / 2.0)) * (1.0 + z * z) ** 0.5 * z)


def gk_f(O, y, seen):
    """device_sources/gk_sample.hip over the oracle's Philox blocks: ceil(DRAWS / 2) blocks, an odd last draw the first normal
    of the last one"""
    def f(θ, pid, it):
        A, B, g, k = (float(t) for t in θ)
        z = np.array([O.normal_pair(SEED, pid, O.PURPOSE_SIM, it, b) for b in range((DRAWS + 1) // 2)]).reshape(-1)[:DRAWS]
        x = np.sort(A + B * (1.0 + GK_C * np.tanh(g * z / 2.0)) * np.exp(k * np.log1p(z * z)) * z)
        rho = (float(R.wasserstein1(x, y)), float(R.ks(x, y)))
        seen.extend(rho)
        return rho
    return f


def oracle_gk_run(O, n, prop="rw"):
    seen = []
    cfg = O.make_config(n_particles=n, n_para=4, n_stats=2, model_id=O.MODEL_HOST, model_params=[], seed=SEED,
                        prior=[(O.PRIOR_UNIFORM, lo, hi) for lo, hi in GK_BOX],
                        host_fn=O.host_simulator(gk_f(O, gk_y_obs(), seen), 4, 2), algorithm=O.ALG_MULTI_EPS)
    run = O.OracleRun(cfg)
    run.initialize((GK_UPDATES + 1) * n)
    run.update(O.make_update_args(n_simulation=GK_UPDATES * n, proposal=oracle_proposal(O, prop, 4), n_para=4, n_particles=n, resample=n // 2))
    # copies: the arrays are read once and shared by the tests below, which leave them unchanged
    return dict(counters=dict(run.counters), theta=np.array(run.theta), rho=np.array(run.rho), eps=np.array(run.eps), seen=np.array(seen))


@pytest.fixture(scope="module")
def oracle_small(O):
    return oracle_gk_run(O, 1000)


@pytest.fixture(scope="module")
def oracle_chain(O):
    return oracle_gk_run(O, 3000)


def device_gk_run(S, n, team_lanes, prop="rw"):
    prior = S.product_distribution([S.Uniform(lo, hi) for lo, hi in GK_BOX])
    model = S.GandKSample(gk_y_obs(), distance=("wasserstein", "ks"), c=GK_C, team_lanes=team_lanes)
    return S.sabc(model, prior, n_particles=n, n_simulation=(GK_UPDATES + 1) * n, proposal=hip_proposal(S, prop, 4), resample=n // 2,
                  algorithm="multi_eps", seed=SEED)


SMALL_ACCEPTS, CHAIN_ACCEPTS = {}, {}


@pytest.mark.gpu
def test_the_four_forms_of_gk_sample_give_the_same_bits(S, gpu, monkeypatch):
    """The same thetas on the same streams through plain arrays and through teams of 1, 4 and 16 lanes: the sorted samples are
    the same bits, and so are both distances -- which are the restatement's of the emitted sample."""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    y = gk_y_obs()
    rng = np.random.default_rng(SEED)
    theta = np.stack([rng.uniform(lo, hi, ROWS) for lo, hi in GK_BOX])              # [d][m]
    prior = S.product_distribution([S.Uniform(lo, hi) for lo, hi in GK_BOX])
    seen = {}
    for lanes in (None, 1, 4, 16):
        model = S.GandKSample(y, distance=("wasserstein", "ks"), c=GK_C, team_lanes=lanes)
        h = S.SabcHandle(n_particles=ROWS, model=model, prior=prior, seed=SEED, algorithm=S._lib.ALG_MULTI_EPS)
        try:
            rho, out = h.simulate_outputs(theta, 0, 3)
            rho_again = h.simulate(theta, 0, 3)
        finally:
            h.close()
        x = out.T
        assert np.isfinite(x).all() and (np.diff(x, axis=1) >= 0).all()
        np.testing.assert_array_equal(rho[0], R.wasserstein1(x, y))
        np.testing.assert_array_equal(rho[1], R.ks(x, y))
        np.testing.assert_array_equal(rho_again, rho)
        seen[lanes] = (x, rho)
    for lanes in (1, 4, 16):
        np.testing.assert_array_equal(seen[lanes][0], seen[None][0])
        np.testing.assert_array_equal(seen[lanes][1], seen[None][1])


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_gk_sample_in_one_launch_against_the_oracle(S, gpu, monkeypatch, oracle_small, lanes):
    """n = 1000: the one-launch form chooses its own team -- a lane, a quad, a row of 16 lanes per particle -- and the
    team-aware source runs cooperatively with it."""
    monkeypatch.setenv("SABC_PERSISTENT", "1")
    monkeypatch.setenv("SABC_PERSISTENT_LANES", str(lanes))
    res = device_gk_run(S, 1000, 16)
    assert res._handle.persistent_lanes == lanes and res._handle.chain_team_lanes == 16
    assert_matches_the_oracle(res, oracle_small)
    SMALL_ACCEPTS[lanes] = res.state.n_accept
    assert len(set(SMALL_ACCEPTS.values())) == 1, SMALL_ACCEPTS


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [None, 1, 4, 16])
def test_gk_sample_on_the_launch_chain_against_the_oracle(S, gpu, monkeypatch, oracle_chain, lanes):
    """n = 3000 is no multiple of the particles a workgroup takes.  None: plain arrays, sabc::tree_sum and the count functions.
    Every form accepts the same number of particles.  (The populations are not compared bit for bit: a team also draws the
    proposal together, and k_update_team's proposal arithmetic differs from k_update's in the last bit of some thetas.)"""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_gk_run(S, 3000, lanes)
    assert res._handle.persistent_lanes == 0 and res._handle.chain_team_lanes == (lanes or 0)
    assert_matches_the_oracle(res, oracle_chain)
    CHAIN_ACCEPTS[lanes] = res.state.n_accept
    assert len(set(CHAIN_ACCEPTS.values())) == 1, CHAIN_ACCEPTS


@pytest.mark.gpu
def test_differential_evolution_against_the_oracle(S, gpu, monkeypatch, O):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_gk_run(S, 3000, 16, prop="de")
    assert res._handle.chain_team_lanes == 16
    assert_matches_the_oracle(res, oracle_gk_run(O, 3000, prop="de"))


@pytest.mark.gpu
def test_posterior_predictive_of_gk_sample(S, gpu, monkeypatch):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    n = 500
    res = device_gk_run(S, n, 4)
    pp = S.posterior_predictive(res, n_rep=2)
    assert pp.shape == (n, 2, DRAWS)
    assert np.isfinite(pp).all() and (np.diff(pp, axis=2) >= 0).all()
    assert len(np.unique(pp[:, 0, :])) > n                                   # samples, not one constant
