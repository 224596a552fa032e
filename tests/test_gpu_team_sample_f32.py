"""sabc::SampleF32 on the device (csrc/team_sample_f32.hpp) and the model shipped on it, GandKSampleF32.

The forward run with a team per row: tests/team_sample_f32/sample_probe_f32.hip emits its sample as drawn and as sorted, and every
read-out and reduction, for 250 rows -- a last wave that is not full, a last team inside it.  The sorted half is np.sort of the
drawn half bit for bit; every emitted value is a binary32 value; the drawn half is what team_lanes = 1 emits, and what a source
registered the plain way emits that fills float x[N] by hand with rng.for_quads_f32 (tests/team_sample_f32/quads_by_hand_probe.hip:
the stream definition tests/test_gpu_f32_draws.py ties to NumPy).  Sizes: one draw, one block, one draw more than a block, a number
of blocks that is no multiple of the width, a full row of blocks and one draw more, 8 and 32 slots per lane, and the replicated
fallback on both widths (N = 32 W + 1).  A NaN, duplicates and ties planted through fill(g).
Reductions at N = 45 and 128 for teams of 1, 4 and 16 lanes: sum, max, min, wasserstein1, ks and quantile are the NumPy
restatement (tests/sample_reduce_ref.py) of the emitted sorted sample bit for bit, and the same bits for the three widths;
moments and wasserstein2_squared, whose products may contract into the additions, are held to the bounds of
tests/test_gpu_sample_reduce.py.  (The quantile is read at p = 1/2: its interpolation weight is 0 or 1/2, so a + g d is the same
bits whether or not the compiler fuses it.)
Population runs of GandKSampleF32 at 45 draws against the oracle driving a Python transcription -- the binary32 normals of
tests/elementary_f32_ref.py over the oracle's Philox blocks, the f64 transform, x rounded to np.float32 --: one launch with teams
of 1, 4 and 16 lanes, the launch chain with 1, 4 and 16 lanes per particle, equal accept counts across them, one
DifferentialEvolution run, one run at 128 draws, and the posterior predictive.

Probes of one size share a compiled unit across the widths.  GPU time on an MI355X: 87 s for the 31 GPU tests, nearly all of it
the run-time compiler -- 2.4 to 6.8 s per probe source (fourteen of them), 15 s once for the model's unit with its one-launch
kernels, 5.7 s and 8 s for its launch-chain units at 45 and 128 draws; the runs and the oracle's transcriptions are 0.3 s or less
each."""
import math
import os

import numpy as np
import pytest

from tests import elementary_f32_ref as E
from tests import sample_reduce_ref as R
from tests.cases import SEED, hip_proposal, oracle_proposal
from tests.test_sort_source import GK_BOX, GK_C, GK_UPDATES, assert_matches_the_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = open(os.path.join(ROOT, "tests", "team_sample_f32", "sample_probe_f32.hip")).read()
HAND_SRC = open(os.path.join(ROOT, "tests", "team_sample_f32", "quads_by_hand_probe.hip")).read()
ROWS = 250
EXTRA = 18                                             # the probe's outputs behind the two halves
U = 2.0 ** -53
P = 0.5
SHORT = np.sort(np.random.default_rng(SEED + 1).normal(size=7))
HAND_BLOCKS = 129                                      # 516 draws: every size below


def observed(n):
    return np.sort(np.random.default_rng(SEED + n).normal(size=n))


FORWARD = {}


def forward(S, n, lanes):
    """drawn, sorted, the 18 further outputs; computed once per (n, lanes) and shared by the tests, which leave it unchanged"""
    if (n, lanes) not in FORWARD:
        model = S.DeviceSource(f"#define PROBE_N {n}\n" + PROBE_SRC, 1, 2, [P], data=[observed(n), SHORT], n_outputs=2 * n + EXTRA, team_lanes=lanes)
        out = S.simulate_outputs(model, np.zeros((ROWS, 1)), seed=SEED)
        assert out.shape == (ROWS, 1, 2 * n + EXTRA)
        FORWARD[(n, lanes)] = (out[:, 0, :n], out[:, 0, n:2 * n], out[:, 0, 2 * n:])
    return FORWARD[(n, lanes)]


def drawn_by_hand(S):
    if "hand" not in FORWARD:
        model = S.DeviceSource(f"#define HAND_BLOCKS {HAND_BLOCKS}\n" + HAND_SRC, 1, 1, [0.0], n_outputs=4 * HAND_BLOCKS)
        out = S.simulate_outputs(model, np.zeros((ROWS, 1)), seed=SEED)
        assert out.shape == (ROWS, 1, 4 * HAND_BLOCKS) and np.isfinite(out).all()
        FORWARD["hand"] = out[:, 0, :]
    return FORWARD["hand"]


def is_binary32(a):
    return np.array_equal(a, a.astype(np.float32).astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,n", [(16, 1), (16, 4), (16, 5), (16, 45), (16, 64), (16, 65), (16, 128), (16, 513),
                                     (4, 3), (4, 16), (4, 17), (4, 100), (4, 128), (4, 129)])
def test_a_team_per_row_draws_the_binary32_stream_and_sorts_it(S, gpu, monkeypatch, lanes, n):
    monkeypatch.setenv("SABC_PERSISTENT", "0")      # a forward run never launches the one-launch kernels
    drawn, ordered, r = forward(S, n, lanes)
    assert np.isfinite(drawn).all() and (n < 2 or (np.diff(drawn, axis=1) < 0).any())      # a sample, not an ascending ramp
    np.testing.assert_array_equal(ordered, np.sort(drawn, axis=1))
    assert is_binary32(drawn) and is_binary32(ordered)
    one_drawn, one_ordered, _ = forward(S, n, 1)
    np.testing.assert_array_equal(one_ordered, np.sort(one_drawn, axis=1))
    np.testing.assert_array_equal(drawn, one_drawn)
    np.testing.assert_array_equal(drawn, drawn_by_hand(S)[:, :n])
    assert len(np.unique(drawn[:, 0])) == ROWS                                              # every row its own stream
    # the read-outs: drawn(0), at(N - 1), at(0) against order_statistic(1), +inf outside [1, N]
    np.testing.assert_array_equal(r[:, 15], drawn[:, 0])
    np.testing.assert_array_equal(r[:, 16], ordered[:, n - 1])
    assert (r[:, 17] == 0.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [4, 16])
def test_a_planted_nan_duplicates_and_ties(S, gpu, monkeypatch, lanes):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    n = 8
    planted = np.array([2.5, np.nan, -1.0, 2.5, 7.0, 2.5, -1.0, 0.0])
    obs = np.array([-1.0, -1.0, 0.0, 1.0, 2.5, 2.5, 3.0, 7.0])          # ties with the planted values
    short = np.array([-1.0, 0.0, 0.0, 2.5, 2.5, 6.0, 7.0])
    model = S.DeviceSource(f"#define PROBE_N {n}\n#define PROBE_PLANTED 1\n" + PROBE_SRC, 1, 2, [P], data=[planted, obs, short],
                           n_outputs=2 * n + EXTRA, team_lanes=lanes)
    out = S.simulate_outputs(model, np.zeros((ROWS, 1)), seed=SEED)[:, 0, :]
    entered = np.where(np.isnan(planted), np.inf, planted)             # the NaN enters as +inf (at fill time) and comes out last
    expect = np.sort(entered)
    assert expect[7] == np.inf
    np.testing.assert_array_equal(out[:, :n], np.tile(entered, (ROWS, 1)))
    np.testing.assert_array_equal(out[:, n:2 * n], np.tile(expect, (ROWS, 1)))
    r = out[:, 2 * n:]
    assert (r[:, 7] == R.ks(expect, obs)).all() and (r[:, 8] == R.ks(expect, short)).all()
    assert (r[:, 1] == np.inf).all() and (r[:, 2] == np.inf).all() and (r[:, 3] == np.inf).all() and (r[:, 4] == -1.0).all()
    assert (r[:, 14] == 2.5).all() and (r[:, 15] == 2.5).all() and (r[:, 16] == np.inf).all() and (r[:, 17] == 0.0).all()


BITS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [45, 128])
@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_the_reductions_in_f64_over_a_binary32_sample(S, gpu, monkeypatch, lanes, n):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    drawn, x, r = forward(S, n, lanes)
    y = observed(n)
    assert np.isfinite(x).all() and np.isfinite(r).all() and is_binary32(x)
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
        assert abs(r[row, 0] - exact) <= bound
    # max and min are order-free
    np.testing.assert_array_equal(r[:, 3], drawn.max(axis=1))
    np.testing.assert_array_equal(r[:, 4], x.min(axis=1))
    np.testing.assert_array_equal(r[:, 12], (np.abs(x) + index).max(axis=1))
    np.testing.assert_array_equal(r[:, 13], (drawn - index).min(axis=1))
    # Kolmogorov-Smirnov: integers, bit for bit; an observed sample of the same and of another length
    np.testing.assert_array_equal(r[:, 7], R.ks(x, y))
    np.testing.assert_array_equal(r[:, 8], R.ks(x, SHORT))
    # the quantile at 1/2: type 7, h = (n - 1) / 2
    h = (n - 1) * P
    i = int(h)
    want_q = x[:, i] if h == i else x[:, i] + (h - i) * (x[:, i + 1] - x[:, i])
    np.testing.assert_array_equal(r[:, 14], want_q)
    # moments and the squared distance: two passes, against extended precision; products may contract into the additions
    wide = x.astype(np.longdouble)
    mean = wide.sum(axis=1) / n
    var = ((wide - mean[:, None]) ** 2).sum(axis=1) / (n - 1)
    err = np.abs((r[:, 6].astype(np.longdouble) - var) / var).max()
    print(f"W={lanes} N={n}: relative error of the variance {float(err):.3e}, bound {4 * (n + 3) * U:.3e}")
    assert err <= 4 * (n + 3) * U
    w2 = ((wide - y.astype(np.longdouble)) ** 2).sum(axis=1) / n
    err2 = np.abs((r[:, 9].astype(np.longdouble) - w2) / w2).max()
    print(f"W={lanes} N={n}: relative error of wasserstein2_squared {float(err2):.3e}, bound {4 * (n + 3) * U:.3e}")
    assert err2 <= 4 * (n + 3) * U
    # the same bits whatever the width
    BITS.setdefault(n, {})[lanes] = (x, r[:, [1, 2, 3, 4, 5, 7, 8, 10, 11, 12, 14]])
    first = next(iter(BITS[n].values()))
    for other in BITS[n].values():
        np.testing.assert_array_equal(other[0], first[0])
        np.testing.assert_array_equal(other[1], first[1])


# ---- population runs of GandKSampleF32 against the oracle ----
DRAWS = 45


def gk_y_obs(n_draws=DRAWS):
    z = np.random.default_rng(SEED).normal(size=n_draws)
    return np.sort(3.0 + 1.0 * (1.0 + GK_C * np.tanh(2.0 * z / 2.0)) * (1.0 + z * z) ** 0.5 * z)


def gk_f(O, y, seen, n, n_draws):
    """device_sources/gk_sample_f32.hip over the oracle's Philox blocks: ceil(n_draws / 4) blocks of four binary32 normals
    (tests/elementary_f32_ref.py), the transform in float64, x rounded to binary32 once.  Inside GK_BOX |z| <= 6.7637 keeps
    |x| <= 6 + 3 * 1.8 * 46.7^1.5 * 6.77 < 1.2e4, far from binary32 overflow.  The oracle asks particle by particle; the normals
    do not depend on theta, so those of a whole iteration are restated at once."""
    normals = {}
    n_blocks = (n_draws + 3) // 4

    def f(θ, pid, it):
        if it not in normals:
            w = E.philox_blocks(SEED, np.arange(n, dtype=np.uint64)[:, None], O.PURPOSE_SIM, it, np.arange(n_blocks)[None, :])
            normals[it] = E.box_muller_quad(w.reshape(-1, 4)).reshape(n, 4 * n_blocks)
        A, B, g, k = (float(t) for t in θ)
        z = normals[it][pid][:n_draws].astype(np.float64)
        x = (A + B * (1.0 + GK_C * np.tanh(g * z / 2.0)) * np.exp(k * np.log1p(z * z)) * z).astype(np.float32)
        x = np.sort(x).astype(np.float64)
        rho = (float(R.wasserstein1(x, y)), float(R.ks(x, y)))
        seen.extend(rho)
        return rho
    return f


def oracle_gk_run(O, n, prop="rw", n_draws=DRAWS):
    seen = []
    cfg = O.make_config(n_particles=n, n_para=4, n_stats=2, model_id=O.MODEL_HOST, model_params=[], seed=SEED,
                        prior=[(O.PRIOR_UNIFORM, lo, hi) for lo, hi in GK_BOX],
                        host_fn=O.host_simulator(gk_f(O, gk_y_obs(n_draws), seen, n, n_draws), 4, 2), algorithm=O.ALG_MULTI_EPS)
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


def device_gk_run(S, n, team_lanes, prop="rw", n_draws=DRAWS):
    prior = S.product_distribution([S.Uniform(lo, hi) for lo, hi in GK_BOX])
    model = S.GandKSampleF32(gk_y_obs(n_draws), distance=("wasserstein", "ks"), c=GK_C, team_lanes=team_lanes)
    return S.sabc(model, prior, n_particles=n, n_simulation=(GK_UPDATES + 1) * n, proposal=hip_proposal(S, prop, 4), resample=n // 2,
                  algorithm="multi_eps", seed=SEED)


SMALL_ACCEPTS, CHAIN_ACCEPTS = {}, {}


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_gk_sample_f32_in_one_launch_against_the_oracle(S, gpu, monkeypatch, oracle_small, lanes):
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
@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_gk_sample_f32_on_the_launch_chain_against_the_oracle(S, gpu, monkeypatch, oracle_chain, lanes):
    """n = 3000 is no multiple of the particles a workgroup takes: the last workgroup's trips end inside a trip."""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_gk_run(S, 3000, lanes)
    assert res._handle.persistent_lanes == 0 and res._handle.chain_team_lanes == lanes
    assert_matches_the_oracle(res, oracle_chain)
    CHAIN_ACCEPTS[lanes] = res.state.n_accept
    assert len(set(CHAIN_ACCEPTS.values())) == 1, CHAIN_ACCEPTS


@pytest.mark.gpu
def test_differential_evolution_with_a_row_per_particle_against_the_oracle(S, gpu, monkeypatch, O):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_gk_run(S, 3000, 16, prop="de")
    assert res._handle.chain_team_lanes == 16
    assert_matches_the_oracle(res, oracle_gk_run(O, 3000, prop="de"))


@pytest.mark.gpu
def test_128_draws_with_a_quad_per_particle_against_the_oracle(S, gpu, monkeypatch, O):
    """the headline shape on the width that runs out of registers in f64: 32 slots per lane"""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_gk_run(S, 512, 4, n_draws=128)
    assert res._handle.chain_team_lanes == 4
    assert_matches_the_oracle(res, oracle_gk_run(O, 512, n_draws=128))


@pytest.mark.gpu
def test_posterior_predictive_of_gk_sample_f32(S, gpu, monkeypatch):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    n = 500
    res = device_gk_run(S, n, 4)
    pp = S.posterior_predictive(res, n_rep=2)
    assert pp.shape == (n, 2, DRAWS)
    assert np.isfinite(pp).all() and (np.diff(pp, axis=2) >= 0).all() and is_binary32(pp)
    assert len(np.unique(pp[:, 0, :])) > n                                   # samples, not one constant
