"""sabc::Series::recur on the device (csrc/team_series.hpp) and the model shipped on it, GARCH11 (device_sources/garch11.hip).

The forward run with a team per row: tests/series_recur/recur_probe.hip emits its series, cumsum() whole with the state the same
sum's recur returns, the AR(2) recurrence with a Carry<2> (first = 0 and 2) whole with both components of the returned state, and
a recur_with against a ramp through exp_tab, for 250 rows -- a last wave that is not full, a last team inside it.  The series is
the Python transcription of the stream's normals bit for bit (shared with tests/test_gpu_team_series.py), and EVERYTHING is held
to the restatement's sequential loop (tests/series_recur_ref.py) bit for bit.  Sizes, the smallest at which the relay can go
wrong: one value; three (two lanes; first = 2 leaves one step); 45 on a row of 16 (M = 4: twelve lanes, the last partly, four
with nothing), on a quad (M = 16, lane 3 empty) and on a lane per row, the three compared with each other; 128 (every slot of
every lane, 32 slots per lane in the quad); 129 on a row of 16 (one element alone on the ninth lane) and on a quad (the
replicated fallback).  Probes of one size share a compiled unit and one reference.

GARCH11 at n_obs = 45, n_lags = 2: the four forms on the same thetas and streams -- the squared returns and all four distances
the transcription's bits, the returns within 1 ulp of copysign(sqrt(r), z) --; population runs against the oracle driving the
Python transcription over the same Philox blocks (one launch with teams of 1, 4 and 16 lanes; the launch chain with the plain
form and 1, 4 and 16 lanes per particle; equal accept counts; one DifferentialEvolution run); the posterior predictive; observe
and from_observations."""
import os

import numpy as np
import pytest

from tests import series_recur_ref as R
from tests.cases import SEED, hip_proposal, oracle_proposal
from tests.test_gpu_team_series import PURPOSE_PREDICT, PURPOSE_SIM, ROWS, assert_same_bits, stream_normals
from tests.test_series_recur_compile import PHI, probe_outputs
from tests.test_sort_source import GK_UPDATES, assert_matches_the_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = open(os.path.join(ROOT, "tests", "series_recur", "recur_probe.hip")).read()

_WANT = {}


def probe_reference(O, n):
    """What recur_probe.hip emits at length n, from the restatement over the transcribed normals: [ROWS, probe_outputs(n)].
    Computed once per size and shared by the widths, which leave it unchanged."""
    if n not in _WANT:
        x = stream_normals(O, PURPOSE_PREDICT, 0, ROWS, n)

        def add(t, s, v):
            s = s + v
            return s, s
        summed, total = R.recur(x, 0.0, add)
        np.testing.assert_array_equal(summed, R.cumsum(x))
        parts = [x, summed, total[:, None]]
        for first in (0, 2) if n > 2 else (0,):
            out, state = R.recur(x, (0.25, -0.5), R.ar2(*PHI), first)
            parts += [out, state]
        parts.append(R.recur(x, 1.5, R.damped_exp, other=0.125 * np.arange(n))[0])
        _WANT[n] = np.concatenate(parts, axis=1)
        assert _WANT[n].shape == (ROWS, probe_outputs(n))
    return _WANT[n]


BITS_AT_45 = {}


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,n", [(16, 1), (16, 3), (4, 3), (16, 45), (4, 45), (1, 45), (16, 128), (4, 128), (16, 129), (4, 129)])
def test_the_recurrences_of_a_team_per_row(S, O, gpu, monkeypatch, lanes, n):
    monkeypatch.setenv("SABC_PERSISTENT", "0")      # a forward run never launches the one-launch kernels
    model = S.DeviceSource(f"#define PROBE_N {n}\n" + PROBE_SRC, 1, 1, list(PHI), n_outputs=probe_outputs(n), team_lanes=lanes)
    out = S.simulate_outputs(model, np.zeros((ROWS, 1)), seed=SEED)
    assert out.shape == (ROWS, 1, probe_outputs(n))
    out = out[:, 0, :]
    assert np.isfinite(out).all()                   # every output was emitted: what is never emitted reads as NaN
    want = probe_reference(O, n)
    assert len(np.unique(want[:, 0])) == ROWS
    names = ["the series", "cumsum and the sum's state", "AR(2) and its state"] + (["AR(2) with first = 2"] if n > 2 else []) + ["recur_with"]
    edges = np.cumsum([0, n, n + 1, n + 2] + ([n + 2] if n > 2 else []) + [n])
    for name, lo, hi in zip(names, edges[:-1], edges[1:]):
        wrong = int((out[:, lo:hi].view(np.uint64) != want[:, lo:hi].view(np.uint64)).sum())
        print(f"N={n} W={lanes}: {name}: {wrong} of {ROWS * (hi - lo)} values differ from the sequential loop's bits")
    assert_same_bits(out, want)
    if n == 45:
        BITS_AT_45[lanes] = out
        first = next(iter(BITS_AT_45.values()))
        for other in BITS_AT_45.values():
            assert_same_bits(other, first)


# ---- GARCH11 ----
N_OBS, N_LAGS, SIGMA2_0 = 45, 2, 0.8
GARCH_BOX = [(0.05, 1.0), (0.0, 0.5), (0.0, 0.9)]
U = 2.0 ** -53


def garch_obs():
    z = np.random.default_rng(SEED).normal(size=N_OBS)
    return R.garch11_summaries_of_squares(R.garch11_squared_returns((0.2, 0.15, 0.7), z, SIGMA2_0), N_LAGS)


def finite_or_big(v):
    return np.where(np.isfinite(v), v, 1e30)


def garch_f(O, obs, seen):
    """device_sources/garch11.hip over the oracle's Philox blocks: ceil(45 / 2) blocks, the odd last normal the first of the last one"""
    def f(θ, pid, it):
        z = np.array([O.normal_pair(SEED, pid, O.PURPOSE_SIM, it, b) for b in range((N_OBS + 1) // 2)]).reshape(-1)[:N_OBS]
        r = R.garch11_squared_returns(θ, z, SIGMA2_0)
        rho = tuple(float(v) for v in finite_or_big(np.abs(R.garch11_summaries_of_squares(r, N_LAGS) - obs)))
        seen.extend(rho)
        return rho
    return f


def oracle_garch_run(O, n, prop="rw"):
    seen = []
    cfg = O.make_config(n_particles=n, n_para=3, n_stats=N_LAGS + 2, model_id=O.MODEL_HOST, model_params=[], seed=SEED,
                        prior=[(O.PRIOR_UNIFORM, lo, hi) for lo, hi in GARCH_BOX],
                        host_fn=O.host_simulator(garch_f(O, garch_obs(), seen), 3, N_LAGS + 2), algorithm=O.ALG_MULTI_EPS)
    run = O.OracleRun(cfg)
    run.initialize((GK_UPDATES + 1) * n)
    run.update(O.make_update_args(n_simulation=GK_UPDATES * n, proposal=oracle_proposal(O, prop, 3), n_para=3, n_particles=n, resample=n // 2))
    # copies: the arrays are read once and shared by the tests below, which leave them unchanged
    return dict(counters=dict(run.counters), theta=np.array(run.theta), rho=np.array(run.rho), eps=np.array(run.eps), seen=np.array(seen))


@pytest.fixture(scope="module")
def oracle_small(O):
    return oracle_garch_run(O, 1000)


@pytest.fixture(scope="module")
def oracle_chain(O):
    return oracle_garch_run(O, 3000)


def garch_prior(S):
    return S.product_distribution([S.Uniform(lo, hi) for lo, hi in GARCH_BOX])


def device_garch_run(S, n, team_lanes, prop="rw"):
    model = S.GARCH11(garch_obs(), n_obs=N_OBS, n_lags=N_LAGS, sigma2_0=SIGMA2_0, team_lanes=team_lanes)
    return S.sabc(model, garch_prior(S), n_particles=n, n_simulation=(GK_UPDATES + 1) * n, proposal=hip_proposal(S, prop, 3), resample=n // 2,
                  algorithm="multi_eps", seed=SEED)


def within_one_ulp(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.abs(got - want) <= np.spacing(np.abs(want))).all() and (np.signbit(got) == np.signbit(want)).all())


SMALL_ACCEPTS, CHAIN_ACCEPTS = {}, {}


@pytest.mark.gpu
def test_the_four_forms_of_garch11_give_the_same_bits(S, O, gpu, monkeypatch):
    """The same thetas on the same streams through the plain form and through teams of 1, 4 and 16 lanes.  The source is the
    model's own with GARCH11_EMIT_SQUARES in front, so the squared returns are outputs too: they are the transcription's bits --
    the sequential loop over the transcribed normals --, the four distances the restatement's of them, and the returns within
    1 ulp of copysign(sqrt(r), z), the bound the project asserts for sqrt_fast on the device."""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    obs = garch_obs()
    rng = np.random.default_rng(SEED)
    theta = np.stack([rng.uniform(lo, hi, ROWS) for lo, hi in GARCH_BOX])              # [d][m]
    z = stream_normals(O, PURPOSE_SIM, 3, ROWS, N_OBS)
    want_r = np.array([R.garch11_squared_returns(theta[:, row], z[row], SIGMA2_0) for row in range(ROWS)])
    want_rho = finite_or_big(np.abs(R.garch11_summaries_of_squares(want_r, N_LAGS) - obs))
    assert np.isfinite(want_r).all() and (want_r > 0).all()
    seen = {}
    for lanes in (None, 1, 4, 16):
        shipped = S.GARCH11(obs, n_obs=N_OBS, n_lags=N_LAGS, sigma2_0=SIGMA2_0, team_lanes=lanes)
        model = S.DeviceSource("#define GARCH11_EMIT_SQUARES 1\n" + shipped.source, 3, N_LAGS + 2, shipped.params, data=[obs],
                               n_outputs=2 * N_OBS, team_lanes=lanes)
        h = S.SabcHandle(n_particles=ROWS, model=model, prior=garch_prior(S), seed=SEED, algorithm=S._lib.ALG_MULTI_EPS)
        try:
            rho, out = h.simulate_outputs(theta, 0, 3)
            rho_again = h.simulate(theta, 0, 3)
        finally:
            h.close()
        y, r = out.T[:, :N_OBS], out.T[:, N_OBS:]
        wrong = int((np.ascontiguousarray(r).view(np.uint64) != want_r.view(np.uint64)).sum())
        worst = float((np.abs(y - R.garch11_returns(want_r, z)) / np.spacing(np.abs(R.garch11_returns(want_r, z)))).max())
        print(f"team_lanes={lanes}: {wrong} of {r.size} squared returns differ from the transcription's bits; the returns are within "
              f"{worst:.2f} ulp of copysign(sqrt(r), z)")
        assert_same_bits(r, want_r)
        assert_same_bits(rho.T, want_rho)
        assert_same_bits(rho_again, rho)
        assert within_one_ulp(y, R.garch11_returns(want_r, z))
        seen[lanes] = (y, r, rho)
    for lanes in (1, 4, 16):
        for got, plain in zip(seen[lanes], seen[None]):
            assert_same_bits(got, plain)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_garch11_in_one_launch_against_the_oracle(S, gpu, monkeypatch, oracle_small, lanes):
    """n = 1000: the one-launch form chooses its own team -- a lane, a quad, a row of 16 lanes per particle -- and the
    team-aware source relays the recurrence over it."""
    monkeypatch.setenv("SABC_PERSISTENT", "1")
    monkeypatch.setenv("SABC_PERSISTENT_LANES", str(lanes))
    res = device_garch_run(S, 1000, 16)
    assert res._handle.persistent_lanes == lanes and res._handle.chain_team_lanes == 16
    assert_matches_the_oracle(res, oracle_small)
    SMALL_ACCEPTS[lanes] = res.state.n_accept
    assert len(set(SMALL_ACCEPTS.values())) == 1, SMALL_ACCEPTS


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [None, 1, 4, 16])
def test_garch11_on_the_launch_chain_against_the_oracle(S, gpu, monkeypatch, oracle_chain, lanes):
    """n = 3000 is no multiple of the particles a workgroup takes.  None: the plain form, Series<45, 1> in sabc_user_simulate.
    Every form accepts the same number of particles."""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_garch_run(S, 3000, lanes)
    assert res._handle.persistent_lanes == 0 and res._handle.chain_team_lanes == (lanes or 0)
    assert_matches_the_oracle(res, oracle_chain)
    CHAIN_ACCEPTS[lanes] = res.state.n_accept
    assert len(set(CHAIN_ACCEPTS.values())) == 1, CHAIN_ACCEPTS


@pytest.mark.gpu
def test_differential_evolution_against_the_oracle(S, gpu, monkeypatch, O):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_garch_run(S, 3000, 16, prop="de")
    assert res._handle.chain_team_lanes == 16
    assert_matches_the_oracle(res, oracle_garch_run(O, 3000, prop="de"))


@pytest.mark.gpu
def test_posterior_predictive_of_garch11(S, gpu, monkeypatch):
    """The distances are the device's, of the squared returns r it holds; the test sees the returns y, within 1 ulp of sqrt(r), and
    squares them back.  With u = 2^-53: y = sqrt(r) (1 + d), |d| <= 3 u (the rounding of a correct sqrt, u, plus one ulp, at most
    2 u relative), so y y rounded is r (1 + e) with |e| <= 2 * 3 u + u + O(u^2) < 8 u.  The mean: every r_t moves by at most 8 u r_t,
    and each of the two tree sums over 64 leaves rounds 6 times and is divided once, 7 u relative each: |mean' - mean| <= 22 u mean
    (all r_t > 0).  The autocovariances: with A = max r_t, |r_t - c| <= A, and a centred value moves by at most 8 u A (r_t) +
    22 u A (c) + u A (the subtraction, in each of the two computations: 2 u A) = 32 u A; a product of two by at most 2 * 32 u A^2 plus
    its own rounding, 2 u A^2; the tree over N / the division add 2 * 7 u A^2: |acov' - acov| <= 80 u A^2.  The final |s - obs| rounds
    once more in each computation, u max(|s|, |obs|) each: 100 u max(mean or A^2, |obs_j|) covers all of it."""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    n = 500
    res = device_garch_run(S, n, 4)
    pp, dist = S.posterior_predictive(res, n_rep=2, return_distances=True)
    assert pp.shape == (n, 2, N_OBS) and dist.shape == (n, 2, N_LAGS + 2)
    assert np.isfinite(pp).all() and len(np.unique(pp[:, 0, :])) > n         # series, not one constant
    assert (pp < 0).any() and (pp > 0).any()                                  # returns: the normals' signs
    obs = garch_obs()
    want = np.abs(S.GARCH11.summaries(pp, N_LAGS) - obs)
    r = pp * pp
    top = r.max(axis=-1)[..., None]
    tol = 100 * U * np.maximum(np.concatenate([top, np.repeat(top * top, N_LAGS + 1, axis=-1)], axis=-1), np.abs(obs))
    print(f"posterior predictive: the largest |distance - restated distance| / tolerance is {float((np.abs(dist - want) / tol).max()):.3f}")
    assert (np.abs(dist - want) <= tol).all()


@pytest.mark.gpu
def test_observe_and_from_observations(S, O, gpu, monkeypatch):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    theta = (0.2, 0.15, 0.7)
    y = S.GARCH11.observe(theta, n_obs=N_OBS, seed=SEED, sigma2_0=SIGMA2_0)
    assert y.shape == (N_OBS,)
    z = stream_normals(O, PURPOSE_PREDICT, 0, 1, N_OBS)[0]
    assert within_one_ulp(y, R.garch11_returns(R.garch11_squared_returns(theta, z, SIGMA2_0), z))
    model = S.GARCH11.from_observations(y, team_lanes=4)
    assert_same_bits(model.data[0], R.garch11_summaries(y, N_LAGS))
    assert model.sigma2_0 == model.data[0][0] and (model.n_obs, model.n_stats) == (N_OBS, N_LAGS + 2)
