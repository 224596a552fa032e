"""Count draws keyed by an index on the device (sabc::CountDraws, csrc/device_rng.hpp; Series::map_poisson, csrc/team_series.hpp)
and the model shipped on them, Ricker (device_sources/ricker.hip).

The forward run with a team per row: tests/series_counts/counts_probe.hip emits (a) keyed Poisson draws on a ramp of lambda --
0, a negative value, NaN, 9.99, 10, 10.01, one above 2^30, values in (0, 10) and up to 3000 --, (b) keyed binomial draws across
the degenerate cases, inversion, BTRS and reflection, both drawn inside fill by the lane that holds the time, (c) the pair()
behind three reservations, (d) a branching process -- a recurrence whose f draws, dying out in some rows and growing to the
clamp at 2^30 in others -- whole with the returned state, and (e) map_poisson on a filled series; for 250 rows, a last wave that
is not full and a last team inside it.  EVERYTHING is held to tests/count_draws_ref.py exactly -- the counts as integers, the
normals of (c) bit for bit.  Sizes as for the recurrences (tests/test_gpu_series_recur.py): 1, 3, 45 on all three widths
(compared with each other), 128, 129; at 3 and 45 also recur itself, the unrolled relay, with the draw inside.  Probes of one size share a compiled
unit and one reference.

Ricker at burn_in 5, n_obs 40, n_lags 2 (N = 45): the four forms on the same thetas and streams -- the latent states the
transcription's bits, the counts exact, all five distances the restatement's bits --; population runs against the oracle driving
the Python transcription over the same Philox blocks (one launch with teams of 1, 4 and 16 lanes; the launch chain with the
plain form and 1, 4 and 16 lanes per particle at n = 1100; equal accept counts; one DifferentialEvolution run); the posterior predictive;
observe and from_observations."""
import numpy as np
import pytest

from tests import count_draws_ref as C
from tests import elementary_ref as E
from tests.cases import SEED, hip_proposal, oracle_proposal
from tests.test_f32_draws import f64_pair
from tests.test_gpu_team_series import PURPOSE_PREDICT, PURPOSE_SIM, ROWS, assert_same_bits, stream_normals
from tests.test_series_counts_compile import PROBE_PARAMS, probe_data, probe_model, probe_outputs
from tests.test_sort_source import GK_UPDATES, assert_matches_the_oracle

OFFSPRING = np.linspace(0.4, 1.6, ROWS)              # theta[0] of the probe: the branching process dies out | grows across the rows

_WANT = {}


def probe_reference(O, n):
    """What counts_probe.hip emits at length n, from the restatement: ([ROWS, probe_outputs(n)], the same with math.log / lgamma
    in the draws).  Computed once per size and shared by the widths, which leave it unchanged."""
    if n not in _WANT:
        x = stream_normals(O, PURPOSE_PREDICT, 0, ROWS, n)
        lam, trials, prob = probe_data(n)
        s0, scale = PROBE_PARAMS
        blocks = (n + 1) // 2
        both = []
        for functions in (C.FUNCTIONS_TABLE, C.FUNCTIONS_MATH):
            rows = []
            for pid in range(ROWS):
                k = blocks
                cd_a, k = C.reserve_counts(O, SEED, pid, 0, PURPOSE_PREDICT, k, n, functions)
                cd_b, k = C.reserve_counts(O, SEED, pid, 0, PURPOSE_PREDICT, k, n, functions)
                cd_d, k = C.reserve_counts(O, SEED, pid, 0, PURPOSE_PREDICT, k, n, functions)
                assert k == blocks + 64 * 3 * n
                a = [cd_a.poisson(t, lam[t]) for t in range(n)]
                b = [cd_b.binomial(t, trials[t], prob[t]) for t in range(n)]
                c = list(f64_pair(O.stream_block(SEED, pid, PURPOSE_PREDICT, 0, k)))
                cd_e, _ = C.reserve_counts(O, SEED, pid, 0, PURPOSE_PREDICT, k + 1, n, functions)
                s, d = s0, []
                for t in range(n):
                    s = float(cd_d.poisson(t, E.fma(float(OFFSPRING[pid]), s, abs(float(x[pid, t])))))
                    d.append(s)
                e = [cd_e.poisson(t, scale * (8.0 * abs(float(x[pid, t])))) for t in range(n)]
                rows.append(a + b + c + d + [s] + e)
            both.append(np.array(rows, dtype=np.float64))
        _WANT[n] = tuple(both)
        assert both[0].shape == (ROWS, probe_outputs(n))
    return _WANT[n]


BITS_AT_45 = {}
# recur itself with the draw inside, the unrolled relay: a copy of the draw per time step, so 3 and 45 values only (at 45 on a row
# of 16: four slots per lane, twelve phases, a lane that holds one value and four that hold none; the compiler takes minutes for 128)
PLAIN = "#define PROBE_PLAIN_RECUR 1\n"


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,n,head", [(16, 1, ""), (16, 3, ""), (4, 3, ""), (16, 3, PLAIN), (4, 3, PLAIN), (16, 45, ""), (4, 45, ""), (1, 45, ""),
                                          (16, 45, PLAIN), (1, 45, PLAIN), (16, 128, ""), (4, 128, ""), (16, 129, ""), (4, 129, "")])
def test_the_keyed_counts_of_a_team_per_row(S, O, gpu, monkeypatch, lanes, n, head):
    monkeypatch.setenv("SABC_PERSISTENT", "0")      # a forward run never launches the one-launch kernels
    out = S.simulate_outputs(probe_model(S, n, lanes, head), OFFSPRING.reshape(ROWS, 1), seed=SEED)
    assert out.shape == (ROWS, 1, probe_outputs(n))
    out = out[:, 0, :]
    assert np.isfinite(out).all()                   # every output was emitted: what is never emitted reads as NaN
    want, with_libm = probe_reference(O, n)
    names = ["(a) poisson on the ramp", "(b) binomial", "(c) the pair behind the reservations", "(d) the branching process and its state", "(e) map_poisson"]
    edges = np.cumsum([0, n, n, 2, n + 1, n])
    for name, lo, hi in zip(names, edges[:-1], edges[1:]):
        wrong = int((out[:, lo:hi].view(np.uint64) != want[:, lo:hi].view(np.uint64)).sum())
        libm = int((out[:, lo:hi] != with_libm[:, lo:hi]).sum())
        print(f"N={n} W={lanes}: {name}: {wrong} of {ROWS * (hi - lo)} values differ from the restatement, {libm} from the one with math.log / lgamma")
    counts = np.delete(out, [2 * n, 2 * n + 1], axis=1)
    assert (counts == np.floor(counts)).all() and (counts >= 0).all()
    np.testing.assert_array_equal(counts.astype(np.int64), np.delete(want, [2 * n, 2 * n + 1], axis=1).astype(np.int64))
    assert_same_bits(out, want)
    if n >= 45:
        d = out[:, 2 * n + 2:3 * n + 3]
        assert (d[:20, -1] < 50).all() and (d[-20:, -1] > 1000).all()           # both fates of the process are among the rows
        assert out[:, 6].min() > 2 ** 29                                        # lambda = 2^31 was drawn as 2^30
    if n == 45:                                     # (the rolled and the unrolled relay included)
        BITS_AT_45[lanes, head] = out
        first = next(iter(BITS_AT_45.values()))
        for other in BITS_AT_45.values():
            assert_same_bits(other, first)


# ---- Ricker ----
N_OBS, BURN_IN, N_LAGS, N0 = 40, 5, 2, 1.0
N_ALL = BURN_IN + N_OBS
RICKER_BOX = [(2.0, 4.5), (0.05, 0.6), (4.0, 16.0)]   # the benchmark's regime, chaotic (log r > 2.69): the forward runs, on given thetas
# The population runs against the oracle stay below log r = 2, where the map's fixed point N* = log r is stable.  The oracle
# proposes on the CPU and agrees with the device's thetas to 1e-9 (assert_matches_the_oracle), not bit for bit; in the chaotic
# regime a last-place difference in log r grows to another trajectory and other counts within the 45 steps, so the distances of
# the few particles whose theta differs in its last place are other numbers, whatever the device computes; below 2 the
# difference shrinks, and a count changes only where a uniform falls within 1e-16 of a threshold.  Both branches of the draw
# stay in play: lambda = phi N is 2 to 40.  The chaotic regime, with its zeros and its lambda in the hundreds, is held to the
# transcription by the forward runs above, on thetas both sides are given.
STABLE_BOX = [(0.5, 1.9), (0.05, 0.6), (4.0, 16.0)]
U = 2.0 ** -53


def ricker_obs(O, theta=(3.8, 0.3, 10.0)):
    _, y = C.ricker_simulation(O, SEED, 0, 0, O.PURPOSE_PRIOR, theta, N_OBS, BURN_IN, N0)
    return C.ricker_summaries_of_series(y, N_LAGS, BURN_IN)


def stable_obs(O):
    return ricker_obs(O, (1.5, 0.3, 10.0))


def ricker_f(O, obs, seen):
    """device_sources/ricker.hip over the oracle's Philox blocks: ceil(45 / 2) blocks of normals -- the device's bit for bit, through
    the transcription of the table-driven Box-Muller pair: the oracle's own normals agree to 1e-9 only, which a chaotic map with
    discrete observations does not forgive --, the counts keyed behind them"""
    def f(θ, pid, it):
        _, y = C.ricker_simulation(O, SEED, pid, it, O.PURPOSE_SIM, θ, N_OBS, BURN_IN, N0)
        rho = tuple(float(v) for v in C.ricker_distances(y, obs, N_LAGS, BURN_IN))
        seen.extend(rho)
        return rho
    return f


def oracle_ricker_run(O, n, prop="rw"):
    seen = []
    cfg = O.make_config(n_particles=n, n_para=3, n_stats=N_LAGS + 3, model_id=O.MODEL_HOST, model_params=[], seed=SEED,
                        prior=[(O.PRIOR_UNIFORM, lo, hi) for lo, hi in STABLE_BOX],
                        host_fn=O.host_simulator(ricker_f(O, stable_obs(O), seen), 3, N_LAGS + 3), algorithm=O.ALG_MULTI_EPS)
    run = O.OracleRun(cfg)
    run.initialize((GK_UPDATES + 1) * n)
    run.update(O.make_update_args(n_simulation=GK_UPDATES * n, proposal=oracle_proposal(O, prop, 3), n_para=3, n_particles=n, resample=n // 2))
    # copies: the arrays are read once and shared by the tests below, which leave them unchanged
    return dict(counters=dict(run.counters), theta=np.array(run.theta), rho=np.array(run.rho), eps=np.array(run.eps), seen=np.array(seen))


@pytest.fixture(scope="module")
def oracle_small(O):
    return oracle_ricker_run(O, 1000)


# The launch chain at n = 1100, not the 3000 of the other series models: the transcription draws its normals through the Python
# Box-Muller pair (6 ms per simulation; 3000 particles would be two minutes of CPU per fixture).  Four workgroups of 256 particles
# and a remainder of 76; N stays 45.
CHAIN_N = 1100


@pytest.fixture(scope="module")
def oracle_chain(O):
    return oracle_ricker_run(O, CHAIN_N)


def ricker_prior(S, box=RICKER_BOX):
    return S.product_distribution([S.Uniform(lo, hi) for lo, hi in box])


def device_ricker_run(S, O, n, team_lanes, prop="rw"):
    model = S.Ricker(stable_obs(O), n_obs=N_OBS, burn_in=BURN_IN, n_lags=N_LAGS, n0=N0, team_lanes=team_lanes)
    return S.sabc(model, ricker_prior(S, STABLE_BOX), n_particles=n, n_simulation=(GK_UPDATES + 1) * n, proposal=hip_proposal(S, prop, 3), resample=n // 2,
                  algorithm="multi_eps", seed=SEED)


SMALL_ACCEPTS, CHAIN_ACCEPTS = {}, {}


@pytest.mark.gpu
def test_the_four_forms_of_ricker_give_the_same_bits(S, O, gpu, monkeypatch):
    """The same thetas on the same streams through the plain form and through teams of 1, 4 and 16 lanes.  The source is the
    model's own with RICKER_EMIT_LATENT in front, so the latent states are outputs too: they are the transcription's bits -- the
    sequential loop with exp_tab's restatement --, the counts the restatement's exactly, the five distances its bits."""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    obs = ricker_obs(O)
    rng = np.random.default_rng(SEED)
    theta = np.stack([rng.uniform(lo, hi, ROWS) for lo, hi in RICKER_BOX])              # [d][m]
    z = stream_normals(O, PURPOSE_SIM, 3, ROWS, N_ALL)
    runs = [C.ricker_simulation(O, SEED, row, 3, PURPOSE_SIM, theta[:, row], N_OBS, BURN_IN, N0, normals=z[row]) for row in range(ROWS)]
    want_latent, want_y = np.array([r[0] for r in runs]), np.array([r[1] for r in runs])
    want_rho = C.ricker_distances(want_y, obs, N_LAGS, BURN_IN)
    assert np.isfinite(want_latent).all() and (want_latent > 0).all() and (want_y == 0).any() and want_y.max() > 50
    seen = {}
    for lanes in (None, 1, 4, 16):
        shipped = S.Ricker(obs, n_obs=N_OBS, burn_in=BURN_IN, n_lags=N_LAGS, n0=N0, team_lanes=lanes)
        model = S.DeviceSource("#define RICKER_EMIT_LATENT 1\n" + shipped.source, 3, N_LAGS + 3, shipped.params, data=[obs],
                               n_outputs=N_OBS + N_ALL, team_lanes=lanes)
        h = S.SabcHandle(n_particles=ROWS, model=model, prior=ricker_prior(S), seed=SEED, algorithm=S._lib.ALG_MULTI_EPS)
        try:
            rho, out = h.simulate_outputs(theta, 0, 3)
            rho_again = h.simulate(theta, 0, 3)
        finally:
            h.close()
        y, latent = np.ascontiguousarray(out.T[:, :N_OBS]), np.ascontiguousarray(out.T[:, N_OBS:])
        print(f"team_lanes={lanes}: {int((latent.view(np.uint64) != want_latent.view(np.uint64)).sum())} of {latent.size} latent states differ from the "
              f"transcription's bits, {int((y != want_y[:, BURN_IN:]).sum())} of {y.size} counts, "
              f"{int((np.ascontiguousarray(rho.T).view(np.uint64) != want_rho.view(np.uint64)).sum())} of {rho.size} distances")
        assert_same_bits(latent, want_latent)
        np.testing.assert_array_equal(y.astype(np.int64), want_y[:, BURN_IN:].astype(np.int64))
        assert_same_bits(y, want_y[:, BURN_IN:])
        assert_same_bits(rho.T, want_rho)
        assert_same_bits(rho_again, rho)
        seen[lanes] = (y, latent, rho)
    for lanes in (1, 4, 16):
        for got, plain in zip(seen[lanes], seen[None]):
            assert_same_bits(got, plain)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_ricker_in_one_launch_against_the_oracle(S, O, gpu, monkeypatch, oracle_small, lanes):
    """n = 1000: the one-launch form chooses its own team -- a lane, a quad, a row of 16 lanes per particle -- and the team-aware
    source divides the count draws over it."""
    monkeypatch.setenv("SABC_PERSISTENT", "1")
    monkeypatch.setenv("SABC_PERSISTENT_LANES", str(lanes))
    res = device_ricker_run(S, O, 1000, 16)
    assert res._handle.persistent_lanes == lanes and res._handle.chain_team_lanes == 16
    assert_matches_the_oracle(res, oracle_small)
    SMALL_ACCEPTS[lanes] = res.state.n_accept
    assert len(set(SMALL_ACCEPTS.values())) == 1, SMALL_ACCEPTS


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [None, 1, 4, 16])
def test_ricker_on_the_launch_chain_against_the_oracle(S, O, gpu, monkeypatch, oracle_chain, lanes):
    """n = 1100 is no multiple of the particles a workgroup takes.  None: the plain form, Series<45, 1> in sabc_user_simulate.
    Every form accepts the same number of particles."""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_ricker_run(S, O, CHAIN_N, lanes)
    assert res._handle.persistent_lanes == 0 and res._handle.chain_team_lanes == (lanes or 0)
    assert_matches_the_oracle(res, oracle_chain)
    CHAIN_ACCEPTS[lanes] = res.state.n_accept
    assert len(set(CHAIN_ACCEPTS.values())) == 1, CHAIN_ACCEPTS


@pytest.mark.gpu
def test_differential_evolution_against_the_oracle(S, gpu, monkeypatch, O):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    res = device_ricker_run(S, O, CHAIN_N, 16, prop="de")
    assert res._handle.chain_team_lanes == 16
    assert_matches_the_oracle(res, oracle_ricker_run(O, CHAIN_N, prop="de"))


@pytest.mark.gpu
def test_posterior_predictive_of_ricker(S, O, gpu, monkeypatch):
    """The outputs are the counts the device summarised, exact integers, so Ricker.summaries restates the device's own operations
    on the same values: the sums of counts and of 0 / 1 terms are exact in any order, and each autocovariance is the same tree of
    the same rounded products.  What may differ is the run-time compiler contracting y - c into the product behind it -- it does
    not: rounded_product takes rounded factors -- so the bound derived as GARCH11's is derives to zero for the summaries, and
    the distances |s - obs| round once in each computation: u max(|s|, |obs|) each, 2 u max(|s|, |obs|) asserted."""
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    n = 500
    res = device_ricker_run(S, O, n, 4)
    pp, dist = S.posterior_predictive(res, n_rep=2, return_distances=True)
    assert pp.shape == (n, 2, N_OBS) and dist.shape == (n, 2, N_LAGS + 3)
    assert np.isfinite(pp).all() and (pp >= 0).all() and (pp == np.floor(pp)).all() and len(np.unique(pp[:, 0, :], axis=0)) > n // 2
    obs = stable_obs(O)
    s = S.Ricker.summaries(pp, N_LAGS, BURN_IN)
    want = np.abs(s - obs)
    tol = 2 * U * np.maximum(np.abs(s), np.abs(obs))
    print(f"posterior predictive: the largest |distance - restated distance| is {float(np.abs(dist - want).max()):.3g}, "
          f"{int((dist != want).sum())} of {dist.size} differ at all")
    assert (np.abs(dist - want) <= tol).all()


@pytest.mark.gpu
def test_observe_and_from_observations(S, O, gpu, monkeypatch):
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    theta = (3.8, 0.3, 10.0)
    y = S.Ricker.observe(theta, n_obs=N_OBS, burn_in=BURN_IN, seed=SEED, n0=N0)
    assert y.shape == (N_OBS,)
    _, want = C.ricker_simulation(O, SEED, 0, 0, PURPOSE_PREDICT, theta, N_OBS, BURN_IN, N0)
    np.testing.assert_array_equal(y, want[BURN_IN:])
    model = S.Ricker.from_observations(y, burn_in=BURN_IN, n_lags=N_LAGS, team_lanes=4)
    assert_same_bits(model.data[0], C.ricker_summaries(y, N_LAGS, BURN_IN))
    assert (model.n_obs, model.burn_in, model.n_stats) == (N_OBS, BURN_IN, N_LAGS + 3)
