"""Count draws keyed by an index (sabc::CountDraws, csrc/device_rng.hpp) through their restatement, tests/count_draws_ref.py, on
the CPU: the draws follow their pmf (the chi-square helper and the cases of tests/test_discrete_draws.py, lambda on both sides
of 10 and p reflected above 1/2, one draw per index); an index owns its 64 blocks -- two indices never share one, a draw does not
depend on which other draws were made or in what order, and with math.log / math.lgamma a keyed draw IS
discrete_draws_ref.Stream positioned at block base + 64 i --; reserve_counts moves the counter by 64 n and the next
uniform_pair() is that block; the degenerate arguments give the header's values and compute no block."""
import math

import numpy as np
import pytest

from tests import count_draws_ref as C
from tests.cases import SEED
from tests.discrete_draws_ref import Stream
from tests.test_discrete_draws import BINOMIAL_CASES, N_DRAWS, POISSON_CASES, chi_square_p

BASE = 23                          # a reservation behind 23 blocks of normals


@pytest.mark.parametrize("case,lam", list(enumerate(POISSON_CASES)))
def test_keyed_poisson_draws_follow_the_pmf(O, case, lam):
    from scipy import stats
    cd = C.CountDraws(O, SEED + 1, 3000 + case, 3, base=BASE)
    draws = np.array([cd.poisson(i, lam) for i in range(N_DRAWS)])
    dist = stats.poisson(lam)
    p = chi_square_p(draws, dist.pmf, int(dist.ppf(1e-9)), int(dist.ppf(1.0 - 1e-9)))
    print(f"keyed poisson({lam}): chi-square p = {p:.4f}, {len(cd.blocks)} blocks for {N_DRAWS} draws")
    assert p > 1e-4
    assert len(cd.blocks) == N_DRAWS if lam < 10.0 else N_DRAWS <= len(cd.blocks) <= 64 * N_DRAWS
    assert max(t for _, t in cd.blocks) < C.COUNT_BLOCKS


@pytest.mark.parametrize("case,n,prob", [(i, n, p) for i, (n, p) in enumerate(BINOMIAL_CASES)])
def test_keyed_binomial_draws_follow_the_pmf(O, case, n, prob):
    from scipy import stats
    cd = C.CountDraws(O, SEED + 2, 4000 + case, 5, base=BASE)
    draws = np.array([cd.binomial(i, n, prob) for i in range(N_DRAWS)])
    dist = stats.binom(n, prob)
    p = chi_square_p(draws, dist.pmf, int(dist.ppf(1e-9)), int(dist.ppf(1.0 - 1e-9)))
    print(f"keyed binomial({n}, {prob}): chi-square p = {p:.4f}, {len(cd.blocks)} blocks for {N_DRAWS} draws")
    assert draws.min() >= 0 and draws.max() <= n
    assert p > 1e-4
    assert max(t for _, t in cd.blocks) < C.COUNT_BLOCKS


def test_an_index_owns_its_blocks(O):
    cd = C.CountDraws(O, SEED, 7, 2, base=BASE)
    owned = [{cd.block_of(i, j) for j in range(C.COUNT_BLOCKS)} for i in range(50)]
    assert all(len(s) == C.COUNT_BLOCKS for s in owned) and len(set().union(*owned)) == 50 * C.COUNT_BLOCKS
    assert min(owned[0]) == BASE and max(owned[49]) == BASE + 64 * 50 - 1
    # a draw is a function of (index, parameters): alone, after others, in any order, made twice
    lam = [0.3, 4.0, 9.99, 10.0, 35.0, 900.0] * 5
    forward = [cd.poisson(i, v) for i, v in enumerate(lam)]
    backward = [cd.poisson(i, lam[i]) for i in reversed(range(len(lam)))][::-1]
    alone = [C.CountDraws(O, SEED, 7, 2, base=BASE).poisson(i, v) for i, v in enumerate(lam)]
    assert forward == backward == alone
    assert [cd.binomial(i, 400, 0.3) for i in (5, 2, 5)][::2] == [cd.binomial(5, 400, 0.3)] * 2
    # ... and with the library's log and lgamma it is the sequential draw from a stream positioned at the index's first block
    plain = C.CountDraws(O, SEED, 7, 2, base=BASE, functions=C.FUNCTIONS_MATH)
    for i, v in enumerate(lam):
        assert plain.poisson(i, v) == Stream(O, SEED, 7, 2, k=BASE + 64 * i).poisson(v)
    for i, (n, p) in enumerate([(10, 0.3), (40, 0.5), (1000, 0.02), (1000, 0.4), (10 ** 6, 0.7), (25, 0.9)] * 3):
        assert plain.binomial(i, n, p) == Stream(O, SEED, 7, 2, k=BASE + 64 * i).binomial(n, p)
    # the table functions and the library's give the same counts here (they differ in the last place of a compared value)
    table = [cd.poisson(i, v) for i, v in enumerate(lam)]
    assert table == [plain.poisson(i, v) for i, v in enumerate(lam)]


def test_the_counter_behind_a_reservation(O):
    """After reserve_counts(n) the next uniform_pair() is block base + 64 n, whatever was drawn; n is clamped to [0, 2^20]."""
    for n in (0, 1, 45, 129):
        cd, k = C.reserve_counts(O, SEED, 9, 4, O.PURPOSE_SIM, BASE, n)
        assert (cd.base, k) == (BASE, BASE + 64 * n)
        [cd.poisson(i, 50.0) for i in range(n)]
        rng = Stream(O, SEED, 9, 4, k=k)
        w = O.stream_block(SEED, 9, O.PURPOSE_SIM, 4, BASE + 64 * n)
        assert rng.uniform_pair() == (O.u52(w[0], w[1]), O.u52(w[2], w[3])) and rng.k == k + 1
    assert C.reserve_counts(O, SEED, 9, 4, O.PURPOSE_SIM, 5, -3)[1] == 5
    assert C.reserve_counts(O, SEED, 9, 4, O.PURPOSE_SIM, 5, (1 << 20) + 7)[1] == 5 + 64 * (1 << 20)
    assert C.reserve_counts(O, SEED, 9, 4, O.PURPOSE_SIM, 0xFFFFFFF0, 1)[1] == 0x30          # the counter has 32 bits


def test_degenerate_arguments_compute_no_block(O):
    cd = C.CountDraws(O, SEED, 1, 1, base=BASE)
    nan, inf = float("nan"), float("inf")
    assert [cd.poisson(0, v) for v in (nan, -1.0, 0.0, -0.0, -inf)] == [0] * 5
    assert [cd.binomial(1, n, p) for n, p in ((0, 0.5), (-4, 0.5), (nan, 0.5), (7, 0.0), (7, -0.2), (7, nan))] == [0] * 6
    assert [cd.binomial(2, n, p) for n, p in ((7, 1.0), (7, 1.5), (7.9, inf), (2.0 ** 31, 1.0), (inf, 2.0))] == [7, 7, 7, 2 ** 30, 2 ** 30]
    assert cd.blocks == []
    # lambda above 2^30 is 2^30, n_trials above 2^30 is 2^30: the same draws, blocks and all
    other = C.CountDraws(O, SEED, 1, 1, base=BASE)
    assert cd.poisson(3, 2.0 ** 31) == other.poisson(3, 2.0 ** 30) and cd.poisson(4, inf) == other.poisson(4, 2.0 ** 30)
    assert cd.binomial(5, 2.0 ** 40, 0.25) == other.binomial(5, 2 ** 30, 0.25) and cd.blocks == other.blocks
    assert abs(cd.poisson(3, inf) - 2 ** 30) < 6 * 2 ** 15 and abs(cd.binomial(5, inf, 0.25) - 2 ** 28) < 6 * 2 ** 15      # six sigma
    # every loop keeps its bound: a draw computes at most 64 blocks
    assert max(t for _, t in cd.blocks) < C.COUNT_BLOCKS
    assert not math.isnan(cd.poisson(6, 1e-300)) and cd.poisson(6, 1e-300) == 0


def test_the_ricker_transcription(O):
    """The latent state is the textbook map up to rounding, the counts are keyed by the time step behind the normals' blocks,
    and the summaries of the observed part do not read the burn-in."""
    theta, n_obs, burn_in = (3.8, 0.3, 10.0), 40, 5
    latent, y = C.ricker_simulation(O, SEED, 11, 2, O.PURPOSE_SIM, theta, n_obs, burn_in, 1.0)
    from tests.test_f32_draws import f64_pair
    z = np.array([f64_pair(O.stream_block(SEED, 11, O.PURPOSE_SIM, 2, b)) for b in range(23)]).reshape(-1)[:45]
    np.testing.assert_allclose(z, np.array([O.normal_pair(SEED, 11, O.PURPOSE_SIM, 2, b) for b in range(23)]).reshape(-1)[:45], rtol=1e-9)
    # step by step from the transcription's own state: at log r = 3.8 the map is chaotic, and a trajectory carried along would
    # leave the transcription's by more than any rounding bound after a few steps
    before = np.concatenate([[1.0], latent[:-1]])
    want = [math.exp(3.8) * s * math.exp(-s + 0.3 * v) for s, v in zip(before, z)]
    np.testing.assert_allclose(latent, want, rtol=1e-13)
    cd = C.CountDraws(O, SEED, 11, 2, O.PURPOSE_SIM, base=23)
    assert [cd.poisson(t, 10.0 * latent[t]) for t in range(45)] == list(y)
    assert (y == np.floor(y)).all() and (y >= 0).all() and (y == 0).any() and y.max() > 20
    got = C.ricker_summaries_of_series(y, 2, burn_in)
    np.testing.assert_array_equal(got, C.ricker_summaries(y[burn_in:], 2, burn_in))
    obs = y[burn_in:]
    assert got[0] == obs.sum() / 40.0 and got[1] == (obs == 0).sum()
    d = obs - obs.mean()
    for j in range(3):
        assert abs(got[2 + j] - np.dot(d[j:], d[:40 - j]) / 40.0) <= 1e-12 * np.abs(d).max() ** 2
    # an overflowing latent state: lambda = inf counts as 2^30, a NaN as 0; the distances stay finite
    assert cd.poisson(0, float("inf")) > 2 ** 29 and cd.poisson(0, float("nan")) == 0
    with np.errstate(invalid="ignore"):
        assert np.isfinite(C.ricker_distances(np.full(45, np.inf), np.zeros(5), 2, burn_in)).all()
