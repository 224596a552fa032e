"""The g-and-k reference of tests/gk_ref.py: it is the model of tests/independent/models_numpy.py::cfg4, its checker tells a
right order statistic from each kind of wrong one a sorting network can produce, the constant behind the device's
gk_increasing (csrc/device_models.hpp) holds, and the configurations that would send a lane index out of the wave are
refused before any device is looked for.  CPU only: the device side is tests/test_gpu_gk_order_statistics.py."""
import numpy as np
import pytest

from tests import gk_ref as G
from tests.independent import models_numpy as M

SEED, PID0, IT, N_PART = 11, 1000, 3, 48
C = 0.8
OBS = (1.9, 2.7, 3.6, 6.4)


def ordinary_theta(m, seed=2):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(2, 8, m), rng.uniform(0.5, 3, m), rng.uniform(0.5, 4, m), rng.uniform(0.0, 1.0, m)])


@pytest.fixture(scope="module")
def Z(O):
    return G.normals(SEED, PID0, N_PART, IT)


def test_normals_are_the_oracles_simulation_stream(O, Z):
    assert Z.shape == (128, N_PART) and not Z.flags.writeable
    for i, b in ((0, 0), (7, 31), (N_PART - 1, 63)):
        np.testing.assert_array_equal(Z[2 * b: 2 * b + 2, i], O.normal_pair(SEED, PID0 + i, O.PURPOSE_SIM, IT, b))
    assert G.normals(SEED, PID0, N_PART, IT) is Z                                   # cached
    z = Z.ravel()
    assert abs(z.mean()) < 4 / np.sqrt(z.size) and abs(z.var() - 1) < 0.1


class _Replay:
    """stands in for the Generator cfg4's sim draws from: hands it the reference's normals"""
    def __init__(self, z):
        self.z = z

    def standard_normal(self, shape):
        m, n = shape
        return self.z[:n, :m].T.copy()


@pytest.mark.parametrize("n_draws,ranks", [(128, None), (100, (10, 40, 60, 95)), (17, (1, 2, 9, 17))])
def test_reference_is_the_independent_model(Z, n_draws, ranks):
    """The same formula and the same 1-based ranks as models_numpy.cfg4 (at its default ranks, and two more sets);
    (1 + z^2)^k is a power there and exp(k log1p(z^2)) here: the last digits."""
    kw = {} if ranks is None else dict(ranks=ranks)
    model = M.cfg4(n_draws=n_draws, c=C, obs=OBS, **kw)
    ranks = (16, 48, 80, 112) if ranks is None else ranks
    th = ordinary_theta(N_PART)
    th[1, 5], th[3, 9], th[3, 13] = -1.5, -0.3, 5000.0                              # the data branch and 1e30 too
    want = model["sim"](th.T.copy(), _Replay(Z)).T
    got = G.expected(th, n_draws, C, ranks, OBS, Z)
    assert np.any(want == G.BIG) and np.any(want[:, 13] == G.BIG)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    x = G.all_ranks(th, n_draws, C, Z)
    assert x.shape == (n_draws, N_PART) and np.all(np.diff(x[:, :5], axis=0) >= 0)
    np.testing.assert_array_equal(G.distance(x[np.array(ranks) - 1], np.array(OBS)[:, None]), got)


def test_nan_data_sort_last():
    """B = 0 with an overflowed (1 + z^2)^k is 0 inf = NaN: those draws sort behind the finite ones (all equal to A)."""
    z = np.array([0.1, 2.0, -0.2, -3.0, 0.3])[:, None]
    th = np.array([[4.0], [0.0], [1.0], [5000.0]])
    x = G.all_ranks(th, 5, C, z)
    assert np.array_equal(x[:3, 0], [4.0, 4.0, 4.0]) and np.all(np.isnan(x[3:, 0]))
    np.testing.assert_array_equal(G.expected(th, 5, C, (1, 3, 4, 5), (1.0, 1.0, 1.0, 1.0), z)[:, 0], [3.0, 3.0, G.BIG, G.BIG])


# ---- the checker catches what it is for ----
RANKS_ALL = np.arange(1, 129)


@pytest.fixture(scope="module")
def ref(Z):
    th = ordinary_theta(N_PART)
    th[1, 3::8] *= -1.0                                                             # B < 0 for particles 3, 11, ...
    x = G.all_ranks(th, 128, C, Z)
    return th, x, G.distance(x, 0.0)


def fails(got, want, **kw):
    with pytest.raises(AssertionError) as e:
        G.assert_rho(got, want, "mutation", **kw)
    return str(e.value)


def test_checker_passes_the_reference_and_a_last_digit(ref):
    th, x, want = ref
    assert G.assert_rho(want, want, "identity") == 0.0
    worst = G.assert_rho(want * (1 + 3e-11), want, "3e-11")
    assert 1e-11 < worst <= G.RTOL
    fails(want * (1 + 3e-10), want)
    got = want.copy()
    got[5, 7] = np.nan
    fails(got, want)


def test_checker_catches_two_neighbours_swapped(ref):
    th, x, want = ref
    for r, i in ((1, 0), (64, 17), (127, N_PART - 1)):
        got = want.copy()
        got[r - 1, i], got[r, i] = want[r, i], want[r - 1, i]
        msg = fails(got, want, sorted_data=x, ranks=RANKS_ALL, obs=0.0)
        assert f"particle {i}, row {r - 1}" in msg and f"the distance of rank [{r + 1}]" in msg and "neighbour" in msg


def test_checker_catches_a_rank_off_by_one(ref, Z):
    th, x, want_all = ref
    for ranks in ((16, 48, 80, 112), (1, 2, 3, 4), (124, 125, 126, 127)):
        want = G.expected(th, 128, C, ranks, OBS, Z)
        msg = fails(G.expected(th, 128, C, tuple(r + 1 for r in ranks), OBS, Z), want, sorted_data=x, ranks=ranks, obs=OBS)
        assert "a neighbour" in msg and "garbage" not in msg
        fails(G.expected(th, 128, C, tuple(max(r - 1, 1) for r in ranks[:3]) + (ranks[3] - 1,), OBS, Z), want)


def test_checker_catches_n_draws_off_by_one(ref, Z):
    th, x, want_all = ref
    for n, ranks in ((128, (16, 48, 80, 112)), (100, (10, 40, 60, 95)), (17, (1, 2, 9, 16))):
        want = G.expected(th, n, C, ranks, OBS, Z)
        fails(G.expected(th, n - 1, C, ranks, OBS, Z), want)
        fails(G.expected(th, n + 1, C, ranks, OBS, Z) if n < 128 else G.expected(th, n - 2, C, ranks, OBS, Z), want)


def test_checker_catches_the_other_slot_of_the_lane(ref, Z):
    """rank r read as ((r - 1) ^ 1) + 1: the v0 / v1 halves of a lane exchanged"""
    th, x, want_all = ref
    for ranks in ((16, 48, 80, 112), (1, 33, 65, 127)):
        want = G.expected(th, 128, C, ranks, OBS, Z)
        fails(G.expected(th, 128, C, tuple(((r - 1) ^ 1) + 1 for r in ranks), OBS, Z), want)


def test_checker_catches_a_descending_block_of_16(ref):
    th, x, want = ref
    for b in (0, 3, 7):
        got = want.copy()
        got[16 * b: 16 * b + 16] = want[16 * b: 16 * b + 16][::-1]
        msg = fails(got, want, sorted_data=x, ranks=RANKS_ALL, obs=0.0)
        assert f"the distance of rank [{16 * b + 16}]" in msg                       # row 16 b holds rank 16 b + 16's
    # ... also where only the block's end is looked at (ranks that are multiples of 16)
    ends = np.arange(16, 129, 16)
    got = want[ends - 1].copy()
    got[2] = want[32]                                                               # rank 48 <- the block's first, rank 33
    fails(got, want[ends - 1])


def test_checker_catches_the_normals_branch_for_negative_b(ref, Z):
    """Q(sort(z)) instead of sort(Q(z)) for a particle whose quantile function decreases: the ranks come out mirrored"""
    th, x, want = ref
    mapped = G.distance(G.quantile(th, C, np.sort(Z, axis=0)), 0.0)
    neg = th[1] < 0
    assert neg.sum() >= 5
    np.testing.assert_allclose(mapped[:, ~neg], want[:, ~neg], rtol=1e-13)          # increasing: the same numbers
    for i in np.flatnonzero(neg)[:3]:
        got = want.copy()
        got[:, i] = mapped[:, i]
        msg = fails(got, want, sorted_data=x, ranks=RANKS_ALL, obs=0.0)
        assert f"particle {i}, row 0" in msg and "the distance of rank [128]" in msg


def test_theta_mix_puts_every_class_into_every_wave():
    th = G.theta_mix(259)
    cls = np.arange(259) % 8
    for w in range(4):
        s = slice(64 * w, 64 * w + 64)
        assert np.sum(th[1, s] < 0) == 16 and np.sum(th[1, s] == 0) == 16 and np.sum(th[3, s] < 0) == 8
        assert np.sum(th[3, s] == 5000.0) == 24
    assert np.all(th[1, cls == 0] > 0) and np.all(th[3, cls == 0] >= 0)
    # the classes do what they are for: ties, +-inf, NaN
    z = G.normals(SEED, PID0, N_PART, IT)
    x = G.all_ranks(th[:, :N_PART], 128, C, z)
    assert np.all(x[:, 3] == th[0, 3]) and np.isinf(x[0, 4]) and np.isinf(x[-1, 4]) and np.mean(np.isinf(x[:, 4])) > 0.5
    assert np.isinf(x[0, 6]) and np.isnan(x[-1, 7]) and x[0, 7] == th[0, 7] and not np.any(np.isnan(x[:, :7]))


# ---- the constant behind gk_increasing ----
def f_peak(a):
    return np.tanh(a) + a / np.cosh(a) ** 2


def test_the_constant_of_gk_increasing():
    """sup (tanh a + a sech^2 a) < 1 / 0.83, in float64 on a grid of 1e-4 over [-40, 40] (the function is flat at its
    peak: a grid point within 5e-5 of it is within 2e-9 of the supremum), and at the stationary point a tanh a = 1,
    where the function equals a itself.  The header of gk_increasing says 1.1997: printed for comparison."""
    a = np.linspace(-40.0, 40.0, 800_001)
    f = f_peak(a)
    sup = float(f.max())
    lo, hi = 1.0, 1.5                                                               # a tanh a = 1 by bisection
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if mid * np.tanh(mid) < 1.0 else (lo, mid)
    print(f"max over the grid of tanh a + a sech^2 a = {sup:.12f} at a = {a[f.argmax()]:.4f}; root of a tanh a = 1: {lo:.12f}; "
          f"1 / 0.83 = {1 / 0.83:.12f}")
    assert abs(sup - lo) < 1e-8 and abs(float(f.min()) + lo) < 1e-8                 # odd function: the minimum mirrors it
    assert sup < 1.1997 < 1.0 / 0.83                                                # the header's figure is an upper bound
    assert 1.0 - 0.83 * sup > 4e-3                                                  # what is left of the slope at c = 0.83
    assert 1.0 - 0.8335 * sup > 0 and 1.0 - 0.8336 * sup < 0                        # (the true threshold is 1 / sup = 0.83356)


def test_the_quantile_function_is_increasing_at_c_083():
    """The bracket of dQ/dz, (1 + c t)(1 + 2 k z^2 / (1 + z^2)) + c w sech^2 w with w = g z / 2, t = tanh w, is positive on a
    grid of (g, k >= 0, z) at c = 0.83 -- and Q itself increases along z there (float64)."""
    c = 0.83
    g = np.concatenate([np.linspace(-20, 20, 81), [1e-3, 100.0, -100.0]])[:, None, None]
    k = np.concatenate([np.linspace(0, 3, 13), [10.0, 50.0]])[None, :, None]
    z = np.linspace(-8.6, 8.6, 1721)[None, None, :]
    w = g * z / 2
    sech2 = 1.0 / np.cosh(np.minimum(np.abs(w), 300.0)) ** 2                        # (cosh(300)^2 is finite, its inverse 0)
    bracket = (1 + c * np.tanh(w)) * (1 + 2 * k * z * z / (1 + z * z)) + c * w * sech2
    print(f"min of the bracket at c = 0.83: {bracket.min():.6f} (1 - 0.83 sup = {1 - 0.83 * 1.19967864:.6f})")
    assert bracket.min() > 4e-3
    q = (1 + c * np.tanh(w)) * np.exp(k * np.log1p(z * z)) * z
    assert np.all(np.diff(q, axis=2) > 0)
    # ... and not at c = 0.84: the bracket dips below zero near w = -1.2, k = 0 -- the device sorts the data there
    c = 0.84
    assert ((1 + c * np.tanh(w)) * (1 + 2 * k * z * z / (1 + z * z)) + c * w * sech2).min() < 0


# ---- refused configurations: Engine::validate() comes before the device is looked for, so nothing can have been launched ----
@pytest.mark.parametrize("what,kw", G.REFUSED, ids=[r[0] for r in G.REFUSED])
def test_out_of_range_and_fractional_ranks_are_refused(S, what, kw):
    """A rank outside 1..n_draws would index a lane outside the wave (v_readlane of lane 64 or -1); a fractional rank or
    draw count is refused rather than truncated -- the host's choice of network and the kernels' (int) casts then
    always see the same integers.  Without a device the refusal is the configuration's (-8), not the missing GPU's (-20)."""
    G.check_refused(S, what, kw)


def test_the_largest_and_smallest_configurations_pass_validation(S):
    """n_draws = 1 with rank 1 and n_draws = 128 with rank 128 are valid: the only error left is the missing device"""
    for kw in (dict(n_draws=1, ranks=(1, 1, 1, 1)), dict(n_draws=128, ranks=(1, 127, 128, 128)), dict(n_draws=128.0, ranks=(16.0, 48, 80, 112))):
        try:
            h = S.SabcHandle(n_particles=64, model=G.raw_gk(S, **kw), prior=S.product_distribution([S.Uniform(0, 10)] * 4))
            h.close()
        except S.SABCError as e:
            assert e.code == -20, str(e)
