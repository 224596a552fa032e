"""Every order statistic of the g-and-k simulator on each of its three sorting networks (csrc/device_models.hpp) against the
NumPy reference of tests/gk_ref.py -- the model's definition on the oracle's normals; tests/test_gk_reference.py shows that
the checker tells a right order statistic from a neighbour, the other slot of a lane, a reversed block, a draw too many.

  network 1  gk_simulate_wave_ranks      k_simulate_gk             h.simulate() (and the prior simulation of initialize())
  network 2  gk_simulate_wave_ranks_x2   k_update_gk<PROP, false>  updates whose wanted ranks are not all multiples of 16
  network 3  gk_simulate_rows4           k_update_gk<PROP, true>   updates whose wanted ranks are all multiples of 16
Which of the two update kernels runs is the host's choice (kernels.hip: launch_update): network 3 if and only if all four
ranks are multiples of 16.  The cases below are labelled by that rule (network_of) and both labels must occur, so a change
of the dispatch cannot silently move all of them onto one network.

(a), (b): h.simulate on 259 parameter vectors (a workgroup of four waves and a wave of 3) of gk_ref.theta_mix -- B < 0, k < 0,
B = 0 (128 ties), k = 5000 (+-inf ties) and B = 0 with k = 5000 (NaN data, which sort last) next to ordinary ones in every
wave --, all 128 ranks at 128 draws and the ranks (1, 2, median, n) at 1 .. 127 draws, particle ids beyond 2^33 included.
(c): one all-accept update (u = 1, a flat prior, eps = 1) of 647 particles: every proposal inside the support is accepted, so
the stored rho of a particle that moved is the simulation AT its new parameters, with the particle's index as id and the
update counter as iteration.  A band of particles sits within one proposal standard deviation of the support's edge, so the
waves have holes: 1, 2, 3 and no particle left over for the last group of four of network 3, an odd one out for network 2 --
asserted to have happened.  With DifferentialEvolution the update is two launches (two half batches, 323 and 324).
(d): c = 0.83 (the normals are sorted and mapped) and c = 0.84 (the data are sorted) where the slope of the quantile function
is smallest.
(e): configurations that are refused (tests/test_gk_reference.py has them without a device).

The bound is gk_ref.RTOL = 1e-10 (atol 1e-12): the project's own for a device simulator against glibc normals.  Worst
deviation |got - want| / (|want| + 0.01) measured on an MI355X, over the (particle, rank) values compared:
  network 1   7.2e-12   over 116 032   (the k = 5000 particles, where a last-digit difference of z is multiplied by
                                        k 2 z / (1 + z^2); 1.5e-15 at k = 0, test (d))
  network 2   1.5e-13   over 106 048   (all 128 ranks and the ten other cases of UPDATE_CASES)
  network 3   9.4e-14   over  30 032   (every multiple of 16)
The two branches either side of c = 0.83 agree with the reference to 1.5e-15 (simulate) and 3.8e-14 (update).
A handle costs 0.3 ms to create and close, the whole module 3 s: most of it the reference's normals (64 oracle calls per
particle, cached per (seed, ids, iteration)).

What the module found: (1 + z^2)^k stopped at e^700 (the clamp of exp_tab), so from k log(1 + z^2) = 700 on a datum was a
finite 1e304 where the model's is +-inf -- a distance of 1e304 instead of 1e30; gk_quantile now overflows as the definition
does, and the NaN that B = 0 makes of it enters the networks as +inf (gk_datum).  No order statistic was wrong on any network."""
import time

import numpy as np
import pytest

from tests import gk_ref as G

pytestmark = pytest.mark.gpu

SEED = 11
M = 259                                        # 4 waves of 64 particles + a wave of 3
PIDS = [(17, 5), (2 ** 34 + 77, 9)]            # (first particle id, iteration)
OBS = (1.9, 2.7, 3.6, 6.4)
N_UPD = 647                                    # 10 waves + 7; half batches of 323 and 324: both end in a partial wave
NO_RESAMPLE = 1e15


def network_of(ranks):
    """the dispatch rule of launch_update, from the rank set alone"""
    return 3 if all(int(r) % 16 == 0 for r in ranks) else 2


def note(network, n_values, worst):
    print(f"[gk] network {network}: {n_values} values, worst deviation {worst:.3g}")


def sim_handle(S, n_draws, c, ranks, obs=(0.0, 0.0, 0.0, 0.0)):
    # (the simulate operator does not look at the prior gate: parameters outside the support are fine)
    return S.SabcHandle(n_particles=256, model=S.GandK(n_draws=n_draws, c=c, ranks=ranks, obs=obs),
                        prior=S.product_distribution([S.Uniform(0, 10)] * 4), seed=SEED)


def simulate_groups(S, theta, n_draws, c, groups, pid0, it, obs=(0.0, 0.0, 0.0, 0.0)):
    """h.simulate with one handle per group of four ranks; [4 len(groups)][m]"""
    rows, t_handle = [], 0.0
    for ranks in groups:
        t0 = time.perf_counter()
        h = sim_handle(S, n_draws, c, ranks, obs)
        t_handle += time.perf_counter() - t0
        try:
            rows.append(h.simulate(theta, pid0, it))
        finally:
            t0 = time.perf_counter()
            h.close()
            t_handle += time.perf_counter() - t0
    print(f"[gk] a handle: {1e3 * t_handle / len(groups):.2f} ms to create and close")
    return np.concatenate(rows)


def check_monotone(got, x, first_rank, where):
    """rho = |x_(r) - 0| is non-decreasing in r wherever the particle's data are finite and not below obs = 0"""
    ok = np.all(np.isfinite(x), axis=0) & (x[0] >= 0.0)
    assert ok.sum() >= got.shape[1] // 5, (where, int(ok.sum()))
    bad = np.argwhere(np.diff(got[:, ok], axis=0) < 0)
    assert len(bad) == 0, (where, [(int(np.flatnonzero(ok)[i]), first_rank + int(r)) for r, i in bad[:8]])


# ---- (a) network 1, every rank ----
@pytest.mark.parametrize("pid0,it", PIDS, ids=["pid17", "pid2^34"])
@pytest.mark.parametrize("part", range(4))
def test_network1_every_rank(S, gpu, part, pid0, it):
    """c = 0.8: the normals are sorted and the wanted ranks mapped for B > 0, k >= 0; the data are sorted for the rest of the
    wave.  Ranks 32 part + 1 .. 32 part + 32 as eight handles (a handle holds four ranks)."""
    theta = G.theta_mix(M)
    ranks = np.arange(32 * part + 1, 32 * part + 33)
    got = simulate_groups(S, theta, 128, 0.8, ranks.reshape(8, 4).tolist(), pid0, it)
    z = G.normals(SEED, pid0, M, it)
    x = G.all_ranks(theta, 128, 0.8, z)
    want = G.distance(x, 0.0)[ranks - 1]
    worst = G.assert_rho(got, want, f"network 1, ranks {ranks[0]}..{ranks[-1]}, pid0 {pid0}", sorted_data=x, ranks=ranks, obs=0.0)
    check_monotone(got, x, int(ranks[0]), "network 1")
    assert np.all(got[:, 3::8] == theta[0, 3::8])                      # B = 0: 128 ties, every order statistic is A
    if part == 3:                                                       # the +inf and the NaN data are at the top
        assert np.all(got[-1, 4::8] == G.BIG) and np.all(got[-1, 7::8] == G.BIG)
    note(1, got.size, worst)


@pytest.mark.parametrize("pid0,it", PIDS, ids=["pid17", "pid2^34"])
def test_network1_sorting_the_data_of_every_particle(S, gpu, pid0, it):
    """c = 0.9: above 0.83 the data are sorted for every particle"""
    theta = G.theta_mix(M)
    groups = [(1, 2, 3, 4), (13, 14, 15, 16), (17, 18, 19, 20), (61, 62, 63, 64), (65, 66, 67, 68), (97, 98, 99, 100),
              (111, 112, 113, 114), (125, 126, 127, 128)]
    ranks = np.array(groups).ravel()
    got = simulate_groups(S, theta, 128, 0.9, groups, pid0, it)
    x = G.all_ranks(theta, 128, 0.9, G.normals(SEED, pid0, M, it))
    worst = G.assert_rho(got, G.distance(x, 0.0)[ranks - 1], f"network 1, c = 0.9, pid0 {pid0}", sorted_data=x, ranks=ranks, obs=0.0)
    check_monotone(got, x, 0, "network 1, c = 0.9")
    note(1, got.size, worst)


# ---- (b) network 1, draw counts ----
def ranks_for(n):
    return (1, min(2, n), (n + 1) // 2, n)


@pytest.mark.parametrize("n_draws", [1, 2, 3, 15, 16, 17, 63, 64, 65, 99, 127])
def test_network1_draw_counts(S, gpu, n_draws):
    """fewer than 128 draws: the rest of the 128 is +inf; an odd count leaves a lane with one draw and one +inf"""
    theta = G.theta_mix(M)
    ranks, (pid0, it) = ranks_for(n_draws), PIDS[n_draws % 2]
    z = G.normals(SEED, pid0, M, it)
    worst = 0.0
    for c in (0.8, 0.9):
        got = simulate_groups(S, theta, n_draws, c, [ranks], pid0, it, OBS)
        want = G.expected(theta, n_draws, c, ranks, OBS, z)
        worst = max(worst, G.assert_rho(got, want, f"network 1, {n_draws} draws, c = {c}", sorted_data=G.all_ranks(theta, n_draws, c, z),
                                        ranks=ranks, obs=OBS))
    note(1, 2 * got.size, worst)


# ---- (c) networks 2 and 3 through one all-accept update ----
BAND = (0, 3, 4, 5, 6, 3, 4, 5, 6, 3, 2)      # particles of the band in wave 0, 1, ..: none in the first


def support(S):
    """flat, and wide enough in B and k for the data branch to lie inside it"""
    return S.product_distribution([S.Uniform(0, 10), S.Uniform(-10, 10), S.Uniform(0, 10), S.Uniform(-10, 10)])


def theta0_with_band(n=N_UPD, seed=3):
    """A tight bulk (A near 5, more than five proposal standard deviations -- RandomWalk: 0.8 cov of the population, read back
    from h.proposal_sigma -- inside the support in every coordinate) with B < 0 and k < 0 particles in every wave, and a band
    of BAND[w] particles per wave with A in (0, 0.8): within one standard deviation (~0.9) of the support's edge at 0."""
    rng = np.random.default_rng(seed)
    th = np.stack([rng.uniform(4.9, 5.1, n), rng.uniform(1.0, 2.0, n), rng.uniform(4.0, 6.0, n), rng.uniform(0.2, 0.8, n)])
    i = np.arange(n)
    th[1, i % 8 == 1] = rng.uniform(-0.6, -0.3, int(np.sum(i % 8 == 1)))
    th[3, i % 8 == 2] = rng.uniform(-0.5, -0.2, int(np.sum(i % 8 == 2)))
    band = np.zeros(n, dtype=bool)
    for w, b in enumerate(BAND):
        lo, hi = 64 * w, min(64 * w + 64, n)
        band[rng.choice(np.arange(lo, hi), b, replace=False)] = True
    th[0, band] = rng.uniform(0.0, 0.8, int(band.sum()))
    return th, band


def theta0_flat_slope(n=N_UPD, seed=4):
    """(d): B > 0 and k within 1e-3 of 0.0025 -- the proposals stay at k ~ 0+, where the slope of Q has nothing to add to
    1 + c (tanh w + w sech^2 w); g in (1, 8) puts the minimum of the slope, at g z / 2 = -1.2, inside the sample"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(3, 7, n), rng.uniform(1, 3, n), rng.uniform(1, 8, n), 2e-3 + rng.uniform(0, 1e-3, n)])


def waves_of(n, proposal):
    """particle ranges a wave of k_update_gk takes: 64 at a time from the start of each launch"""
    launches = [(0, n)] if proposal == "rw" else [(0, n // 2), (n // 2, n)]
    return [(lo, min(lo + 64, hi)) for a, hi in launches for lo in range(a, hi, 64)]


def all_accept_update(S, n_draws, c, ranks, theta0, proposal="rw", expect_holes=True):
    """-> (number of values compared, worst deviation)"""
    n = theta0.shape[1]
    net = network_of(ranks)
    h = S.SabcHandle(n_particles=n, model=S.GandK(n_draws=n_draws, c=c, ranks=ranks, obs=OBS), prior=support(S), seed=SEED)
    try:
        h.initialize(n)
        h.set_population(theta=theta0, u=np.ones((4, n)), rho=np.full((4, n), 1e3))
        h.set_eps(np.ones(len(h.eps)))
        c0 = h.counters["n_accept"]
        prop = S.RandomWalk(n_para=4) if proposal == "rw" else S.DifferentialEvolution(n_para=4)
        h.update(n_simulation=n, proposal=prop, resample=NO_RESAMPLE)
        th1, _, rho = h.get_population()
        it = h.counters["n_population_updates"]          # engine.cpp: c.iter = n_population_updates_ + ix, ix = 1 here
        accepted = h.counters["n_accept"] - c0
        sigma = h.proposal_sigma
    finally:
        h.close()
    assert it == 1
    moved = np.any(th1 != theta0, axis=0)
    assert accepted == moved.sum() > n // 2, (accepted, int(moved.sum()))
    # a particle that did not move was stopped at the prior gate: it was not simulated, its rho is what was set
    assert np.all(rho[:, ~moved] == 1e3)
    inside = np.all((th1 >= np.array([0, -10, 0, -10])[:, None]) & (th1 <= 10), axis=0)
    assert np.all(inside)
    z = G.normals(SEED, 0, n, it)
    th, zz = th1[:, moved], z[:, moved]
    where = f"network {net}, {n_draws} draws, ranks {tuple(ranks)}, c = {c}, {proposal}"
    worst = G.assert_rho(rho[:, moved], G.expected(th, n_draws, c, ranks, OBS, zz), where,
                         sorted_data=G.all_ranks(th, n_draws, c, zz), ranks=ranks, obs=OBS)
    if expect_holes and proposal == "rw":
        # what the wave's loop over `todo` met: particles left for the last group of four (network 3) / pair (network 2)
        counts = [int(moved[lo:hi].sum()) for lo, hi in waves_of(n, proposal)]
        full = [hi - lo == cnt for (lo, hi), cnt in zip(waves_of(n, proposal), counts)]
        assert {cnt % 4 for cnt in counts} == {0, 1, 2, 3} and {cnt % 2 for cnt in counts} == {0, 1}, counts
        assert any(full) and not all(full), counts
        assert len(counts) == 11 and counts[-1] <= 7
        # the band is where the issue wants it: within one proposal standard deviation of the edge
        assert 0.5 < np.sqrt(sigma[0, 0]) < 2.0, sigma
        # both branches inside every full wave: the data are sorted for B <= 0 or k < 0 (or c > 0.83)
        for lo, hi in waves_of(n, proposal)[:-1]:
            mv = moved[lo:hi]
            data = (th1[1, lo:hi] <= 0) | (th1[3, lo:hi] < 0)
            assert np.sum(mv & data) >= 4 and np.sum(mv & ~data) >= 4 and np.sum(mv & (th1[1, lo:hi] < 0)) >= 1 \
                and np.sum(mv & (th1[3, lo:hi] < 0)) >= 1, (lo, hi)
    note(net, int(rho[:, moved].size), worst)
    return int(rho[:, moved].size), worst


@pytest.mark.parametrize("part", range(4))
def test_network2_every_rank(S, gpu, part):
    """all 128 ranks at 128 draws, 32 part + 1 .. 32 part + 32 as eight updates (a handle holds four ranks); each group has
    at least three ranks that are no multiple of 16"""
    theta0, _ = theta0_with_band()
    for ranks in np.arange(32 * part + 1, 32 * part + 33).reshape(8, 4).tolist():
        assert network_of(ranks) == 2
        all_accept_update(S, 128, 0.8, ranks, theta0)


UPDATE_CASES = [
    # (network, n_draws, c, ranks, proposal)
    (2, 128, 0.8, (16, 48, 80, 113), "rw"),            # one rank off the multiples of 16: the nearest miss of the dispatch
    (2, 128, 0.9, (16, 48, 80, 113), "rw"),            # the data sorted for every particle
    (2, 128, 0.8, (16, 48, 80, 113), "de"),            # two launches: the second starts at particle 323
    (2, 128, 0.8, (100, 100, 100, 100), "rw"),         # a rank repeated
    (2, 128, 0.9, (1, 64, 65, 128), "de"),
    (2, 1, 0.8, ranks_for(1), "rw"),
    (2, 2, 0.8, ranks_for(2), "rw"),
    (2, 17, 0.8, ranks_for(17), "rw"),
    (2, 99, 0.8, ranks_for(99), "rw"),
    (2, 127, 0.8, ranks_for(127), "rw"),
    (3, 128, 0.8, (16, 32, 48, 64), "rw"),
    (3, 128, 0.8, (80, 96, 112, 128), "rw"),           # rank 128: the last pair of lanes of the row
    (3, 128, 0.9, (80, 96, 112, 128), "rw"),
    (3, 128, 0.8, (128, 16, 128, 16), "rw"),
    (3, 128, 0.8, (16, 32, 48, 64), "de"),
    (3, 128, 0.9, (16, 48, 80, 112), "de"),
    (3, 16, 0.8, (16, 16, 16, 16), "rw"),              # one block of draws: its maximum is the sample's
    (3, 17, 0.8, (16, 16, 16, 16), "rw"),              # one draw in the second block
    (3, 100, 0.8, (16, 32, 64, 96), "rw"),
    (3, 127, 0.8, (16, 48, 80, 112), "rw"),
]


@pytest.mark.parametrize("net,n_draws,c,ranks,proposal", UPDATE_CASES,
                         ids=[f"net{k[0]}-n{k[1]}-c{k[2]}-{'_'.join(map(str, k[3]))}-{k[4]}" for k in UPDATE_CASES])
def test_update_networks(S, gpu, net, n_draws, c, ranks, proposal):
    assert network_of(ranks) == net                     # the case is labelled by the dispatch rule, not by hope
    theta0, _ = theta0_with_band()
    all_accept_update(S, n_draws, c, ranks, theta0, proposal)


def test_update_cases_reach_both_networks():
    nets = [network_of(k[3]) for k in UPDATE_CASES]
    assert nets.count(2) >= 8 and nets.count(3) >= 8
    assert network_of((16, 48, 80, 113)) == 2 and network_of((128, 16, 128, 16)) == 3 and network_of((1, 2, 3, 4)) == 2


# ---- (d) the two branches either side of 0.83 ----
@pytest.mark.parametrize("c", [0.83, 0.84])
def test_the_two_branches_either_side_of_083(S, gpu, c):
    """At c = 0.83 the normals are sorted and Q is applied to the four wanted ones; at 0.84 Q is applied to all and the data
    are sorted.  The parameters are where the two could differ most: k = 0 and g z / 2 = -1.2 inside the sample (g = 1, 2, 4,
    8: z = -2.4, -1.2, -0.6, -0.3), where tanh w + w sech^2 w is at its minimum of -1.19968 and the slope of Q is
    B (1 - 1.19968 c): 0.0043 B at 0.83 -- two normals 1e-7 apart map to data 4e-10 B apart, far above their rounding --, and
    negative at 0.84.  device_models.hpp says of the first branch that rounding can order two normals differently from their
    images and that 'the order statistic then differs in its last digits only': if that did not hold, the bound of assert_rho
    would be exceeded here first."""
    rng = np.random.default_rng(8)
    theta = np.stack([rng.uniform(2, 8, M), rng.uniform(0.5, 3, M), np.resize([1.0, 2.0, 4.0, 8.0], M), np.zeros(M)])
    groups = [(1, 2, 3, 4), (16, 48, 80, 112), (29, 30, 31, 32), (61, 62, 63, 64), (125, 126, 127, 128)]
    ranks = np.array(groups).ravel()
    pid0, it = PIDS[0]
    got = simulate_groups(S, theta, 128, c, groups, pid0, it)
    x = G.all_ranks(theta, 128, c, G.normals(SEED, pid0, M, it))
    worst = G.assert_rho(got, G.distance(x, 0.0)[ranks - 1], f"network 1, c = {c}", sorted_data=x, ranks=ranks, obs=0.0)
    note(1, got.size, worst)
    if c == 0.84:                                       # the quantile function does turn there: sorting the data matters
        mapped = G.quantile(theta, c, np.sort(G.normals(SEED, pid0, M, it), axis=0))
        assert np.any(np.diff(mapped, axis=0) < 0)
    all_accept_update(S, 128, c, (16, 48, 80, 112), theta0_flat_slope(), expect_holes=False)


# ---- (e) refused configurations ----
@pytest.mark.parametrize("what,kw", G.REFUSED, ids=[r[0] for r in G.REFUSED])
def test_refused_configurations_on_the_device(S, gpu, what, kw):
    """With a device present too: SABC_ERR_BAD_CONFIG from Engine::validate(), which runs before the handle allocates or
    launches anything (capi.hip: sabc_create) -- and the next handle works."""
    G.check_refused(S, what, kw)
    h = sim_handle(S, 128, 0.8, (1, 2, 127, 128))
    try:
        theta = G.theta_mix(8)
        got = h.simulate(theta, 17, 5)
        G.assert_rho(got, G.expected(theta, 128, 0.8, (1, 2, 127, 128), (0.0,) * 4, G.normals(SEED, 17, 8, 5)), what)
    finally:
        h.close()
