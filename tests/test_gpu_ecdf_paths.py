"""u = F(rho) on every update path, and the sums the control step reduces, against the NumPy reference of tests/ecdf_ref.py --
recomputed from the state the handle returns, no oracle run.

Each case sets its own ECDF tables (sabc_set_cdf_knots) in one of three index regimes of build_coarse: "lds" (shift 0: the
table is the coarse level), "block" (shift 1-4: a block search in the table) and "mid" (shift >= 5: through the mid level).
The tables are made of values on a grid of 1/64, and the simulator's even statistics are floor(r * 64) / 64 (zeros
included), so the distances land ON runs of equal knots, where a rank off by one or a last-duplicate convention moves u by
a whole step (tests/test_ecdf_reference.py shows the checkers catch both).  The odd statistics stay continuous.

Per table set: (1) the tables read back bit for bit; (2) cdf_apply on every knot, its neighbours, 0, +inf, midpoints;
(3) a population with u = 1 in a flat prior: one update must accept every proposal -- a NaN u would be a silent rejection;
(4) K more updates, then every particle's u is the plain search of its rho within 2 ulp, exactly 0 / 1 on the flat parts,
and the ties really happened; (5) the last history row's means, epsilon, the RandomWalk covariance and the acceptance
count against the returned population.

The cases (path: lookup, reduction as dispatched at these sizes -- kernels.hip launch_reduce_control, kFuseReduceMaxDoubles):
  chain (SABC_PERSISTENT=0), k_update: cdf_apply_3level
    (1,1)  n = 40 001   lds, block, mid          fused k_reduce_control, a wave per column, 256 threads
    (1,1)  n = 400 003  mid                      fused, a wave per column, 1024 threads
    (3,3)  n = 40 001   mixed shifts, all mid    k_reduce_partials then k_reduce_control (SABC_FUSE_REDUCE_MAX=0)
    (3,3)  n = 130      lds                      fused, one partial row
    (5,12) n = 40 001   mixed shifts             fused, tree over 45 columns, 256 threads
  one launch, k_update_persistent: cdf_apply_lds (s = 1, shift 0), cdf_apply_3level_lockstep (s >= 2), the row exchange
    (1,1)  n = 40 001, 1 lane    lds, block, mid
    (1,1)  n = 16 001, 4 lanes   lds, block      (a 4-lane team takes <= 16 384 particles: no table beyond 16 016 knots)
    (1,1)  n = 2 001, 16 lanes   lds, block      (<= 2 048 particles)
    (3,3)  n = 40 001            all lds (the LDS branch), uniform shift 1 ("block="), uniform shift 5 (mid), shifts 1/2/3 and
                                 0/2/5 (same == false)
    (5,12) n = 40 001            mixed shifts
  wide, k_update_wide (3,48) n = 40 001: cdf_apply_3level, coarse level from memory, mixed shifts; two launches, 1024 threads
    (no one-launch form exists for s > 16: persistent_fits)
  host mode, k_host_accept (2,2) n = 40 001: cdf_apply_mid; batched NumPy f_dist with zeros; k_stats_rt
  g-and-k, k_update_gk (4,4) n = 40 001: cdf_apply_mid_lockstep, duplicate-heavy tables, its own continuous rho
    (no one-launch form: persistent_workgroups takes only the Gaussian and Lotka-Volterra built-ins)
plus the population centred at 1e6 with spread 1e-2 (the pivot of the moment sums) at d = 3 and d = 5."""
import numpy as np
import pytest

from tests import ecdf_ref as E

pytestmark = pytest.mark.gpu

Q = 64.0              # the grid of the discrete statistics
BETA = 0.8            # RandomWalk's scale of the population covariance
K = 3                 # updates after the all-accept one
NO_RESAMPLE = 1e15    # simulations between resamplings: never (a resampling permutes theta and u, not rho: :197, :380)

# statistic j from parameters j % d and (j + 1) % d; the even statistics on the grid of 1/p[4]
GRID_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const int d = (int)p[0], s = (int)p[1];
  for (int j = 0; j < s; ++j) {
    const double z = rng.next();
    const double r = fabs(theta[j % d] + 0.5 * theta[(j + 1) % d] + p[2] * z - p[3] - 0.3 * ((j % 5) - 2));
    rho[j] = (j & 1) ? r : floor(r * p[4]) / p[4];
  }
}
"""


def source_model(S, d, s, center):
    return S.DeviceSource(GRID_SRC, d, s, [d, s, 0.4, 1.5 * center, Q])


def flat_prior(S, d, center, half):
    u = S.Uniform(center - half, center + half)
    return u if d == 1 else S.product_distribution([S.Uniform(center - half, center + half) for _ in range(d)])


def host_fdist(theta):
    th = np.atleast_2d(theta)
    z = np.random.default_rng(int(th[0, 0] * 1e6) & 0xFFFF).normal(size=(len(th), 2))
    r0 = np.floor(np.abs(th[:, 0] + 0.5 * th[:, 1] + 0.4 * z[:, 0] - 0.3) * Q) / Q
    r1 = np.abs(th[:, 1] - 0.5 * th[:, 0] + 0.4 * z[:, 1] + 0.2)
    return np.stack([r0, r1], axis=1)


def make_handle(S, kind, d, s, n, center=0.0, alg="single_eps"):
    a = S._lib.ALG_MULTI_EPS if alg == "multi_eps" else S._lib.ALG_SINGLE_EPS
    if kind == "gk":
        model = S.GandK(n_draws=128, c=0.8, ranks=(16, 48, 80, 112), obs=(1.9, 2.7, 3.6, 6.4))
        return S.SabcHandle(n_particles=n, model=model, prior=flat_prior(S, 4, 5.0, 5.0), seed=11, algorithm=a)
    if kind == "host":
        model = S.HostDistance(host_fdist, 2, 2, False, batched=True)
        return S.SabcHandle(n_particles=n, model=model, prior=flat_prior(S, 2, center, 5.0), seed=11, algorithm=a)
    return S.SabcHandle(n_particles=n, model=source_model(S, d, s, center), prior=flat_prior(S, d, center, 1.0 if center else 5.0),
                        seed=11, algorithm=a)


def box(kind, d, n, center, rng, spread):
    if kind == "gk":
        c = np.array([3.0, 1.0, 2.0, 1.0])[:, None]
        return c + rng.uniform(-0.2, 0.2, (4, n))
    return center + spread * rng.uniform(-0.5, 0.5, (d, n))


def tables_for(h, kind, regimes, n, theta, rng, rot=0):
    """One table per statistic in its regime, from the distances the simulator gives in the box (so the tables span them)."""
    s = h.s
    if kind == "host":
        pool = host_fdist(theta[:, :4000].T).T
    else:
        pool = h.simulate(theta[:, :4000], 7_000_000, 1)
    pats = ("runs", "dominant", "spread")
    out = []
    for j in range(s):
        reg = regimes[j % len(regimes)]
        L = E.regime_length(reg.rstrip("="), s, n, variant=0 if reg.endswith("=") else j)     # "block=": one length, one shift
        reg = reg.rstrip("=")
        assert L is not None and E.regime_of(L, s) == reg, (reg, s, n)
        out.append(E.make_table(L, pool[j], Q, pats[(j + rot) % 3] if kind != "gk" else ("dominant", "runs")[j % 2], rng))
    return out


def check_tables(h, tables):
    for j, T in enumerate(tables):
        h.set_cdf_knots(j, T)
    for j, T in enumerate(tables):
        np.testing.assert_array_equal(h.cdf_knots(j), T)
    P = [E.probes(T) for T in tables]
    m = max(len(p) for p in P)
    U = h.cdf_apply(np.stack([np.resize(p, m) for p in P]))
    for j, T in enumerate(tables):
        E.assert_u(T, np.resize(P[j], m), U[j], f"cdf_apply, statistic {j}")


def check_population(h, S, tables, kind, theta0, rho_grid_rows, alg):
    """Steps (3)-(5) of the module docstring."""
    d, s, n = h.d, h.s, h.n_local
    h.set_population(theta=theta0, u=np.ones((s, n)), rho=np.full((s, n), 1e3))
    h.set_eps(np.ones(len(h.eps)))       # (the multi-eps schedule of a population replaced at will may have left a negative one)
    c0 = h.counters["n_accept"]
    h.update(n_simulation=n, proposal=S.RandomWalk(n_para=d), resample=NO_RESAMPLE)
    th1, _, _ = h.get_population()
    moved = int(np.sum(np.any(th1 != theta0, axis=0)))
    assert h.counters["n_accept"] - c0 == n == moved, (h.counters["n_accept"] - c0, n, moved)
    h.update(n_simulation=K * n, proposal=S.RandomWalk(n_para=d), resample=NO_RESAMPLE)
    th, u, rho = h.get_population()
    assert not np.any(np.isnan(u))
    for j, T in enumerate(tables):
        E.assert_u(T, rho[j], u[j], f"population, statistic {j}")
        assert np.all(u[j][rho[j] > T[-1]] == 1.0) and np.all(u[j][rho[j] == 0.0] == 0.0)
    for j in rho_grid_rows:                          # the ties happened: on a knot, mostly inside runs of equal knots
        T, r = tables[j], rho[j]
        pos = r[r > 0]
        on = np.isin(pos, T[1:-1])
        runs = E.run_lengths(T)
        multi = np.isin(pos, T[1:-1][runs[1:-1] >= 2])
        if n >= 2000:                                # (a table of 144 knots holds a few dozen grid values)
            assert on.mean() > 0.5 and multi.mean() > 0.1, (j, on.mean(), multi.mean())
        assert multi.sum() > 0, j
    # the sums: the last history row against the returned population, epsilon against its equation
    e, ub, rb = h.history
    assert len(E.mean_mismatch(ub[-1], u, 1e-12)) == 0, (ub[-1], [E.fsum_mean(x) for x in u])
    assert len(E.mean_mismatch(rb[-1], rho, 1e-10)) == 0, (rb[-1], [E.fsum_mean(x) for x in rho])
    ubar = np.array([E.fsum_mean(x) for x in u])
    eps = h.eps
    if alg == "multi_eps":
        np.testing.assert_allclose(eps, S.op_eps_multi(ubar, 1.0), rtol=1e-9)
    else:
        ua, ep = E.fsum_mean(u), eps[0]
        assert abs(ep * ep + ep ** 1.5 - ua * ua) < 1e-9 * ua * ua                 # :93, v = 1
    sig, want = h.proposal_sigma, E.cov_ref(th, BETA)
    assert np.max(np.abs(sig - np.asarray(want, dtype=np.float64))) <= 1e-9 * np.max(np.abs(sig)), (sig, want)
    # the acceptance count of a one-update call is the number of particles that moved
    c1 = h.counters["n_accept"]
    h.update(n_simulation=n, proposal=S.RandomWalk(n_para=d), resample=NO_RESAMPLE)
    th2, _, _ = h.get_population()
    assert h.counters["n_accept"] - c1 == int(np.sum(np.any(th2 != th, axis=0))) > 0


# (id, kind, d, s, n, env, table sets, form: launches > 0?, lanes, algorithm)
CHAIN = {"SABC_PERSISTENT": "0"}
CASES = [
    ("chain-1x1", "src", 1, 1, 40_001, CHAIN, [["lds"], ["block"], ["mid"]], False, None, "single_eps"),
    ("chain-1x1-400k", "src", 1, 1, 400_003, CHAIN, [["mid"]], False, None, "single_eps"),
    ("chain-3x3-two-launch", "src", 3, 3, 40_001, dict(CHAIN, SABC_FUSE_REDUCE_MAX="0"), [["lds", "block", "mid"], ["mid"]],
     False, None, "multi_eps"),
    ("chain-3x3-130", "src", 3, 3, 130, CHAIN, [["lds"]], False, None, "multi_eps"),
    ("chain-5x12", "src", 5, 12, 40_001, CHAIN, [["lds", "block", "mid"]], False, None, "multi_eps"),
    ("one-launch-1x1-lanes1", "src", 1, 1, 40_001, {"SABC_PERSISTENT_LANES": "1"}, [["lds"], ["block"], ["mid"]], True, 1,
     "single_eps"),
    ("one-launch-1x1-lanes4", "src", 1, 1, 16_001, {"SABC_PERSISTENT_LANES": "4"}, [["lds"], ["block"]], True, 4, "single_eps"),
    ("one-launch-1x1-lanes16", "src", 1, 1, 2_001, {"SABC_PERSISTENT_LANES": "16"}, [["lds"], ["block"]], True, 16, "single_eps"),
    ("one-launch-3x3", "src", 3, 3, 40_001, {"SABC_PERSISTENT_LANES": "1"}, [["lds"], ["block="], ["mid"], ["block"], ["lds", "block", "mid"]], True, 1, "multi_eps"),
    ("one-launch-5x12", "src", 5, 12, 40_001, {"SABC_PERSISTENT_LANES": "1"}, [["mid", "lds", "block"]], True, 1, "single_eps"),
    ("wide-3x48", "src", 3, 48, 40_001, {}, [["lds", "block", "mid"]], False, None, "multi_eps"),
    ("host-2x2", "host", 2, 2, 40_001, {}, [["lds", "mid"], ["block"]], False, None, "multi_eps"),
    ("gk-4x4", "gk", 4, 4, 40_001, {}, [["mid"], ["lds", "block", "mid", "block"]], False, None, "single_eps"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_ecdf_lookups_and_sums_on_every_path(S, gpu, monkeypatch, case):
    name, kind, d, s, n, env, sets, one_launch, lanes, alg = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(abs(hash(name)) % (1 << 32))
    h = make_handle(S, kind, d, s, n, alg=alg)
    try:
        h.initialize(2 * n)
        for rot, regimes in enumerate(sets):
            theta0 = box(kind, d, n, 0.0, rng, 1.0)
            tables = tables_for(h, kind, regimes, n, theta0, rng, rot)
            check_tables(h, tables)
            assert [E.regime_of(len(T), s) for T in tables] == [regimes[j % len(regimes)].rstrip("=") for j in range(s)]
            l0 = h.persistent_launches
            grid_rows = [] if kind == "gk" else [j for j in range(s) if j % 2 == 0]
            check_population(h, S, tables, kind, theta0, grid_rows, alg)
            launched = h.persistent_launches - l0
            assert (launched > 0) == one_launch, (name, regimes, launched)
            if one_launch:
                assert h.persistent_lanes == lanes
    finally:
        h.close()


@pytest.mark.parametrize("d,s,form", [(3, 3, "chain"), (5, 12, "one-launch")])
def test_moment_sums_far_from_the_origin(S, gpu, monkeypatch, d, s, form):
    """The population at 1e6 with spread 1e-2: one-pass sums without the pivot would lose every digit of the covariance."""
    if form == "chain":
        monkeypatch.setenv("SABC_PERSISTENT", "0")
    else:
        monkeypatch.setenv("SABC_PERSISTENT_LANES", "1")
    n, center = 40_001, 1e6
    rng = np.random.default_rng(d * 100 + s)
    h = make_handle(S, "src", d, s, n, center=center, alg="multi_eps")
    try:
        h.initialize(2 * n)
        theta0 = box("src", d, n, center, rng, 1e-2)
        tables = tables_for(h, "src", ["mid", "lds", "block"], n, theta0, rng)
        check_tables(h, tables)
        l0 = h.persistent_launches
        check_population(h, S, tables, "src", theta0, [], "multi_eps")
        assert (h.persistent_launches > l0) == (form == "one-launch")
        sig = h.proposal_sigma
        assert np.all(np.diag(sig) > 0.5 * BETA * 1e-4 / 12)          # the spread, not rounding noise
    finally:
        h.close()


def test_set_cdf_knots_refuses_a_bad_table(S, gpu):
    """Unsorted, NaN, +-inf or negative knots: SABC_ERR_BAD_CONFIG, and the handle keeps its previous table -- the same u."""
    n = 1000
    h = make_handle(S, "src", 1, 1, n)
    try:
        h.initialize(2 * n)
        T = h.cdf_knots(0)
        q = np.concatenate([E.probes(T), np.linspace(0, T[-1] * 1.1, 301)])
        u0 = h.cdf_apply(q[None, :])
        E.assert_u(T, q, u0[0], "before")
        bad = {"unsorted": T[::-1].copy(), "nan": T.copy(), "+inf": T.copy(), "-inf": T.copy(), "negative": T.copy()}
        bad["nan"][len(T) // 2] = np.nan
        bad["+inf"][-1] = np.inf
        bad["-inf"][0] = -np.inf
        bad["negative"][0] = -1e-300
        bad["too long"] = np.linspace(0.0, 1.0, E.knot_stride(n) + 1)
        for what, B in bad.items():
            with pytest.raises(S.SABCError) as e:
                h.set_cdf_knots(0, B)
            assert "BAD_CONFIG" in str(e.value) and "knots" in str(e.value) or what == "too long", (what, str(e.value))
            np.testing.assert_array_equal(h.cdf_knots(0), T)
            np.testing.assert_array_equal(h.cdf_apply(q[None, :]), u0)
        T2 = T[: len(T) // 2].copy()                                   # a valid, shorter table is taken
        h.set_cdf_knots(0, T2)
        E.assert_u(T2, q, h.cdf_apply(q[None, :])[0], "after")
    finally:
        h.close()
