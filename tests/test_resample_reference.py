"""The long-double resample reference of tests/resample_ref.py: proof that its criterion tells a right draw from a wrong one on
every planted population, and the whole planted-population procedure on the CPU engine (engine.cpp over the oracle-backed
Backend).  CPU only: the device side, the same procedure, is tests/test_gpu_resample_paths.py."""
import numpy as np
import pytest

from tests import resample_ref as R

SEED = 11


def every_plan(s, group):
    rng = np.random.default_rng(100 * s + group)
    for n in R.SIZES + (R.N_ISLANDS,):
        for name, v, delta in R.plans(n, s, group, rng):
            yield n, name, v, delta


def test_the_patterns_are_what_they_claim():
    rng = np.random.default_rng(1)
    for s in (1, 3, 8):
        names = set()
        for n, name, v, delta in every_plan(s, 4):
            u = v * R.SCALE
            assert u.shape == (s, n) and u.min() > 2.0 ** -45 and u.max() <= R.SCALE * 53.0
            ref = R.Reference(u, delta)
            names.add(name)
            if name in R.SEPARATED:
                assert ref.min_share >= 1000 * ref.rel_tol, (name, n, s)
            if name == "one survivor":
                assert ref.pos.sum() == 1 and ref.ess == 1.0
            if name == "geometric" and n == R.SIZES[-1]:
                assert 69 < float(ref.a.min()) < 70 and 425 < float(ref.a.max()) < 435 and ref.pos.all()
                np.testing.assert_allclose(np.asarray(ref.w[8:] / ref.w[:-8], dtype=np.float64), 0.5, rtol=1e-12)
            if name == "dynamic range" and n >= 1023:
                decades = float(ref.a.max() - ref.a.min()) * np.log10(np.e)     # (a sum of s uniforms spreads less than one)
                assert ref.pos.all() and decades > (250 if s == 1 else 100), (n, s, decades)
            if name == "equal":
                assert ref.ess == pytest.approx(n, rel=1e-15)
        assert names == {"one survivor", *R.PATTERNS}
    # the islands: chunk 0 all but weightless, chunk 3 entirely, a weightless tail; runs across and at the chunk boundaries
    v, delta = R.islands(R.N_ISLANDS, 1, 4, rng)
    ref = R.Reference(v * R.SCALE, delta)
    live = np.nonzero(ref.pos)[0]
    assert live.tolist() == [i for lo, hi in R.ISLANDS for i in range(lo, hi)]
    assert not ref.pos[3 * R.CHUNK:4 * R.CHUNK].any() and ref.pos[:R.CHUNK].sum() == 4 and not ref.pos[live[-1] + 1:].any()
    assert R.survivor_positions(4163, 4) == [0, 3, 4, 1023, 1024, 1025, 2047, 4162]
    assert R.survivor_positions(5, 2) == [0, 1, 2, 4]
    assert [R.group_of(*ds) for ds in ((1, 1), (2, 3), (2, 2), (4, 4), (5, 5), (8, 8))] == [4, 2, 2, 1, 1, 16]


@pytest.mark.parametrize("s,group", [(1, 4), (3, 2), (8, 16)])
def test_the_checker_passes_the_oracles_draws_and_refuses_their_neighbours(O, s, group):
    """On every pattern and size: the oracle's own draws (binary64 weights, orc_weight_scan, orc_resample_index) satisfy the
    criterion and are the long-double answer; the same draws moved by one particle in either direction, or onto the nearest
    weightless particle, do not -- not even one in a thousand of them slips through where the weights are separated."""
    it = 3
    for n, name, v, delta in every_plan(s, group):
        u = v * R.SCALE
        ref = R.Reference(u, delta)
        un = R.uniforms(O, SEED, 0, n, it)
        t = ref.targets(un)
        idx, tot = R.oracle_draws(O, u, delta, un)
        assert len(ref.wrong(idx, t)) == 0, (name, n)
        assert abs(tot[0] - float(ref.total)) <= float(ref.tol) and abs(tot[0] ** 2 / tot[1] - ref.ess) <= 3 * ref.rel_tol * ref.ess
        assert ref.ambiguous(t) <= ref.ambiguous_allowed(n), (name, n, ref.ambiguous(t))
        assert np.sum(idx != ref.exact(t)) <= ref.ambiguous(t), (name, n)
        if n == 1:
            continue
        for shift in (-1, 1):
            moved = (idx + shift) % n
            bad = ref.wrong(moved, t)
            assert len(bad) > 0, (name, n, shift)
            if name in R.SEPARATED or n >= 1023:
                assert len(bad) >= n - ref.ambiguous(t) - 1, (name, n, shift, len(bad))
        dead = R.nearest_weightless(ref, idx)
        if name in ("one survivor", "islands"):
            assert dead is not None and len(ref.wrong(dead, t)) == n, (name, n)
        else:
            assert dead is None
        # out of range, and a tolerance a neighbour would fit in: the criterion as written is what refuses them
        assert len(ref.wrong(np.full(n, n), t)) == n and len(ref.wrong(np.full(n, -1), t)) == n
        if name in ("equal", "smooth"):
            loose = ref.wrong((idx + 1) % n, t, tol_factor=2.0 / (n * ref.rel_tol))
            assert len(loose) < n // 2 + 1, (name, n, len(loose))


CPU_CASES = [("gauss1", 1, 1, "single_eps"), ("gauss2d", 2, 3, "multi_eps")]


@pytest.mark.parametrize("kind,d,s,alg", CPU_CASES, ids=[c[0] for c in CPU_CASES])
def test_the_whole_procedure_on_the_cpu_engine(S, O, kind, d, s, alg):
    """Plant, one update that accepts nothing, the resample, read back: rows bit for bit, rho untouched, every draw against
    the weights, the ESS, and the control step behind the resample -- every pattern at every size."""
    from tests import cpu_engine
    H = cpu_engine.handle_class()
    rng = np.random.default_rng(7 * d + s)
    for n in R.SIZES + (R.N_ISLANDS,):
        h = R.builtin_handle(H, S, kind, n, alg, SEED)
        try:
            h.initialize(n)
            ran = R.run_single_shard(h, S, O, SEED, alg, rng)
            assert set(ran) == {"one survivor", *R.PATTERNS} - ({"islands"} if n != R.N_ISLANDS else set()), (n, ran)
        finally:
            h.close()


def test_the_procedure_refuses_a_corrupted_read_back(S, O):
    """A correct resample of the CPU engine (Gaussian2D, n = 1025, smooth weights) passes; the same read-back with every row
    taken from the neighbouring particle, u paired with another draw's theta, rho permuted, an ESS off by 1e-6, or the sums
    of a population that lost one block of 64, does not."""
    import copy
    from tests import cpu_engine
    from tests import ecdf_ref as E
    n, d, s, alg = 1025, 2, 3, "multi_eps"
    h = R.builtin_handle(cpu_engine.handle_class(), S, "gauss2d", n, alg, SEED)
    try:
        h.initialize(n)
        theta = R.planted_theta(d, 0, n)
        v, delta = R.smooth(n, s, 2, np.random.default_rng(5))
        u = v * R.SCALE
        ref = R.Reference(u, delta)
        _, _, rho0 = h.get_population()
        c0 = R.plant(h, theta, u)
        h.update(n_simulation=n, proposal=S.RandomWalk(β=R.BETA, n_para=d), resample=R.RESAMPLE_NOW, delta=delta)
        got = R.read_back(h, c0)
    finally:
        h.close()
    it = c0["n_population_updates"] + 1

    def check(g):
        R.check_shard(O, ref, "smooth", theta, u, rho0, g, 0, SEED, it)
        R.check_control(S, "smooth", g, alg, d, theta)

    check(got)
    idx = np.rint(got["theta"][0] / R.THETA_GRID).astype(np.int64)
    assert len(np.unique(idx)) > n // 2 and idx[0] != idx[1]
    for shift in (-1, 1):
        g = copy.deepcopy(got)
        g["theta"], g["u"] = theta[:, (idx + shift) % n], u[:, (idx + shift) % n]
        with pytest.raises(AssertionError, match="draws are wrong"):
            check(g)
    g = copy.deepcopy(got)
    g["u"][:, [0, 1]] = g["u"][:, [1, 0]]
    with pytest.raises(AssertionError, match="u rows"):
        check(g)
    g = copy.deepcopy(got)
    g["theta"][1, 0] = g["theta"][1, 1]
    with pytest.raises(AssertionError, match="theta rows"):
        check(g)
    g = copy.deepcopy(got)
    g["rho"] = np.roll(g["rho"], 1, axis=1)
    with pytest.raises(AssertionError, match="rho moved"):
        check(g)
    g = copy.deepcopy(got)
    g["ess"] *= 1 + 1e-6
    with pytest.raises(AssertionError):
        check(g)
    for key, rows in (("ubar", got["u"]), ("rhobar", got["rho"])):
        g = copy.deepcopy(got)
        g[key] = E.drop_block(rows, 3)
        with pytest.raises(AssertionError):
            check(g)
    g = copy.deepcopy(got)
    g["sigma"] = g["sigma"] * (1 + 1e-8)
    with pytest.raises(AssertionError):
        check(g)


@pytest.mark.parametrize("transport", ["alltoallv", "p2p"])
def test_the_sharded_procedure_on_the_cpu_engine(S, O, transport):
    """Two shards as host threads, GaussianIID (1, 1), n = 6211: the survivor at every position and the islands, over the
    personalised exchange and over the peer-to-peer paths of the CPU harness; every shard's draws against the global weights."""
    from tests import cpu_engine
    from tests.test_capi_shared_cpu import ThreadAllToAll, install, shard_threads
    from tests.test_p2p_cpu_engine import manual_setup
    H = cpu_engine.handle_class()
    plans = R.sharded_plans()
    n, world = R.N_ISLANDS, 2
    coll = ThreadAllToAll(world)
    descs = [None] * world
    records = [[None] * len(plans) for _ in range(world)]

    def body(rank, barrier):
        h = R.builtin_handle(H, S, "gauss1", n, "single_eps", SEED, rank=rank, world=world)
        try:
            install(h, coll, rank, 0, alltoallv=True)
            if transport == "p2p":
                manual_setup(h, descs, rank, barrier, 20_000.0)
            h.initialize(n)
            lo, m = h.local_offset, h.n_local
            for k, (name, theta, u, delta, ref) in enumerate(plans):
                _, _, rho0 = h.get_population()
                barrier.wait()                     # (p2p: no shard replaces its particles while the other still reads them)
                c0 = R.plant(h, theta[:, lo:lo + m], u[:, lo:lo + m])
                h.update(n_simulation=n, proposal=S.RandomWalk(β=R.BETA, n_para=1), resample=R.RESAMPLE_NOW, delta=delta)
                records[rank][k] = (c0, lo, rho0, R.read_back(h, c0))
            assert h.p2p_active == (transport == "p2p")
        finally:
            h.close()

    shard_threads(world, coll, body)
    R.check_shards(S, O, plans, records, SEED)
