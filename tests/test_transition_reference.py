"""The long-double transition reference of tests/transition_ref.py on the CPU: (i) the whole procedure on the CPU engine
(engine.cpp over the oracle-backed Backend), one shard and worlds of 2 and 3 with ragged last shards, zero undecided particles;
(ii) proof that the checker refuses after-populations built with one deliberate error each; (iii) the two spellings of log U
against the exact log.  The device side, the same procedure on every kernel path, is tests/test_gpu_transition_paths.py.

The CPU engine has the built-in simulators only, so the cases take the shapes it has: (1, 1) and (2, 2) GaussianIID, (2, 3)
Gaussian2D, (4, 4) g-and-k; rho_of is the oracle's simulator, a function of (theta, gid, it)."""
import copy
import math

import numpy as np
import pytest

from tests import elementary_ref as R
from tests import transition_ref as T
from tests.cases import oracle_model_params

SEED = 11
MODELS = {
    "gauss1": (("GaussianIID", dict(n_obs=20, sd=1.0, obs_mean=0.3)), 1, 1),
    "gauss2s2": (("GaussianIID", dict(n_obs=10, sd=1.0, obs_mean=0.0, obs_m2=1.0)), 2, 2),
    "gauss2d": (("Gaussian2D", dict(n_obs=50, r=0.6, obs_mean=(1.2, -0.7), obs_varsum=2.1, obs_cov=0.55)), 2, 3),
    "gk": (("GandK", dict(n_draws=128, c=0.8, ranks=(16, 48, 80, 112), obs=(1.9, 2.7, 3.6, 6.4))), 4, 4),
}
GK_LO = [[2.55, 0.65, 1.65, 0.65], [3.15, 1.05, 2.05, 1.05]]
GK_HI = [[2.85, 0.95, 1.95, 0.95], [3.45, 1.35, 2.35, 1.35]]
MIXED = T.Prior(dims=[("T", 3.0, 1.0, 1.5, 4.5), ("G", 4.0, 0.25), ("L", 0.7, 0.3), ("U", 0.0, 10.0)])
EDGE2 = T.Prior(dims=[("U", -1.0, 1.0), ("U", 0.2, 2.0)])
EDGE2_LO, EDGE2_HI = [[-1.0, 0.2], [0.5, 1.5]], [[-0.5, 0.6], [1.0, 2.0]]


def case(name, model, n, prop, alg, prior, lo, hi, eps, **kw):
    _, d, s = MODELS[model]
    return T.Case(name, d, s, n, prop, alg, prior, np.broadcast_to(lo, (2, d)), np.broadcast_to(hi, (2, d)), eps, model=model, **kw)


CASES = [
    case("rw-1x1-normal", "gauss1", 1027, ("rw", 0.8, 0.0), "single_eps", T.Prior(dims=[("N", 0.0, 0.7)]), -1.0, 1.0, [0.5]),
    case("de-2x2-uniform-edge", "gauss2s2", 1027, ("de", 1.19, 0.05), "multi_eps", EDGE2, EDGE2_LO, EDGE2_HI, T.ladder(2), edge=True),
    case("de-2x2-uniform-edge-n4", "gauss2s2", 4, ("de", 1.19, 0.05), "multi_eps", EDGE2, EDGE2_LO, EDGE2_HI, T.ladder(2), edge=True,
         collide=True, seed=3),
    case("stretch-4x4-mixed", "gk", 1027, ("stretch", 2.0, 0.0), "multi_eps", MIXED, GK_LO, GK_HI, T.ladder(4)),
    case("rw-4x4-normal", "gk", 1027, ("rw", 0.8, 0.0), "multi_eps",
         T.Prior(dims=[("N", 3.0, 0.3), ("N", 1.0, 0.2), ("N", 2.0, 0.3), ("N", 1.0, 0.2)]), GK_LO[0], GK_HI[1], T.ladder(4)),
    case("rw-2x3-mvnormal-130", "gauss2d", 130, ("rw", 0.8, 0.0), "multi_eps",
         T.Prior(mv=([0.5, -0.5], np.linalg.cholesky(np.array([[0.5, -0.2], [-0.2, 0.4]])))), [0.4, -1.5], [2.0, 0.1], T.ladder(3)),
    case("de-2x3-uniform-edge", "gauss2d", 1027, ("de", 1.19, 0.05), "multi_eps", T.Prior(dims=[("U", 0.0, 2.4), ("U", -1.9, 0.5)]),
         [[0.0, -1.9], [1.6, -0.4]], [[0.8, -1.0], [2.4, 0.5]], T.ladder(3), edge=True),
    case("stretch-4x4-flat", "gk", 1027, ("stretch", 2.0, 0.0), "single_eps", T.Prior(dims=[("U", 0.0, 10.0)] * 4), GK_LO, GK_HI, [0.15]),
]
BY_NAME = {c.name: c for c in CASES}


def oracle_rho_of(O, c, gid0, model=None):
    """rho_of(theta [d][m], it) -> [s][m]: the oracle's simulator for particles gid0 .."""
    spec, d, s = MODELS[model or c.extra["model"]]
    mid, params = oracle_model_params(O, {"model": spec})
    cfg = O.make_config(n_particles=c.n, n_para=d, n_stats=s, model_id=mid, model_params=params,
                        prior=[(O.PRIOR_NORMAL, 0.0, 1.0)] * d, seed=SEED)

    def rho_of(theta, it):
        theta = np.asarray(theta, dtype=np.float64)
        return np.stack([O.simulate(cfg, theta[:, i].copy(), gid0 + i, it) for i in range(theta.shape[1])], axis=1)
    return rho_of


def cpu_handle(S, c, **kw):
    from tests import cpu_engine
    spec, d, s = MODELS[c.extra["model"]]
    a = S._lib.ALG_MULTI_EPS if c.alg == "multi_eps" else S._lib.ALG_SINGLE_EPS
    return cpu_engine.handle_class()(n_particles=c.n, model=getattr(S, spec[0])(**spec[1]), prior=c.prior.make(S), seed=SEED,
                                     algorithm=a, **kw)


# ---------------------------------------------------------------- (i)
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_every_case_passes_on_the_cpu_engine_with_nothing_undecided(S, O, c):
    h = cpu_handle(S, c)
    try:
        h.initialize(c.n)
        rep = T.run_single_shard(h, S, O, c, SEED, oracle_rho_of(O, c, 0))
    finally:
        h.close()
    assert len(rep.undecided) == 0
    assert rep.theta_ratio <= 1.0 and rep.margin > 1.0
    print(f"{c.name}: accepted {int(rep.accepted.sum())} of {c.n}, |theta_new - thp| / tol_theta <= {rep.theta_ratio:.3f}, "
          f"|log U - log_alpha| / tol_alpha >= {rep.margin:.3g}")


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["rw-4x4-normal", "de-2x2-uniform-edge", "stretch-4x4-mixed"])
def test_shards_with_a_ragged_last_one_on_the_cpu_engine(S, O, name, world):
    """1027 particles on 2 shards (514, 513) and on 3 (343, 343, 341): every shard's half batches take their partners from
    the inactive halves of ALL shards, the second from what every shard's first half batch left."""
    from tests.test_capi_shared_cpu import ThreadAllToAll, install, shard_threads
    c = BY_NAME[name]
    lay = T.Layout(c.n, world)
    assert lay.sizes[-1] < lay.cap
    theta_all, u_all = T.planted(c, lay)
    pool_all = np.abs(oracle_rho_of(O, c, 0)(theta_all, 1))
    coll = ThreadAllToAll(world)
    before, after = [None] * world, [None] * world

    def body(rank, barrier):
        h = cpu_handle(S, c, rank=rank, world=world)
        try:
            install(h, coll, rank, 0, alltoallv=True)
            h.initialize(c.n)
            before[rank] = T.prepare(h, S, c, lay, theta_all, u_all, pool_all)
            h.update(n_simulation=c.n, proposal=c.proposal(S), resample=T.NO_RESAMPLE)
            after[rank] = (h.get_population(), h.counters)
        finally:
            h.close()

    shard_threads(world, coll, body)
    theta0s, theta1s = [b.theta0 for b in before], [a[0][0] for a in after]
    accepted = 0
    for rank in range(world):
        gid0 = lay.offset(rank)
        rho_of = oracle_rho_of(O, c, gid0)
        inp = T.inputs(c, lay, rank, before[rank], theta0s, theta1s, T.Streams(O, SEED, gid0, lay.sizes[rank]), rho_of)
        rep = T.check(inp, after[rank][0])
        T.premises(c, rep.ref)
        T.assert_ok(rep, f"{name}, shard {rank} of {world}")
        assert len(rep.undecided) == 0
        accepted += int(rep.accepted.sum())
        np.testing.assert_array_equal(before[rank].sigma, before[0].sigma)
    assert after[0][1]["n_accept"] - before[0].counters["n_accept"] == accepted


def stand_in_rho_of(O, c):
    """The simulators of the device cases on the CPU: the oracle's for the built-in ones, f_dist itself for host mode, and for
    the source of tests/test_gpu_transition_paths.py its formula over the oracle's normals of the SIM stream (the device's
    bits up to an ulp: enough to know a case's accepted fraction before it runs on a device)."""
    from tests import test_gpu_transition_paths as G
    kind = c.extra["kind"]
    if kind == "host":
        return lambda theta, it: G.host_rho(np.asarray(theta, dtype=np.float64))
    if kind != "src":
        return oracle_rho_of(O, c, 0, {"gauss": "gauss1", "gk": "gk"}[kind])
    zs = {}

    def rho_of(theta, it):
        theta = np.asarray(theta, dtype=np.float64)
        n = theta.shape[1]
        if it not in zs:
            zs[it] = np.array([np.concatenate([O.normal_pair(SEED, i, O.PURPOSE_SIM, it, k) for k in range((c.s + 1) // 2)])
                               for i in range(n)]).T
        j = np.arange(c.s)[:, None]
        return np.abs(theta[j[:, 0] % c.d] + 0.5 * theta[(j[:, 0] + 1) % c.d] + G.NOISE * zs[it][:c.s] - 0.3 * ((j % 5) - 2))
    return rho_of


def test_the_device_cases_bite_before_they_run_on_a_device(O):
    """Every case of tests/test_gpu_transition_paths.py in the reference alone, with stand-ins for the device's simulators:
    20 to 80 % accepted, the edge cases' 5 % outside the support, cond(Sigma) < 1e3, the collision at n = 4, different
    epsilons -- and nothing undecided."""
    from tests import test_gpu_transition_paths as G
    assert G.SEED == SEED
    for c in G.CASES:
        inp = reference_world(O, c, updates_before=0, rho_of=stand_in_rho_of(O, c))
        ref = T.restate(inp)
        T.premises(c, ref)
        rep = judged(inp, ref.P1)
        T.assert_ok(rep, c.name)
        assert len(rep.undecided) == 0, c.name
        u = inp.u0
        assert u.min() > 0 and u.max() < 1 and u.std() > 0.2
        if c.prop[0] != "rw":                       # the halves of P0 come from boxes that do not overlap
            assert np.all((c.lo[1] >= c.hi[0]) | (c.hi[1] <= c.lo[0]))


# ---------------------------------------------------------------- (ii)
def reference_world(O, c, updates_before=4, rho_of=None):
    """The inputs of case c without an engine: the planted population, Sigma = beta (cov + 1e-8 I) of it (ecdf_ref.cov_ref),
    and the reference's own after-population."""
    lay = T.Layout(c.n, 1)
    theta, u = T.planted(c, lay)
    rho_of = rho_of or oracle_rho_of(O, c, 0)
    pool = np.abs(rho_of(theta, 1))
    from tests import ecdf_ref as E
    before = T.SimpleNamespace(theta0=theta, u0=u, rho0=pool, tables=T.tables_for(c, pool, np.random.default_rng(c.seed + 1)),
                               sigma=np.asarray(E.cov_ref(theta, c.prop[1]), dtype=np.float64).reshape(c.d, c.d), eps=c.eps,
                               counters=dict(n_population_updates=updates_before), gid0=0)
    streams = T.Streams(O, SEED, 0, c.n)
    inp = T.inputs(c, lay, 0, before, [theta], None, streams, rho_of)
    return inp


def judged(inp, P1, ties=()):
    j = copy.copy(inp)
    j.theta1s = [P1.theta]
    return T.check(j, (P1.theta, P1.u, P1.rho), ties=ties)


@pytest.fixture(scope="module")
def worlds(O):
    out = {}
    for name in ("rw-2x3-mvnormal-130", "rw-4x4-normal", "de-2x2-uniform-edge", "stretch-4x4-mixed"):
        inp = reference_world(O, BY_NAME[name])
        ref = T.restate(inp)
        rep = judged(inp, ref.P1)
        T.premises(BY_NAME[name], rep.ref)
        T.assert_ok(rep, name)
        assert len(rep.undecided) == 0 and not rep.any_bad.any()
        out[name] = (inp, ref)
    return out


# (the error, the case it is planted in, the assertion that must refuse it); on at least 10 % of the particles, but
# logf_d: on 5 % -- d log z in place of (d - 1) log z moves log_alpha by |log z| <= log 2, 0.35 on average, which changes the
# decision of about one particle in fifteen
SCOPE = {"logf_d": 0.05}
MUTATIONS = [
    ("LT", "rw-4x4-normal", "theta"), ("LT", "rw-2x3-mvnormal-130", "theta"),
    ("purpose", "rw-4x4-normal", "theta"), ("it+1", "rw-4x4-normal", "theta"),
    ("active", "de-2x2-uniform-edge", "theta"), ("active", "stretch-4x4-mixed", "theta"),
    ("stale", "de-2x2-uniform-edge", None), ("stale", "stretch-4x4-mixed", None),
    ("gamma", "de-2x2-uniform-edge", "theta"),
    ("logf_d", "stretch-4x4-mixed", "decision"),
    ("lp_swapped", "rw-4x4-normal", "decision"), ("lp_swapped", "rw-2x3-mvnormal-130", "decision"),
    ("lp_swapped", "stretch-4x4-mixed", "decision"),
    ("eps0", "rw-4x4-normal", "decision"), ("eps0", "stretch-4x4-mixed", "decision"),
    ("u_swapped", "de-2x2-uniform-edge", "decision"), ("u_swapped", "rw-4x4-normal", "decision"),
    ("accept_zw", "rw-4x4-normal", "decision"),
]


@pytest.mark.parametrize("mut,name,category", MUTATIONS, ids=[f"{m}-{n}" for m, n, _ in MUTATIONS])
def test_a_population_built_with_one_error_is_refused(worlds, mut, name, category):
    """The after-population the reference itself builds with the error `mut` in it: refused on at least 10 % of the
    particles (SCOPE: a stated smaller share), by the assertion named."""
    inp, _ = worlds[name]
    wrong = T.restate(inp, mut={mut})
    rep = judged(inp, wrong.P1)
    n = BY_NAME[name].n * SCOPE.get(mut, 0.1)
    assert rep.any_bad.sum() >= n, (mut, name, {c: int(b.sum()) for c, b in rep.bad.items()})
    if category is not None:
        assert rep.bad[category].sum() >= n, (mut, name, {c: int(b.sum()) for c, b in rep.bad.items()})
    with pytest.raises(AssertionError, match="particles fail"):
        T.assert_ok(rep, name)


def test_wrong_stores_are_refused(worlds):
    """Errors in what is written, on the reference's own after-population of the DifferentialEvolution edge case: a proposal
    outside the support accepted (scope: the proposals outside, at least 5 %); an accepted particle whose u, or whose rho, was
    not stored; a rejected particle whose rho was overwritten (at least 10 % each)."""
    name = "de-2x2-uniform-edge"
    inp, ref = worlds[name]
    n, h = ref.n, ref.h
    acc, out = ref.decision > 0, ref.outside
    rej = (ref.decision < 0) & ~out

    def fresh():
        return copy.deepcopy(ref.P1)

    P = fresh()
    P.theta[:, out], P.u[:, out], P.rho[:, out] = ref.thp64[:, out], ref.up[:, out], ref.rp[:, out]
    rep = judged(inp, P)
    assert out.sum() >= 0.05 * n and rep.bad["support"].sum() >= 0.9 * out.sum(), (out.sum(), rep.bad["support"].sum())
    P = fresh()
    P.u[:, acc] = inp.u0[:, acc]
    assert judged(inp, P).bad["u"].sum() == acc.sum() >= 0.1 * n
    P = fresh()
    P.rho[:, acc] = inp.rho0[:, acc]
    assert judged(inp, P).bad["rho"].sum() == acc.sum() >= 0.1 * n
    P = fresh()
    P.rho[:, rej] = ref.rp[:, rej]
    assert judged(inp, P).bad["store"].sum() == rej.sum() >= 0.1 * n


def test_a_particle_left_untouched_at_the_end_of_a_half_is_refused(O):
    """The last particle of each half -- the second is also the last of the shard -- left as it was (scope: those two
    particles; the update index is chosen so that the reference accepts both, which is asserted)."""
    c = BY_NAME["de-2x2-uniform-edge"]
    inp = reference_world(O, c, updates_before=2)
    ref = T.restate(inp)
    n, h = ref.n, ref.h
    assert inp.it == 3 and ref.decision[h - 1] > 0 and ref.decision[n - 1] > 0
    assert not judged(inp, ref.P1).any_bad.any()
    for i in (h - 1, n - 1):
        P = copy.deepcopy(ref.P1)
        P.theta[:, i], P.u[:, i], P.rho[:, i] = inp.theta0s[0][:, i], inp.u0[:, i], inp.rho0[:, i]
        rep = judged(inp, P)
        assert rep.bad["decision"][i]
        if i == n - 1:                                # (nobody's partner: nothing else changes)
            assert np.nonzero(rep.any_bad)[0].tolist() == [i]
        with pytest.raises(AssertionError, match="particles fail"):    # (h - 1 is also a partner: a second-half theta follows)
            T.assert_ok(rep, c.name)


def test_less_or_equal_is_refused_on_planted_ties(worlds):
    """`<=` in place of `<` differs from the rule only on a tie, log U == log_alpha, which no tolerance can see: refused only
    on planted ties -- particles whose log_alpha the test sets to their log U with tolerance zero.  The rule rejects them; a
    population that accepted them is refused on exactly those, and on nothing without the ties planted."""
    name = "rw-4x4-normal"
    inp, ref0 = worlds[name]
    ties = tuple(int(i) for i in np.nonzero(ref0.decision < 0)[0][:5])
    ref = T.restate(inp, ties=ties)
    assert np.all(ref.decision[list(ties)] == -1) and np.all(ref.logU[list(ties)] == ref.log_alpha[list(ties)])
    assert not judged(inp, ref.P1, ties=ties).any_bad.any()
    P = copy.deepcopy(ref.P1)
    t = list(ties)
    P.theta[:, t], P.u[:, t], P.rho[:, t] = ref.thp64[:, t], ref.up[:, t], ref.rp[:, t]
    rep = judged(inp, P, ties=ties)
    assert np.nonzero(rep.bad["decision"])[0].tolist() == sorted(t)
    assert judged(inp, P).bad["decision"][t].all()


# ---------------------------------------------------------------- (iii)
def test_the_two_spellings_of_log_u_stay_inside_their_part_of_tol_alpha(O):
    """-0.5 neg2_log_tab(x) (k_update, k_update_wide, k_update_gk, the one-launch form) and log_fast(x) (k_host_accept),
    restated with elementary_ref, on the accept uniforms of every case: each within its proven bound of the exact log (2.0 and
    1.0 ulp), and their disagreement with each other within LOGU_ULPS = 3 ulp of log U, the part of tol_alpha granted to
    them."""
    worst = {"neg2_log_tab": 0.0, "log_fast": 0.0, "disagreement": 0.0}
    seen = set()
    for c in CASES:
        for it in (1, 5):
            key = (c.n, it)
            if key in seen:
                continue
            seen.add(key)
            x = T.accept_uniforms(T.Streams(O, SEED, 0, c.n), it)
            for v in x:
                v = float(v)
                ex = R.exact("log_fast", v)
                a, b = -0.5 * R.neg2_log_tab(v), R.log_fast(v)
                worst["neg2_log_tab"] = max(worst["neg2_log_tab"], R.ulps(a, ex))
                worst["log_fast"] = max(worst["log_fast"], R.ulps(b, ex))
                worst["disagreement"] = max(worst["disagreement"], abs(a - b) / math.ulp(abs(float(ex))))
    assert worst["neg2_log_tab"] <= 2.0 and worst["log_fast"] <= 1.0, worst
    assert worst["disagreement"] <= T.LOGU_ULPS, worst
    print(worst)
