"""Plain NumPy restatement of the resample (SimulatedAnnealingABC.jl:124-137) in long double, the planted populations and the
procedure that tests/test_resample_reference.py (CPU engine) and tests/test_gpu_resample_paths.py (device) share.

Nothing here knows how the kernels find a draw (chunks, packed lines, the guide, the walk, the fallback onto the next chunk):
a drawn index k is judged against the weights themselves.  With a_i = sum_j delta u_ij / mean_j(u), w_i = exp(-a_i) (0 from
a_i >= 800; binary64 exp gives 0 above 745.2, and every pattern keeps a out of (700, 800), so neither side sees a denormal),
F = cumsum(w), total = F[-1] and t = u52(Philox block (seed, gid, PURPOSE_RESAMPLE, it, 0)) total:

    k is right  iff  w_k > 0  and  F[k-1] - tol <= t <= F[k] + tol,    tol = (a_max (n + 16) + 2 n) 2^-53 total

a_max the largest a_i with w_i > 0.  The bound is derived, not measured: any order of summation is within n 2^-53 of the exact
sum (for the means of u, the running sums and the total), and a relative error e of a is a relative error a e of exp(-a).
Every draw is checked.  Two neighbours can both pass only where t lies within tol of a boundary: the patterns in SEPARATED
assert that their smallest positive w_i / total is at least 1000 tol, so there an index off by one particle cannot pass.  The
geometric pattern beyond n = 70 and the dynamic-range pattern cannot assert that (their smallest weights are 1e-150 and
1e-260 of the total); for them -- and for all others too -- `ambiguous` counts the draws that more than one index would
satisfy, from the reference alone, and the procedure bounds that count by its expectation 2 tol / total per boundary and draw.

The patterns are functions (n, s, group, rng) -> (v [s][n], delta), planted as u = v 2^-30: small enough that the update in
front of the resample accepts nothing at epsilon = 1e-300, and above 2^-45, so that the multi-epsilon guard mean(u) <= eps()
(:107-109) cannot fire on the resampled population.  delta carries a factor 1 / s wherever the issue's figure was given for
one statistic (2000, and ln 2 mean(v) / 0.01): a_i then spans the same range for every s, which the separation and the
(700, 800) rule need -- with s = 8 statistics delta = 2000 would put the islands' own weights 20 decades apart."""
import math

import numpy as np

CHUNK = 1024                    # kScanChunk: particles per scan chunk
SCALE = 2.0 ** -30              # u = v * SCALE
THETA_GRID = 2.0 ** -13         # theta[0][i] = gid * THETA_GRID: exact, decodable
EPS_NO_ACCEPT = 1e-300
RESAMPLE_NOW = 1e-9             # update(resample=): n_accept = 1 reaches (n_resampling + 1) * 1e-9
BETA = 0.8
LD = np.longdouble
SIZES = (5, 70, 1023, 1025, 4 * CHUNK + 16 * 4 + 3)       # inside a line, a group, one short of / past a chunk, 4163
N_ISLANDS = 6 * CHUNK + 67                                 # 6211
ISLANDS = ((1020, 1027), (2048, 2049), (5117, 5120), (6150, 6152))
SEPARATED = ("one survivor", "islands", "equal", "smooth")
CONTROL_CHECKED = ("islands", "geometric", "dynamic range", "smooth")


# ---------------------------------------------------------------- the reference
class Reference:
    """Weights, running sums and the tolerance of the module docstring for u [s][n] (the whole population) and delta."""

    def __init__(self, u, delta):
        u = np.asarray(u, dtype=np.float64).astype(LD)
        s, n = u.shape
        ubar = u.sum(axis=1) / LD(n)
        self.a = (LD(delta) * u / ubar[:, None]).sum(axis=0)
        assert not np.any((self.a > 700) & (self.a < 800)), "a pattern must keep a_i out of (700, 800)"
        self.w = np.where(self.a >= 800, LD(0), np.exp(-self.a))
        self.pos = self.w > 0
        assert self.pos.any()
        self.F = np.cumsum(self.w)
        self.Flo = np.concatenate([[LD(0)], self.F[:-1]])
        self.total = self.F[-1]
        self.ess = float(self.total * self.total / np.sum(self.w * self.w))
        self.n = n
        a_max = self.a[self.pos].max()
        self.tol = (a_max * (n + 16) + 2 * n) * LD(2.0) ** -53 * self.total
        self.rel_tol = float(self.tol / self.total)
        self.min_share = float(self.w[self.pos].min() / self.total)
        self._npos = np.concatenate([[0], np.cumsum(self.pos)])

    def targets(self, uniforms):
        return np.asarray(uniforms, dtype=np.float64).astype(LD) * self.total

    def wrong(self, idx, t, tol_factor=1.0):
        """Positions of the draws idx (one per target t) that do not satisfy the criterion."""
        idx = np.asarray(idx, dtype=np.int64)
        inside = (idx >= 0) & (idx < self.n)
        k = np.clip(idx, 0, self.n - 1)
        tol = self.tol * tol_factor
        ok = inside & self.pos[k] & (self.Flo[k] - tol <= t) & (t <= self.F[k] + tol)
        return np.nonzero(~ok)[0]

    def exact(self, t):
        """The first k with F[k] > t in long double: what a draw is when no rounding is in the way."""
        return np.minimum(np.searchsorted(self.F, t, side="right"), self.n - 1)

    def ambiguous(self, t):
        """How many of the targets t more than one index would satisfy."""
        lo = np.searchsorted(self.F, t - self.tol, side="left")
        hi = np.searchsorted(self.Flo, t + self.tol, side="right")          # indices [lo, hi)
        hi = np.maximum(hi, lo)
        return int(np.sum(self._npos[hi] - self._npos[lo] > 1))

    def ambiguous_allowed(self, n_draws):
        """Expectation 2 tol / total per boundary between two positive weights and per draw; ten times that, and 2."""
        return 2 + 10.0 * n_draws * int(self.pos.sum()) * 2.0 * self.rel_tol


_uniform_cache = {}


def uniforms(O, seed, gid0, m, it):
    """u52 of the first two words of the Philox blocks (seed, gid, PURPOSE_RESAMPLE, it, 0), gid = gid0 .. gid0 + m - 1."""
    key = (int(seed), int(gid0), int(m), int(it))
    if key not in _uniform_cache:
        out = np.empty(m)
        for i in range(m):
            b = O.stream_block(int(seed), int(gid0) + i, O.PURPOSE_RESAMPLE, int(it), 0)
            out[i] = O.u52(b[0], b[1])
        if len(_uniform_cache) > 256:
            _uniform_cache.clear()
        _uniform_cache[key] = out
    return _uniform_cache[key]


def oracle_draws(O, u, delta, un):
    """The oracle's own draws for the uniforms un: binary64 weights as resample_population forms them, orc_weight_scan,
    orc_resample_index."""
    u = np.asarray(u, dtype=np.float64)
    ubar = u.mean(axis=1)
    a = np.zeros(u.shape[1])
    for j in range(u.shape[0]):
        a += u[j] * delta / ubar[j]
    cum, bs, tot = O.weight_scan(np.exp(-a))
    return np.array([O.resample_index(cum, bs, x * tot[0]) for x in un], dtype=np.int64), tot


def nearest_weightless(ref, idx):
    """Every draw moved to the weightless particle nearest to it (None where the population has none)."""
    dead = np.nonzero(~ref.pos)[0]
    if len(dead) == 0:
        return None
    j = np.searchsorted(dead, idx)
    left, right = dead[np.clip(j - 1, 0, len(dead) - 1)], dead[np.clip(j, 0, len(dead) - 1)]
    return np.where(np.abs(idx - left) <= np.abs(right - idx), left, right)


# ---------------------------------------------------------------- the planted populations
def one_survivor(n, s, p):
    v = np.ones((s, n))
    v[:, p] = 1e-3
    return v, 2000.0 / s


def survivor_positions(n, group):
    """The first particle, the last of the first line (group) and the one behind it, both sides of the chunk boundaries, the
    last particle of a chunk and of the population."""
    return sorted({p for p in (0, group - 1, group, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, n - 1) if 0 <= p < n})


def islands(n, s, group, rng):
    """All weightless but four short runs: across the boundary of chunks 0 and 1, a chunk's first particle alone, a chunk's
    last particles, and two particles of the last chunk with a weightless tail behind them; chunk 3 has no weight at all."""
    if n != N_ISLANDS:
        return None
    v = np.ones((s, n))
    for lo, hi in ISLANDS:
        v[:, lo:hi] = rng.uniform(1e-4, 3e-3, (s, hi - lo))
    return v, 2000.0 / s


def geometric(n, s, group, rng):
    """w proportional to 2^-(i // 8): nearly every guide bucket points into the first lines."""
    v = np.tile(1.0 + 0.01 * (np.arange(n) // 8), (s, 1))
    return v, math.log(2.0) * float(v[0].mean()) / (0.01 * s)


def dynamic_range(n, s, group, rng):
    """v ~ U(2^-12, 1), delta = 300 / s: about 260 decades of weight (redrawn until no a_i lies in (700, 800): a small
    population's mean can be far from 1/2)."""
    delta = 300.0 / s
    while True:
        v = rng.uniform(2.0 ** -12, 1.0, (s, n))
        a = (delta * v / v.mean(axis=1, keepdims=True)).sum(axis=0)
        if not np.any((a > 690) & (a < 810)):
            return v, delta


def equal(n, s, group, rng):
    return np.ones((s, n)), 0.1


def smooth(n, s, group, rng):
    """The production regime: u from an ECDF, delta = 0.1."""
    return rng.uniform(2.0 ** -12, 1.0, (s, n)), 0.1


PATTERNS = {"islands": islands, "geometric": geometric, "dynamic range": dynamic_range, "equal": equal, "smooth": smooth}


def plans(n, s, group, rng, names=None):
    """(name, v, delta) for a population of n: the one-survivor pattern at each of its positions, then every pattern that
    fits n."""
    out = []
    if names is None or "one survivor" in names:
        for p in survivor_positions(n, group):
            out.append(("one survivor", *one_survivor(n, s, p)))
    for name, fn in PATTERNS.items():
        if names is not None and name not in names:
            continue
        made = fn(n, s, group, rng)
        if made is not None:
            out.append((name, *made))
    return out


def planted_theta(d, gid0, m):
    """theta[0] = gid 2^-13; the other rows a fixed function of gid inside (1, 9) that no two rows share."""
    gid = np.arange(gid0, gid0 + m, dtype=np.int64)
    th = np.empty((d, m))
    th[0] = gid * THETA_GRID
    for r in range(1, d):
        th[r] = 2.0 + 0.25 * r + ((gid * (2 * r + 3)) % 17) / 64.0 + ((gid * 5 + r) % 11) / 128.0
    return th


def group_of(d, s):
    """Particles per 128-byte line of the packed resample (16 for rows that do not fit a line: the unpacked search's
    groups of 16 running sums)."""
    per = 16 // (1 + d + s)
    return 4 if per >= 4 else 2 if per >= 2 else 1 if per >= 1 else 16


# ---------------------------------------------------------------- the procedure
def flat_box(S, d, lo=-1.0, hi=9.0):
    """A flat prior over a box that holds every planted theta."""
    return S.Uniform(lo, hi) if d == 1 else S.product_distribution([S.Uniform(lo, hi) for _ in range(d)])


def builtin_handle(H, S, kind, n, alg, seed, **kw):
    """A handle of class H (the product's, or the CPU engine's) for one of the built-in models."""
    if kind == "gauss1":
        model, d = S.GaussianIID(n_obs=100, sd=1.0, obs_mean=0.3), 1
    elif kind == "gauss2d":
        model, d = S.Gaussian2D(n_obs=50, r=0.6, obs_mean=(1.2, 2.4), obs_varsum=2.1, obs_cov=0.55), 2
    elif kind == "gk":
        model, d = S.GandK(n_draws=128, c=0.8, ranks=(16, 48, 80, 112), obs=(1.9, 2.7, 3.6, 6.4)), 4
    else:
        raise KeyError(kind)
    a = S._lib.ALG_MULTI_EPS if alg == "multi_eps" else S._lib.ALG_SINGLE_EPS
    return H(n_particles=n, model=model, prior=flat_box(S, d, 0.0 if kind == "gk" else -1.0, 10.0 if kind == "gk" else 9.0),
             seed=seed, algorithm=a, **kw)


def plant(h, theta, u):
    """Step 1: the planted shard, an epsilon that accepts nothing, n_accept = 1.  Returns the counters as planted."""
    h.set_population(theta=theta, u=u)                                 # rho stays as it is
    h.set_eps(np.full(len(h.eps), EPS_NO_ACCEPT))
    c = h.counters
    h.set_counters(c["n_simulation"], 1, c["n_resampling"], c["n_population_updates"])
    return h.counters


def read_back(h, c0):
    """Steps 3 and 4a: the premise (nothing accepted, exactly one resample, one population update) and the shard's state."""
    c = h.counters
    assert c["n_accept"] == 1, ("the update in front of the resample accepted a proposal", c0, c)
    assert c["n_resampling"] == c0["n_resampling"] + 1, (c0, c)
    assert c["n_population_updates"] == c0["n_population_updates"] + 1, (c0, c)
    th, u, rho = h.get_population()
    e, ub, rb = h.history
    return dict(theta=th, u=u, rho=rho, ess=h.ess, eps=h.eps.copy(), counters=c, ubar=ub[-1].copy(), rhobar=rb[-1].copy(),
                eps_hist=e[-1].copy(), sigma=h.proposal_sigma)


def check_shard(O, ref, name, theta_all, u_all, rho_before, got, gid0, seed, it, survivor=None, where=""):
    """Step 4 for one shard: rows bit for bit, rho untouched, every draw against the weights, the ESS."""
    m = got["theta"].shape[1]
    idx = np.rint(got["theta"][0] / THETA_GRID).astype(np.int64)
    assert np.all((idx >= 0) & (idx < ref.n)), (name, idx.min(), idx.max())
    np.testing.assert_array_equal(got["theta"], theta_all[:, idx], err_msg=f"{name}{where}: theta rows")
    np.testing.assert_array_equal(got["u"], u_all[:, idx], err_msg=f"{name}{where}: u rows")
    np.testing.assert_array_equal(got["rho"], rho_before, err_msg=f"{name}{where}: rho moved")
    t = ref.targets(uniforms(O, seed, gid0, m, it))
    bad = ref.wrong(idx, t)
    if len(bad):
        i = bad[0]
        raise AssertionError(f"{name}{where}: {len(bad)} of {m} draws are wrong, first local particle {i} (gid {gid0 + i}, iteration "
                             f"{it}): drew {idx[i]} (w = {float(ref.w[idx[i]])!r}), t / total = {float(t[i] / ref.total)!r}, "
                             f"long double says {int(ref.exact(t[i:i + 1])[0])}, tol / total = {ref.rel_tol!r}")
    if name in SEPARATED:
        assert ref.min_share >= 1000 * ref.rel_tol, (name, ref.min_share, ref.rel_tol)
    assert ref.ambiguous(t) <= ref.ambiguous_allowed(m), (name, ref.ambiguous(t), ref.ambiguous_allowed(m))
    if survivor is not None:
        assert np.all(idx == survivor), (name, survivor, np.unique(idx))
        assert ref.ess == 1.0
    if "ess" in got:                       # (a caller that could not read the ESS of this resample leaves it out)
        assert abs(got["ess"] - ref.ess) <= 3 * ref.rel_tol * ref.ess, (name, got["ess"], ref.ess)
    return idx


def check_control(S, name, got_all, alg, d, theta_planted):
    """Step 5: what the control step behind the resample made of the resampled population (theta, u, rho: all shards).
    The covariance has the tolerance of tests/test_gpu_ecdf_paths.py, 1e-9 of its largest entry, plus the floor no one-pass
    sum can go below: a resample of ESS ~ 1 (the dynamic-range pattern at small n) returns n copies of one particle, whose
    exact covariance is 0, and sums of n terms (x - pivot)(y - pivot) about the planted population's mean carry
    n 2^-53 of n dev^2 each -- 4 n 2^-53 dev^2 after the subtraction and the division by n - 1, dev the planted theta's
    largest distance from its mean.  With a spread-out population the floor is 1e-4 of the relative term."""
    from tests import ecdf_ref as E
    th, u, rho = got_all["theta"], got_all["u"], got_all["rho"]
    assert len(E.mean_mismatch(got_all["ubar"], u, 1e-12)) == 0, (name, got_all["ubar"], [E.fsum_mean(x) for x in u])
    assert len(E.mean_mismatch(got_all["rhobar"], rho, 1e-10)) == 0, (name, got_all["rhobar"], [E.fsum_mean(x) for x in rho])
    if alg == "multi_eps":
        ubar = np.array([E.fsum_mean(x) for x in u])
        np.testing.assert_allclose(got_all["eps"], S.op_eps_multi(ubar, 1.0), rtol=1e-9, err_msg=name)
    else:
        np.testing.assert_allclose(got_all["eps"], [S.op_eps_single(E.fsum_mean(u), 1.0)], rtol=1e-9, err_msg=name)
    np.testing.assert_array_equal(got_all["eps_hist"], got_all["eps"])
    sig, want = got_all["sigma"], np.asarray(E.cov_ref(th, BETA), dtype=np.float64)
    dev = np.max(np.abs(theta_planted - theta_planted.mean(axis=1, keepdims=True)))
    floor = 4.0 * theta_planted.shape[1] * 2.0 ** -53 * dev * dev
    assert np.max(np.abs(sig - want)) <= 1e-9 * np.max(np.abs(sig)) + floor, (name, sig, want, floor)


def run_single_shard(h, S, O, seed, alg, rng, names=None):
    """The whole procedure on an initialised handle that holds the whole population; returns the names it ran."""
    d, s, n = h.d, h.s, h.n_local
    assert h.local_offset == 0 and n == h.cfg.n_particles
    theta = planted_theta(d, 0, n)
    ran = []
    for name, v, delta in plans(n, s, group_of(d, s), rng, names):
        u = v * SCALE
        assert u.min() > 2.0 ** -45
        ref = Reference(u, delta)
        _, _, rho0 = h.get_population()
        c0 = plant(h, theta, u)
        h.update(n_simulation=n, proposal=S.RandomWalk(β=BETA, n_para=d), resample=RESAMPLE_NOW, delta=delta)
        got = read_back(h, c0)
        survivor = int(np.argmin(v[0])) if name == "one survivor" else None
        check_shard(O, ref, name, theta, u, rho0, got, 0, seed, c0["n_population_updates"] + 1, survivor)
        if name in CONTROL_CHECKED:
            check_control(S, name, got, alg, d, theta)
        ran.append(name)
    return ran


# ---------------------------------------------------------------- two shards
def sharded_plans():
    """The survivor at every position, then the islands: (name, theta [1][n], u [1][n], delta, reference), made once."""
    n = N_ISLANDS
    rng = np.random.default_rng(62)
    theta = planted_theta(1, 0, n)
    out = []
    for name, v, delta in plans(n, 1, group_of(1, 1), rng, names=("one survivor", "islands")):
        u = v * SCALE
        out.append((name, theta, u, delta, Reference(u, delta)))
    assert len(out) == 9 and {p[3] for p in out} == {2000.0}
    return out


def check_shards(S, O, plans, records, seed):
    """records[rank][k]: (c0, offset, rho before, what read_back returned) of plan k.  Every shard's draws against the same
    global weights; the same counters and epsilon on both shards; the control step against the whole resampled population."""
    world = len(records)
    for k, (name, theta, u, delta, ref) in enumerate(plans):
        c0 = records[0][k][0]
        for rank in range(world):
            c, offset, rho0, got = records[rank][k]
            assert c == c0
            survivor = int(np.argmin(u[0])) if name == "one survivor" else None
            check_shard(O, ref, name, theta, u, rho0, got, offset, seed, c0["n_population_updates"] + 1, survivor,
                        where=f" (plan {k}, shard {rank})")
            assert got["counters"] == records[0][k][3]["counters"]
            np.testing.assert_array_equal(got["eps"], records[0][k][3]["eps"])
        assert sum(records[r][k][3]["theta"].shape[1] for r in range(world)) == ref.n
        if name in CONTROL_CHECKED:
            whole = dict(records[0][k][3])
            for key in ("theta", "u", "rho"):
                whole[key] = np.concatenate([records[r][k][3][key] for r in range(world)], axis=1)
            check_control(S, name, whole, "single_eps", 1, theta)
