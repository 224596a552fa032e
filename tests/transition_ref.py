"""One population update (SimulatedAnnealingABC.jl:300-331, proposals.jl) restated particle by particle in NumPy long double, and
the checker, the cases and the procedure that tests/test_transition_reference.py (CPU engine) and
tests/test_gpu_transition_paths.py (device) share.

Nothing here calls the oracle's update, the handle's prior or any kernel.  What comes from outside is data: the population
before and after, epsilon, the ECDF tables, Sigma, the counters, the Philox words and normals of the particles' streams (the
generator has its own tests: test_generator_bits.py, test_elementary_functions.py) and a callable rho_of(theta, it) that gives
the distances of the shard's particles at `theta` -- the simulator, which has its own tests and is here only a function of
(theta, gid, it).

For particle i of a shard, gid = gid0 + i, at update index it = n_population_updates + 1 (the loop index ix of :294 counted
over the handle's life; the engine passes it as StepArgs::iter):

  proposal   RandomWalk: thp = theta + L z, L the lower Cholesky factor of Sigma (sqrt for d = 1) factored HERE in long double,
             z the first d normals of stream (seed, gid, PROP, it).  DifferentialEvolution: i1, i2 = mulhi64 of the word pairs
             (x, y), (z, w) of blocks a = 0, 1, .. of that stream with m_total, redrawn until distinct; gamma = p0 (1 + p1 z0),
             z0 the first normal of block 0 of PROP2; thp = theta + gamma (P[i1] - P[i2]).  StretchMove: partner from words
             (x, y) of block 0, U = u52(z, w), tt = (a - 1) U + 1, z = tt^2 / a, thp = p + z (theta - p), logf = (d - 1) log z.
  halves     a shard of n_local particles is updated as [0, h) then [h, n_local), h = n_local // 2 (engine.cpp:
             enqueue_update; RandomWalk takes the shard in one piece, which is the same update).  The partners of the first
             half batch are the second halves of ALL shards before the update, in rank order; those of the second half batch
             the first halves as the first half batch left them (Engine::partner_view: a full shard of cap particles gives
             cap // 2 and cap - cap // 2, the last one n_last // 2 and the rest).
  gate       lpp = log p(thp), lp = log p(theta) in long double (constants through mpmath); lpp = -inf: nothing is stored.
  distances  rp = rho_of(thp); up_j the plain search of ecdf_ref.cdf_ref in table j.
  decision   log_alpha = lpp - lp + sum_j (u_j - up_j) / eps_j + logf; accept iff log U < log_alpha, log U the exact log
             (mpmath) of u52(words x, y of block (seed, gid, ACCEPT, it, 0)).

The tolerances (derived; U = 2^-52, one ulp, is granted per binary64 operation -- twice a correctly rounded one, which
covers the device's division and square root, held to one ulp by test_elementary_functions.py):

  tol_theta  per component.  RandomWalk: the kernel's sum has k + 1 products and additions for row k, d + 1 at the most, fused
             or not: (d + 1) U (|theta_k| + sum_l |L_kl z_l|).  Its factor comes from a binary64 Cholesky factorisation of the
             Sigma read back: L^ L^' = Sigma + E, |E| <= (d + 1) U |L^||L^'| (Higham, Accuracy and Stability, thm 10.3), and
             ||L^ - L||_F <= cond_2(Sigma) ||E||_F / ||Sigma||_2 ||L||_F / sqrt 2 to first order (thm 10.8); with
             ||E||_F <= (d + 1) U d ||Sigma||_2 the term is cond d (d + 1) U ||L||_F ||z||_2.  The cases keep cond below 1e3.
             (d = 1: the factor is one square root, held to one ulp, which with the product and the sum stays inside 2 U of the
             magnitudes: U / 2 |thp| + 3 U / 2 |L z|.)
             DifferentialEvolution: three operations for gamma, three for theta + gamma (p1 - p2): 6 U (|theta_k| + |gamma (p1 -
             p2)_k|).  StretchMove: five for z, three for p + z (theta - p): 11 U (|p_k| + |z (theta - p)_k|).
  tol_alpha  per particle, the sum of
             - (s + 5) U M: the 2 s + 3 operations of the sum, M the sum of its terms' magnitudes;
             - sum_j dup_j / eps_j: dup_j = 2 ulp of 1 (what ecdf_ref.assert_u grants a lookup) plus the change of up_j over
               the image of tol_theta, estimated by simulating at thp -+ (tol_theta + one ulp of thp);
             - the log densities as the device evaluates them, log held to one ulp (the ROCm device library's documented bound
               for binary64 log; lgamma and erfc enter through constants computed once on the host, which cancel in lpp -
               lp up to the roundings counted here): 8 U of a family's terms (Normal, TruncNormal: z^2 / 2, log(2 pi) / 2, the
               constant; LogNormal: also log x, and U |z| |log x| / sigma for the log inside z; Gamma: 4 U of |(a - 1) log x|,
               x / b, the constant); MvNormal: forward substitution, (d + 2) U sum_k |y_k| (|L^-1||L||y|)_k, and (d + 1) U q /
               2; d U sum_k |l_k| for the product;
             - sum_k |d log p / d theta_k| tol_theta_k;
             - StretchMove: (d - 1) (9 U + U |log z|) + U |logf|: eight roundings in z, one ulp of the log, the product;
             - LOGU_ULPS = 3 ulp of log U: the proven bounds of the two spellings together, -0.5 neg2_log_tab (2.0 ulp, the
               worst region "near 1" of test_elementary_functions.CPU_BOUNDS; the device computes the restatement's bits) and
               log_fast (1.0 ulp, GPU_BOUNDS).  Each spelling is inside it, and so is their disagreement: this is the budget
               that lets host mode decide with log_fast.  tests/test_transition_reference.py holds both to it.
No constant in either is measured.

A particle is undecided when |log U - log_alpha| <= tol_alpha, or when a knot lies within the image of tol_theta around some
rp_j; it is not judged, everything about what was stored still is.  A case may have one undecided particle, none with
n <= 200.  (A tie planted by a test sets a particle's tolerance to zero: the rule `<` then rejects it.)

The engine recomputes RandomWalk's Sigma from a statistics pass at the entry of every update call (engine.cpp: update_loop,
update_proposal! of :284).  The procedure therefore runs a RandomWalk update call of zero simulations behind the planting: its
control step factors the Sigma of exactly this population, about the pivot the checked call then keeps, and the checked
call's own pass gives the same bits.  (A whole update in that place, with u planted again behind it, would have the checked
call centre its sums anew and factor a Sigma an ulp away from the one read back.)"""
import math
from types import SimpleNamespace

import numpy as np

from tests import ecdf_ref as E
from tests import elementary_ref as R

LD = np.longdouble
U = LD(2.0) ** -52
PURPOSE_PROP, PURPOSE_PROP2, PURPOSE_ACCEPT = 2, 3, 4
LOGU_ULPS = 3.0
NO_RESAMPLE = 1e15
Q = 64.0
MAX_COND = 1e3


def mpf_to_ld(v):
    hi = float(v)
    return LD(hi) + LD(float(v - R.mp().mpf(hi)))


LOG2PI = None


def log2pi():
    global LOG2PI
    if LOG2PI is None:
        LOG2PI = mpf_to_ld(R.mp().log(2 * R.mp().pi))
    return LOG2PI


# ---------------------------------------------------------------- shards and halves
class Layout:
    """make_shard (sabc_types.hpp): contiguous blocks of cap = ceil(n / world) global ids per rank; the halves of
    Engine::partner_view and enqueue_update."""

    def __init__(self, n_global, world=1):
        self.n, self.world = int(n_global), int(world)
        self.cap = -(-self.n // self.world)
        self.sizes = [max(0, min(self.n, (r + 1) * self.cap) - r * self.cap) for r in range(self.world)]

    def offset(self, rank):
        return rank * self.cap

    def half(self, rank):
        return self.sizes[rank] // 2

    def pool(self, thetas, inactive_half):
        """The partners [d][m_total] of the half batch whose inactive half is `inactive_half`, in rank order."""
        parts = [th[:, self.half(r):] if inactive_half == 1 else th[:, :self.half(r)] for r, th in enumerate(thetas)]
        return np.concatenate(parts, axis=1)


# ---------------------------------------------------------------- streams
class Streams:
    """The Philox words and the normal pairs of the streams (seed, gid0 + i, purpose, it, k), i < n.  The words come from the
    oracle's Philox (integers: exact); normal_pairs(purpose, it, k) -> [n][2] is the oracle's pair on the CPU and
    op_normal_pairs on the device."""

    def __init__(self, O, seed, gid0, n, normal_pairs=None):
        self.O, self.seed, self.gid0, self.n = O, int(seed), int(gid0), int(n)
        self._pairs = normal_pairs
        self._cache = {}

    def blocks(self, purpose, it, k):
        key = ("b", purpose, it, k)
        if key not in self._cache:
            self._cache[key] = [self.O.stream_block(self.seed, self.gid0 + i, purpose, int(it), int(k)) for i in range(self.n)]
        return self._cache[key]

    def normals(self, purpose, it, k):
        key = ("n", purpose, it, k)
        if key not in self._cache:
            if self._pairs is not None:
                z = np.asarray(self._pairs(purpose, int(it), int(k)), dtype=np.float64)
            else:
                z = np.array([self.O.normal_pair(self.seed, self.gid0 + i, purpose, int(it), int(k)) for i in range(self.n)])
            assert z.shape == (self.n, 2)
            self._cache[key] = z
        return self._cache[key]


def mulhi64(hi, lo, m):
    return (((int(hi) << 32) | int(lo)) * int(m)) >> 64


# ---------------------------------------------------------------- the prior, as data
class Prior:
    """dims: one tuple per parameter -- ("N", mu, sd), ("U", a, b), ("T", mu, sd, lo, hi), ("G", shape, scale), ("L", mu, sd) --
    or mv = (mu, chol): MvNormal(mu, chol chol'), chol the lower factor the handle is given (prior_chol)."""

    def __init__(self, dims=None, mv=None):
        self.dims, self.mv = dims, mv
        self.d = len(dims) if dims is not None else len(mv[0])
        c = R.mp()
        self.lc = []
        for p in dims or []:
            k = p[0]
            if k in ("N", "L"):
                v = c.log(c.mpf(p[2]))
            elif k == "U":
                v = c.log(c.mpf(p[2]) - c.mpf(p[1]))
            elif k == "T":
                mu, sd, lo, hi = (c.mpf(x) for x in p[1:5])
                cdf = lambda x: c.erfc(-(x - mu) / sd / c.sqrt(2)) / 2
                v = c.log(sd) + c.log(cdf(hi) - cdf(lo))
            elif k == "G":
                v = c.loggamma(c.mpf(p[1])) + c.mpf(p[1]) * c.log(c.mpf(p[2]))
            else:
                raise KeyError(k)
            self.lc.append(mpf_to_ld(v))
        if mv is not None:
            L = np.asarray(mv[1], dtype=np.float64)
            assert np.all(np.triu(L, 1) == 0)
            self.L = L.astype(LD)
            self.mu = np.asarray(mv[0], dtype=np.float64).astype(LD)
            self.logc = LD(self.d) / 2 * log2pi() + np.sum(np.log(np.diag(self.L)))
            Linv = np.linalg.inv(L).astype(LD)             # (only weighs an error bound)
            self.M = np.abs(Linv) @ np.abs(self.L)
            self.LinvT = Linv.T

    def make(self, S):
        if self.mv is not None:
            L = np.asarray(self.mv[1], dtype=np.float64)
            p = S.MvNormal(self.mv[0], L @ L.T)
            p.chol = L                                       # the factor itself is the datum
            return p
        mk = {"N": lambda a, b: S.Normal(a, b), "U": lambda a, b: S.Uniform(a, b), "L": lambda a, b: S.LogNormal(a, b),
              "G": lambda a, b: S.Gamma(a, b), "T": lambda a, b, lo, hi: S.truncated(S.Normal(a, b), lo, hi)}
        comps = [mk[p[0]](*p[1:]) for p in self.dims]
        return comps[0] if len(comps) == 1 else S.product_distribution(comps)

    def logpdf(self, th):
        """th long double [d][m] -> (log p [m], -inf outside the support; the device's evaluation error [m]; |d log p / d
        theta| [d][m]), all long double."""
        th = np.asarray(th, dtype=LD)
        d, m = th.shape
        if self.mv is not None:
            y = np.zeros((d, m), dtype=LD)
            for k in range(d):
                r = th[k] - self.mu[k]
                for l in range(k):
                    r = r - self.L[k, l] * y[l]
                y[k] = r / self.L[k, k]
            q = np.sum(y * y, axis=0)
            lp = -q / 2 - self.logc
            err = (d + 2) * U * np.sum(np.abs(y) * (self.M @ np.abs(y)), axis=0) + (d + 1) * U * q / 2 + 2 * U * abs(self.logc)
            return lp, err, np.abs(self.LinvT @ y)
        lp, err, grad, mag = np.zeros(m, dtype=LD), np.zeros(m, dtype=LD), np.zeros((d, m), dtype=LD), np.zeros(m, dtype=LD)
        inside = np.ones(m, dtype=bool)
        half = log2pi() / 2
        with np.errstate(invalid="ignore", divide="ignore"):
            for k, p in enumerate(self.dims):
                x, kind, lc = th[k], p[0], self.lc[k]
                a, b = LD(p[1]), LD(p[2])
                if kind in ("N", "T"):
                    z = (x - a) / b
                    l = -(z * z) / 2 - half - lc
                    e = 8 * U * (z * z / 2 + half + abs(lc))
                    g = np.abs(z) / b
                    ok = np.ones(m, dtype=bool) if kind == "N" else (x >= LD(p[3])) & (x <= LD(p[4]))
                elif kind == "U":
                    ok = (x >= a) & (x <= b)
                    l, e, g = np.full(m, -lc), np.zeros(m, dtype=LD), np.zeros(m, dtype=LD)
                elif kind == "L":
                    ok = x > 0
                    lx = np.log(np.where(ok, x, LD(1)))
                    z = (lx - a) / b
                    l = -(z * z) / 2 - half - lc - lx
                    e = 8 * U * (z * z / 2 + half + abs(lc) + np.abs(lx)) + U * np.abs(z) * np.abs(lx) / b
                    g = np.abs(z / b + 1) / np.where(ok, x, LD(1))
                elif kind == "G":
                    ok = x > 0
                    xs = np.where(ok, x, LD(1))
                    lx = np.log(xs)
                    l = (a - 1) * lx - xs / b - lc
                    e = 4 * U * (np.abs((a - 1) * lx) + xs / b + abs(lc))
                    g = np.abs((a - 1) / xs - 1 / b)
                inside &= ok
                lp, err, mag = lp + np.where(ok, l, 0), err + np.where(ok, e, 0), mag + np.where(ok, np.abs(l), 0)
                grad[k] = np.where(ok, g, 0)
        err = err + d * U * mag
        return np.where(inside, lp, -np.inf), np.where(inside, err, 0), np.where(inside[None, :], grad, 0)


# ---------------------------------------------------------------- the restatement
def chol_ld(sigma):
    """Lower Cholesky factor in long double (sqrt for d = 1)."""
    A = np.asarray(sigma, dtype=np.float64).astype(LD)
    d = A.shape[0]
    L = np.zeros((d, d), dtype=LD)
    for k in range(d):
        for l in range(k + 1):
            v = A[k, l] - np.sum(L[k, :l] * L[l, :l])
            L[k, l] = np.sqrt(v) if k == l else v / L[l, l]
    return L


def exact_log(x):
    return np.array([mpf_to_ld(R.exact("log_fast", float(v))) for v in x], dtype=LD)


def accept_uniforms(streams, it, words=(0, 1)):
    return np.array([R.u52(b[words[0]], b[words[1]]) for b in streams.blocks(PURPOSE_ACCEPT, it, 0)])


def _half_batch(inp, idx, pool, mut):
    """The restatement for the local particles idx, whose partners are the columns of pool."""
    kind, p0, p1 = inp.prop
    th0 = inp.theta0s[inp.rank]
    d, n = th0.shape
    s = inp.u0.shape[0]
    m = len(idx)
    th = th0[:, idx].astype(LD)
    st, it = inp.streams, inp.it
    logf = np.zeros(m, dtype=LD)
    tlogf = np.zeros(m, dtype=LD)
    out = SimpleNamespace(collided=np.zeros(m, dtype=bool))
    if kind == "rw":
        L = chol_ld(inp.sigma)
        cond = float(np.linalg.cond(np.asarray(inp.sigma, dtype=np.float64))) if d > 1 else 1.0
        out.cond = cond
        if "LT" in mut:
            L = L.T.copy()
        purpose = PURPOSE_PROP2 if "purpose" in mut else PURPOSE_PROP
        zit = it + 1 if "it+1" in mut else it
        z = np.concatenate([st.normals(purpose, zit, k)[idx].T for k in range((d + 1) // 2)], axis=0)[:d].astype(LD)
        step = np.abs(L)[:, :, None] * np.abs(z)[None, :, :]                       # |L_kl z_l|
        thp = th + np.einsum("kl,lm->km", L, z)
        frob = np.sqrt(np.sum(L * L))
        tol = (d + 1) * U * (np.abs(th) + step.sum(axis=1))
        if d > 1:
            tol = tol + LD(cond) * d * (d + 1) * U * frob * np.sqrt(np.sum(z * z, axis=0))[None, :]
    elif kind == "de":
        mt = pool.shape[1]
        i1, i2 = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
        for q, i in enumerate(idx):
            a = 0
            while True:
                w = st.blocks(PURPOSE_PROP, it, a)[i]
                i1[q], i2[q] = mulhi64(w[0], w[1], mt), mulhi64(w[2], w[3], mt)
                if i1[q] != i2[q] or a > 64:
                    break
                a += 1
            out.collided[q] = a > 0
        z0 = st.normals(PURPOSE_PROP2, it, 0)[idx, 0].astype(LD)
        gamma = LD(p0) * (1 + LD(p1) * z0) if "gamma" not in mut else np.full(m, LD(p0))
        diff = gamma[None, :] * (pool[:, i1].astype(LD) - pool[:, i2].astype(LD))
        thp = th + diff
        tol = 6 * U * (np.abs(th) + np.abs(diff))
        out.i1, out.i2 = i1, i2
    elif kind == "stretch":
        mt = pool.shape[1]
        w = [st.blocks(PURPOSE_PROP, it, 0)[i] for i in idx]
        ip = np.array([mulhi64(b[0], b[1], mt) for b in w], dtype=np.int64)
        Uu = np.array([R.u52(b[2], b[3]) for b in w]).astype(LD)
        a = LD(p0)
        tt = (a - 1) * Uu + 1
        z = tt * tt / a
        p = pool[:, ip].astype(LD)
        move = z[None, :] * (th - p)
        thp = p + move
        tol = 11 * U * (np.abs(p) + np.abs(move))
        logf = np.log(z) * (d if "logf_d" in mut else d - 1)
        tlogf = (d - 1) * (9 * U + U * np.abs(np.log(z))) + U * np.abs(logf)
        out.i1 = ip
    else:
        raise KeyError(kind)
    out.thp, out.tol_theta, out.logf, out.tlogf = thp, tol, logf, tlogf
    return out


def restate(inp, mut=(), ties=()):
    """The reference's quantities for every local particle.  inp.theta1s = None: the after-population is the reference's own
    (first half batch, then the second on what the first left) -- what the mutation tests build their populations from.
    mut names the deliberate errors of tests/test_transition_reference.py; ties: local particles whose log_alpha is set to
    their log U with no tolerance."""
    mut = set(mut)
    kind = inp.prop[0]
    lay, rank = inp.layout, inp.rank
    th0 = inp.theta0s[rank]
    d, n = th0.shape
    s = inp.u0.shape[0]
    h = lay.half(rank)
    assert n == lay.sizes[rank]
    synth = inp.theta1s is None
    assert not synth or lay.world == 1
    ref = SimpleNamespace(n=n, d=d, s=s, h=h, kind=kind)
    for name, shape in (("thp", (d, n)), ("tol_theta", (d, n)), ("logf", n), ("tlogf", n)):
        setattr(ref, name, np.zeros(shape, dtype=LD))
    ref.collided = np.zeros(n, dtype=bool)
    ref.partner = np.full((2, n), -1, dtype=np.int64)
    P1 = SimpleNamespace(theta=th0.copy(), u=inp.u0.copy(), rho=inp.rho0.copy())
    batches = [np.arange(n)] if kind == "rw" else [np.arange(0, h), np.arange(h, n)]
    for b, idx in enumerate(batches):
        pool = None
        if kind != "rw":
            inactive = 1 - b
            if "active" in mut:
                inactive = b
            if b == 0 or "stale" in mut:
                pool = lay.pool(inp.theta0s, inactive)
            else:
                pool = lay.pool([P1.theta] if synth else inp.theta1s, inactive)
        hb = _half_batch(inp, idx, pool, mut)
        ref.thp[:, idx], ref.tol_theta[:, idx], ref.logf[idx], ref.tlogf[idx] = hb.thp, hb.tol_theta, hb.logf, hb.tlogf
        ref.collided[idx] = hb.collided
        if hasattr(hb, "i1"):
            ref.partner[0, idx] = hb.i1
        if hasattr(hb, "i2"):
            ref.partner[1, idx] = hb.i2
        if hasattr(hb, "cond"):
            ref.cond = hb.cond
        _decide(inp, ref, idx, mut, ties)
        if synth:
            acc = idx[ref.decision[idx] > 0]
            P1.theta[:, acc], P1.u[:, acc], P1.rho[:, acc] = ref.thp64[:, acc], ref.up[:, acc], ref.rp[:, acc]
    ref.P1 = P1 if synth else None
    return ref


def _decide(inp, ref, idx, mut, ties):
    """Gate, distances, ECDF, log_alpha, log U, tol_alpha and the decision (+1 accept, -1 reject, 0 undecided) for idx."""
    d, n, s = ref.d, ref.n, ref.s
    if not hasattr(ref, "decision"):
        for name in ("lpp", "lp", "log_alpha", "logU", "tol_alpha"):
            setattr(ref, name, np.zeros(n, dtype=LD))
        ref.thp64, ref.rp, ref.up = np.zeros((d, n)), np.zeros((s, n)), np.zeros((s, n))
        ref.decision = np.zeros(n, dtype=np.int64)
        ref.knot_near = np.zeros(n, dtype=bool)
        ref.outside = np.zeros(n, dtype=bool)
        # log U of every local particle, once
        words = (2, 3) if "accept_zw" in mut else (0, 1)
        ref.uacc = accept_uniforms(inp.streams, inp.it, words)
        ref.logU[:] = exact_log(ref.uacc)
    th0 = inp.theta0s[inp.rank]
    thp = ref.thp[:, idx]
    lpp, epp, gpp = inp.prior.logpdf(thp)
    lp, ep, _ = inp.prior.logpdf(th0[:, idx].astype(LD))
    assert np.all(np.isfinite(lp.astype(np.float64))), "a planted particle lies outside the prior's support"
    # the distances at the proposal rounded to binary64, and over the image of tol_theta (+ the rounding just made)
    full = th0.copy()
    full[:, idx] = thp.astype(np.float64)
    delta = np.zeros_like(full)
    delta[:, idx] = (ref.tol_theta[:, idx] + np.spacing(np.abs(full[:, idx]))).astype(np.float64)
    rp = inp.rho_of(full, inp.it)
    r_lo, r_hi = inp.rho_of(full - delta, inp.it), inp.rho_of(full + delta, inp.it)
    eps = np.asarray(inp.eps, dtype=np.float64)
    a = np.zeros(len(idx), dtype=LD)
    mag = np.zeros(len(idx), dtype=LD)
    tu = np.zeros(len(idx), dtype=LD)
    knot = np.zeros(len(idx), dtype=bool)
    up_all = np.zeros((s, len(idx)))
    with np.errstate(invalid="ignore"):
        for j in range(s):
            T = inp.tables[j]
            r = rp[j, idx]
            drp = np.maximum(np.abs(r_lo[j, idx] - r), np.abs(r_hi[j, idx] - r)) + 4 * np.spacing(np.abs(r))
            drp = np.where(np.isfinite(drp), drp, 0.0)
            up = E.cdf_ref(T, r)
            lo, hi = E.cdf_ref(T, np.maximum(r - drp, 0.0)), E.cdf_ref(T, r + drp)
            dup = np.maximum(hi - up, up - lo) + E.U_TOL
            knot |= np.searchsorted(T, r - drp, side="left") != np.searchsorted(T, r + drp, side="right")
            e = LD(eps[0] if len(eps) == 1 or "eps0" in mut else eps[j])
            term = (inp.u0[j, idx].astype(LD) - up.astype(LD)) / e
            if "u_swapped" in mut:
                term = -term
            a, mag, tu = a + term, mag + np.abs(term), tu + dup.astype(LD) / abs(e)
            up_all[j] = up
    inside = np.isfinite(lpp.astype(np.float64))
    dl = np.where(inside, lpp, 0) - lp
    if "lp_swapped" in mut:
        dl = -dl
    la = dl + a + ref.logf[idx]
    M = np.abs(np.where(inside, lpp, 0)) + np.abs(lp) + mag + np.abs(ref.logf[idx])
    logU = ref.logU[idx]
    tol = ((s + 5) * U * M + tu + epp + ep + np.sum(gpp * ref.tol_theta[:, idx], axis=0) + ref.tlogf[idx]
           + LOGU_ULPS * np.spacing(np.abs(logU).astype(np.float64)).astype(LD))
    la = np.where(inside, la, -np.inf)
    for q, i in enumerate(idx):
        if i in ties:
            la[q], tol[q], knot[q] = logU[q], 0, False
    undecided = inside & (((np.abs(logU - la) <= tol) & (tol > 0)) | knot)
    dec = np.where(undecided, 0, np.where(logU < la, 1, -1))
    ref.lpp[idx], ref.lp[idx], ref.log_alpha[idx], ref.tol_alpha[idx] = lpp, lp, la, tol
    ref.thp64[:, idx], ref.rp[:, idx], ref.up[:, idx] = full[:, idx], rp[:, idx], up_all
    ref.decision[idx], ref.knot_near[idx], ref.outside[idx] = dec, knot & inside, ~inside


# ---------------------------------------------------------------- the checker
CATEGORIES = ("theta", "rho", "u", "support", "decision", "store")


def check(inp, P1, ref=None, ties=()):
    """Judge the after-population P1 = (theta, u, rho) of shard inp.rank.  Returns a report: bad[c] the local particles that
    fail assertion c, accepted (theta changed), undecided, theta_ratio = max |theta_new - thp| / tol_theta over the accepted,
    margin = min |log U - log_alpha| / tol_alpha over the judged."""
    th1, u1, rho1 = (np.asarray(x, dtype=np.float64) for x in P1)
    th0, u0, rho0 = inp.theta0s[inp.rank], inp.u0, inp.rho0
    ref = ref or restate(inp, ties=ties)
    n, s = ref.n, ref.s
    changed = np.any(th1 != th0, axis=0)
    bad = {c: np.zeros(n, dtype=bool) for c in CATEGORIES}
    with np.errstate(invalid="ignore"):
        ratio = np.abs(th1.astype(LD) - ref.thp) / ref.tol_theta
    bad["theta"] = changed & ~np.all(ratio <= 1, axis=0)
    rho_again = inp.rho_of(th1, inp.it)
    bad["rho"] = changed & ~np.all(rho1 == rho_again, axis=0)
    for j in range(s):
        miss = np.zeros(n, dtype=bool)
        miss[E.u_mismatch(inp.tables[j], rho1[j], u1[j])] = True
        bad["u"] |= changed & miss
    bad["support"] = changed & ref.outside
    bad["decision"] = (changed & (ref.decision < 0) & ~ref.outside) | (~changed & (ref.decision > 0))
    bad["store"] = ~changed & (np.any(u1 != u0, axis=0) | np.any(rho1 != rho0, axis=0))
    judged = ref.decision != 0
    inside = ~ref.outside
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.abs(ref.logU - ref.log_alpha) / ref.tol_alpha
    m = margin[judged & inside & (ref.tol_alpha > 0)]
    rep = SimpleNamespace(bad=bad, accepted=changed, undecided=np.nonzero(ref.decision == 0)[0], ref=ref, n=n,
                          theta_ratio=float(ratio[:, changed & ~bad["theta"]].max()) if np.any(changed & ~bad["theta"]) else 0.0,
                          margin=float(m.min()) if len(m) else math.inf)
    rep.any_bad = np.zeros(n, dtype=bool)
    for c in CATEGORIES:
        rep.any_bad |= bad[c]
    return rep


def assert_ok(rep, name=""):
    """Every assertion of the checker, and the cap on the undecided."""
    ref = rep.ref
    for c in CATEGORIES:
        w = np.nonzero(rep.bad[c])[0]
        if len(w):
            i = w[0]
            raise AssertionError(
                f"{name}: {len(w)} of {rep.n} particles fail '{c}', first local particle {i}: decision {ref.decision[i]}, "
                f"log U - log_alpha = {float(ref.logU[i] - ref.log_alpha[i])!r}, tol_alpha = {float(ref.tol_alpha[i])!r}, "
                f"outside = {bool(ref.outside[i])}, thp = {ref.thp[:, i].astype(np.float64)!r}, "
                f"tol_theta = {ref.tol_theta[:, i].astype(np.float64)!r}")
    cap = 0 if rep.n <= 200 else 1
    assert len(rep.undecided) <= cap, (name, "undecided particles", rep.undecided[:8], cap)


def premises(case, ref):
    """What makes the checks bite, asserted on the reference's side."""
    frac = float(np.mean(ref.decision > 0))
    assert 0.2 <= frac <= 0.8, (case.name, "accepted fraction", frac)
    if case.edge:
        assert np.mean(ref.outside) >= 0.05, (case.name, "outside the support", float(np.mean(ref.outside)))
    if getattr(ref, "cond", None) is not None:
        assert ref.cond < MAX_COND, (case.name, ref.cond)
    if case.collide:
        assert ref.collided.any(), (case.name, "no first partner draw collided")


# ---------------------------------------------------------------- the cases
class Case:
    """name; (d, s); n; prop = (kind, p0, p1); alg; prior; lo / hi: the boxes [2][d] of the two halves of P0; eps; the
    table length per statistic is min(n + 2, 600) - 7 j % 5 ("spread" tables: this test is about decisions, not ties)."""

    def __init__(self, name, d, s, n, prop, alg, prior, lo, hi, eps, seed=1, edge=False, collide=False, **extra):
        self.name, self.d, self.s, self.n, self.prop, self.alg, self.prior = name, d, s, n, prop, alg, prior
        self.lo, self.hi = np.asarray(lo, dtype=np.float64).reshape(2, d), np.asarray(hi, dtype=np.float64).reshape(2, d)
        self.eps = np.asarray(eps, dtype=np.float64)
        self.seed, self.edge, self.collide = seed, edge, collide
        self.extra = extra
        assert len(self.eps) == (s if alg == "multi_eps" else 1)
        if alg == "multi_eps" and s > 1:
            e = np.sort(self.eps)
            assert np.all(e[1:] / e[:-1] >= 3.0), "the epsilons of a multi-eps case differ pairwise by a factor of 3"

    def proposal(self, S):
        kind, p0, p1 = self.prop
        if kind == "rw":
            return S.RandomWalk(β=p0, n_para=self.d)
        if kind == "de":
            return S.DifferentialEvolution(γ0=p0, σ_gamma=p1)
        return S.StretchMove(a=p0)


def ladder(s, first=0.3, ratio=3.2):
    return [first * ratio ** j for j in range(s)]


def plant(case, layout, rng):
    """theta [d][n] of the whole population -- every shard's first half from the first box, its second from the second --, u
    spread over (0, 1)."""
    th = np.empty((case.d, layout.n))
    for r in range(layout.world):
        o, m, h = layout.offset(r), layout.sizes[r], layout.half(r)
        for b, (lo, hi) in enumerate(((o, o + h), (o + h, o + m))):
            th[:, lo:hi] = case.lo[b][:, None] + (case.hi[b] - case.lo[b])[:, None] * rng.uniform(0.0, 1.0, (case.d, hi - lo))
    u = rng.uniform(0.02, 0.98, (case.s, layout.n))
    return th, u


def tables_for(case, pool, rng):
    out = []
    for j in range(case.s):
        length = min(case.n + 2, 600) - (7 * j) % 5
        out.append(E.make_table(length, pool[j], Q, "spread", rng))
    return out


# ---------------------------------------------------------------- the procedure
def planted(case, layout):
    return plant(case, layout, np.random.default_rng(case.seed))


def prepare(h, S, case, layout, theta_all, u_all, pool_all):
    """Steps 1-6 on an initialised handle: the tables (from pool_all [s][n], distances of the whole planted population, which
    also serve as rho before), P0, epsilon, (RandomWalk) the Sigma of this population; reads P0, Sigma, epsilon and the
    counters back.  Returns what `inputs` needs of this shard."""
    lo, m = h.local_offset, h.n_local
    assert lo == layout.offset(h.cfg.rank) and m == layout.sizes[h.cfg.rank]
    tables = tables_for(case, pool_all, np.random.default_rng(case.seed + 1))
    for j, T in enumerate(tables):
        h.set_cdf_knots(j, T)
    h.set_population(theta=theta_all[:, lo:lo + m], u=u_all[:, lo:lo + m], rho=pool_all[:, lo:lo + m])
    h.set_eps(case.eps)
    if case.prop[0] == "rw":
        h.update(n_simulation=0, proposal=case.proposal(S), resample=NO_RESAMPLE)
    th0, u0, rho0 = h.get_population()
    np.testing.assert_array_equal(th0, theta_all[:, lo:lo + m])
    np.testing.assert_array_equal(u0, u_all[:, lo:lo + m])
    np.testing.assert_array_equal(h.eps, case.eps)
    for j, T in enumerate(tables):
        np.testing.assert_array_equal(h.cdf_knots(j), T)
    return SimpleNamespace(theta0=th0, u0=u0, rho0=rho0, tables=tables, sigma=h.proposal_sigma.copy(), eps=h.eps.copy(),
                           counters=h.counters, gid0=lo)


def inputs(case, layout, rank, before, theta0s, theta1s, streams, rho_of):
    return SimpleNamespace(layout=layout, rank=rank, theta0s=theta0s, theta1s=theta1s, u0=before.u0, rho0=before.rho0,
                           eps=before.eps, tables=before.tables, sigma=before.sigma, seed=streams.seed,
                           it=before.counters["n_population_updates"] + 1, prop=case.prop, prior=case.prior, streams=streams,
                           rho_of=rho_of)


def run_single_shard(h, S, O, case, seed, rho_of, normal_pairs=None):
    """The whole procedure on an initialised handle that holds the whole population: returns the checker's report."""
    layout = Layout(case.n, 1)
    theta_all, u_all = planted(case, layout)
    before = prepare(h, S, case, layout, theta_all, u_all, np.abs(rho_of(theta_all, 1)))
    h.update(n_simulation=case.n, proposal=case.proposal(S), resample=NO_RESAMPLE)
    P1 = h.get_population()
    c1 = h.counters
    assert c1["n_population_updates"] == before.counters["n_population_updates"] + 1
    assert c1["n_resampling"] == before.counters["n_resampling"]
    streams = Streams(O, seed, 0, case.n, normal_pairs)
    inp = inputs(case, layout, 0, before, [before.theta0], [P1[0]], streams, rho_of)
    rep = check(inp, P1)
    premises(case, rep.ref)
    assert_ok(rep, case.name)
    assert c1["n_accept"] - before.counters["n_accept"] == int(rep.accepted.sum()), (case.name, c1, before.counters)
    return rep
