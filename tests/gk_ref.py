"""The g-and-k simulator from its definition, in float64 NumPy, and the checker the device's order statistics are held to.
TEST INFRASTRUCTURE: no device, nothing taken from the kernels.

  x_i = A + B (1 + c tanh(g z_i / 2)) (1 + z_i^2)^k z_i,   i < n_draws,   theta = (A, B, g, k)
  rho_j = |x_(rank_j) - obs_j|   (1-based order statistics of the sorted data; a non-finite distance counts as 1e30)

The normals are the oracle's (glibc Box-Muller on the Philox stream): draw 2 b and 2 b + 1 of particle `pid` at iteration `it`
are the pair of block b of its simulation stream.  NaN data (B = 0 or 1 + c tanh = 0 times an overflowed (1 + z^2)^k) sort
last, as np.sort and the reference's `sort` put them: such an order statistic is a distance of 1e30."""
import numpy as np

PURPOSE_SIM = 1
MAX_DRAWS = 128
BIG = 1e30
# the project's bound for a device simulator against glibc normals (tests/test_gpu_parity.py::test_device_simulators_match_oracle):
# the table-driven log / sincos / exp / tanh of the device against libm, and nothing else
RTOL, ATOL = 1e-10, 1e-12

_normals = {}


def normals(seed, pid0, m, it):
    """[128][m]: the 128 simulation normals of particles pid0 .. pid0 + m - 1 at iteration `it` (cached: every rank group of a
    test reuses them; callers must not write into the result)."""
    key = (int(seed), int(pid0), int(m), int(it))
    if key not in _normals:
        from oracle import oracle as O
        O.build()
        L, z = O.lib(), np.zeros(2)
        zp = O._dp(z)
        out = np.empty((MAX_DRAWS, m))
        for i in range(m):
            for b in range(MAX_DRAWS // 2):
                L.orc_normal_pair(key[0], key[1] + i, PURPOSE_SIM, key[3], b, zp)
                out[2 * b, i], out[2 * b + 1, i] = z[0], z[1]
        out.setflags(write=False)
        _normals[key] = out
    return _normals[key]


def quantile(theta, c, z):
    """Q(z) for theta [4][m] and z [n][m] (left to right, as the definition is written: B = 0 times an overflow is NaN)."""
    A, B, g, k = (np.asarray(theta, dtype=np.float64)[j][None, :] for j in range(4))
    with np.errstate(over="ignore", invalid="ignore"):
        return A + B * (1.0 + c * np.tanh(g * z / 2.0)) * np.exp(k * np.log1p(z * z)) * z


def all_ranks(theta, n_draws, c, normals):
    """The sorted data [n_draws][m]; NaN last."""
    z = np.asarray(normals)[:n_draws]
    return np.sort(quantile(theta, c, z), axis=0)


def distance(x, obs):
    with np.errstate(invalid="ignore"):
        r = np.abs(x - obs)
    r[~np.isfinite(r)] = BIG
    return r


def expected(theta, n_draws, c, ranks, obs, normals):
    """rho [4][m]."""
    x = all_ranks(theta, n_draws, c, normals)
    idx = np.asarray(ranks, dtype=np.int64) - 1
    assert np.all(idx >= 0) and np.all(idx < n_draws), (ranks, n_draws)
    return distance(x[idx], np.asarray(obs, dtype=np.float64)[:, None])


CLASSES = ("ordinary", "B < 0", "k < 0", "B = 0", "overflow", "ordinary", "B < 0, overflow", "B = 0, overflow")


def theta_mix(m, seed=5):
    """theta [4][m]; particle i is of CLASSES[i % 8], so every wave of 64 holds all of them, side by side:
    ordinary         B > 0, k >= 0: the order statistics of the normals are mapped (c <= 0.83), A large against B so that
                     most of these particles have positive data throughout
    B < 0, k < 0     the data are sorted whatever c is
    B = 0            all data equal A: 128 ties
    overflow         k = 5000: (1 + z^2)^k overflows for |z| > 0.39, about 70 % of the data are +-inf
    B = 0, overflow  0 times inf: NaN data, which sort last"""
    rng = np.random.default_rng(seed)
    th = np.stack([rng.uniform(6.0, 10.0, m), rng.uniform(0.3, 1.2, m), rng.uniform(0.0, 4.0, m), rng.uniform(0.0, 0.6, m)])
    cls = np.arange(m) % 8
    th[1, (cls == 1) | (cls == 6)] *= -1.0
    th[3, cls == 2] = rng.uniform(-0.45, -0.05, int(np.sum(cls == 2)))
    th[1, (cls == 3) | (cls == 7)] = 0.0
    th[3, (cls == 4) | (cls == 6) | (cls == 7)] = 5000.0
    return th


def deviation(got, want):
    """|got - want| / (|want| + ATOL / RTOL): the relative deviation with |want| floored at 0.01; the bound is RTOL."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        dev = np.abs(got - want) / (np.abs(want) + ATOL / RTOL)
    dev[np.isnan(dev)] = np.inf              # a NaN where a number is due
    return dev


def assert_rho(got, want, where, sorted_data=None, ranks=None, obs=None):
    """|got - want| <= ATOL + RTOL |want| for rho [R][m]; returns the worst deviation().  With the sorted data
    (all_ranks), the ranks of the R rows and their obs, a failure names the order statistic that was taken instead."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    dev = deviation(got, want)
    bad = np.argwhere(dev > RTOL)
    if len(bad) == 0:
        return float(dev.max()) if dev.size else 0.0
    lines = [f"{where}: {len(bad)} of {got.size} distances off by more than rtol={RTOL:g}, atol={ATOL:g}"]
    for j, i in bad[:8]:
        line = f"  particle {i}, row {j}: got {got[j, i]!r}, want {want[j, i]!r}"
        if sorted_data is not None:
            n = sorted_data.shape[0]
            r = int(ranks[j])
            ob = float(np.broadcast_to(np.asarray(obs, dtype=np.float64), (len(ranks),))[j])
            col = sorted_data[:, i]
            near = {q: col[q - 1] for q in (r - 1, r, r + 1) if 1 <= q <= n}
            line += f" (rank {r} of {n}, obs {ob!r}; x_(q) around it: {near})"
            alt = distance(col.copy(), ob)
            same = [int(q) + 1 for q in np.flatnonzero(deviation(np.full(n, got[j, i]), alt) <= RTOL) if q + 1 != r]
            if same:
                line += f": that is the distance of rank {same[:6]}" + (" (a neighbour)" if r - 1 in same or r + 1 in same else "")
            else:
                line += ": the distance of no order statistic of this particle (garbage)"
        lines.append(line)
    raise AssertionError("\n".join(lines))


# ---- configurations Engine::validate() refuses: a rank outside 1..n_draws, a draw count outside 1..128, fractions, NaN ----
REFUSED = [
    ("rank 0", dict(n_draws=128, ranks=(0, 48, 80, 112))),
    ("rank n_draws + 1", dict(n_draws=100, ranks=(16, 32, 64, 101))),
    ("rank 129 of 128", dict(n_draws=128, ranks=(16, 48, 80, 129))),
    ("rank -1", dict(n_draws=128, ranks=(-1, 48, 80, 112))),
    ("no draws", dict(n_draws=0, ranks=(1, 1, 1, 1))),
    ("129 draws", dict(n_draws=129, ranks=(16, 48, 80, 112))),
    ("rank 16.5", dict(n_draws=128, ranks=(16.5, 48, 80, 112))),
    ("rank 128.5 of 128", dict(n_draws=128, ranks=(16, 48, 80, 128.5))),
    ("127.5 draws", dict(n_draws=127.5, ranks=(16, 48, 80, 112))),
    ("rank NaN", dict(n_draws=128, ranks=(16, 48, 80, float("nan")))),
    ("NaN draws", dict(n_draws=float("nan"), ranks=(16, 48, 80, 112))),
]


def raw_gk(S, n_draws, ranks, c=0.8, obs=(0.0, 0.0, 0.0, 0.0)):
    """A GandK whose parameters reach the C ABI as given (the Python class truncates them to integers first)."""
    model = S.GandK()
    model.n_draws, model.c, model.ranks, model.obs = n_draws, c, tuple(ranks), tuple(obs)
    return model


def check_refused(S, what, kw):
    import pytest
    with pytest.raises(S.SABCError) as e:
        h = S.SabcHandle(n_particles=64, model=raw_gk(S, **kw), prior=S.product_distribution([S.Uniform(0, 10)] * 4))
        h.close()
    assert e.value.code == -8 and "BAD_CONFIG" in str(e.value), (what, str(e.value))
