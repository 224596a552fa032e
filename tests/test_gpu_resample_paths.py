"""Every resample path's draws against the weights themselves (tests/resample_ref.py: long double, no oracle run, nothing of
the kernels' chunks, lines, guide or fallback), on populations planted to break them: one surviving particle at the edges of
lines and chunks, islands of weight across a chunk boundary with whole weightless chunks and a weightless tail between them
(the `walked > 8` bisection of packed_search), weights halving every 8 particles (the backward walk), 260 decades of dynamic
range, equal weights, and the smooth weights of production.

Per case one handle per population size (5, 70, 1023, 1025, 4163 and 6211 for the islands), per pattern: plant theta (row 0 =
gid 2^-13, decodable) and u = v 2^-30, epsilon = 1e-300, n_accept = 1; one update with resample = 1e-9 -- the update accepts
nothing (asserted), exactly one resample runs (asserted); then theta and u must be the planted columns of the decoded indices
bit for bit, rho untouched, EVERY draw must satisfy the criterion, the ESS must be the reference's, and the history row,
epsilon and the RandomWalk covariance the control step behind the resample produced must belong to the population read back.
tests/test_resample_reference.py runs the same function on the CPU engine and shows the criterion refuses a neighbour.

The cases (path as dispatched by kernels.hip: launch_resample_local and engine.cpp: Engine::resample; SABC_PERSISTENT=0), with
the seconds each took on an MI355X (the run-time compiler's share included; the first case also pays for the Philox blocks
all cases share, tests/resample_ref.py: uniforms):
  stats-pg4       0.5 s  GaussianIID (1,1), single-eps     k_resample_gather_stats, 4 particles per line
  stats-pg2       0.1 s  Gaussian2D (2,3), multi-eps       k_resample_gather_stats, 2 per line
  stats-pg1       0.1 s  GandK (4,4), single-eps           k_resample_gather_stats, 1 per line
  packed-src-1x1  0.7 s  DeviceSource (1,1), single-eps    k_resample_gather_packed, pg = 4
  packed-src-2x3  1.1 s  DeviceSource (2,3), multi-eps     k_resample_gather_packed, pg = 2
  packed-src-5x5  2.1 s  DeviceSource (5,5), single-eps    k_resample_gather_packed, pg = 1
  packed-host-2x2 0.1 s  HostDistance (2,2), multi-eps     k_resample_gather_packed, pg = 2
  unpacked-8x8    3.1 s  DeviceSource (8,8), multi-eps     k_resample_gather<true> + resample_search (d + s > 15)
  two shards in one process, n = 6211, GaussianIID (1,1), the islands and the survivor at every position:
    peer to peer  0.3 s  k_scan_sums unfused with parked weights, k_scan_final with w_in_cum, rows read through split_index
                         from their owner's memory
    loopback      0.2 s  k_resample_gather<false>, k_bucket_count, k_bucket_scatter, k_resample_serve, k_resample_scatter
                         over tests/loopback_collectives.py with its alltoallv"""
import threading

import numpy as np
import pytest

from tests import resample_ref as R

pytestmark = pytest.mark.gpu

SEED = 11

# statistic j from parameters j % d and (j + 1) % d, continuous (a distance of exactly 0 would be u = 0: an accepted proposal)
SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const int d = (int)p[0], s = (int)p[1];
  for (int j = 0; j < s; ++j) {
    const double z = rng.next();
    rho[j] = fabs(theta[j % d] + 0.5 * theta[(j + 1) % d] + p[2] * z - 0.3 * ((j % 5) - 2)) + 1e-6;
  }
}
"""


def host_fdist(theta):
    th = np.atleast_2d(theta)
    z = np.random.default_rng(int(abs(th[0, 0]) * 1e6) & 0xFFFF).normal(size=(len(th), 2))
    r0 = np.abs(th[:, 0] + 0.5 * th[:, 1] + 0.4 * z[:, 0] - 0.3) + 1e-6
    r1 = np.abs(th[:, 1] - 0.5 * th[:, 0] + 0.4 * z[:, 1] + 0.2) + 1e-6
    return np.stack([r0, r1], axis=1)


def make_handle(S, kind, d, s, n, alg, **kw):
    if kind in ("gauss1", "gauss2d", "gk"):
        return R.builtin_handle(S.SabcHandle, S, kind, n, alg, SEED, **kw)
    a = S._lib.ALG_MULTI_EPS if alg == "multi_eps" else S._lib.ALG_SINGLE_EPS
    if kind == "host":
        model = S.HostDistance(host_fdist, s, d, False, batched=True)
    else:
        model = S.DeviceSource(SRC, d, s, [d, s, 0.4])
    return S.SabcHandle(n_particles=n, model=model, prior=R.flat_box(S, d), seed=SEED, algorithm=a, **kw)


# (id, kind, d, s, algorithm)
CASES = [
    ("stats-pg4", "gauss1", 1, 1, "single_eps"),
    ("stats-pg2", "gauss2d", 2, 3, "multi_eps"),
    ("stats-pg1", "gk", 4, 4, "single_eps"),
    ("packed-src-1x1", "src", 1, 1, "single_eps"),
    ("packed-src-2x3", "src", 2, 3, "multi_eps"),
    ("packed-src-5x5", "src", 5, 5, "single_eps"),
    ("packed-host-2x2", "host", 2, 2, "multi_eps"),
    ("unpacked-8x8", "src", 8, 8, "multi_eps"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_draw_of_every_pattern_on_every_resample_path(S, O, gpu, monkeypatch, case):
    name, kind, d, s, alg = case
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    assert R.group_of(d, s) == {"stats-pg4": 4, "stats-pg2": 2, "stats-pg1": 1, "packed-src-1x1": 4, "packed-src-2x3": 2,
                                "packed-src-5x5": 1, "packed-host-2x2": 2, "unpacked-8x8": 16}[name]
    rng = np.random.default_rng(1000 * d + s)
    for n in R.SIZES + (R.N_ISLANDS,):
        h = make_handle(S, kind, d, s, n, alg)
        try:
            h.initialize(n)
            ran = R.run_single_shard(h, S, O, SEED, alg, rng)
            assert set(ran) == {"one survivor", *R.PATTERNS} - ({"islands"} if n != R.N_ISLANDS else set()), (n, ran)
            assert h.persistent_launches == 0
        finally:
            h.close()


# ---------------------------------------------------------------- two shards in one process
def test_planted_resamples_two_shards_peer_to_peer(S, O, gpu, monkeypatch):
    """Both shards scan the owners' weight rows (parked on the first pass) and read the rows they drew from their owner's
    memory.  tests/test_p2p.py's helper runs the shards; its before_update hook reads the previous plan's result and plants
    the next, so a last call repeats the first plan and is checked without its ESS."""
    from tests.cases import SEED as CASE_SEED
    from tests.test_p2p import run_shards_in_one_process
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    plans = R.sharded_plans()
    plans.append(plans[0])
    n, world = R.N_ISLANDS, 2
    records = [[None] * len(plans) for _ in range(world)]
    pending = [None] * world
    meet = threading.Barrier(world)

    def hook(rank, h, call):
        meet.wait(timeout=120)                     # no shard replaces its particles while the other still reads them
        if call > 0:
            c0, rho0 = pending[rank]
            records[rank][call - 1] = (c0, h.local_offset, rho0, R.read_back(h, c0))
        name, theta, u, delta, ref = plans[call]
        lo, m = h.local_offset, h.n_local
        _, _, rho0 = h.get_population()
        pending[rank] = (R.plant(h, theta[:, lo:lo + m], u[:, lo:lo + m]), rho0)

    out = run_shards_in_one_process(S, "gauss1_cfg2", "single_eps", "rw", n, 1, R.RESAMPLE_NOW, world=world,
                                    before_update=hook, calls=len(plans), delta=2000.0)
    for rank, o in enumerate(out):
        assert o["errors"] == [None] * len(plans)
        c0, rho0 = pending[rank]
        c = o["counters"]
        assert c["n_accept"] == 1 and c["n_resampling"] == c0["n_resampling"] + 1
        assert c["n_population_updates"] == c0["n_population_updates"] + 1
        records[rank][-1] = (c0, o["offset"], rho0, dict(theta=o["theta"], u=o["u"], rho=o["rho"], eps=o["eps"], counters=c))
        assert o["collective_calls"] == 0
    assert sorted(o["offset"] for o in out) == [0, out[0]["theta"].shape[1]]
    R.check_shards(S, O, plans, records, CASE_SEED)


def test_planted_resamples_two_shards_over_alltoallv(S, O, gpu, monkeypatch):
    """The weights are gathered, every shard draws global indices, asks each owner for the rows it drew and scatters the
    replies: the request / reply pairing of k_bucket_scatter, k_resample_serve and k_resample_scatter on planted rows."""
    import torch
    from tests.loopback_collectives import Loopback
    monkeypatch.setenv("SABC_PERSISTENT", "0")
    plans = R.sharded_plans()
    n, world = R.N_ISLANDS, 2
    lb = Loopback(world)
    records = [[None] * len(plans) for _ in range(world)]
    err = [None] * world

    def shard(rank):
        try:
            torch.cuda.set_device(0)
            h = make_handle(S, "gauss1", 1, 1, n, "single_eps", rank=rank, world=world)
            ar, ag, a2a = lb.hooks(rank)
            h.set_collectives(ar, ag, True)
            h.set_alltoallv(a2a)
            h.comm_selftest()
            h.initialize(n)
            lo, m = h.local_offset, h.n_local
            for k, (name, theta, u, delta, ref) in enumerate(plans):
                _, _, rho0 = h.get_population()
                c0 = R.plant(h, theta[:, lo:lo + m], u[:, lo:lo + m])
                h.update(n_simulation=n, proposal=S.RandomWalk(β=R.BETA, n_para=1), resample=R.RESAMPLE_NOW, delta=delta)
                records[rank][k] = (c0, lo, rho0, R.read_back(h, c0))
            assert h.collective_calls > 0
            h.close()
        except BaseException as e:                          # a failing shard must not leave the other at a barrier
            err[rank] = e
            lb.barrier.abort()

    threads = [threading.Thread(target=shard, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert all(e is None for e in err), err
    assert all(r is not None for rec in records for r in rec)
    R.check_shards(S, O, plans, records, SEED)
