"""One update's proposals and accept decisions, particle by particle, on every update path, against the long-double reference of
tests/transition_ref.py (whose docstring has the procedure and the tolerances; tests/test_transition_reference.py shows on
the CPU that the checker tells right from wrong).

The transition is written four times: update_particle_draft / update_particle_decide (k_update, the kernels compiled from
source, k_update_persistent with 1, 4 and 16 lanes), k_update_wide, k_update_gk and k_host_propose / k_host_accept.  Each
case plants P0, epsilon and the tables, runs ONE update of n simulations with resampling off and holds the population it
leaves to the reference; the launch counters say which kernel ran.

  path (asserted)                      (d, s)   n          proposal, schedule, prior
  chain, built-in Gaussian             (1, 1)   1027       RandomWalk, single, Normal
  chain, source                        (2, 2)   1027, 4    DifferentialEvolution, multi, Uniform edge (n = 4: a first partner
                                                           draw collides and is redrawn)
  chain, source                        (3, 3)   1027       StretchMove, multi, TruncNormal x Gamma x LogNormal
  chain, source                        (5, 12)  1027       RandomWalk (Cholesky with d at run time), multi, Normal
  chain, source                        (2, 2)   130        RandomWalk (rw_proposal_from_sums<2>), multi, MvNormal
  one launch, 1 | 4 | 16 lanes         (1, 1)   1027       RandomWalk, single, Normal
  one launch, 1 lane                   (3, 3)   1027       DifferentialEvolution, multi, Uniform edge (agent-scope partner loads)
  one launch, 1 lane                   (3, 3)   1027       StretchMove, single, flat
  wide, k_update_wide                  (3, 48)  1027       DifferentialEvolution, multi, Normal
  g-and-k, k_update_gk                 (4, 4)   1027       StretchMove, single, flat, n_draws = 128
  host mode                            (2, 2)   1027       RandomWalk (Normal) and DifferentialEvolution (Uniform edge), multi; the
                                                           prior on the device and as host callbacks

1027 particles: halves of 513 and 514, more than one workgroup on every path, a partial last wave.  No path refused its size
or proposal: nothing is substituted.  The simulator from source is a smaller one of the kind of tests/test_gpu_ecdf_paths.py's
grid simulator, without the flooring: statistic j from parameters j % d and (j + 1) % d and the j-th normal of the stream.

Host mode (hostmode_kernel.hpp, hip_backend_hostmode.hip): k_host_propose gates with the device prior, or the host's logpdf
callback is asked about EVERY proposal of a chunk followed by its current particles; f_dist is asked only about the
proposals inside the support, compacted, with their particle ids.  The test records both: every proposal the callbacks see is
held to the reference's thp within tol_theta -- rejected ones included, and with the host prior those outside the support
too --, and f_dist is asked about exactly the particles whose proposal the reference finds inside the support.

Per path also: three updates in one call equal three one-update calls of the same loop (history_phase, as the wrapper cuts a
call: tests/test_history_chunks.py has this for the CPU engine and for sabc() on the device) bit for bit in theta, u and rho
-- the only handle on the later updates inside one persistent launch; and the checked update raised n_accept by the number of
particles the checker saw accepted (run_single_shard)."""
import numpy as np
import pytest

from tests import transition_ref as T

pytestmark = pytest.mark.gpu

SEED = 11
NOISE = 0.4
SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const int d = (int)p[0], s = (int)p[1];
  for (int j = 0; j < s; ++j) {
    const double z = rng.next();
    rho[j] = fabs(theta[j % d] + 0.5 * theta[(j + 1) % d] + p[2] * z - 0.3 * ((j % 5) - 2));
  }
}
"""
CHAIN = {"SABC_PERSISTENT": "0"}
GK_LO = [[2.55, 0.65, 1.65, 0.65], [3.15, 1.05, 2.05, 1.05]]
GK_HI = [[2.85, 0.95, 1.95, 0.95], [3.45, 1.35, 2.35, 1.35]]
EDGE2 = T.Prior(dims=[("U", -1.0, 1.0), ("U", 0.2, 2.0)])
EDGE2_LO, EDGE2_HI = [[-1.0, 0.2], [0.5, 1.5]], [[-0.5, 0.6], [1.0, 2.0]]
EDGE3 = T.Prior(dims=[("U", 0.0, 1.0), ("U", -5.0, 5.0), ("U", -5.0, 5.0)])
BOX3_LO, BOX3_HI = [[0.0, 0.0, 0.0], [0.65, 0.65, 0.65]], [[0.35, 0.35, 0.35], [1.0, 1.0, 1.0]]
NORMAL1 = T.Prior(dims=[("N", 0.0, 0.7)])
NORMAL2 = T.Prior(dims=[("N", 0.0, 0.7), ("N", 0.0, 0.7)])
DE2, RW = ("de", 1.19, 0.05), ("rw", 0.8, 0.0)


def case(name, kind, d, s, n, prop, alg, prior, lo, hi, eps, env, one_launch=False, lanes=None, **kw):
    return T.Case(name, d, s, n, prop, alg, prior, np.broadcast_to(lo, (2, d)), np.broadcast_to(hi, (2, d)), eps, kind=kind, env=env,
                  one_launch=one_launch, lanes=lanes, **kw)


def lanes_case(lanes):
    return case(f"one-launch-1x1-lanes{lanes}", "src", 1, 1, 1027, RW, "single_eps", NORMAL1, -1.0, 1.0, [0.5],
                {"SABC_PERSISTENT_LANES": str(lanes)}, one_launch=True, lanes=lanes)


CASES = [
    case("chain-gauss-1x1", "gauss", 1, 1, 1027, RW, "single_eps", NORMAL1, -1.0, 1.0, [0.5], CHAIN),
    case("chain-src-2x2-de-edge", "src", 2, 2, 1027, DE2, "multi_eps", EDGE2, EDGE2_LO, EDGE2_HI, T.ladder(2), CHAIN, edge=True),
    case("chain-src-2x2-de-edge-n4", "src", 2, 2, 4, DE2, "multi_eps", EDGE2, EDGE2_LO, EDGE2_HI, T.ladder(2), CHAIN, edge=True,
         collide=True, seed=3),
    case("chain-src-3x3-stretch", "src", 3, 3, 1027, ("stretch", 2.0, 0.0), "multi_eps",
         T.Prior(dims=[("T", 3.0, 1.0, 1.5, 4.5), ("G", 4.0, 0.25), ("L", 0.7, 0.3)]), [g[:3] for g in GK_LO], [g[:3] for g in GK_HI],
         T.ladder(3), CHAIN),
    case("chain-src-5x12-rw", "src", 5, 12, 1027, RW, "multi_eps", T.Prior(dims=[("N", 0.0, 0.5)] * 5), -0.6, 0.6, T.ladder(12), CHAIN),
    case("chain-src-2x2-rw-130", "src", 2, 2, 130, RW, "multi_eps",
         T.Prior(mv=([0.5, -0.5], np.linalg.cholesky(np.array([[0.5, -0.2], [-0.2, 0.4]])))), [0.4, -1.5], [2.0, 0.1], T.ladder(2), CHAIN),
    lanes_case(1), lanes_case(4), lanes_case(16),
    case("one-launch-3x3-de-edge", "src", 3, 3, 1027, ("de", 0.97, 0.05), "multi_eps", EDGE3, BOX3_LO, BOX3_HI, T.ladder(3),
         {"SABC_PERSISTENT_LANES": "1"}, one_launch=True, lanes=1, edge=True),
    case("one-launch-3x3-stretch", "src", 3, 3, 1027, ("stretch", 2.0, 0.0), "single_eps", T.Prior(dims=[("U", -5.0, 5.0)] * 3),
         BOX3_LO, BOX3_HI, [0.15], {"SABC_PERSISTENT_LANES": "1"}, one_launch=True, lanes=1),
    case("wide-3x48-de", "src", 3, 48, 1027, ("de", 0.97, 0.05), "multi_eps", T.Prior(dims=[("N", 0.5, 0.6)] * 3), BOX3_LO, BOX3_HI,
         T.ladder(48), {}),
    case("gk-4x4-stretch", "gk", 4, 4, 1027, ("stretch", 2.0, 0.0), "single_eps", T.Prior(dims=[("U", 0.0, 10.0)] * 4), GK_LO, GK_HI,
         [0.15], {}),
    case("host-2x2-rw", "host", 2, 2, 1027, RW, "multi_eps", NORMAL2, -1.0, 1.0, T.ladder(2), {}),
    case("host-2x2-rw-host-prior", "host", 2, 2, 1027, RW, "multi_eps", NORMAL2, -1.0, 1.0, T.ladder(2), {}, host_prior=True),
    case("host-2x2-de-edge", "host", 2, 2, 1027, DE2, "multi_eps", EDGE2, EDGE2_LO, EDGE2_HI, T.ladder(2), {}, edge=True),
    case("host-2x2-de-edge-host-prior", "host", 2, 2, 1027, DE2, "multi_eps", EDGE2, EDGE2_LO, EDGE2_HI, T.ladder(2), {}, edge=True,
         host_prior=True),
]


def host_rho(theta):
    """f_dist of the host cases for theta [2][m]: a function of theta alone."""
    return np.stack([np.abs(theta[0] + 0.5 * theta[1] - 0.3), np.abs(theta[1] - 0.5 * theta[0] + 0.2)])


class Recorder:
    """What the host callbacks are shown during the checked update."""

    def __init__(self, prior):
        self.prior, self.on = prior, False
        self.fdist, self.logpdf_calls = {}, []

    def f_dist(self, theta, pid, it):
        if self.on:
            assert pid not in self.fdist
            self.fdist[pid] = (np.array(theta, dtype=np.float64), it)
        return host_rho(np.asarray(theta, dtype=np.float64).reshape(2, 1))[:, 0]

    def sample(self, ids):
        rng = np.random.default_rng(5)
        return 0.3 + 0.2 * rng.uniform(size=(len(ids), 2))

    def logpdf(self, th):
        if self.on:
            self.logpdf_calls.append(np.array(th, dtype=np.float64))
        lp = self.prior.logpdf(np.asarray(th, dtype=np.float64).T.astype(T.LD))[0]
        return lp.astype(np.float64)


def make_handle(S, c, rec=None):
    kind = c.extra["kind"]
    a = S._lib.ALG_MULTI_EPS if c.alg == "multi_eps" else S._lib.ALG_SINGLE_EPS
    prior = c.prior.make(S)
    if kind == "gauss":
        model = S.GaussianIID(n_obs=20, sd=1.0, obs_mean=0.3)
    elif kind == "gk":
        model = S.GandK(n_draws=128, c=0.8, ranks=(16, 48, 80, 112), obs=(1.9, 2.7, 3.6, 6.4))
    elif kind == "host":
        model = S.HostDistance(rec.f_dist, 2, 2, False, with_ids=True)
        if c.extra.get("host_prior"):
            prior = S.HostPrior(rec.sample, rec.logpdf, 2, univariate=False)
    else:
        model = S.DeviceSource(SRC, c.d, c.s, [c.d, c.s, NOISE])
    return S.SabcHandle(n_particles=c.n, model=model, prior=prior, seed=SEED, algorithm=a)


def rho_of_for(S, h, c):
    if c.extra["kind"] == "host":
        return lambda theta, it: host_rho(np.asarray(theta, dtype=np.float64))
    return lambda theta, it: h.simulate(theta, 0, it)


def normal_pairs_for(S, c):
    return lambda purpose, it, k: S.op_normal_pairs(SEED, 0, c.n, purpose, it, k)


def assert_path(h, c, launches0, kernels0):
    launched = h.persistent_launches - launches0
    assert (launched > 0) == c.extra["one_launch"], (c.name, launched)
    assert h.kernel_launches > kernels0
    if c.extra["one_launch"]:
        assert h.persistent_lanes == c.extra["lanes"], (c.name, h.persistent_lanes)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_one_update_against_the_reference_on_every_path(S, O, gpu, monkeypatch, c):
    for k, v in c.extra["env"].items():
        monkeypatch.setenv(k, v)
    rec = Recorder(c.prior) if c.extra["kind"] == "host" else None
    h = make_handle(S, c, rec)
    try:
        h.initialize(c.n)
        l0, k0 = h.persistent_launches, h.kernel_launches
        rho_of = rho_of_for(S, h, c)
        if rec is None:
            rep = T.run_single_shard(h, S, O, c, SEED, rho_of, normal_pairs_for(S, c))
        else:
            rep = host_case(h, S, O, c, rec, rho_of)
        assert_path(h, c, l0, k0)
    finally:
        h.close()
    print(f"{c.name}: accepted {int(rep.accepted.sum())} of {c.n}, undecided {len(rep.undecided)}, "
          f"max |theta_new - thp| / tol_theta = {rep.theta_ratio:.3f}, min |log U - log_alpha| / tol_alpha = {rep.margin:.3g}")


def host_case(h, S, O, c, rec, rho_of):
    """run_single_shard with the callbacks' view recorded during the checked update."""
    lay = T.Layout(c.n, 1)
    theta_all, u_all = T.planted(c, lay)
    before = T.prepare(h, S, c, lay, theta_all, u_all, np.abs(rho_of(theta_all, 1)))
    rec.on = True
    h.update(n_simulation=c.n, proposal=c.proposal(S), resample=T.NO_RESAMPLE)
    rec.on = False
    P1 = h.get_population()
    c1 = h.counters
    streams = T.Streams(O, SEED, 0, c.n, normal_pairs_for(S, c))
    inp = T.inputs(c, lay, 0, before, [before.theta0], [P1[0]], streams, rho_of)
    rep = T.check(inp, P1)
    ref = rep.ref
    T.premises(c, ref)
    T.assert_ok(rep, c.name)
    assert c1["n_accept"] - before.counters["n_accept"] == int(rep.accepted.sum())
    # f_dist: exactly the proposals inside the support, each within tol_theta of the reference's, at this update's index
    assert sorted(rec.fdist) == np.nonzero(~ref.outside)[0].tolist(), (c.name, len(rec.fdist), int((~ref.outside).sum()))
    for pid, (th, it) in rec.fdist.items():
        assert it == inp.it
        assert np.all(np.abs(th.astype(T.LD) - ref.thp[:, pid]) <= ref.tol_theta[:, pid]), (c.name, pid, th, ref.thp[:, pid])
    if c.extra.get("host_prior"):
        # logpdf: every chunk's proposals followed by its current particles, in particle order, outside the support or not
        seen, cur = [], []
        for th in rec.logpdf_calls:
            m = len(th) // 2
            seen.append(th[:m])
            cur.append(th[m:])
        seen, cur = np.concatenate(seen).T, np.concatenate(cur).T
        assert seen.shape == (c.d, c.n)
        assert np.all(np.abs(seen.astype(T.LD) - ref.thp) <= ref.tol_theta), c.name
        # (the second half batch's current particles are P0's: a half batch only writes its own half)
        np.testing.assert_array_equal(cur, before.theta0)
        if c.edge:
            assert ref.outside.sum() > 0
    else:
        assert not rec.logpdf_calls
    return rep


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_three_updates_in_one_call_equal_three_calls(S, gpu, monkeypatch, c):
    """K = 3 updates in one call against three one-update calls that continue one loop (history_phase 0, 1, 2), from the same
    planted state on two handles: theta, u and rho bit for bit, and the same counters."""
    for k, v in c.extra["env"].items():
        monkeypatch.setenv(k, v)
    lay = T.Layout(c.n, 1)
    theta_all, u_all = T.planted(c, lay)
    got = []
    for cuts in ((3,), (1, 1, 1)):
        rec = Recorder(c.prior) if c.extra["kind"] == "host" else None
        h = make_handle(S, c, rec)
        try:
            h.initialize(c.n)
            l0, k0 = h.persistent_launches, h.kernel_launches
            T.prepare(h, S, c, lay, theta_all, u_all, np.abs(rho_of_for(S, h, c)(theta_all, 1)))
            done = 0
            for m in cuts:
                h.update(n_simulation=m * c.n, proposal=c.proposal(S), resample=T.NO_RESAMPLE, history_phase=done,
                         more_chunks_follow=done + m < 3)
                done += m
            assert_path(h, c, l0, k0)
            got.append((h.get_population(), h.counters, h.eps.copy()))
        finally:
            h.close()
    (pa, ca, ea), (pb, cb, eb) = got
    assert ca == cb and ca["n_accept"] > 0
    for a, b, what in zip(pa, pb, ("theta", "u", "rho")):
        np.testing.assert_array_equal(a, b, err_msg=f"{c.name}: {what}")
    np.testing.assert_array_equal(ea, eb)
