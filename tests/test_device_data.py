"""Observed data for simulators from source (include/sabc_hip.h: sabc_set_device_data; device side sabc::data_len / data_at /
data / data_segments): the reference hands y_obs to f_dist as args... / kwargs... (SimulatedAnnealingABC.jl:164,175,315), here
they live in device memory the handle owns and every kernel of the run-time compiled unit reads them in place.

CPU: the compiler stage of the shipped sources and of a source using every accessor, the argument rules of sabc /
initialization / update_population_, header and binding.  GPU: reads are exact at every length, segments, the same run bit for
bit as the same simulator with its observations in `params` (launch chain, one-launch forms, wide kernels), the two shipped
simulators against the oracle / a Python restatement, replacing the data between two calls, two handles on one source, and
ownership of the copy."""
import ctypes as C

import numpy as np
import pytest

from tests.cases import SEED, hip_proposal, oracle_proposal
from tests.discrete_draws_ref import Stream

# ---- sources ----
# no draws; summed in index order without a multiply, so nothing contracts to an FMA
READ_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const long long n = sabc::data_len();
  double acc = 0.0;
  for (long long j = 0; j < n; ++j) acc += fabs(theta[0] - sabc::data_at(j));
  rho[0] = acc;
  rho[1] = sabc::data_at(sabc::data_len() - 1);
}
"""

# the same with a second statistic that depends on theta (a population can be updated with it)
READ_OWN_LAST_SRC = READ_SRC.replace("rho[1] = sabc::data_at(sabc::data_len() - 1);",
                                     "rho[1] = fabs(theta[0] - sabc::data_at(sabc::data_len() - 1)) + 0.5;")

# what a unit sees while nothing is set (and the segment bookkeeping in general): reads no value
SHAPE_OF_DATA_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  rho[0] = (double)sabc::data_len();
  rho[1] = (double)sabc::data_segments();
  rho[2] = sabc::data() == nullptr ? 1.0 : 0.0;
}
"""

# per segment k: its length, its first value (through the plain pointer) and its last (through data_at); then the segment count
SEGMENTS_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  for (int k = 0; k < 3; ++k) {
    const long long n = sabc::data_len(k);
    rho[3 * k] = (double)n;
    rho[3 * k + 1] = n > 0 ? sabc::data(k)[0] : -1.0;
    rho[3 * k + 2] = n > 0 ? sabc::data_at(n - 1, k) : -1.0;
  }
  rho[9] = (double)sabc::data_segments();
}
"""

# the decay model of tests/test_user_simulator.py (DECAY_SRC), its 8 observations in params[1..8] ...
DECAY_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const double amp = theta[0], rate = theta[1], noise = p[0];
  double acc = 0.0, last = 0.0;
  for (int k = 0; k < 4; ++k) {
    double z0, z1;
    rng.pair(z0, z1);
    const double t0 = 0.5 * (2 * k), t1 = 0.5 * (2 * k + 1);
    const double y0 = amp * exp(-rate * t0) + noise * z0, y1 = amp * exp(-rate * t1) + noise * z1;
    acc += fabs(y0 - p[1 + 2 * k]);
    acc += fabs(y1 - p[2 + 2 * k]);
    last = y1;
  }
  double u0, u1;
  rng.uniform_pair(u0, u1);                       // a multiplicative jitter on the second statistic
  rho[0] = acc / 8.0;
  rho[1] = fabs(last - p[8]) * (0.9 + 0.2 * u0) + 1e-3 * u1;
}
"""
# ... and the same text reading them with data_at(k)
DECAY_DATA_SRC = DECAY_SRC.replace("p[1 + 2 * k]", "sabc::data_at(2 * k)").replace("p[2 + 2 * k]", "sabc::data_at(2 * k + 1)") \
                          .replace("p[8]", "sabc::data_at(7)")
DECAY_OBS = [3.0 * np.exp(-0.7 * 0.5 * k) for k in range(8)]

# s = 20: the wide form of the kernels
WIDE_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const double z = rng.next();
  for (int j = 0; j < 20; ++j) rho[j] = fabs(theta[0] - OBS(j)) + fabs(z);
}
"""
WIDE_OBS = [0.25 * j - 2.0 for j in range(20)]

ALL_ACCESSORS_SRC = r"""
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  const double *a = sabc::data(), *b = sabc::data(1);
  rho[0] = fabs(sabc::data_at(0) + sabc::data_at(1, 1) + (double)(sabc::data_len() + sabc::data_len(1) + sabc::data_segments()))
           + (a && b ? a[0] + b[0] : 0.0) + theta[0] * rng.next();
}
"""


def usage_prior(S):
    """docs/src/usage.md:20-21"""
    return S.product_distribution([S.Normal(0, 2), S.Uniform(0, 2)])


# ---- without a GPU ----
def test_sources_using_the_data_compile_without_a_device(S):
    assert S.NormalMoments().compile_check()
    assert S.StochasticSIRSeries().compile_check()
    assert S.DeviceSource(ALL_ACCESSORS_SRC, 1, 1).compile_check()


def test_argument_rules(S):
    prior, kw = usage_prior(S), dict(n_particles=100, n_simulation=1000)
    y = np.arange(4.0)
    one, two = S.NormalMoments(), S.StochasticSIRSeries()
    sir_prior = S.product_distribution([S.Uniform(0.1, 1.0), S.Uniform(0.05, 0.5)])
    cases = [
        (one, prior, (y, y), {}),                                     # too many values
        (two, sir_prior, (y,), {}),                                   # too few
        (two, sir_prior, (), dict(t_obs=y)),                          # too few, by keyword
        (one, prior, (), dict(y_observed=y)),                         # an unknown keyword
        (one, prior, (y,), dict(y_obs=y)),                            # the same segment twice
        (one, prior, (), {}),                                         # no data anywhere
    ]
    for model, pr, args, kwargs in cases:
        with pytest.raises(TypeError, match="data_names"):
            S.sabc(model, pr, *args, **kwargs, **kw)
        with pytest.raises(TypeError, match="data_names"):
            S.initialization(model, pr, *args, **kwargs, **kw)
    # every other DeviceDistance, and a DeviceSource without data_names, keep refusing extra arguments
    with pytest.raises(TypeError, match="extra args/kwargs are not forwarded"):
        S.sabc(S.GaussianIID(), S.Normal(0, 1), y_obs=y, **kw)
    with pytest.raises(TypeError, match="extra args/kwargs are not forwarded"):
        S.sabc(S.GaussianIID(), S.Normal(0, 1), y, **kw)
    with pytest.raises(TypeError, match="extra args/kwargs are not forwarded"):
        S.sabc(S.DeviceSource(READ_SRC, 1, 2, data=y), S.Normal(0, 1), y_obs=y, **kw)
    # the segments: one array-like is one segment, a sequence of array-likes one each, float64 in C order
    m = S.DeviceSource(READ_SRC, 1, 2, data=np.arange(6, dtype=np.int32).reshape(2, 3))
    assert len(m.data) == 1 and m.data[0].dtype == np.float64 and m.data[0].tolist() == [0, 1, 2, 3, 4, 5]
    assert [d.tolist() for d in S.DeviceSource(READ_SRC, 1, 2, data=([1, 2], np.zeros(0), [3.5])).data] == [[1, 2], [], [3.5]]
    assert [d.tolist() for d in S.DeviceSource(READ_SRC, 1, 2, data=[1, 2, 3]).data] == [[1, 2, 3]]
    assert [d.tolist() for d in two.bind_data((y,), dict(I_obs=[7, 8, 9, 10]))] == [y.tolist(), [7, 8, 9, 10]]
    with pytest.raises(ValueError):
        S.DeviceSource(READ_SRC, 1, 2, data=[[0.0]] * 9)
    with pytest.raises(ValueError):
        S.DeviceSource(READ_SRC, 1, 2, data=[[0.0], [1.0]], data_names=("y_obs",))
    with pytest.raises(ValueError, match="increasing"):
        S.StochasticSIRSeries([0.0, 2.0, 1.0], [1, 2, 3])


def test_data_given_with_the_call_get_the_checks_of_the_constructor(S, tmp_path):
    """sir_series.hip reads I_obs[k] for every k < len(t_obs) and both shipped sources divide by the length: what the
    constructors refuse is refused wherever data enter, before anything reaches the device."""
    y, kw = np.arange(4.0), dict(n_particles=100, n_simulation=1000)
    one, two = S.NormalMoments(), S.StochasticSIRSeries()
    sir_prior = S.product_distribution([S.Uniform(0.1, 1.0), S.Uniform(0.05, 0.5)])
    for bad in (dict(t_obs=y, I_obs=y[:3]), dict(t_obs=y[::-1], I_obs=y), dict(t_obs=[], I_obs=[])):
        with pytest.raises(ValueError):
            S.sabc(two, sir_prior, **bad, **kw)
        with pytest.raises(ValueError):
            two.bind_data((), bad)
        with pytest.raises(ValueError):
            S.StochasticSIRSeries(**bad)
    with pytest.raises(ValueError):
        S.sabc(one, usage_prior(S), y_obs=[], **kw)
    with pytest.raises(ValueError):
        S.NormalMoments([])
    # SabcHandle.set_data asks the model of its handle (no device needed to see that: the hook is the model's)
    with pytest.raises(ValueError):
        two.validate_data([y, y[:3]])
    assert S.DeviceSource(READ_SRC, 1, 2).validate_data([y, y[:3]]) is None
    # a stored result is loaded with a model constructed on its data: one without is refused like in initialization
    np.savez(tmp_path / "res.npz", algorithm="single_eps", n_particles=np.int64(100), seed=np.uint64(SEED))
    with pytest.raises(TypeError, match="data_names"):
        S.load_result(str(tmp_path / "res"), S.NormalMoments(), usage_prior(S))


def julia_call_arities(src, name):
    """(line, positional arguments) of every `name(` in the Julia text, definitions included: arguments at nesting depth 0
    before a `;`"""
    import re
    code = "\n".join(ln.split("#")[0] if '"' not in ln else ln for ln in src.splitlines())
    out = []
    for m in re.finditer(r"(?<![\w.])%s\(" % name, code):
        i, depth, n, seen, in_str, keywords = m.end(), 0, 0, False, False, False
        while True:
            c = code[i]
            if in_str:
                in_str = not (c == '"' and code[i - 1] != "\\")
            elif c == '"':
                in_str, seen = True, True
            elif c in "([{":
                depth += 1
                seen = True
            elif c in ")]}":
                if depth == 0:
                    break
                depth -= 1
            elif depth == 0 and c == ";":
                keywords = True
                n += seen
                seen = False
            elif depth == 0 and c == ",":
                n += seen and not keywords
                seen = False
            elif not c.isspace():
                seen = True
            i += 1
        n += seen and not keywords
        out.append((code.count("\n", 0, m.start()) + 1, n))
    return out


def test_every_julia_devicesource_call_matches_a_method():
    """The struct's implicit constructor takes one argument per field; the keyword constructor three; and the four positional
    arguments the struct took before it carried data still work (StochasticSIR calls it so, and so may a user's code)."""
    import re
    from tests.test_julia_binding import jl_source
    src = jl_source()
    fields = re.search(r"^struct DeviceSource <: DeviceDistance\n(.*?)^end", src, re.S | re.M).group(1).strip().splitlines()
    assert re.search(r"^DeviceSource\(source, n_para, n_stats, params\) = ", src, re.M)
    assert re.search(r"^function DeviceSource\(source, n_para, n_stats; ", src, re.M)
    defined = {len(fields), 3, 4}
    calls = julia_call_arities(src, "DeviceSource")
    assert len(calls) >= 8
    for line, n in calls:
        assert n in defined, f"DeviceSource(...) with {n} positional arguments at line {line}: no such method"
    assert (dict((n, line) for line, n in calls).keys()) >= {3, 4, len(fields)}


def test_header_and_binding_agree(S):
    from tests.test_julia_binding import header_prototypes
    protos = header_prototypes()
    assert protos["sabc_set_device_data"] == ("i32", ["ptr", "ptr", "i64", "ptr", "i32"])
    assert protos["sabc_device_data_len"] == ("i64", ["ptr"])
    kinds = {C.c_void_p: "ptr", C.POINTER(C.c_double): "ptr", C.POINTER(C.c_int64): "ptr", C.c_int64: "i64", C.c_int32: "i32",
             C.c_int: "i32"}
    L = S.lib()
    for name in ("sabc_set_device_data", "sabc_device_data_len"):
        fn = getattr(L, name)
        assert (kinds[fn.restype], [kinds[a] for a in fn.argtypes]) == protos[name], name
    import re
    from tests.test_host_api import ROOT
    hdr = open(ROOT + "/include/sabc_hip.h").read()
    assert int(re.search(r"#define SABC_MAX_DATA_SEGMENTS (\d+)", hdr).group(1)) == S._lib.MAX_DATA_SEGMENTS == 8
    assert int(re.search(r"#define SABC_ABI_VERSION (\d+)", hdr).group(1)) == 6


# ---- on the GPU ----
def read_handle(S, data=None, src=READ_SRC, s=2, n=256):
    return S.SabcHandle(n_particles=n, model=S.DeviceSource(src, 1, s, data=data), prior=S.Normal(0.0, 2.0), seed=SEED)


def read_expected(theta, data, own_last=False):
    out = np.empty((2, len(theta)))
    for i, th in enumerate(theta.tolist()):
        acc = 0.0
        for y in data.tolist():
            acc += abs(th - y)
        out[0, i], out[1, i] = acc, abs(th - float(data[-1])) + 0.5 if own_last else data[-1]
    return out


@pytest.mark.gpu
def test_reads_are_exact_at_every_length(S, gpu):
    rng = np.random.default_rng(SEED)
    theta = np.array([0.3, -1.7, 2.5])
    h = read_handle(S, src=SHAPE_OF_DATA_SRC, s=3)
    np.testing.assert_array_equal(h.simulate(theta[None, :1], 0, 0)[:, 0], [0.0, 0.0, 1.0])      # nothing set
    assert h.data_len == 0
    h.close()
    h = read_handle(S)
    for n in (1, 2, 63, 64, 65, 1000, 100_000):            # 100 000: more than a source could sensibly carry
        data = rng.normal(1.0, 2.0, n)
        h.set_data(data)
        assert h.data_len == n
        np.testing.assert_array_equal(h.simulate(theta[None, :], 5, 3), read_expected(theta, data))
    h.close()


@pytest.mark.gpu
def test_segments(S, gpu):
    a, c = np.array([1.5, -2.25, 3.125]), np.array([10.0, 11.0, 12.0, 13.0, 14.5])
    h = read_handle(S, data=(a, np.zeros(0), c), src=SEGMENTS_SRC, s=10)
    assert h.data_len == 8
    rho = h.simulate(np.zeros((1, 2)), 0, 0)
    h.close()
    want = [3.0, a[0], a[-1], 0.0, -1.0, -1.0, 5.0, c[0], c[-1], 3.0]
    np.testing.assert_array_equal(rho, np.array([want, want]).T)


def set_form(monkeypatch, lanes):
    """lanes = 0: the launch chain | 1, 4, 16: one launch per stretch, that many lanes per particle (tests/test_persistent.py)"""
    monkeypatch.setenv("SABC_PERSISTENT", "1" if lanes else "0")
    monkeypatch.setenv("SABC_PERSISTENT_MAX", "65536")
    if lanes:
        monkeypatch.setenv("SABC_PERSISTENT_LANES", str(lanes))
    else:
        monkeypatch.delenv("SABC_PERSISTENT_LANES", raising=False)


def assert_same_run(a, b, min_resamples=3):
    assert (a.state.n_accept, a.state.n_resampling) == (b.state.n_accept, b.state.n_resampling)
    assert a.state.n_resampling >= min_resamples
    np.testing.assert_array_equal(a.population, b.population)
    np.testing.assert_array_equal(a.u, b.u)
    np.testing.assert_array_equal(a.ρ, b.ρ)
    np.testing.assert_array_equal(a.state.ϵ, b.state.ϵ)
    np.testing.assert_array_equal(np.array(a.state.ϵ_history), np.array(b.state.ϵ_history))


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [0, 1, 4, 16])
@pytest.mark.parametrize("prop", ["rw", "de", "stretch"])
def test_same_run_as_the_observations_in_params(S, gpu, monkeypatch, prop, lanes):
    """Both forms load run-time doubles into the same arithmetic: equality, not a tolerance."""
    set_form(monkeypatch, lanes)
    n, k = 3000, 12
    prior = S.product_distribution([S.Uniform(0.5, 6.0), S.Uniform(0.05, 2.0)])
    runs = []
    for model in (S.DeviceSource(DECAY_SRC, 2, 2, [0.1] + DECAY_OBS), S.DeviceSource(DECAY_DATA_SRC, 2, 2, [0.1], data=DECAY_OBS)):
        runs.append(S.sabc(model, prior, n_particles=n, n_simulation=(k + 1) * n, proposal=hip_proposal(S, prop, 2),
                           resample=n // 2, algorithm="multi_eps", seed=SEED))
        assert runs[-1]._handle.persistent_lanes == lanes
    assert_same_run(*runs)


@pytest.mark.gpu
def test_the_wide_kernels_see_the_data(S, gpu, monkeypatch):
    set_form(monkeypatch, 0)                                # s = 20 is the wide, launch-chain form
    n, k = 2000, 6
    runs = []
    for model in (S.DeviceSource("#define OBS(j) p[j]\n" + WIDE_SRC, 1, 20, WIDE_OBS),
                  S.DeviceSource("#define OBS(j) sabc::data_at(j)\n" + WIDE_SRC, 1, 20, data=WIDE_OBS)):
        runs.append(S.sabc(model, S.Normal(0.0, 2.0), n_particles=n, n_simulation=(k + 1) * n, proposal=hip_proposal(S, "rw", 1),
                           resample=n // 2, algorithm="multi_eps", seed=SEED))
    # (the issue asks for at least 3 resamples of test 6's 12 updates only; these 6 updates are not long enough to promise them:
    # the initial resample is what every run has)
    assert_same_run(*runs, min_resamples=1)


def normal_moments_f(O, y_obs):
    """device_sources/normal_moments.hip over the oracle's Philox blocks"""
    y_obs = [float(y) for y in y_obs]
    n = len(y_obs)

    def f(θ, pid, it):
        mu, sd = float(θ[0]), float(θ[1])
        s1 = s2 = 0.0
        for b in range(n // 2):
            for z in O.normal_pair(SEED, pid, O.PURPOSE_SIM, it, b):
                y = mu + sd * float(z)
                s1 += y
                s2 += y * y
        if n & 1:
            y = mu + sd * float(O.normal_pair(SEED, pid, O.PURPOSE_SIM, it, n // 2)[0])
            s1 += y
            s2 += y * y
        o1 = o2 = 0.0
        for y in y_obs:
            o1 += y
            o2 += y * y
        return abs(o1 / n - s1 / n), abs(o2 - s2)
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("n_obs", [10, 7])
def test_normal_moments_against_the_oracle(S, O, gpu, n_obs):
    """The getting-started example of the reference (docs/src/usage.md:8-46) with its call shape; 7 observations: the odd draw."""
    n, k = 2000, 8
    y_obs = np.random.default_rng(SEED).normal(2.0, 0.5, 10)[:n_obs]
    res = S.sabc(S.NormalMoments(), usage_prior(S), n_particles=n, n_simulation=(k + 1) * n, proposal=S.RandomWalk(n_para=2),
                 resample=n // 2, algorithm="multi_eps", seed=SEED, y_obs=y_obs)
    cfg = O.make_config(n_particles=n, n_para=2, n_stats=2, model_id=O.MODEL_HOST, model_params=[], seed=SEED,
                        prior=[(O.PRIOR_NORMAL, 0.0, 2.0), (O.PRIOR_UNIFORM, 0.0, 2.0)],
                        host_fn=O.host_simulator(normal_moments_f(O, y_obs), 2, 2), algorithm=O.ALG_MULTI_EPS)
    run = O.OracleRun(cfg)
    run.initialize((k + 1) * n)
    run.update(O.make_update_args(n_simulation=k * n, proposal=oracle_proposal(O, "rw", 2), n_para=2, n_particles=n, resample=n // 2))
    c = run.counters
    assert (res.state.n_accept, res.state.n_resampling) == (c["n_accept"], c["n_resampling"])
    np.testing.assert_allclose(res.population.T, run.theta, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(res.ρ.T, run.rho, rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(res.state.ϵ, run.eps, rtol=1e-9)


# ---- StochasticSIRSeries ----
SIR_PRIOR = [(0.1, 1.0), (0.05, 0.5)]
# before the first event (0), two times between the same two events of most runs (12, 12.001), after every epidemic has ended (1000)
SIR_T_OBS = np.array([0.0, 2.0, 5.0, 12.0, 12.001, 20.0, 35.0, 60.0, 100.0, 1000.0])


def sir_series_restated(O, pid, it, theta, params, t_obs, I_obs):
    """device_sources/sir_series.hip over tests/discrete_draws_ref.Stream -> (rho, events, time of the last event)"""
    beta, gamma = float(theta[0]), float(theta[1])
    S0, I0, R0, t_max = int(params[0]), int(params[1]), int(params[2]), float(params[3])
    N = float(S0 + I0 + R0)
    st = dict(S=S0, I=I0, t=0.0, k=0, acc=0.0, between=0)
    K = len(t_obs)

    def event(e, u):
        infection_rate = beta * st["S"] * st["I"] / N
        recovery_rate = gamma * st["I"]
        total_rate = infection_rate + recovery_rate
        if not total_rate > 0.0:
            return False
        st["t"] += e / total_rate
        seen = 0
        while st["k"] < K and t_obs[st["k"]] < st["t"]:
            st["acc"] += abs(st["I"] - I_obs[st["k"]])
            st["k"] += 1
            seen += 1
        st["between"] = max(st["between"], seen)
        if u < infection_rate / total_rate:
            st["S"] -= 1
            st["I"] += 1
        else:
            st["I"] -= 1
        return st["t"] < t_max and st["I"] > 0

    events = Stream(O, SEED, pid, it).while_events(2 * S0 + I0, event) if t_max > 0 and I0 > 0 else 0
    for k in range(st["k"], K):
        st["acc"] += abs(st["I"] - I_obs[k])
    return st["acc"] / K, events, st["t"], st["between"]


@pytest.fixture(scope="module")
def sir_series_case(S):
    from sabc_amd.examples import sir_series_observation
    t_obs, I_obs = sir_series_observation((0.3, 0.1), SIR_T_OBS, seed=123)
    return S.StochasticSIRSeries(t_obs, I_obs), t_obs, I_obs


@pytest.mark.gpu
def test_sir_series_simulations_equal_the_restatement(S, O, gpu, sir_series_case):
    model, t_obs, I_obs = sir_series_case
    m, pid0, it = 200, 31, 4
    rng = np.random.default_rng(8)
    theta = np.stack([rng.uniform(*SIR_PRIOR[0], m), rng.uniform(*SIR_PRIOR[1], m)])
    prior = S.product_distribution([S.Uniform(*SIR_PRIOR[0]), S.Uniform(*SIR_PRIOR[1])])
    h = S.SabcHandle(n_particles=256, model=model, prior=prior, seed=SEED)
    rho = h.simulate(theta, pid0, it)
    h.close()
    want = [sir_series_restated(O, pid0 + i, it, theta[:, i], model.params, t_obs, I_obs) for i in range(m)]
    events = np.array([w[1] for w in want])
    assert events.min() <= 5 and events.max() > 100        # an epidemic that dies at once and one that takes off
    assert max(w[2] for w in want) < t_obs[-1]             # the last observation time lies after every epidemic
    assert max(w[3] for w in want) >= 2                    # two observation times between two consecutive events
    tol = 1e-9                                             # tests/test_sir_device.py: TOL["rw"]
    np.testing.assert_allclose(rho[0], [w[0] for w in want], rtol=tol, atol=tol * 1e-3)


def run_sir_series_form(S, monkeypatch, model, lanes, n=2000, k=5):
    set_form(monkeypatch, lanes)
    prior = S.product_distribution([S.Uniform(*SIR_PRIOR[0]), S.Uniform(*SIR_PRIOR[1])])
    h = S.SabcHandle(n_particles=n, model=model, prior=prior, seed=SEED)
    h.initialize((k + 1) * n)
    h.update(n_simulation=k * n, proposal=hip_proposal(S, "rw", 2), resample=n // 2)
    out = dict(zip(("theta", "u", "rho"), h.get_population()), eps=h.eps.copy(), counters=dict(h.counters), lanes=h.persistent_lanes)
    h.close()
    return out


@pytest.fixture(scope="module")
def sir_series_chain(S, gpu, sir_series_case):
    """the launch-chain run every one-launch form is compared with: computed once"""
    mp = pytest.MonkeyPatch()
    try:
        return run_sir_series_form(S, mp, sir_series_case[0], 0)
    finally:
        mp.undo()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_sir_series_one_launch_equals_the_launch_chain(S, gpu, monkeypatch, sir_series_case, sir_series_chain, lanes):
    a, b = sir_series_chain, run_sir_series_form(S, monkeypatch, sir_series_case[0], lanes)
    assert a["counters"] == b["counters"] and a["counters"]["n_population_updates"] == 5
    assert (a["lanes"], b["lanes"]) == (0, lanes)
    tol = 1e-10                                            # tests/test_persistent.py, RandomWalk
    for key in ("theta", "u", "rho", "eps"):
        np.testing.assert_allclose(b[key], a[key], rtol=tol, atol=tol * 1e-2)


# ---- replacing the data ----
def assert_same_result(a, b):
    for f in ("n_simulation", "n_accept", "n_resampling", "n_population_updates"):
        assert getattr(a.state, f) == getattr(b.state, f), f
    np.testing.assert_array_equal(a.population, b.population)
    np.testing.assert_array_equal(a.u, b.u)
    np.testing.assert_array_equal(a.ρ, b.ρ)
    np.testing.assert_array_equal(a.state.ϵ, b.state.ϵ)
    for x, y in ((a.state.ϵ_history, b.state.ϵ_history), (a.state.u_history, b.state.u_history), (a.state.ρ_history, b.state.ρ_history)):
        assert len(x) == len(y) > 0
        np.testing.assert_array_equal(np.array(x), np.array(y))


@pytest.mark.gpu
def test_replacing_the_data_is_the_reference_s_second_call(S, O, gpu, tmp_path):
    """res = sabc(f_dist, prior; y_obs = A); update_population!(res, f_dist, prior; y_obs = B) (docs/src/usage.md:39-45) against
    the same first call stored, loaded with a model constructed on B, and updated.  No proposal is named, as in the reference's
    example: both calls run DifferentialEvolution, the default (:254, :454).  (With RandomWalk the two routes differ in the last
    bit of 0.6 % of the particles, with or without data: a live handle centres the moment sums of Sigma on the previous call's
    pivot, a loaded one on zero -- tests/test_gpu_parity.py compares that resume at rtol 1e-12.)"""
    n = 2000
    rng = np.random.default_rng(SEED + 1)
    A, B = rng.normal(2.0, 0.5, 10), rng.normal(1.0, 0.8, 13)
    prior = usage_prior(S)

    def first():
        model = S.NormalMoments()
        return model, S.sabc(model, prior, y_obs=A, n_particles=n, n_simulation=5 * n, seed=SEED)

    model, a = first()
    S.update_population_(a, model, prior, n_simulation=4 * n, y_obs=B)
    _, b0 = first()
    S.save_result(str(tmp_path / "res"), b0)
    model_b = S.NormalMoments(B)
    b = S.load_result(str(tmp_path / "res"), model_b, prior)
    S.update_population_(b, model_b, prior, n_simulation=4 * n)
    assert a.state.n_population_updates == 8 and a._handle.data_len == b._handle.data_len == 13
    assert_same_result(a, b)
    # and the handle of route A now simulates against B
    theta = np.array([[1.2, 0.4], [0.7, 1.1]])
    rho = a._handle.simulate(theta, 11, 3)
    np.testing.assert_array_equal(rho, b._handle.simulate(theta, 11, 3))
    f_b, f_a = normal_moments_f(O, B), normal_moments_f(O, A)
    np.testing.assert_allclose(rho.T, [f_b(theta[:, i], 11 + i, 3) for i in range(2)], rtol=1e-9)
    assert not np.allclose(rho.T, [f_a(theta[:, i], 11 + i, 3) for i in range(2)], rtol=1e-3)


@pytest.mark.gpu
def test_two_live_handles_on_one_source_keep_their_own_data(S, gpu):
    """One source, so one cached code object -- but a module, and a descriptor, per handle."""
    rng = np.random.default_rng(SEED + 2)
    A, B = rng.uniform(0.5, 2.0, 40), rng.uniform(3.0, 5.0, 75)
    theta = np.array([0.3, -1.7, 2.5])
    ha, hb = read_handle(S, data=A, src=READ_OWN_LAST_SRC), read_handle(S, data=B, src=READ_OWN_LAST_SRC)
    want_a, want_b = read_expected(theta, A, own_last=True), read_expected(theta, B, own_last=True)
    np.testing.assert_array_equal(ha.simulate(theta[None, :], 0, 0), want_a)
    np.testing.assert_array_equal(hb.simulate(theta[None, :], 0, 0), want_b)
    hb.initialize(256)
    hb.update(n_simulation=2 * 256, proposal=hip_proposal(S, "rw", 1))
    np.testing.assert_array_equal(ha.simulate(theta[None, :], 0, 0), want_a)
    ha.initialize(256)
    ha.update(n_simulation=2 * 256, proposal=hip_proposal(S, "rw", 1))
    np.testing.assert_array_equal(hb.simulate(theta[None, :], 0, 0), want_b)
    np.testing.assert_array_equal(ha.simulate(theta[None, :], 0, 0), want_a)
    ha.close()
    np.testing.assert_array_equal(hb.simulate(theta[None, :], 0, 0), want_b)
    hb.close()


def live_bytes(S):
    out = (C.c_int64 * 2)()
    assert S.lib().sabc_debug_live_bytes(out) == 0
    return np.array([out[0], out[1]], dtype=np.int64)


@pytest.mark.gpu
def test_the_handle_owns_the_copy(S, gpu):
    n = 1000
    rng = np.random.default_rng(SEED + 3)
    old = rng.normal(0.0, 1.0, n)
    theta = np.array([0.3, -1.7])
    before = live_bytes(S)
    h = read_handle(S)
    opened = live_bytes(S)
    h.set_data(old)
    with_data = live_bytes(S)
    assert with_data[0] - opened[0] >= 8 * n and with_data[1] == opened[1]
    np.testing.assert_array_equal(h.simulate(theta[None, :], 0, 0), read_expected(theta, old))
    second = rng.normal(0.0, 1.0, n)
    h.set_data(second)                                     # the same length again: the allocation is reused ...
    assert (live_bytes(S) == with_data).all()
    np.testing.assert_array_equal(h.simulate(theta[None, :], 0, 0), read_expected(theta, second))   # ... and read at the old address
    h.set_data(old)
    # the errors leave the old data in place
    L, dp, ip = S.lib(), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    vals = np.arange(6.0)

    def call(handle, n_values, lens):
        arr = (C.c_int64 * max(len(lens), 1))(*lens)
        return L.sabc_set_device_data(handle._h, vals.ctypes.data_as(dp), n_values, C.cast(arr, ip), len(lens))
    bad = S._lib.ERR_NAMES
    for n_values, lens in ((-1, [1]), (6, [-1, 7]), (6, [7, -1]), (6, [2, 3]), (6, [3, 4]), (6, [1] * 5 + [0] * 3 + [1])):
        assert bad[call(h, n_values, lens)] == "BAD_CONFIG", (n_values, lens)
    assert h.data_len == n and (live_bytes(S) == with_data).all()
    np.testing.assert_array_equal(h.simulate(theta[None, :], 0, 0), read_expected(theta, old))
    other = S.SabcHandle(n_particles=256, model=S.GaussianIID(n_obs=10), prior=S.Normal(0.0, 2.0), seed=SEED)
    assert bad[call(other, 6, [6])] == "BAD_CONFIG" and other.data_len == 0
    other.close()
    h.set_data(None)                                       # n = 0 drops the data
    assert h.data_len == 0 and (live_bytes(S) == opened).all()
    h.set_data(old)
    h.close()
    assert (live_bytes(S) == before).all()
