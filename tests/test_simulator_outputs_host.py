"""Outputs of device-coded simulators (sabc::emit, sabc_op_simulate_outputs), the part that needs no GPU: the C entry is
declared, exported, bound and called from the Julia wrapper; the shipped sources and a source that uses all three device
functions compile into every kernel of the unit (narrow and wide); and the argument errors of the Python interface are raised
before any handle exists."""
import ctypes as C
import os
import re

import pytest

import sabc_amd as S
from sabc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "simulatedannealingabc.jl_amd", "julia", "SimulatedAnnealingABCHIP.jl")


def emitting_source(s):
    """All three device functions: s distances, outputs 0..2 (and n_outputs itself as output 3, behind the guard)."""
    return """
__device__ void sabc_user_simulate(const double *theta, const double *p, sabc::NormalStream &rng, double *rho) {
  for (int j = 0; j < %d; ++j) rho[j] = fabs(theta[j %% 2] + 0.1 * rng.next());
  sabc::emit(rng, 0, theta[0]);
  sabc::emit(rng, 1, rho[0]);
  if (sabc::emitting(rng)) {
    const long long n = sabc::n_outputs(rng);
    sabc::emit(rng, 2, theta[1]);
    sabc::emit(rng, 3, (double)n);
  }
}
""" % s


def test_entry_is_declared_exported_bound_and_called_from_julia():
    hdr = open(_lib.HEADER).read()
    proto = re.search(r"SABC_API int sabc_op_simulate_outputs\(([^;]*)\);", hdr)
    assert proto, "include/sabc_hip.h does not declare sabc_op_simulate_outputs"
    args = re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["h", "theta", "m", "pid0", "iter", "stream", "n_out", "rho_out", "out"]
    assert re.search(r"#define SABC_STREAM_UPDATE\s+0\b", hdr) and re.search(r"#define SABC_STREAM_PREDICT\s+1\b", hdr)
    assert int(re.search(r"#define SABC_ABI_VERSION (\d+)", hdr).group(1)) == 6          # no struct changed
    for name in ("sabc::emitting", "sabc::n_outputs", "sabc::emit"):
        assert name in hdr, f"{name} is not documented in the header"
    S.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "sabc_op_simulate_outputs")
    fn = _lib.bind(C.CDLL(_lib.LIB_PATH)).sabc_op_simulate_outputs
    dp = C.POINTER(C.c_double)
    assert fn.argtypes == [C.c_void_p, dp, C.c_int64, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, dp, dp] and fn.restype is C.c_int
    assert (_lib.STREAM_UPDATE, _lib.STREAM_PREDICT) == (0, 1)
    jl = open(JL, encoding="utf-8").read()
    call = re.search(r"ccall\(\(:sabc_op_simulate_outputs,\s*libsabc\),\s*Cint,\s*\(([^()]*)\)", jl)
    assert call, "the Julia wrapper does not ccall sabc_op_simulate_outputs"
    assert [a.strip() for a in call.group(1).split(",")] == ["Ptr{Cvoid}", "Ptr{Float64}", "Int64", "UInt64", "UInt64", "Int32", "Int32",
                                                           "Ptr{Float64}", "Ptr{Float64}"]
    assert "function simulate_outputs(" in jl and "function posterior_predictive(" in jl


@pytest.mark.parametrize("name", ["sir", "sir_series", "normal_moments"])
def test_shipped_sources_emit_and_compile(name):
    S.build()
    text = S.models.device_source_text(name)
    assert "sabc::emit(rng," in text, f"device_sources/{name}.hip emits nothing"
    model = {"sir": lambda: S.StochasticSIR((10.0, 5.0, 3.0)),
             "sir_series": lambda: S.StochasticSIRSeries([0.0, 5.0], [1.0, 2.0]),
             "normal_moments": lambda: S.NormalMoments([0.1, 0.2, 0.3])}[name]()
    assert model.compile_check()
    assert model.n_outputs_for() == {"sir": 3, "sir_series": 2, "normal_moments": 3}[name]


@pytest.mark.parametrize("s", [2, 48])
def test_a_source_with_all_three_functions_compiles(s):
    """2 statistics: the narrow kernels (and the one-launch ones); 48: the wide ones."""
    S.build()
    assert S.DeviceSource(emitting_source(s), 2, s, n_outputs=4).compile_check()


def test_argument_errors_come_before_any_handle(monkeypatch):
    def no_handle(*a, **k):
        raise AssertionError("a handle was made")
    monkeypatch.setattr(S.api, "SabcHandle", no_handle)
    theta = [[0.3, 0.1]]
    with pytest.raises(TypeError, match="host"):
        S.simulate_outputs(S.HostDistance(lambda th: abs(th[0]), 1, 2, False), theta)
    with pytest.raises(TypeError, match="host"):
        S.simulate_outputs(lambda th: abs(th[0]), theta)
    with pytest.raises(TypeError, match="built-in"):
        S.simulate_outputs(S.GaussianIID(n_obs=10), [0.5])
    with pytest.raises(TypeError, match="declares no outputs"):
        S.simulate_outputs(S.DeviceSource(emitting_source(2), 2, 2), theta)
    with pytest.raises(ValueError, match="n_outputs"):
        S.DeviceSource(emitting_source(2), 2, 2, n_outputs=-1)
    with pytest.raises(ValueError, match="output_names"):
        S.DeviceSource(emitting_source(2), 2, 2, n_outputs=4, output_names=("a", "b", "c"))
    # ... and what is declared is kept
    m = S.DeviceSource(emitting_source(2), 2, 2, output_names=("a", "b", "c", "d"))
    assert m.n_outputs == 4 and m.n_outputs_for() == 4
    series = S.StochasticSIRSeries()
    with pytest.raises(TypeError, match="has no data"):
        S.simulate_outputs(series, theta)
    assert series.n_outputs_for([[0.0, 1.0, 2.0], [1.0, 1.0, 1.0]]) == 3
