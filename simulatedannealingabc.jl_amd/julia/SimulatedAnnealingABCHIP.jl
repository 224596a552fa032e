# SimulatedAnnealingABCHIP.jl -- thin Julia binding of libsabc_hip.so (include/sabc_hip.h).
#
# Keeps the reference's public surface for the hot path -- `sabc`, `update_population!`,
# `SABCresult`, `SABCstate`, `RandomWalk`, `DifferentialEvolution`, `StretchMove`
# (src/SimulatedAnnealingABC.jl:19,28-60,251-259,451-460; src/proposals.jl:6) -- and does
# nothing but marshal arguments into `ccall`s.  All numerics live in the library.
#
# NOT EXECUTED IN THE BUILD CONTAINER: Julia is not installed there (SURVEY.md section 8c).  The
# Python mirror in ../api.py makes exactly the same calls and is what the test-suite drives; what CAN be
# checked without Julia is checked by tests/test_julia_binding.py: the field order, widths and offsets of
# CConfig / CUpdateArgs against sizeof / offsetof of the C structs, every ccall's symbol, return type and
# argument list against the prototypes of include/sabc_hip.h, and the enum values used below.
module SimulatedAnnealingABCHIP

using Distributions: Distribution, Normal, Uniform, Exponential, LogNormal, Gamma, Beta, Truncated, MvNormal, UnivariateDistribution,
                     ContinuousMultivariateDistribution, logpdf
using LinearAlgebra: cholesky, Symmetric
using ProgressMeter: Progress, next!, finish!          # same progress UI as the reference (:290-292,374)
import Dates
import Base: show

export sabc, update_population!, RandomWalk, DifferentialEvolution, StretchMove,
       DeviceDistance, GaussianIID, Gaussian2D, GandK, LotkaVolterra, DeviceSource, StochasticSIR, LotkaVolterraF32, NormalMoments, StochasticSIRSeries, GandKQuantiles, GandKSample, GandKSampleF32, MA2, GARCH11, Ricker, SourcePrior,
       comm_unique_id, simulate_outputs, posterior_predictive

const libsabc = get(ENV, "SABC_HIP_LIB", joinpath(@__DIR__, "..", "libsabc_hip.so"))

const MAX_PARA, MAX_STATS, MAX_MODEL_PARAMS = 16, 64, 32
const MAX_PARA2 = MAX_PARA * MAX_PARA      # the row-major Cholesky factor of an MvNormal prior

# ---- C structs (must match include/sabc_hip.h field for field) ----
struct CConfig
    abi_version::Int32
    device::Int32
    n_particles::Int64
    n_para::Int32
    n_stats::Int32
    model_id::Int32
    n_model_params::Int32
    model_params::NTuple{MAX_MODEL_PARAMS,Float64}
    prior_kind::NTuple{MAX_PARA,Int32}
    prior_a::NTuple{MAX_PARA,Float64}
    prior_b::NTuple{MAX_PARA,Float64}
    prior_c::NTuple{MAX_PARA,Float64}
    prior_d::NTuple{MAX_PARA,Float64}
    prior_joint::Int32
    reserved2::Int32
    prior_chol::NTuple{MAX_PARA2,Float64}
    algorithm::Int32
    rank::Int32
    world::Int32
    reserved::Int32
    v::Float64
    delta::Float64
    seed::UInt64
end

struct CUpdateArgs
    n_simulation::Int64
    v::Float64
    delta::Float64
    resample::Float64
    checkpoint_history::Int64
    proposal_kind::Int32
    more_chunks_follow::Int32
    proposal_p0::Float64
    proposal_p1::Float64
    history_phase::Int64
end

# ---- proposals: same constructors and errors as src/proposals.jl ----
abstract type Proposal end

mutable struct RandomWalk{T} <: Proposal
    β::Float64
    Σ::T
end
function RandomWalk(; β=0.8, n_para)
    (0 < β <= 1) || error("Mixing parameter `β` must be between zero and one.")   # proposals.jl:30
    n_para == 1 ? RandomWalk(β, -1.0) : RandomWalk(β, -ones(n_para, n_para))
end

struct DifferentialEvolution <: Proposal
    γ0::Float64
    σ_gamma::Float64
    function DifferentialEvolution(; γ0=nothing, n_para=nothing, σ_gamma=1e-5)
        if !isnothing(γ0) && isnothing(n_para)
            new(γ0, σ_gamma)
        elseif !isnothing(n_para) && isnothing(γ0)
            new(2.38 / sqrt(2 * n_para), σ_gamma)                                  # proposals.jl:93
        else
            throw(ArgumentError("Provide either `γ0` or `n_para`, not both."))   # proposals.jl:96
        end
    end
end

struct StretchMove <: Proposal
    a::Float64
end
StretchMove(; a=2) = StretchMove(a)

descriptor(p::RandomWalk) = (Int32(0), p.β, 0.0)
descriptor(p::DifferentialEvolution) = (Int32(1), p.γ0, p.σ_gamma)
descriptor(p::StretchMove) = (Int32(2), p.a, 0.0)

# ---- device-coded simulators: `f_dist` as data (<: Function so that sabc(f_dist::Function, ...) dispatches) ----
abstract type DeviceDistance <: Function end
struct GaussianIID <: DeviceDistance
    n_obs::Int; sd::Float64; obs_mean::Float64; obs_m2::Union{Nothing,Float64}
end
GaussianIID(; n_obs=100, sd=1.0, obs_mean=0.0, obs_m2=nothing) = GaussianIID(n_obs, sd, obs_mean, obs_m2)
struct Gaussian2D <: DeviceDistance
    n_obs::Int; r::Float64; obs_mean::NTuple{2,Float64}; obs_varsum::Float64; obs_cov::Float64
end
struct GandK <: DeviceDistance
    n_draws::Int; c::Float64; ranks::NTuple{4,Int}; obs::NTuple{4,Float64}
end
struct LotkaVolterra <: DeviceDistance
    n_steps::Int; dt::Float64; σ::Float64; x0::Float64; y0::Float64; obs::NTuple{4,Float64}
end
model_id(::GaussianIID) = Int32(1); model_id(::Gaussian2D) = Int32(2)
model_id(::GandK) = Int32(3); model_id(::LotkaVolterra) = Int32(4)
n_stats(m::GaussianIID) = isnothing(m.obs_m2) ? 1 : 2
n_stats(::Gaussian2D) = 3; n_stats(::GandK) = 4; n_stats(::LotkaVolterra) = 4
params(m::GaussianIID) = Float64[m.n_obs, m.sd, m.obs_mean, something(m.obs_m2, 0.0)]
params(m::Gaussian2D) = Float64[m.n_obs, m.r, m.obs_mean..., m.obs_varsum, m.obs_cov]
params(m::GandK) = Float64[m.n_draws, m.c, m.ranks..., m.obs...]
params(m::LotkaVolterra) = Float64[m.n_steps, m.dt, m.σ, m.x0, m.y0, m.obs...]

# ---- any other f_dist: stays a Julia function, called back by the library for the proposals that
#      passed the prior gate (include/sabc_hip.h: sabc_simulate_fn); everything else runs on the GPU
struct HostDistance{F} <: DeviceDistance
    f::F
    n_stats::Int
    n_para::Int
    args::Tuple
    kwargs::NamedTuple
end
model_id(::HostDistance) = Int32(0)

# ---- f_dist as HIP source, compiled at run time into the fused update kernel (include/sabc_hip.h:
#      sabc_register_device_simulator); with a SourcePrior the same source also defines the prior (prior_joint = 3).
#      n_stats <= 64; params holds at most 32 values.  Observations are `data`: one array or a tuple / vector of arrays, one
#      segment each (at most 8), kept in device memory by the handle (sabc_set_device_data) and read by the source through
#      sabc::data_len(segment) / sabc::data_at(i, segment); an array of several dimensions is flattened in Julia's own
#      (column-major) order.  With `data_names = (:y_obs, :t_obs)`, `sabc` and `update_population!` take that many extra
#      positional arguments or keywords of those names, as the reference forwards args... / kwargs... to f_dist (:164,175,315):
#      they become the segments in that order; in `update_population!` data that are not given leave the handle's.
#      `team_lanes` = 1, 4 or 16 (default `nothing`): the source is TEAM-AWARE -- it defines, instead of sabc_user_simulate,
#          template <int W> __device__ void sabc_user_simulate_team(const double *theta, const double *params, sabc::NormalStream &rng, double *rho_out);
#      with W the lanes that run one particle side by side, holds its sample in a sabc::Sample<N, W> (csrc/team_sample.hpp:
#      fill_normals, fill, drawn, sort, at, order_statistic, quantile, emit; sum, max, min, mean, moments and, against a sorted
#      data segment, wasserstein1, wasserstein2_squared, ks -- csrc/sample_reduce.hpp) and runs with that many lanes per particle on the
#      launch chain and in the forward run (sabc_register_device_simulator_team); n_stats <= 16 ----
struct DeviceSource <: DeviceDistance
    source::String
    n_para::Int
    n_stats::Int
    params::Vector{Float64}
    data::Vector{Vector{Float64}}
    data_names::Tuple
    validate::Function                   # segments -> nothing, or throws: what this model's source requires of its data
    team_lanes::Int                      # 0: sabc_user_simulate | 1, 4, 16: sabc_user_simulate_team<W>, that many lanes per particle
end
no_data_check(segs) = nothing
data_segment(x) = vec(collect(Float64, x))
data_segments(x) = x === nothing ? Vector{Float64}[] :
                   (x isa Tuple || (x isa Vector && !(eltype(x) <: Real))) ? Vector{Float64}[data_segment(y) for y in x] :
                   Vector{Float64}[data_segment(x)]
function DeviceSource(source, n_para, n_stats; params=Float64[], data=nothing, data_names=(), validate=no_data_check, team_lanes=nothing)
    team_lanes === nothing || team_lanes in (1, 4, 16) || throw(ArgumentError("team_lanes is nothing, 1, 4 or 16"))
    team_lanes === nothing || n_stats <= 16 || throw(ArgumentError("a team-aware source has at most 16 statistics"))
    segs = data_segments(data)
    isempty(segs) || validate(segs)
    length(segs) <= 8 || throw(ArgumentError("at most 8 data segments"))
    names = Tuple(Symbol(n) for n in data_names)
    (isempty(names) || isempty(segs) || length(names) == length(segs)) || throw(ArgumentError("one name in data_names per data segment"))
    DeviceSource(source, n_para, n_stats, collect(Float64, params), segs, names, validate, team_lanes === nothing ? 0 : Int(team_lanes))
end
# the four positional arguments the struct took before it carried data (StochasticSIR, and callers' own code)
DeviceSource(source, n_para, n_stats, params) = DeviceSource(source, n_para, n_stats; params=params)
with_data(m::DeviceSource, segs) = DeviceSource(m.source, m.n_para, m.n_stats, m.params, segs, m.data_names, m.validate, m.team_lanes)

# the extra arguments of sabc / update_population! as data segments in the order of data_names; nothing if there are none
function bind_data(f_dist::DeviceDistance, kwargs)
    isempty(kwargs) && return nothing
    names = f_dist isa DeviceSource ? f_dist.data_names : ()
    isempty(names) && throw(ArgumentError("a DeviceDistance takes its data at construction; extra args/kwargs are not forwarded"))
    for k in keys(kwargs)
        k in names || throw(ArgumentError("unexpected keyword argument $(k): data_names = $(names)"))
    end
    for k in names
        haskey(kwargs, k) || throw(ArgumentError("missing data argument $(k): data_names = $(names)"))
    end
    segs = Vector{Float64}[data_segment(kwargs[k]) for k in names]
    f_dist.validate(segs)                # the checks of the constructor, for data that arrive with the call
    segs
end
# positional data -> keywords of the first names
function positional_data(f_dist::DeviceSource, args, kwargs)
    names = f_dist.data_names
    length(args) <= length(names) || throw(ArgumentError("$(length(args)) positional data arguments given, data_names = $(names)"))
    for k in names[1:length(args)]
        haskey(kwargs, k) && throw(ArgumentError("data argument $(k) given both by position and by keyword: data_names = $(names)"))
    end
    NamedTuple{names[1:length(args)]}(args)
end
function set_device_data!(h::Ptr{Cvoid}, segs)
    flat = reduce(vcat, segs; init=Float64[])
    lens = Int64[length(s) for s in segs]
    GC.@preserve flat lens check(h, ccall((:sabc_set_device_data, libsabc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int64}, Int32),
                                          h, flat, length(flat), lens, length(lens)))
end
model_id(::DeviceSource) = Int32(5)
n_stats(m::DeviceSource) = m.n_stats
params(m::DeviceSource) = m.params

"""
    StochasticSIR(data_obs; S0=99, I0=1, R0=0, t_max=160.0, n_stats=3)

The reference's documentation example (docs/src/example.md:75-198) on the device: Gillespie's direct method for θ = (β, γ),
`data_obs = (total_infected = ..., peak_infected = ..., t_peak = ...)`; ρ = the three squared differences (`n_stats = 3`) or
their sum (`n_stats = 1`).  A `DeviceSource` of the HIP text shipped next to the library (device_sources/sir.hip).
"""
function StochasticSIR(data_obs; t_max=160.0, n_stats::Integer=3, compartments...)
    # keywords S0, I0, R0 (the reference's spelling), collected here so that the defaults sit next to their names
    c = merge(NamedTuple{(Symbol("S0"), Symbol("I0"), Symbol("R0"))}((99, 1, 0)), values(compartments))
    length(c) == 3 || throw(ArgumentError("unknown keyword: the compartments are S0, I0, R0"))
    s0, i0, r0 = Int(c[1]), Int(c[2]), Int(c[3])
    (s0 >= 0 && r0 >= 0) || throw(ArgumentError("compartments must be non-negative"))
    i0 >= 1 || throw(ArgumentError("I0 must be at least 1"))
    n_stats in (1, 3) || throw(ArgumentError("n_stats is 3 (one distance per statistic) or 1 (their sum)"))
    text = read(joinpath(@__DIR__, "..", "device_sources", "sir.hip"), String)
    obs = Float64[data_obs.total_infected, data_obs.peak_infected, data_obs.t_peak]
    DeviceSource("#define SIR_N_STATS $(n_stats)\n" * text, 2, Int(n_stats), Float64[s0, i0, r0, t_max, obs...])
end
"""
    LotkaVolterraF32(; n_steps=256, dt=0.05, σ=0.1, x0=50.0, y0=50.0, obs=(0.0, 0.0, 0.0, 0.0), n_stats=4)

`LotkaVolterra` -- the same factored Euler–Maruyama step and statistics -- with its noise, state and step in binary32: a
`DeviceSource` of device_sources/lotka_volterra_f32.hip, two steps per Philox block through `rng.for_quads_f32`.  θ, params and ρ
stay Float64.
"""
function LotkaVolterraF32(; n_steps::Integer=256, dt=0.05, σ=0.1, x0=50.0, y0=50.0, obs=(0.0, 0.0, 0.0, 0.0), n_stats::Integer=4)
    n_steps >= 2 || throw(ArgumentError("n_steps must be at least 2"))
    n_stats in 1:4 || throw(ArgumentError("n_stats is 1..4"))
    length(obs) == 4 || throw(ArgumentError("obs holds (mean X, sd X, mean Y, sd Y)"))
    text = read(joinpath(@__DIR__, "..", "device_sources", "lotka_volterra_f32.hip"), String)
    DeviceSource("#define LV_N_STATS $(n_stats)\n" * text, 3, Int(n_stats), Float64[n_steps, dt, σ, x0, y0, obs...])
end
"""
    NormalMoments(; y_obs=nothing)

The `f_dist` of the reference's getting-started example (docs/src/usage.md:15-35) on the device: θ = (μ, σ), `length(y_obs)` draws
of Normal(μ, σ), ρ = (|mean(y_obs) − mean(y_sim)|, |Σ y_obs² − Σ y_sim²|).  `y_obs` is data: give it here or, the reference's
call shape, as `sabc(model, prior; y_obs=...)` / `update_population!(res, model, prior; y_obs=...)`.
"""
NormalMoments(; y_obs=nothing) =
    DeviceSource(read(joinpath(@__DIR__, "..", "device_sources", "normal_moments.hip"), String), 2, 2;
                 data=y_obs === nothing ? nothing : (y_obs,), data_names=(:y_obs,), validate=check_moments_data)
check_moments_data(segs) = (length(segs) == 1 && length(segs[1]) >= 1) || throw(ArgumentError("y_obs holds at least one value"))

"""
    StochasticSIRSeries(; t_obs=nothing, I_obs=nothing, S0=99, I0=1, R0=0, t_max=160.0)

The Gillespie epidemic of `StochasticSIR` compared with a whole observed curve: two data segments, `t_obs` (increasing) and
`I_obs`; ρ = (mean_k |I(t_k) − I_obs[k]|,), I(t_k) the number infected just before the first event later than t_k.
"""
function StochasticSIRSeries(; t_obs=nothing, t_max=160.0, rest...)
    # keywords I_obs and S0, I0, R0 (the reference's spelling), collected here so that the defaults sit next to their names
    kw = values(rest)
    i_obs = get(kw, :I_obs, nothing)
    c = merge(NamedTuple{(Symbol("S0"), Symbol("I0"), Symbol("R0"))}((99, 1, 0)), Base.structdiff(kw, NamedTuple{(:I_obs,)}))
    length(c) == 3 || throw(ArgumentError("unknown keyword: I_obs and the compartments S0, I0, R0"))
    s0, i0, r0 = Int(c[1]), Int(c[2]), Int(c[3])
    (s0 >= 0 && r0 >= 0 && i0 >= 1) || throw(ArgumentError("compartments must be non-negative, I0 at least 1"))
    (t_obs === nothing) == (i_obs === nothing) || throw(ArgumentError("t_obs and I_obs come together"))
    DeviceSource(read(joinpath(@__DIR__, "..", "device_sources", "sir_series.hip"), String), 2, 1; params=Float64[s0, i0, r0, t_max],
                 data=t_obs === nothing ? nothing : (t_obs, i_obs), data_names=(:t_obs, :I_obs), validate=check_series_data)
end
# the source reads I_obs[k] for every k < length(t_obs): a shorter I_obs would be read past its end
check_series_data(segs) = (length(segs) == 2 && length(segs[1]) == length(segs[2]) >= 1 && issorted(segs[1]; lt=<=)) ||
    throw(ArgumentError("t_obs is increasing, holds at least one value and is as long as I_obs"))

"""
    GandKQuantiles(probs, q_obs; n_draws=128, c=0.8, team_lanes=nothing)
    GandKQuantiles(y_obs; probs=(1:7) ./ 8, n_draws=length(y_obs), c=0.8, team_lanes=nothing)

g-and-k, θ = (A, B, g, k), with any number of draws and any set of quantiles: ρ_j = |quantile(x_sim, probs[j]) − q_obs[j]| with
Julia's default `quantile`.  Two data segments, `probs` and `q_obs` (1 to 16 values each); the second method takes `q_obs`
from a sample.  A `DeviceSource` of device_sources/gk_quantiles.hip, which sorts the draws with `sabc::sort_ascending`.
`team_lanes` = 1, 4 or 16: its team-aware form -- the sample in a `sabc::Sample`, drawn and sorted by that many lanes together.
"""
function GandKQuantiles(probs, q_obs; n_draws::Integer=128, c=0.8, team_lanes=nothing)
    2 <= n_draws <= 1024 || throw(ArgumentError("n_draws must be in 2..1024"))
    1 <= length(probs) <= 16 || throw(ArgumentError("1 to 16 quantiles"))
    text = read(joinpath(@__DIR__, "..", "device_sources", "gk_quantiles.hip"), String)
    n_q = length(probs)
    team = team_lanes === nothing ? "" : "#define GKQ_TEAM 1\n"
    DeviceSource("#define GKQ_N_DRAWS $(n_draws)\n#define GKQ_N_STATS $(n_q)\n" * team * text, 4, n_q; params=Float64[n_draws, c],
                 data=(probs, q_obs), data_names=(:probs, :q_obs), validate=segs -> check_quantile_data(segs, n_q), team_lanes=team_lanes)
end
GandKQuantiles(y_obs; probs=(1:7) ./ 8, n_draws::Integer=length(y_obs), c=0.8, team_lanes=nothing) =
    GandKQuantiles(probs, type7_quantiles(sort(data_segment(y_obs)), probs); n_draws=n_draws, c=c, team_lanes=team_lanes)
# Julia's default quantile (Statistics.quantile, type 7) of an ascending vector, without the dependency
function type7_quantiles(x, probs)
    map(probs) do p
        h = (length(x) - 1) * clamp(p, 0.0, 1.0)
        i = floor(Int, h)
        i >= length(x) - 1 ? x[end] : x[i + 1] + (h - i) * (x[i + 2] - x[i + 1])
    end
end
# the source reads probs[j] and q_obs[j] and writes ρ[j] for every j < n_stats
check_quantile_data(segs, n_q) = (length(segs) == 2 && length(segs[1]) == length(segs[2]) == n_q && all(p -> 0 <= p <= 1, segs[1])) ||
    throw(ArgumentError("probs and q_obs hold $(n_q) values each, every probability in [0, 1]"))
"""
    GandKSample(y_obs; distance=(:wasserstein, :ks), n_draws=length(y_obs), c=0.8, team_lanes=nothing)

g-and-k, θ = (A, B, g, k), compared with the observed sample as a whole: `distance` = `:wasserstein` (ρ = Σ_i |x_(i) − y_(i)| / n
between the sorted samples; `n_draws == length(y_obs)`), `:ks` (Kolmogorov–Smirnov; any two lengths) or both, one statistic per
name in the order given.  One data segment, `y_obs`, kept sorted (the constructor sorts it; data that arrive with a call must be
ascending).  A `DeviceSource` of device_sources/gk_sample.hip on `sabc::tree_sum`, `sabc::count_less` and `sabc::count_less_equal`
(csrc/sample_reduce.hpp); `team_lanes` = 1, 4 or 16: the same through `sabc::Sample` (`wasserstein1`, `ks`), the same bits.
"""
GandKSample(y_obs; distance=(:wasserstein, :ks), n_draws::Integer=length(y_obs), c=0.8, team_lanes=nothing) =
    gk_sample_source("gk_sample.hip", team_lanes === nothing ? "" : "#define GKS_TEAM 1\n", y_obs, distance, n_draws, c, team_lanes)
"""
    GandKSampleF32(y_obs; distance=(:wasserstein, :ks), n_draws=length(y_obs), c=0.8, team_lanes=4)

`GandKSample` with a binary32 sample: the stream's binary32 normals, four per Philox block, the f64 g-and-k transform of the widened
normal rounded to binary32 once, kept and sorted as floats in a `sabc::SampleF32` (csrc/team_sample_f32.hpp); both distances
accumulate in Float64 against `y_obs`, which stays Float64.  A `DeviceSource` of device_sources/gk_sample_f32.hip, which has the
team-aware form only: `team_lanes` = 1, 4 or 16 (`nothing`: use `GandKSample`), the same bits for the three.
"""
function GandKSampleF32(y_obs; distance=(:wasserstein, :ks), n_draws::Integer=length(y_obs), c=0.8, team_lanes=4)
    team_lanes === nothing &&
        throw(ArgumentError("team_lanes is 1, 4 or 16: GandKSampleF32 has the team-aware form only; the plain-array form is GandKSample"))
    gk_sample_source("gk_sample_f32.hip", "", y_obs, distance, n_draws, c, team_lanes)
end
function gk_sample_source(file, team, y_obs, distance, n_draws, c, team_lanes)
    names = distance isa Union{Symbol,String} ? (Symbol(distance),) : Tuple(Symbol(d) for d in distance)
    (!isempty(names) && allunique(names) && all(d -> d in (:wasserstein, :ks), names)) ||
        throw(ArgumentError("distance is :wasserstein, :ks or both, each once"))
    1 <= n_draws <= 1024 || throw(ArgumentError("n_draws must be in 1..1024"))
    text = read(joinpath(@__DIR__, "..", "device_sources", file), String)
    head = "#define GKS_N_DRAWS $(n_draws)\n" * join("#define GKS_$(uppercase(String(d))) $(j - 1)\n" for (j, d) in enumerate(names))
    rank_with_rank = :wasserstein in names
    DeviceSource(head * team * text, 4, length(names); params=Float64[n_draws, c], data=(sort(data_segment(y_obs)),), data_names=(:y_obs,),
                 validate=segs -> check_sample_data(segs, Int(n_draws), rank_with_rank), team_lanes=team_lanes)
end
# the source reads y[i] for every i < n_draws (:wasserstein) and searches an ascending y (:ks); the counts are exact below 2^53
check_sample_data(segs, n_draws, rank_with_rank) =
    (length(segs) == 1 && length(segs[1]) >= 1 && all(isfinite, segs[1]) && issorted(segs[1]) &&
     (!rank_with_rank || length(segs[1]) == n_draws) && n_draws * length(segs[1]) < 2^53) ||
    throw(ArgumentError("y_obs is one ascending segment of finite values" * (rank_with_rank ? ", $(n_draws) of them (distance :wasserstein)" : "")))
"""
    MA2(; acov_obs=nothing, n_obs=100, n_lags=2, team_lanes=nothing)
    MA2(y_obs; n_lags=2, team_lanes=nothing)

MA(2) with autocovariance summaries (Marin et al. 2012): θ = (θ1, θ2), y_t = e_{t+2} + θ1 e_{t+1} + θ2 e_t for `n_obs` times,
τ_j = Σ_{t ≥ j} y_t y_{t−j} / n_obs for j = 0 .. `n_lags` (at most 7), ρ_j = |τ_j − acov_obs[j]|.  One data segment, `acov_obs`, of
`n_lags + 1` finite values; the second method takes it from an observed series (`ma2_autocovariances`: the device's own sum).
A `DeviceSource` of device_sources/ma2.hip on `sabc::Series` (csrc/team_series.hpp): the innovations in time order over the
team, `lag<1>`, `lag<2>` and two `zip`s, `autocovariance<j>`.  `team_lanes` = 1, 4 or 16: that many lanes per particle, the same
bits as the default (`nothing`: a private array per lane).
"""
function MA2(; acov_obs=nothing, n_obs::Integer=100, n_lags::Integer=2, team_lanes=nothing)
    0 <= n_lags <= 7 || throw(ArgumentError("n_lags must be in 0..7"))
    n_lags < n_obs <= 1022 || throw(ArgumentError("n_obs must be above n_lags and at most 1022"))
    text = read(joinpath(@__DIR__, "..", "device_sources", "ma2.hip"), String)
    head = "#define MA2_N_OBS $(n_obs)\n#define MA2_N_LAGS $(n_lags)\n" * (team_lanes === nothing ? "" : "#define MA2_TEAM 1\n")
    DeviceSource(head * text, 2, Int(n_lags) + 1; params=Float64[n_obs, n_lags], data=acov_obs === nothing ? nothing : (acov_obs,),
                 data_names=(:acov_obs,), validate=segs -> check_acov_data(segs, Int(n_lags)), team_lanes=team_lanes)
end
MA2(y_obs; n_lags::Integer=2, team_lanes=nothing) =
    MA2(; acov_obs=ma2_autocovariances(data_segment(y_obs), n_lags), n_obs=length(y_obs), n_lags=n_lags, team_lanes=team_lanes)
# the source reads acov_obs[j] and writes ρ[j] for every j <= n_lags
check_acov_data(segs, n_lags) = (length(segs) == 1 && length(segs[1]) == n_lags + 1 && all(isfinite, segs[1])) ||
    throw(ArgumentError("acov_obs is one segment of $(n_lags + 1) finite values"))
# the canonical sum of csrc/sample_reduce.hpp: the balanced binary tree over the index, padded with +0.0 to a power of two, + 0.0 last
function tree_sum(s)
    a = vcat(collect(Float64, s), zeros(nextpow(2, max(length(s), 1)) - length(s)))
    while length(a) > 1
        a = a[1:2:end] .+ a[2:2:end]
    end
    a[1] + 0.0
end
# τ_0 .. τ_n_lags as the device computes them: rounded products, the tree over the innovations' n + 2 times (two leading zeros)
ma2_autocovariances(y, n_lags) =
    Float64[tree_sum(vcat(zeros(2 + j), y[(j + 1):end] .* y[1:(end - j)])) / length(y) for j in 0:n_lags]
"""
    GARCH11(; summaries_obs=nothing, n_obs=100, n_lags=2, sigma2_0=1.0, team_lanes=nothing)
    GARCH11(y_obs; n_lags=2, team_lanes=nothing)

GARCH(1,1): θ = (ω, α, β), y_t = σ_t z_t and σ²_{t+1} = ω + α y_t² + β σ²_t for `n_obs` times from σ²_0 = `sigma2_0` (a positive
number; the second method sets it to the mean of y_obs²).  Summaries of r_t = y_t²: the mean and the autocovariances about it at
lags 0 .. `n_lags` (at most 7), ρ_0 = |mean(r) − obs[0]|, ρ_{1+j} = |acov_j(r) − obs[1+j]|.  One data segment, `summaries_obs`, of
`n_lags + 2` finite values; the second method takes it from an observed series of returns (`garch11_summaries`: the device's own
sums).  A `DeviceSource` of device_sources/garch11.hip on `sabc::Series::recur` (csrc/team_series.hpp): one recurrence in time
order over the normals.  `team_lanes` = 1, 4 or 16: that many lanes per particle, the state relayed from lane to lane, the same
bits as the default (`nothing`: a private array per lane).
"""
function GARCH11(; summaries_obs=nothing, n_obs::Integer=100, n_lags::Integer=2, sigma2_0::Real=1.0, team_lanes=nothing)
    0 <= n_lags <= 7 || throw(ArgumentError("n_lags must be in 0..7"))
    n_lags < n_obs <= 1024 || throw(ArgumentError("n_obs must be above n_lags and at most 1024"))
    (isfinite(sigma2_0) && sigma2_0 > 0) || throw(ArgumentError("sigma2_0 must be a positive finite number"))
    text = read(joinpath(@__DIR__, "..", "device_sources", "garch11.hip"), String)
    head = "#define GARCH11_N_OBS $(n_obs)\n#define GARCH11_N_LAGS $(n_lags)\n" * (team_lanes === nothing ? "" : "#define GARCH11_TEAM 1\n")
    DeviceSource(head * text, 3, Int(n_lags) + 2; params=Float64[n_obs, n_lags, sigma2_0],
                 data=summaries_obs === nothing ? nothing : (summaries_obs,), data_names=(:summaries_obs,),
                 validate=segs -> check_garch11_data(segs, Int(n_lags)), team_lanes=team_lanes)
end
function GARCH11(y_obs; n_lags::Integer=2, team_lanes=nothing)
    obs = garch11_summaries(data_segment(y_obs), n_lags)
    GARCH11(; summaries_obs=obs, n_obs=length(y_obs), n_lags=n_lags, sigma2_0=obs[1], team_lanes=team_lanes)
end
# the source reads summaries_obs[j] and writes ρ[j] for every j < n_lags + 2
check_garch11_data(segs, n_lags) = (length(segs) == 1 && length(segs[1]) == n_lags + 2 && all(isfinite, segs[1])) ||
    throw(ArgumentError("summaries_obs is one segment of $(n_lags + 2) finite values"))
# mean(r), acov_0(r) .. acov_n_lags(r) of r = y² as the device computes them: rounded products, the tree over the n times
function garch11_summaries(y, n_lags)
    r = y .* y
    c = tree_sum(r) / length(r)
    d = r .- c
    vcat(c, Float64[tree_sum(vcat(zeros(j), d[(j + 1):end] .* d[1:(end - j)])) / length(r) for j in 0:n_lags])
end
"""
    Ricker(; summaries_obs=nothing, n_obs=50, burn_in=50, n_lags=5, n0=1.0, team_lanes=nothing)
    Ricker(y_obs; burn_in=50, n_lags=5, n0=1.0, team_lanes=nothing)

The Ricker map with Poisson observations (Wood 2010): θ = (log r, σ, φ), N_{t+1} = r N_t exp(−N_t + σ z_t) from N_0 = `n0` for
`burn_in + n_obs` times, y_t ~ Poisson(φ N_{t+1}), the last `n_obs` counts observed.  Summaries: the mean, the number of zeros and
the autocovariances about the mean at lags 0 .. `n_lags` (at most 7): ρ_0 = |mean(y) − obs[0]|, ρ_1 = |#{y_t = 0} − obs[1]|,
ρ_{2+j} = |acov_j(y) − obs[2+j]|.  One data segment, `summaries_obs`, of `n_lags + 3` finite values; the second method takes it
from an observed series of counts (`ricker_summaries`: the device's own sums).  A `DeviceSource` of device_sources/ricker.hip on
`sabc::Series` (csrc/team_series.hpp): one recurrence in time order, then `map_poisson` -- count draws keyed by the time step
(`sabc::CountDraws`), which a team divides among its lanes.  `team_lanes` = 1, 4 or 16: that many lanes per particle, the same
bits as the default (`nothing`: a private array per lane).
"""
function Ricker(; summaries_obs=nothing, n_obs::Integer=50, burn_in::Integer=50, n_lags::Integer=5, n0::Real=1.0, team_lanes=nothing)
    0 <= n_lags <= 7 || throw(ArgumentError("n_lags must be in 0..7"))
    n_lags < n_obs || throw(ArgumentError("n_obs must be above n_lags"))
    (burn_in >= 0 && burn_in + n_obs <= 1024) || throw(ArgumentError("burn_in must be non-negative and burn_in + n_obs at most 1024"))
    (isfinite(n0) && n0 > 0) || throw(ArgumentError("n0 must be a positive finite number"))
    text = read(joinpath(@__DIR__, "..", "device_sources", "ricker.hip"), String)
    head = "#define RICKER_N_OBS $(n_obs)\n#define RICKER_BURN_IN $(burn_in)\n#define RICKER_N_LAGS $(n_lags)\n" *
           (team_lanes === nothing ? "" : "#define RICKER_TEAM 1\n")
    DeviceSource(head * text, 3, Int(n_lags) + 3; params=Float64[n_obs, burn_in, n_lags, n0],
                 data=summaries_obs === nothing ? nothing : (summaries_obs,), data_names=(:summaries_obs,),
                 validate=segs -> check_ricker_data(segs, Int(n_lags)), team_lanes=team_lanes)
end
function Ricker(y_obs; burn_in::Integer=50, n_lags::Integer=5, n0::Real=1.0, team_lanes=nothing)
    obs = ricker_summaries(data_segment(y_obs), n_lags, burn_in)
    Ricker(; summaries_obs=obs, n_obs=length(y_obs), burn_in=burn_in, n_lags=n_lags, n0=n0, team_lanes=team_lanes)
end
# the source reads summaries_obs[j] and writes ρ[j] for every j < n_lags + 3
check_ricker_data(segs, n_lags) = (length(segs) == 1 && length(segs[1]) == n_lags + 3 && all(isfinite, segs[1])) ||
    throw(ArgumentError("summaries_obs is one segment of $(n_lags + 3) finite values"))
# mean(y), #{y_t = 0}, acov_0(y) .. acov_n_lags(y) as the device computes them: the tree over the burn_in + n times, the burn-in's
# terms +0.0, rounded products, divided by n
function ricker_summaries(y, n_lags, burn_in)
    lead = zeros(burn_in)
    c = tree_sum(vcat(lead, y)) / length(y)
    d = y .- c
    vcat(c, tree_sum(vcat(lead, Float64.(y .== 0))),
         Float64[tree_sum(vcat(lead, zeros(j), d[(j + 1):end] .* d[1:(end - j)])) / length(y) for j in 0:n_lags])
end
"""
    SourcePrior(d)

ANY prior of `d` parameters next to a `DeviceSource`: its HIP source defines `sabc_user_prior_sample` / `sabc_user_prior_logpdf`
(include/sabc_hip.h), and rand / logpdf of SimulatedAnnealingABC.jl:174,314,318 run inside the fused kernel.
"""
struct SourcePrior <: ContinuousMultivariateDistribution
    d::Int
end
Base.length(p::SourcePrior) = p.d
n_stats(m::HostDistance) = m.n_stats
params(::HostDistance) = Float64[]

# `@cfunction($cb, ...)` builds a runtime closure: supported on x86-64 / aarch64 Linux (where MI355X hosts run), not on
# every platform Julia supports.  The returned Base.CFunction must stay rooted for as long as the library may call it:
# it is kept in HOST_CALLBACKS until the handle's finalizer has run.
function host_callback(m::HostDistance)
    function cb(ctx::Ptr{Cvoid}, theta::Ptr{Float64}, ids::Ptr{Int64}, n::Int64, iter::UInt64, rho::Ptr{Float64})::Cint
        try
            Θ = unsafe_wrap(Array, theta, (Int(n), m.n_para))        # column-major n x d
            R = unsafe_wrap(Array, rho, (Int(n), m.n_stats))
            Threads.@threads for i in 1:n                             # like SimulatedAnnealingABC.jl:308
                θ = m.n_para == 1 ? Θ[i, 1] : Θ[i, :]
                R[i, :] .= collect(Float64, m.f(θ, m.args...; m.kwargs...))
            end
            return Cint(0)
        catch
            return Cint(-1)
        end
    end
    @cfunction($cb, Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Int64, UInt64, Ptr{Float64}))
end

# ---- priors as data: (kind, a, b, c, d) per dimension, include/sabc_hip.h SABC_PRIOR_* ----
prior_descriptor(d::Normal) = (Int32(0), d.μ, d.σ, 0.0, 0.0)
prior_descriptor(d::Uniform) = (Int32(1), d.a, d.b, 0.0, 0.0)
prior_descriptor(d::Exponential) = (Int32(2), d.θ, 0.0, 0.0, 0.0)
prior_descriptor(d::LogNormal) = (Int32(3), d.μ, d.σ, 0.0, 0.0)
prior_descriptor(d::Gamma) = (Int32(4), d.α, d.θ, 0.0, 0.0)
prior_descriptor(d::Beta) = (Int32(5), d.α, d.β, 0.0, 0.0)
prior_descriptor(d::Truncated{<:Normal}) = (Int32(6), d.untruncated.μ, d.untruncated.σ, Float64(d.lower), Float64(d.upper))
prior_descriptors(d::UnivariateDistribution) = [prior_descriptor(d)]
# MvNormal(mu, Sigma): mu travels in the per-dimension descriptors, the lower Cholesky factor of Sigma in prior_chol
prior_descriptors(d::MvNormal) = [(Int32(0), d.μ[k], sqrt(d.Σ[k, k]), 0.0, 0.0) for k in 1:length(d)]
prior_chol(d::Distribution) = (Int32(0), Float64[])
function prior_chol(d::MvNormal)
    n = length(d)
    L = cholesky(Symmetric(Matrix(d.Σ))).L
    (Int32(1), Float64[l <= k ? L[k, l] : 0.0 for k in 1:n for l in 1:n])        # row-major n x n
end
# product_distribution([...]): Distributions.jl names the vector of marginals `v` (Product, <= 0.25.x) or `dists`
# (ProductDistribution); neither has an exported accessor, so both spellings are accepted and anything else is refused
function prior_descriptors(d::Distribution)
    comps = hasproperty(d, :v) ? getproperty(d, :v) : hasproperty(d, :dists) ? getproperty(d, :dists) :
            error("prior must be Normal, Uniform, Exponential, LogNormal, Gamma, Beta, truncated(Normal), product_distribution([...]) of those, or MvNormal")
    [prior_descriptor(c) for c in comps]
end

# ANY other Distribution (SimulatedAnnealingABC.jl:151): rand(prior) (:174) and logpdf(prior, θ) (:314, :318) stay Julia calls,
# handed to the library as two host callbacks (sabc_set_host_prior, prior_joint = 2) -- next to a Julia `f_dist`, where the
# per-particle body is already cut at the host, or next to a device-coded one, which then runs as its own launch between the
# proposal and the accept kernel.
is_data_prior(d::Distribution) =
    d isa MvNormal || d isa Union{Normal,Uniform,Exponential,LogNormal,Gamma,Beta,Truncated{<:Normal}} ||
    ((hasproperty(d, :v) || hasproperty(d, :dists)) &&
     all(c -> c isa Union{Normal,Uniform,Exponential,LogNormal,Gamma,Beta,Truncated{<:Normal}}, hasproperty(d, :v) ? d.v : d.dists))

function host_prior_callbacks(prior::Distribution)
    d = length(prior)
    function sample_cb(ctx::Ptr{Cvoid}, m::Int64, ids::Ptr{Int64}, theta::Ptr{Float64})::Cint
        try
            Θ = unsafe_wrap(Array, theta, (Int(m), d))                # column-major m x d
            for i in 1:m
                Θ[i, :] .= rand(prior)
            end
            return Cint(0)
        catch
            return Cint(-1)
        end
    end
    function logpdf_cb(ctx::Ptr{Cvoid}, m::Int64, theta::Ptr{Float64}, lp::Ptr{Float64})::Cint
        try
            Θ = unsafe_wrap(Array, theta, (Int(m), d))
            L = unsafe_wrap(Array, lp, (Int(m),))
            Threads.@threads for i in 1:m
                L[i] = d == 1 ? logpdf(prior, Θ[i, 1]) : logpdf(prior, Θ[i, :])
            end
            return Cint(0)
        catch
            return Cint(-1)
        end
    end
    (@cfunction($sample_cb, Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64})),
     @cfunction($logpdf_cb, Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64})))
end

# ---- result types: same field names as SimulatedAnnealingABC.jl:28-60 ----
mutable struct SABCstate
    ϵ::Vector{Float64}
    algorithm::Symbol
    ϵ_history::Vector{Vector{Float64}}
    ρ_history::Vector{Vector{Float64}}
    u_history::Vector{Vector{Float64}}
    cdfs_dist_prior
    n_simulation::Int
    n_accept::Int
    n_resampling::Int
    n_population_updates::Int
end

struct SABCresult{T,S}                  # the reference's four fields, nothing else (:55-60)
    population::Vector{T}
    u::Array{S}
    ρ::Array{S}
    state::SABCstate
end

# The device-resident population behind a result: a side table keyed by the (mutable) state object, so that the handle
# lives exactly as long as the result and SABCresult keeps the reference's constructor.
const HANDLES = WeakKeyDict{SABCstate,Base.RefValue{Ptr{Cvoid}}}()
handle_of(res::SABCresult) = get(() -> error("this SABCresult has no device population (it was not created by sabc of SimulatedAnnealingABCHIP)"),
                                 HANDLES, res.state)

function check(h::Ptr{Cvoid}, rc::Integer)
    rc == 0 && return
    msg = unsafe_string(h == C_NULL ? ccall((:sabc_last_global_error, libsabc), Cstring, ()) :
                                      ccall((:sabc_last_error, libsabc), Cstring, (Ptr{Cvoid},), h))
    error(msg)                           # ErrorException, like the reference's error(...) sites
end

padtuple(v, n, T) = ntuple(i -> i <= length(v) ? T(v[i]) : zero(T), n)

"""
    comm_unique_id() -> Vector{UInt8}

The 128-byte RCCL id of a multi-GPU run: rank 0 calls this and hands the bytes to the other ranks (MPI.jl `bcast`, a
file, a socket ...); every rank then passes them as `comm_id` to `sabc`.
"""
function comm_unique_id()
    id = Vector{UInt8}(undef, 128)
    check(C_NULL, ccall((:sabc_comm_unique_id, libsabc), Cint, (Ptr{Cvoid},), id))
    id
end

function create_handle(f_dist::DeviceDistance, prior; n_particles, algorithm, v, δ, seed, device=0, rank=0, world=1,
                       comm_id=nothing, p2p=true)
    source_prior = prior isa SourcePrior
    source_prior && !(f_dist isa DeviceSource) && error("a SourcePrior is device code inside the HIP source of a DeviceSource")
    host_prior = !source_prior && !is_data_prior(prior)
    pd = (host_prior || source_prior) ? [(Int32(0), 0.0, 1.0, 0.0, 0.0) for _ in 1:length(prior)] : prior_descriptors(prior)
    joint, chol = host_prior ? (Int32(2), Float64[]) : source_prior ? (Int32(3), Float64[]) : prior_chol(prior)
    p = params(f_dist)
    cfg = Ref(CConfig(6, device, n_particles, length(pd), n_stats(f_dist), model_id(f_dist), length(p),
                      padtuple(p, MAX_MODEL_PARAMS, Float64),
                      padtuple(first.(pd), MAX_PARA, Int32),
                      padtuple(getindex.(pd, 2), MAX_PARA, Float64), padtuple(getindex.(pd, 3), MAX_PARA, Float64),
                      padtuple(getindex.(pd, 4), MAX_PARA, Float64), padtuple(getindex.(pd, 5), MAX_PARA, Float64),
                      joint, Int32(0), padtuple(chol, MAX_PARA2, Float64),
                      algorithm == :multi_eps ? 1 : 0, rank, world, 0, v, δ, seed))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(C_NULL, ccall((:sabc_create, libsabc), Cint, (Ref{CConfig}, Ref{Ptr{Cvoid}}), cfg, h))
    # A finalizer runs whenever the collector pleases, at a different time on every rank: it must neither free memory a peer
    # shard may be reading nor wait for peers.  sabc_destroy takes care of the first in any case (the shard LEAVES its
    # peer-to-peer group in order, include/sabc_hip.h "LEAVING"); a destroy wait of 0 makes it park what a peer has not
    # released instead of waiting for it.  `close(res)` is the orderly way out: it waits (bounded) and frees.
    finalizer(h) do r
        if r[] != C_NULL
            ccall((:sabc_comm_p2p_set_destroy_wait, libsabc), Cint, (Ptr{Cvoid}, Cdouble), r[], 0.0)
            ccall((:sabc_destroy, libsabc), Cvoid, (Ptr{Cvoid},), r[])
            delete!(HOST_CALLBACKS, r[])               # the library can no longer call back: release the closure
            r[] = C_NULL
        end
    end
    if world > 1                                       # one process per GPU: RCCL bound inside the library
        (comm_id isa Vector{UInt8} && length(comm_id) == 128) ||
            error("world > 1 needs `comm_id`: the 128 bytes of comm_unique_id() from rank 0")
        GC.@preserve comm_id check(h[], ccall((:sabc_comm_init_rccl, libsabc), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h[], comm_id))
        check(h[], ccall((:sabc_comm_selftest, libsabc), Cint, (Ptr{Cvoid},), h[]))
        # on top of RCCL: the peer-to-peer transport (the shards of one node exchange through each other's HBM: one launch per
        # population update instead of reduce -> allreduce -> control).  ONE collective call: the descriptors travel over
        # the RCCL allgather just installed, every rank maps its peers and runs the self-test, and the ranks AGREE inside the
        # library after every step -- either all of them now run peer to peer (1) or all of them stay on RCCL (0): no rank
        # switches alone and leaves the others to wait out the bound of their first exchange.
        if p2p && world <= 8 && !(f_dist isa HostDistance)
            rc = ccall((:sabc_comm_p2p_setup, libsabc), Cint, (Ptr{Cvoid},), h[])
            rc < 0 && check(h[], rc)
        end
    end
    if f_dist isa DeviceSource
        if f_dist.team_lanes == 0
            check(h[], ccall((:sabc_register_device_simulator, libsabc), Cint, (Ptr{Cvoid}, Cstring), h[], f_dist.source))
        else
            check(h[], ccall((:sabc_register_device_simulator_team, libsabc), Cint, (Ptr{Cvoid}, Cstring, Int32), h[], f_dist.source,
                             Int32(f_dist.team_lanes)))
        end
        isempty(f_dist.data) || set_device_data!(h[], f_dist.data)
    end
    if f_dist isa HostDistance
        cb = host_callback(f_dist)
        pcb = host_prior ? host_prior_callbacks(prior) : nothing
        HOST_CALLBACKS[h[]] = (cb, f_dist, pcb, prior) # keep the closures (and what they wrap) alive with the handle
        check(h[], ccall((:sabc_set_host_simulator, libsabc), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h[], cb, C_NULL))
        if host_prior
            check(h[], ccall((:sabc_set_host_prior, libsabc), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                             h[], pcb[1], pcb[2], C_NULL))
        end
    elseif host_prior                                  # any Distribution next to a device-coded simulator
        pcb = host_prior_callbacks(prior)
        HOST_CALLBACKS[h[]] = (nothing, f_dist, pcb, prior)
        check(h[], ccall((:sabc_set_host_prior, libsabc), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                         h[], pcb[1], pcb[2], C_NULL))
    end
    h
end
const HOST_CALLBACKS = Dict{Ptr{Cvoid},Any}()

# the reference's own signature (SimulatedAnnealingABC.jl:451): any Function; the number of statistics is
# probed with one call on a prior draw, as at :163-165
function sabc(f_dist::Function, prior::Distribution, args...; kwargs...)
    f_dist isa DeviceDistance && return invoke(sabc, Tuple{DeviceDistance,Distribution}, f_dist, prior; kwargs...)
    own = (:n_particles, :n_simulation, :algorithm, :proposal, :resample, :v, :δ, :checkpoint_history,
           :show_progressbar, :show_checkpoint, :seed, :device, :rank, :world, :comm_id)
    mine = (; (k => v for (k, v) in kwargs if k in own)...)
    theirs = (; (k => v for (k, v) in kwargs if !(k in own))...)
    ρ = f_dist(rand(prior), args...; theirs...)
    hd = HostDistance(f_dist, length(ρ), length(prior), args, theirs)
    invoke(sabc, Tuple{DeviceDistance,Distribution}, hd, prior; mine...)
end

# copies device state into the Julia arrays in place (`.=` at SimulatedAnnealingABC.jl:395-397)
function refresh!(res::SABCresult, d::Int, s::Int)
    h = handle_of(res)[]
    n = length(res.population)
    θ = Matrix{Float64}(undef, n, d)               # column-major n x d == the library's [d][n]
    GC.@preserve θ check(h, ccall((:sabc_get_population, libsabc), Cint,
                                  (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, θ, res.u, res.ρ))
    if eltype(res.population) <: Real
        res.population .= vec(θ)
    else
        for i in 1:n
            res.population[i] = θ[i, :]
        end
    end
    st = res.state
    eps = Vector{Float64}(undef, MAX_STATS); len = Ref{Int32}(0)
    check(h, ccall((:sabc_get_epsilon, libsabc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Int32}), h, eps, len))
    st.ϵ = eps[1:len[]]
    c = Vector{Int64}(undef, 4)
    check(h, ccall((:sabc_get_counters, libsabc), Cint, (Ptr{Cvoid}, Ptr{Int64}), h, c))
    st.n_simulation, st.n_accept, st.n_resampling, st.n_population_updates = c
    m = ccall((:sabc_history_len, libsabc), Int64, (Ptr{Cvoid},), h)
    le = length(st.ϵ)
    eh = Matrix{Float64}(undef, le, m); uh = Matrix{Float64}(undef, s, m); rh = Matrix{Float64}(undef, s, m)
    check(h, ccall((:sabc_get_history, libsabc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, eh, uh, rh))
    st.ϵ_history = [eh[:, k] for k in 1:m]; st.u_history = [uh[:, k] for k in 1:m]; st.ρ_history = [rh[:, k] for k in 1:m]
    res
end

# ---- outputs of a simulator from source: what its HIP text hands to sabc::emit(rng, i, v) (include/sabc_hip.h, OUTPUTS) ----
# θ: m x d, column-major == the library's [d][m]; row i runs as particle pid0 + i - 1 at iteration `iter`, on the stream its
# update simulated on or (predict) on a stream no update uses.  -> (ρ m x s, out m x n_out), NaN where nothing was emitted
function forward_run(h::Ptr{Cvoid}, θ::Matrix{Float64}, s::Integer, pid0::Integer, iter::Integer, predict::Bool, n_out::Integer)
    m = size(θ, 1)
    ρ = Matrix{Float64}(undef, m, s)
    out = Matrix{Float64}(undef, m, n_out)
    GC.@preserve θ ρ out check(h, ccall((:sabc_op_simulate_outputs, libsabc), Cint,
                                        (Ptr{Cvoid}, Ptr{Float64}, Int64, UInt64, UInt64, Int32, Int32, Ptr{Float64}, Ptr{Float64}),
                                        h, θ, m, pid0, iter, predict ? 1 : 0, n_out, ρ, out))
    ρ, out
end

"""
    simulate_outputs(f_dist::DeviceSource, θ, n_out; n_rep=1, seed, device=0, data...) -> Array (m, n_rep, n_out)

A forward run without a population: what the source of `f_dist` emits for every row of `θ` (m x d), `n_rep` times.  `data...`
are bound as `sabc` binds them.  Row i, replicate j is particle i - 1 at iteration j - 1 on the predictive streams of `seed`.
"""
function simulate_outputs(f_dist::DeviceSource, θ::AbstractMatrix, n_out::Integer; n_rep::Integer=1, seed=rand(UInt64) >> 1,
                          device=0, data...)
    segs = bind_data(f_dist, data)
    segs === nothing || (f_dist = with_data(f_dist, segs))
    !isempty(f_dist.data_names) && isempty(f_dist.data) &&
        throw(ArgumentError("the model has no data: give them at construction or to this call, data_names = $(f_dist.data_names)"))
    size(θ, 2) == f_dist.n_para || throw(ArgumentError("θ is m x $(f_dist.n_para)"))
    prior = MvNormal(zeros(f_dist.n_para), 1.0)          # the handle wants a prior; a forward run never consults it
    h = create_handle(f_dist, prior; n_particles=128, algorithm=:single_eps, v=1.0, δ=0.1, seed, device)
    th = collect(Float64, θ)
    res = Array{Float64}(undef, size(th, 1), n_rep, n_out)
    for j in 1:n_rep
        res[:, j, :] = forward_run(h[], th, f_dist.n_stats, 0, j - 1, true, n_out)[2]
    end
    finalize(h)
    res
end

"""
    posterior_predictive(res::SABCresult, n_out; n_rep=1, return_distances=false) -> Array (n, n_rep, n_out)

Simulations at the particles of `res`, on its own handle and therefore the data it holds now; with `return_distances` also
the distances (n, n_rep, s).  Predictive streams: no update has drawn from them.  `res` is left untouched.
"""
function posterior_predictive(res::SABCresult, n_out::Integer; n_rep::Integer=1, return_distances::Bool=false)
    h = handle_of(res)[]
    n, s = size(res.ρ)
    th = eltype(res.population) <: Real ? reshape(collect(Float64, res.population), n, 1) :
         collect(Float64, transpose(reduce(hcat, res.population)))
    pid0 = ccall((:sabc_local_offset, libsabc), Int64, (Ptr{Cvoid},), h)
    out = Array{Float64}(undef, n, n_rep, n_out)
    dist = Array{Float64}(undef, n, n_rep, s)
    for j in 1:n_rep
        ρ, o = forward_run(h, th, s, pid0, j - 1, true, n_out)
        out[:, j, :] = o
        dist[:, j, :] = ρ
    end
    return_distances ? (out, dist) : out
end

# Check if a stream is logged (SimulatedAnnealingABC.jl:500)
is_logging(io) = isa(io, Base.TTY) == false || (get(ENV, "CI", nothing) == "true")

# Progress output needs the device loop to come up for air: `update_population!` is cut into several sabc_update calls.
# Returns the update counts after which a call ends: every multiple of `show_checkpoint` (:359), every step of the progress
# bar (a fiftieth of the run), and n_pop.  The cuts may fall anywhere: each call is told how many updates of the loop came
# before it (history_phase) and whether another follows (more_chunks_follow), so `ix % checkpoint_history` (:367) and the
# final push (:378-382) see the loop's own numbering -- `show_checkpoint` and `checkpoint_history` are independent moduli,
# as in the reference.  Same rule as progress_stops() in ../api.py.
function progress_stops(n_pop, show_checkpoint, show_progressbar)
    stops = Set{Int}([n_pop])
    if isfinite(show_checkpoint) && show_checkpoint >= 1
        union!(stops, Int(show_checkpoint):Int(show_checkpoint):(n_pop - 1))
    end
    if show_progressbar && n_pop > 0
        union!(stops, max(n_pop ÷ 50, 1):max(n_pop ÷ 50, 1):(n_pop - 1))
    end
    sort!(collect(stops))
end

# Where the next sabc_update call ends.  A call costs ~65 us beyond its updates, and ProgressMeter redraws every 0.1 s at most:
# progress-bar stops closer than 0.1 s of work (rate = population updates per second on the previous call, 0: unknown) are
# passed over; multiples of `show_checkpoint` and n_pop never are.  Same rule as next_stop() in ../api.py.
function next_stop(stops, n_pop, show_checkpoint, done, rate)
    target = done + (rate > 0 ? max(1, floor(Int, rate * 0.1)) : 1)
    chk = (isfinite(show_checkpoint) && show_checkpoint >= 1) ? Int(show_checkpoint) : 0
    for s in stops
        s <= done && continue
        (s >= target || s == n_pop || (chk > 0 && s % chk == 0)) && return s
    end
    n_pop
end

"""
    close(res::SABCresult)

Release the device population behind `res` now instead of whenever the collector finalizes it.  On a multi-GPU run this is
the orderly way out: the shard leaves its peer-to-peer group, waits (bounded) until its peers have unmapped its memory, and
frees it.  No barrier with the other ranks is needed -- a rank that is still inside `update_population!` when a peer closes
ends that call over RCCL (or with an error if RCCL is gone too), never with a memory fault.
"""
function Base.close(res::SABCresult)
    r = handle_of(res)
    if r[] != C_NULL
        ccall((:sabc_destroy, libsabc), Cvoid, (Ptr{Cvoid},), r[])
        delete!(HOST_CALLBACKS, r[])
        r[] = C_NULL
    end
    nothing
end

"""
    update_population!(population_state, f_dist, prior; n_simulation, v=1.0, δ=0.1, proposal, resample, checkpoint_history=1,
                       show_progressbar, show_checkpoint)

Same keywords and defaults as SimulatedAnnealingABC.jl:251-259.  Mutates and returns `population_state`.
"""
function update_population!(res::SABCresult, f_dist::DeviceDistance, prior::Distribution;
                            n_simulation, v=1.0, δ=0.1,
                            proposal::Proposal=DifferentialEvolution(n_para=length(prior)),
                            resample=nothing, checkpoint_history=1,
                            show_progressbar::Bool=!is_logging(stderr),
                            show_checkpoint=is_logging(stderr) ? 100 : Inf, data...)
    v <= 0 && error("Annealing speed `v` must be positive.")                       # :261
    δ <= 0 && error("Resamping intensity `δ` must be positive.")                   # :262
    h = handle_of(res)[]
    segs = bind_data(f_dist, data)                                                 # y_obs of this call, forwarded like :315
    segs === nothing || set_device_data!(h, segs)
    d, s = length(prior), size(res.u, 2)
    n_global = ccall((:sabc_n_global, libsabc), Int64, (Ptr{Cvoid},), h)           # == length(population) on one GPU
    resample = something(resample, 2 * n_global)                                   # :255
    θ = eltype(res.population) <: Real ? reshape(copy(res.population), :, 1) : permutedims(reduce(hcat, res.population))
    GC.@preserve θ check(h, ccall((:sabc_set_population, libsabc), Cint,
                                  (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, θ, res.u, res.ρ))
    kind, p0, p1 = descriptor(proposal)
    n_pop = n_simulation ÷ n_global                                                # :275
    n_pop > 0 && checkpoint_history == 0 && throw(DivideError())                   # `ix % checkpoint_history`, :367
    pmeter = Progress(n_pop; desc="$n_pop population updates:", output=stderr, enabled=show_progressbar)   # :290-291
    t_start = Dates.now()
    done = 0
    stops = progress_stops(n_pop, show_checkpoint, show_progressbar)
    rate, first = 0.0, true
    while first || done < n_pop                                                    # (n_pop = 0: one call)
        first = false
        stop = next_stop(stops, n_pop, show_checkpoint, done, rate)
        todo = stop - done
        budget = n_pop > 0 ? todo * n_global : n_simulation                        # a top-up below one update is a no-op (:275)
        args = Ref(CUpdateArgs(budget, v, δ, resample, checkpoint_history, kind, stop < n_pop ? 1 : 0, p0, p1, done))
        t_call = time()
        check(h, ccall((:sabc_update, libsabc), Cint, (Ptr{Cvoid}, Ref{CUpdateArgs}), h, args))
        rate = todo / max(time() - t_call, 1e-9)
        done = stop
        if show_progressbar || (isfinite(show_checkpoint) && show_checkpoint >= 1)
            eps = Vector{Float64}(undef, MAX_STATS); len = Ref{Int32}(0)
            check(h, ccall((:sabc_get_epsilon, libsabc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Int32}), h, eps, len))
            ϵ = round.(eps[1:len[]], sigdigits=4)
            show_progressbar && next!(pmeter; step=todo, showvalues=[("ϵ", ϵ)])    # :292,374
            if done > 0 && isfinite(show_checkpoint) && show_checkpoint >= 1 && done % Int(show_checkpoint) == 0   # :359-364
                eta = ((Dates.now() - t_start) ÷ done) * (n_pop - done)
                etastr = eta > Dates.Second(1) ? Dates.canonicalize(round(eta, Dates.Second)) : "< 1 Second"
                @info "Update $done of $n_pop. ϵ: $ϵ, ETA: $(etastr)"; flush(stderr)
            end
        end
    end
    show_progressbar && finish!(pmeter)
    if proposal isa RandomWalk
        Σ = Matrix{Float64}(undef, d, d)
        check(h, ccall((:sabc_get_proposal_sigma, libsabc), Cint, (Ptr{Cvoid}, Ptr{Float64}), h, Σ))
        d == 1 ? (proposal.Σ = Σ[1, 1]) : (proposal.Σ .= Σ)
    end
    refresh!(res, d, s)
    @info "All particles have been updated $(n_pop) times."; flush(stderr)          # :399
    res
end

# data by position: update_population!(res, model, prior, y_obs; ...) -> the keywords of data_names
update_population!(res::SABCresult, f_dist::DeviceSource, prior::Distribution, arg1, args...; kwargs...) =
    update_population!(res, f_dist, prior; positional_data(f_dist, (arg1, args...), kwargs)..., kwargs...)
sabc(f_dist::DeviceSource, prior::Distribution, arg1, args...; kwargs...) =
    sabc(f_dist, prior; positional_data(f_dist, (arg1, args...), kwargs)..., kwargs...)

# update_population!(res, f_dist, prior, args...; kwargs...) with the plain function the result was created
# with (SimulatedAnnealingABC.jl:251): look the wrapped model up by handle; args/kwargs go to f_dist (:315)
function update_population!(res::SABCresult, f_dist::Function, prior::Distribution, args...; kwargs...)
    f_dist isa DeviceDistance && return invoke(update_population!, Tuple{SABCresult,DeviceDistance,Distribution}, res, f_dist, prior; kwargs...)
    haskey(HOST_CALLBACKS, handle_of(res)[]) || error("this SABCresult was not created with a host `f_dist`")
    hd = HOST_CALLBACKS[handle_of(res)[]][2]
    (hd isa HostDistance && hd.f === f_dist) || error("`f_dist` differs from the one this SABCresult was initialised with")
    own = (:n_simulation, :v, :δ, :proposal, :resample, :checkpoint_history, :show_progressbar, :show_checkpoint)
    mine = (; (k => v for (k, v) in kwargs if k in own)...)
    invoke(update_population!, Tuple{SABCresult,DeviceDistance,Distribution}, res, hd, prior; mine...)
end

"""
    sabc(f_dist::DeviceDistance, prior; n_particles=100, n_simulation=10_000, algorithm=:single_eps, ...)

Same keywords as SimulatedAnnealingABC.jl:451-460, plus `seed` (Philox key), `device` and -- one process per GPU --
`rank`, `world`, `comm_id` (see `comm_unique_id`).  On a sharded run `n_particles` is the GLOBAL count, the result holds
this rank's shard and every rank must pass the same `seed`.
"""
function sabc(f_dist::DeviceDistance, prior::Distribution;
              n_particles=100, n_simulation=10_000, algorithm=:single_eps,
              proposal::Proposal=DifferentialEvolution(n_para=length(prior)),
              resample=2 * n_particles, v=1.0, δ=0.1, checkpoint_history=1,
              show_progressbar::Bool=!is_logging(stderr), show_checkpoint=is_logging(stderr) ? 100 : Inf,
              seed=nothing, device=0, rank=0, world=1, comm_id=nothing, data...)
    (algorithm == :multi_eps || algorithm == :single_eps) ||
        error("Argument `algorithm` must be :multi_eps or :single_eps, not `$algorithm`!")   # :462-464
    n_simulation < n_particles &&
        error("`n_simulation = $n_simulation` is too small for $n_particles particles.")     # :155-156
    world > 1 && isnothing(seed) && error("world > 1 needs an explicit `seed`: every shard must use the same Philox key")
    seed = something(seed, rand(UInt64) >> 1)
    @info "Initialization for '$(algorithm)'"                                                # :158
    segs = bind_data(f_dist, data)                       # y_obs = ... replaces what the model was constructed with
    segs === nothing || (f_dist = with_data(f_dist, segs))
    f_dist isa DeviceSource && !isempty(f_dist.data_names) && isempty(f_dist.data) &&
        throw(ArgumentError("the model has no data: give them at construction or to this call, data_names = $(f_dist.data_names)"))
    h = create_handle(f_dist, prior; n_particles, algorithm, v, δ, seed, device, rank, world, comm_id)
    check(h[], ccall((:sabc_initialize, libsabc), Cint, (Ptr{Cvoid}, Int64), h[], n_simulation))
    d, s = length(prior), n_stats(f_dist)
    n_local = ccall((:sabc_n_local, libsabc), Int64, (Ptr{Cvoid},), h[])
    T = d == 1 ? Float64 : Vector{Float64}
    pop = d == 1 ? zeros(n_local) : [zeros(d) for _ in 1:n_local]
    cdf = ρ -> begin
        out = Vector{Float64}(undef, s)
        r = collect(Float64, ρ)
        check(h[], ccall((:sabc_cdf_apply, libsabc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}), h[], r, 1, out))
        out
    end
    st = SABCstate(Float64[], algorithm, [], [], [], cdf, 0, 0, 0, 0)
    HANDLES[st] = h
    res = SABCresult{T,Float64}(pop, zeros(n_local, s), zeros(n_local, s), st)
    refresh!(res, d, s)
    n_sim_remaining = n_simulation - st.n_simulation                                         # :478
    n_sim_remaining < n_particles && @warn "`n_simulation` too small to update all particles!"
    update_population!(res, f_dist, prior; n_simulation=n_sim_remaining, resample, proposal, v, δ, checkpoint_history,
                       show_progressbar, show_checkpoint)
end

function show(io::IO, s::SABCresult)     # SimulatedAnnealingABC.jl:65-82
    n = length(s.population)
    println(io, "Approximate posterior sample with $n particles:")
    println(io, "  - algorithm: :$(s.state.algorithm)")
    println(io, "  - simulations used: $(s.state.n_simulation)")
    println(io, "  - number of population updates: $(s.state.n_population_updates)")
    println(io, "  - ϵ: $(round.(s.state.ϵ, sigdigits=4))")
    println(io, "  - number of population resamplings: $(s.state.n_resampling)")
    println(io, "  - acceptance rate: $(round(s.state.n_accept / (s.state.n_simulation - n), sigdigits=4))")
end

end # module
