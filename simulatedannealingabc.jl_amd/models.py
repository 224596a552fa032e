"""Device-coded simulators.  In the reference `f_dist` is an arbitrary Julia closure
(SimulatedAnnealingABC.jl:164,175,315); a GPU kernel needs it as data, so `sabc` takes a
`DeviceDistance` descriptor naming one of the simulators compiled into csrc/device_models.hpp.
Definitions (and the observed summaries each one is compared with) are in DESIGN.md."""
from __future__ import annotations

import os

import numpy as np

from . import _lib


class DeviceDistance:
    model_id: int = 0
    n_stats: int = 0
    n_para: tuple = ()

    @property
    def params(self):
        raise NotImplementedError

    def __call__(self, θ, *a, **k):
        raise TypeError("a DeviceDistance is evaluated on the GPU; use SabcHandle.simulate() to call it directly")


class GaussianIID(DeviceDistance):
    """y_1..n_obs ~ Normal(θ[1], sd) with sd = θ[2] when the prior has two dimensions;
    ρ = (|obs_mean − mean(y)|,) or with `obs_m2` also |obs_m2 − mean(y.^2)|.
    Covers test/runtests.jl:35,86,128-131,167-170 and BASELINE configs 1-2."""
    model_id = _lib.MODEL_GAUSS_IID
    n_para = (1, 2)

    def __init__(self, n_obs=100, sd=1.0, obs_mean=0.0, obs_m2=None):
        self.n_obs, self.sd, self.obs_mean, self.obs_m2 = int(n_obs), float(sd), float(obs_mean), obs_m2
        self.n_stats = 1 if obs_m2 is None else 2

    @property
    def params(self):
        return [self.n_obs, self.sd, self.obs_mean, 0.0 if self.obs_m2 is None else float(self.obs_m2)]


class Gaussian2D(DeviceDistance):
    """x_1..n_obs ~ N(θ, [[1,r],[r,1]]); ρ = (‖mean − obs‖₂, |var₁+var₂ − obs|, |cov₁₂ − obs|)."""
    model_id = _lib.MODEL_GAUSS2D
    n_para = (2,)
    n_stats = 3

    def __init__(self, n_obs=50, r=0.6, obs_mean=(0.0, 0.0), obs_varsum=2.0, obs_cov=0.6):
        self.n_obs, self.r = int(n_obs), float(r)
        self.obs_mean, self.obs_varsum, self.obs_cov = tuple(map(float, obs_mean)), float(obs_varsum), float(obs_cov)

    @classmethod
    def from_observations(cls, y, r=0.6):
        y = np.asarray(y, dtype=np.float64)
        c = np.cov(y.T)
        return cls(n_obs=len(y), r=r, obs_mean=y.mean(0), obs_varsum=c[0, 0] + c[1, 1], obs_cov=c[0, 1])

    @property
    def params(self):
        return [self.n_obs, self.r, self.obs_mean[0], self.obs_mean[1], self.obs_varsum, self.obs_cov]


class GandK(DeviceDistance):
    """g-and-k: x = A + B(1 + c·tanh(g z/2))(1+z²)^k z, z~N(0,1), n_draws draws;
    ρ_j = |x_(rank_j) − obs_j| for four order statistics (1-based ranks)."""
    model_id = _lib.MODEL_GK
    n_para = (4,)
    n_stats = 4

    def __init__(self, n_draws=128, c=0.8, ranks=(16, 48, 80, 112), obs=(0.0, 0.0, 0.0, 0.0)):
        self.n_draws, self.c = int(n_draws), float(c)
        self.ranks, self.obs = tuple(int(r) for r in ranks), tuple(float(o) for o in obs)

    @property
    def params(self):
        return [self.n_draws, self.c, *self.ranks, *self.obs]


class LotkaVolterra(DeviceDistance):
    """Stochastic Lotka–Volterra by Euler–Maruyama: dX = (aX − bXY)dt + σX dW₁,
    dY = (bXY − cY)dt + σY dW₂, clamped at 0; ρ = |mean X, sd X, mean Y, sd Y − obs|."""
    model_id = _lib.MODEL_LV
    n_para = (3,)
    n_stats = 4

    def __init__(self, n_steps=256, dt=0.05, σ=0.1, x0=50.0, y0=50.0, obs=(0.0, 0.0, 0.0, 0.0)):
        self.n_steps, self.dt, self.σ, self.x0, self.y0 = int(n_steps), float(dt), float(σ), float(x0), float(y0)
        self.obs = tuple(float(o) for o in obs)

    @property
    def params(self):
        return [self.n_steps, self.dt, self.σ, self.x0, self.y0, *self.obs]


class HostDistance(DeviceDistance):
    """Any host callable as `f_dist` (SimulatedAnnealingABC.jl:164,175,315): `fn(θ, *args, **kwargs)` returning a
    scalar, tuple or vector of non-negative distances, exactly what the reference accepts.  The proposal,
    prior gate, ECDF transform, acceptance, reductions and resampling still run on the GPU; only the
    simulator is called on the host, for the proposals that passed the prior gate.

    batched=True: `fn(Θ, ...)` gets all m proposals at once (Θ is m×d, or length m for a univariate
    prior) and returns m×s.  with_ids=True: `fn(θ, particle_id, iteration, ...)`, so that a simulator can
    key its own random streams (used by the parity tests)."""
    model_id = _lib.MODEL_HOST
    params = ()

    def __init__(self, fn, n_stats, n_para, univariate, args=(), kwargs=None, batched=False, with_ids=False):
        self.fn, self.n_stats, self.n_para = fn, int(n_stats), (int(n_para),)
        self.univariate, self.args, self.kwargs = bool(univariate), tuple(args), dict(kwargs or {})
        self.batched, self.with_ids = bool(batched), bool(with_ids)
        self.error = None            # an exception raised inside the callback, re-raised by the caller

    def callback(self):
        d, s = self.n_para[0], self.n_stats

        def cb(ctx, theta, ids, m, it, rho_out):
            try:
                th = np.ctypeslib.as_array(theta, shape=(d, m))
                out = np.ctypeslib.as_array(rho_out, shape=(s, m))
                if self.batched:
                    arg = th[0].copy() if self.univariate else np.ascontiguousarray(th.T)
                    r = np.asarray(self.fn(arg, *self.args, **self.kwargs), dtype=np.float64).reshape(m, s)
                    out[...] = r.T
                else:
                    for i in range(m):
                        x = float(th[0, i]) if self.univariate else th[:, i].copy()
                        extra = (int(ids[i]), int(it)) if self.with_ids else ()
                        out[:, i] = np.atleast_1d(np.asarray(self.fn(x, *extra, *self.args, **self.kwargs), dtype=np.float64))
                return 0
            except Exception as e:   # never raise through the C frame; sabc() re-raises it
                self.error = e
                return -1

        return _lib.SIMULATE_FN(cb)


def _segment(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1)      # float64, flattened in C order


def data_segments(data):
    """`data` of a DeviceSource as a list of float64 vectors, one per segment: an array (of any shape) or a sequence of
    numbers is ONE segment; a list or tuple holding array-likes is one segment per element."""
    if isinstance(data, (list, tuple)) and any(np.ndim(x) > 0 for x in data):
        segs = [_segment(x) for x in data]
    else:
        segs = [_segment(data)]
    if len(segs) > _lib.MAX_DATA_SEGMENTS:
        raise ValueError(f"at most {_lib.MAX_DATA_SEGMENTS} data segments")
    return segs


class DeviceSource(DeviceDistance):
    """`f_dist` as HIP source (SimulatedAnnealingABC.jl:164,175,315 for a simulator of your own ON the device):

        __device__ void sabc_user_simulate(const double *theta, const double *params, sabc::NormalStream &rng, double *rho_out);

    `rng.next()` / `rng.pair(z0, z1)` are N(0,1) draws, `rng.uniform_pair(u0, u1)` U(0,1) draws of the particle's
    simulation stream; `rng.for_pairs(n, [&](double z0, double z1) { ... })` hands the next n pairs to the lambda in stream
    order -- the loop to draw the bulk of a simulation with: small populations (one launch per call, a team of 4 or 16
    lanes per particle) then generate 16 or 64 pairs at a time, four blocks per lane.  The simulator must be a function of its arguments and
    its draws alone (the lanes of a quad run it side by side).

    Discrete-event and count models draw whole blocks of the same stream: `rng.exponential_pair(e0, e1)` two Exp(1) draws,
    `rng.event_pair(e, u)` the waiting time -log(u0) and the event-choice uniform u1 of one step of Gillespie's direct method,
    `rng.poisson(lambda)` (inversion below 10, PTRS above; lambda <= 2^30) and `rng.binomial(n, p)` (inversion for n p < 10, BTRS
    above) counts, and `rng.while_events(max_events, [&](double e, double u) { ...; return go_on; })` -- the loop whose trip
    count depends on the draws: the lambda gets the event pairs of successive blocks until it returns false or `max_events`
    calls are made (the bound is mandatory), the call returns their number and the stream has advanced by exactly that many
    blocks; a team of lanes generates a group of events side by side and drops the rest at the first false.  `params` is the `params` list given here.  The source is compiled at run time (hipRTC, gfx950) into
    the same fused propose -> simulate -> ECDF -> accept kernel as the built-in simulators.  n_stats <= 64 (_lib.MAX_SOURCE_STATS;
    above 16 the wide form of the kernels).  `params` holds at most 32 values.

    Binary32 draws, for simulators whose noise needs no more: `rng.quad_f32(z0, z1, z2, z3)` four N(0,1) floats from one block
    ((z0, z1) from its first two words, (z2, z3) from the others; |z| <= sqrt(66 ln 2) = 6.7637, the f64 draws reach 8.57),
    `rng.uniform_quad_f32(u0, u1, u2, u3)` four U(0,1) floats ((w >> 9) + 1/2) 2^-23, and
    `rng.for_quads_f32(n, [&](float z0, float z1, float z2, float z3) { ... })` the next n blocks in stream order -- the loop to
    draw the bulk with: half the generator's instructions per normal.  They consume whole blocks of the same stream and mix freely
    with the f64 draws.  `theta`, `params`, `rho_out`, `sabc::data_at` and `sabc::emit` stay `double`.

    Observations the simulator compares against (a time series) are `data`: one array-like, or a sequence of array-likes -- one
    segment each, at most 8 --, float64, flattened in C order and kept in device memory by the handle.  The source -- the
    simulator and, with a SourcePrior, the prior -- reads them with `sabc::data_len(segment = 0)`, `sabc::data_at(i, segment = 0)`
    (through the constant address space: an index shared by the wave's lanes is one scalar load), `sabc::data(segment = 0)` (the
    plain pointer; nullptr while nothing is set) and `sabc::data_segments()`; indices are not checked.  Another data set is another
    `SabcHandle.set_data(...)`, never another source or another compilation.  With `data_names=("y_obs", "t_obs")`, `sabc`,
    `initialization` and `update_population_` take that many extra positional arguments, or keywords of those names, the way
    the reference hands `args...` / `kwargs...` to `f_dist`: they become the segments in the order of `data_names` and replace
    what the model was constructed with (in `update_population_`: what the handle holds; data not given leave it).

    Outputs -- what a simulation looks like, not only its distance: the source hands values out with
    `sabc::emit(rng, i, v)` (output i of this simulation; `sabc::emitting(rng)` and `sabc::n_outputs(rng)` tell whether and how
    many).  Population updates never emit -- the calls are dead code there --; `simulate_outputs`, `posterior_predictive` and
    `SabcHandle.simulate_outputs` run the source forward and return what it emitted, NaN where it emitted nothing.  `n_outputs`
    declares how many there are: an int, or a callable of the data segments (a series model emits one value per observation
    time); None: the model declares no outputs.  `output_names` names them (then n_outputs may be left out).

    Order statistics of a simulated sample (csrc/sort_network.hpp): `sabc::sort_ascending(x)` for `double x[N]` with N a
    compile-time constant (up to 32 the sorting network unrolled, on registers where the array's other indices are constants
    too), `sabc::sort_ascending(x, n)` for any n >= 0 (loops), float twins of both, `sabc::order_statistic(sorted, n, rank)`
    (1-based; +inf outside [1, n]) and `sabc::quantile(sorted, n, p)` (Julia's default, type 7; NumPy's "linear"; p clamped to
    [0, 1]).  The sort is a data-oblivious network -- Batcher's odd-even merge sort, a compare-exchange being one min and one
    max, never a branch --: which elements meet depends on n alone, so the lanes of a wave index their arrays alike, and a
    lane, a quad or a row of lanes per particle return the same bits (a sorted array is unique).  A NaN enters as +inf, the
    built-in g-and-k model's policy, and comes out last; -0.0 and +0.0 compare equal.  A sort written by hand in the source is a
    data-dependent loop that diverges across the wave.  `GandKQuantiles` is the shipped model on it.

    The cooperative form, `team_lanes` = 1, 4 or 16 (None: everything above, the entry point `sabc_user_simulate`): the source
    defines instead
        template <int W> __device__ void sabc_user_simulate_team(const double *theta, const double *params,
                                                                 sabc::NormalStream &rng, double *rho_out);
    with W = 1, 4 or 16 the lanes that run this particle side by side, and runs with `team_lanes` lanes per particle on the launch
    chain and in the forward run (`simulate_outputs`, `posterior_predictive`); the one-launch form of small populations keeps
    choosing its own team.  All lanes of a team see the same data and must make the same requests, in the same order.
    `sabc::Sample<N, W> x` (csrc/team_sample.hpp) holds N doubles of the particle spread over the team, in registers:
    `x.fill_normals(rng, f)` (element i = f(z_i), the next N normals in stream order -- ceil(N / 2) whole blocks, each lane
    generating and transforming its own), `x.fill(g)` (element i = g(i)), `x.drawn(i)` before and `x.at(i)`,
    `x.order_statistic(rank)`, `x.quantile(p)` after `x.sort()` -- a bitonic network, min and max between registers of a lane,
    DPP between lanes, no LDS --, and `x.emit(rng, first_output)` (the current order, each value written once).  A NaN enters as
    +inf.  More than 32 slots per lane (N > 32 W), or W = 1: every lane holds the whole sample as before, so any N compiles.
    n_stats <= 16.

    Sums and two-sample distances (csrc/sample_reduce.hpp).  The sum is ONE definition, the balanced binary tree over the
    element's index (neighbours first, padded with +0.0 to a power of two): `sabc::tree_sum(x, n)` and `sabc::tree_sum(n, g)`
    (g(i) -> double) for an array, `x.sum(g)`, `x.max(g)`, `x.min(g)` with g(i, value) -> double, `x.sum()`, `x.mean()` and
    `x.moments(mean, var)` (two passes, var over N - 1) for a `Sample` -- i the draw index before `x.sort()`, the 0-based rank
    after it; each lane adds its own slots, the team follows with a butterfly over DPP, every lane gets the value.  After the
    sort all forms give the same bits, whatever the team's width; before it a team sums in the layout of its draws (the same
    value up to rounding).  Against an ASCENDING data segment `seg`: `sabc::count_less(v, seg)` and
    `sabc::count_less_equal(v, seg)` (#{j: y_j < v}, <= v; a binary search without a data-dependent branch, a NaN v as +inf),
    and after `x.sort()` `x.wasserstein1(seg)` = sum_i |x_(i) - y_i| / N and `x.wasserstein2_squared(seg)` (data_len(seg) == N) and
    `x.ks(seg)`, the Kolmogorov-Smirnov distance for any data_len(seg) >= 1 (N data_len(seg) < 2^53; exact for distinct sample
    values, with r equal ones at most (r - 1) / N above).  `GandKSample` is the shipped model on them.

    `sabc::SampleF32<N, W> x` (csrc/team_sample_f32.hpp) is `Sample` for binary32 values, for simulators whose noise needs no
    more: `x.fill_normals(rng, f)` with f(float) -> float takes the stream's binary32 normals, four per block (the
    ceil(N / 4) blocks of `rng.for_quads_f32`), a slot is one register and a cross-lane exchange one word; `x.drawn(i)`,
    `x.at(i)` and `x.order_statistic(rank)` return float, `x.quantile(p)` double, `x.emit` writes (double)value; the
    reductions and distances above take g(i, float value) -> double and accumulate in double -- the same canonical tree, the
    same bits for every width.  `GandKSampleF32` is the shipped model on it.

    `sabc::Series<N, W> x` (csrc/team_series.hpp) holds a time series x_0 .. x_{N-1} of doubles in time order over the team --
    time t on lane t / M in slot t mod M, where a `Sample` holds rank t after its sort -- for models compared through lagged
    summaries: `x.fill_normals(rng, f)` (x_t = f(t, z_t), a lane generating the consecutive blocks of its own times),
    `x.fill(g)`, `x.map(g)` (x_t <- g(t, x_t)), `x.zip(other, g)` (x_t <- g(t, x_t, other_t)), `x.at(t)`,
    `x.emit(rng, first_output, first = 0)`, and `x.lag<L>(before = 0.0)` -- the series whose element t is x_{t-L}, `before` for
    t < L: a register move inside a lane, one row_shr DPP move per 32-bit half between lanes, no LDS.  `x.lagged_sum<L>(g, first = 0)`
    is the canonical sum of g(t, x_t, x_{t-L}) over t >= first + L, `x.autocovariance<L>(center = 0.0, first = 0)` that sum of
    (x_t - c)(x_{t-L} - c), each product rounded on its own, over N - first; `sum`, `max`, `min`, `mean`, `moments` as for a
    `Sample`, over the time index.  Position equals index for every width, so all of them give the same bits for 1, 4 and 16
    lanes, always.  Values pass through unchanged (no NaN policy: nothing is sorted).  `MA2` is the shipped model on these.
    Recurrences run in time order: `x.recur(s0, f, first = 0)` is the sequential loop x_t <- f(t, s, x_t) for t = first .. N-1 with
    `State &s` carried from step to step (State: double or `sabc::series::Carry<K>`, K <= 4 doubles) and returns the last state;
    `x.recur_with(other, s0, f, first = 0)` passes other_t as well; `x.cumsum()`.  A team relays the state from lane to lane, so
    the bits are the plain loop's for every width.  f must be a pure function of its arguments -- no emit, no draw from rng, no
    memory indexed by the state: the team evaluates it on lanes that discard the result -- and the rounding inside f is the
    caller's (write `fma` and `sabc::series::rounded_product`; a bare a * b + c may fuse).  `GARCH11` is the shipped model on it.
    Counts keyed by the time step: `sabc::CountDraws cd = rng.reserve_counts(n)` (csrc/device_rng.hpp) reserves 64 blocks of the
    stream's counter for each draw index 0 .. n-1 (n <= 2^20; no block is generated) and `cd.poisson(i, lambda)`,
    `cd.binomial(i, n_trials, p)` are PURE functions of their arguments -- `rng.poisson` / `rng.binomial` from a stream positioned
    at the index's first block, computed by the calling lane alone --, so the lanes of a team may draw for different indices side
    by side (inside `map`, `fill`, `zip`) and a draw is legal inside `recur`'s f (every lane then issues all N draws).  They are
    total: lambda NaN or <= 0 gives 0, lambda and n_trials above 2^30 count as 2^30, p NaN or <= 0 gives 0, p >= 1 n_trials.
    `x.map_poisson(rng, scale = 1.0)` is x_t <- Poisson(scale x_t) with index t.  `Ricker` is the shipped model on these.
    Not there: a parallel scan for associative operations, a binary32 twin."""
    model_id = _lib.MODEL_USER

    def __init__(self, hip_source: str, n_para: int, n_stats: int, params=(), data=None, data_names=None, n_outputs=None,
                 output_names=None, team_lanes=None):
        if team_lanes is not None:
            if isinstance(team_lanes, bool) or team_lanes not in (1, 4, 16):
                raise ValueError(f"team_lanes is None (sabc_user_simulate) or 1, 4 or 16 lanes per particle (sabc_user_simulate_team<W>), got {team_lanes!r}")
            if int(n_stats) > _lib.NARROW_STATS:
                raise ValueError(f"a team-aware source has at most {_lib.NARROW_STATS} statistics (the kernels for more run a lane per "
                                 f"particle), got n_stats = {n_stats}")
            team_lanes = int(team_lanes)
        self.team_lanes = team_lanes
        self.output_names = None if output_names is None else tuple(str(x) for x in output_names)
        if n_outputs is None and self.output_names is not None:
            n_outputs = len(self.output_names)
        if n_outputs is not None and not callable(n_outputs):
            if isinstance(n_outputs, bool) or int(n_outputs) != n_outputs or int(n_outputs) < 0:
                raise ValueError(f"n_outputs is a non-negative integer or a callable of the data segments, got {n_outputs!r}")
            n_outputs = int(n_outputs)
            if self.output_names is not None and len(self.output_names) != n_outputs:
                raise ValueError(f"output_names = {self.output_names!r} names {len(self.output_names)} outputs, n_outputs = {n_outputs}")
        self.n_outputs = n_outputs
        self.source = str(hip_source)
        self.n_para = (int(n_para),)
        self.n_stats = int(n_stats)
        self._params = [float(p) for p in params]
        if len(self._params) > _lib.MAX_MODEL_PARAMS:
            raise ValueError(f"at most {_lib.MAX_MODEL_PARAMS} parameters")
        self.data_names = None if data_names is None else tuple(str(x) for x in data_names)
        if self.data_names is not None and not 1 <= len(self.data_names) <= _lib.MAX_DATA_SEGMENTS:
            raise ValueError(f"data_names: 1 to {_lib.MAX_DATA_SEGMENTS} names, one per data segment")
        self.data = None if data is None else data_segments(data)
        if self.data is not None and self.data_names is not None and len(self.data) != len(self.data_names):
            raise ValueError(f"data holds {len(self.data)} segments, data_names = {self.data_names!r} names {len(self.data_names)}")
        if self.data is not None:
            self.validate_data(self.data)

    def validate_data(self, segments):
        """What this model's source requires of its data (the source itself checks no index): called wherever data enter --
        the constructor, the extra arguments of sabc / initialization / update_population_, and SabcHandle.set_data of a handle
        made for this model.  Raises ValueError.  The base class accepts anything; the shipped models override it."""

    def n_outputs_for(self, segments=None):
        """How many outputs a simulation emits for these data segments (None: the data the model was constructed with).
        TypeError if the model declares no outputs."""
        if self.n_outputs is None:
            raise TypeError(f"{type(self).__name__} declares no outputs: construct it with n_outputs= (and let its source "
                            "call sabc::emit)")
        if not callable(self.n_outputs):
            return self.n_outputs
        segments = self.data if segments is None else segments
        if segments is None:
            raise TypeError(f"{type(self).__name__} has no data, and its number of outputs depends on them")
        n = self.n_outputs(segments)
        if isinstance(n, bool) or int(n) != n or int(n) < 0:
            raise ValueError(f"n_outputs(data) must be a non-negative integer, got {n!r}")
        if self.output_names is not None and len(self.output_names) != int(n):
            raise ValueError(f"output_names = {self.output_names!r} names {len(self.output_names)} outputs, n_outputs(data) = {n}")
        return int(n)

    def bind_data(self, args, kwargs):
        """The extra arguments of sabc / initialization / update_population_ as data segments in the order of `data_names`;
        None if there are none.  A wrong count or an unknown name is a TypeError naming `data_names`."""
        if not args and not kwargs:
            return None
        if not self.data_names:
            raise TypeError("a DeviceDistance takes its data at construction; extra args/kwargs are not forwarded "
                            "(a DeviceSource takes them when it is constructed with data_names)")
        names = self.data_names
        unknown = sorted(set(kwargs) - set(names))
        if unknown:
            raise TypeError(f"unexpected keyword argument(s) {unknown}: data_names = {names!r}")
        if len(args) > len(names):
            raise TypeError(f"{len(args)} positional data arguments given, data_names = {names!r} takes {len(names)}")
        twice = [n for n in names[:len(args)] if n in kwargs]
        if twice:
            raise TypeError(f"data argument(s) {twice} given both by position and by keyword: data_names = {names!r}")
        missing = [n for n in names[len(args):] if n not in kwargs]
        if missing:
            raise TypeError(f"missing data argument(s) {missing}: data_names = {names!r}")
        segments = [_segment(a) for a in (*args, *(kwargs[n] for n in names[len(args):]))]
        self.validate_data(segments)
        return segments

    @property
    def params(self):
        return list(self._params)

    def compile_check(self, with_prior=False):
        """Run the compiler stage only (no GPU needed); raises SABCError with the compiler log on failure.
        with_prior: the source also defines the prior (SourcePrior)."""
        import ctypes as C
        log = C.create_string_buffer(1 << 16)
        L = _lib.lib()
        if self.team_lanes is not None:
            fn = L.sabc_op_compile_device_simulator_team_with_prior if with_prior else L.sabc_op_compile_device_simulator_team
        else:
            fn = L.sabc_op_compile_device_simulator_with_prior if with_prior else L.sabc_op_compile_device_simulator
        rc = fn(self.source.encode(), self.n_para[0], self.n_stats, log, len(log))
        if rc:
            raise _lib.SABCError(rc, "compiling the device simulator failed:\n" + log.value.decode("utf-8", "replace"))
        return True


_SOURCES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_sources")


def device_source_text(name):
    """The text of a simulator shipped with the package as HIP source (device_sources/<name>.hip)."""
    with open(os.path.join(_SOURCES, name + ".hip"), encoding="utf-8") as f:
        return f.read()


class StochasticSIR(DeviceSource):
    """The reference's documentation example (docs/src/example.md:75-198) on the device: a stochastic SIR epidemic by
    Gillespie's direct method, theta = (beta, gamma), started at (S0, I0, R0) and run while t < t_max and I > 0.
    `data_obs` = (total_infected, peak_infected, t_peak) -- a sequence, or a mapping with those keys --; rho = the three squared
    differences to it (n_stats=3, `f_dist_multi_stats`) or their sum (n_stats=1, `f_dist_single_stat`).  The model is the HIP
    source device_sources/sir.hip, compiled like any `DeviceSource`; `StochasticSIR.observe` simulates an observation with it (`examples.sir_observation`: on the
    host, with NumPy).  Outputs: (total_infected, peak_infected, t_peak)."""

    def __init__(self, data_obs, S0=99, I0=1, R0=0, t_max=160.0, n_stats=3):
        comp = []
        for name, v in (("S0", S0), ("I0", I0), ("R0", R0)):
            if isinstance(v, bool) or float(v) != int(v) or int(v) < 0:
                raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
            comp.append(int(v))
        if comp[1] < 1:
            raise ValueError("I0 must be at least 1: an epidemic without an infected individual has no events")
        if int(n_stats) not in (1, 3):
            raise ValueError("n_stats is 3 (one distance per statistic) or 1 (their sum)")
        if hasattr(data_obs, "keys"):
            data_obs = [data_obs[k] for k in ("total_infected", "peak_infected", "t_peak")]
        obs = [float(x) for x in data_obs]
        if len(obs) != 3:
            raise ValueError("data_obs holds (total_infected, peak_infected, t_peak)")
        self.S0, self.I0, self.R0 = comp
        self.t_max, self.data_obs = float(t_max), tuple(obs)
        super().__init__(f"#define SIR_N_STATS {int(n_stats)}\n" + device_source_text("sir"), 2, int(n_stats),
                         [*comp, self.t_max, *obs], output_names=("total_infected", "peak_infected", "t_peak"))

    @classmethod
    def observe(cls, theta=(0.3, 0.1), S0=99, I0=1, R0=0, t_max=160.0, seed=None, device=None):
        """An observation made by the device source itself: one forward run at theta = (beta, gamma) on the predictive stream
        of particle 0, iteration 0 of `seed`, as the dict `examples.sir_observation` returns."""
        from .api import simulate_outputs
        model = cls((0.0, 0.0, 0.0), S0=S0, I0=I0, R0=R0, t_max=t_max)
        out = simulate_outputs(model, np.asarray(theta, dtype=np.float64).reshape(1, 2), seed=seed, device=device)[0, 0]
        return {name: float(v) for name, v in zip(model.output_names, out)}


class LotkaVolterraF32(DeviceSource):
    """`LotkaVolterra` -- the same factored Euler-Maruyama step, the same four statistics -- with its noise, state and step
    in binary32, as HIP source (device_sources/lotka_volterra_f32.hip): two steps per Philox block through
    `rng.for_quads_f32`, about half the generator's instructions per normal of the f64 model.  For simulators whose noise is
    binary32-grade anyway (an SDE path compared at 1e-2); theta, params and rho stay float64, and the running sums are sums of
    deviations from (x0, y0), finished in float64.  n_stats = 1..4: the first so many of |mean X, sd X, mean Y, sd Y - obs|.
    Outputs: the two paths, X at 0..n_steps-1 and Y behind it (`posterior_predictive` gives [n, n_rep, 2 n_steps])."""

    def __init__(self, n_steps=256, dt=0.05, σ=0.1, x0=50.0, y0=50.0, obs=(0.0, 0.0, 0.0, 0.0), n_stats=4):
        if isinstance(n_steps, bool) or int(n_steps) != n_steps or int(n_steps) < 2:
            raise ValueError(f"n_steps must be an integer of at least 2 (the standard deviations divide by n_steps - 1), got {n_steps!r}")
        if int(n_stats) not in (1, 2, 3, 4):
            raise ValueError("n_stats is 1..4")
        self.n_steps, self.dt, self.σ, self.x0, self.y0 = int(n_steps), float(dt), float(σ), float(x0), float(y0)
        self.obs = tuple(float(o) for o in obs)
        if len(self.obs) != 4:
            raise ValueError("obs holds (mean X, sd X, mean Y, sd Y)")
        super().__init__(f"#define LV_N_STATS {int(n_stats)}\n" + device_source_text("lotka_volterra_f32"), 3, int(n_stats),
                         [self.n_steps, self.dt, self.σ, self.x0, self.y0, *self.obs], n_outputs=2 * self.n_steps)


class NormalMoments(DeviceSource):
    """The `f_dist` of the reference's getting-started example (docs/src/usage.md:15-35) on the device: theta = (mu, sigma),
    y_sim = len(y_obs) draws of Normal(mu, sigma), rho = (|mean(y_obs) - mean(y_sim)|, |sum(y_obs^2) - sum(y_sim^2)|).  `y_obs`
    is data, not source text or parameters: give it here, or -- the reference's call shape -- to `sabc(model, prior,
    y_obs=...)` and `update_population_(res, model, prior, y_obs=...)`.  Source: device_sources/normal_moments.hip."""

    def __init__(self, y_obs=None, data_names=("y_obs",)):
        super().__init__(device_source_text("normal_moments"), 2, 2, (), data=None if y_obs is None else [_segment(y_obs)],
                         data_names=data_names, n_outputs=lambda segments: len(segments[0]))      # y_sim, one per observation

    @classmethod
    def observe(cls, theta, n, seed=None, device=None):
        """A sample y of n draws of Normal(theta[0], theta[1]) made by the device source itself (the predictive stream of
        particle 0, iteration 0 of `seed`)."""
        from .api import simulate_outputs
        model = cls(y_obs=np.zeros(int(n)))
        return simulate_outputs(model, np.asarray(theta, dtype=np.float64).reshape(1, 2), seed=seed, device=device)[0, 0]

    def validate_data(self, segments):
        if len(segments) != 1 or len(segments[0]) < 1:
            raise ValueError("y_obs is one segment of at least one value (both distances divide by or sum over its length)")


class StochasticSIRSeries(DeviceSource):
    """The Gillespie epidemic of `StochasticSIR` compared with a whole observed curve: `t_obs` (increasing) and `I_obs` are two
    data segments, rho = (mean_k |I(t_k) - I_obs[k]|,) with I(t_k) the number infected just before the first event later than
    t_k (the final number once no event follows).  Source: device_sources/sir_series.hip; `examples.sir_series_observation`
    simulates an observation on the host."""

    def __init__(self, t_obs=None, I_obs=None, S0=99, I0=1, R0=0, t_max=160.0, data_names=("t_obs", "I_obs")):
        comp = []
        for name, v in (("S0", S0), ("I0", I0), ("R0", R0)):
            if isinstance(v, bool) or float(v) != int(v) or int(v) < 0:
                raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
            comp.append(int(v))
        if comp[1] < 1:
            raise ValueError("I0 must be at least 1: an epidemic without an infected individual has no events")
        if (t_obs is None) != (I_obs is None):
            raise ValueError("t_obs and I_obs come together")
        data = None
        if t_obs is not None:
            data = [_segment(t_obs), _segment(I_obs)]
        self.S0, self.I0, self.R0 = comp
        self.t_max = float(t_max)
        super().__init__(device_source_text("sir_series"), 2, 1, [*comp, self.t_max], data=data, data_names=data_names,
                         n_outputs=lambda segments: len(segments[0]))                             # I(t_k), one per observation time

    @classmethod
    def observe(cls, theta, t_obs=None, S0=99, I0=1, R0=0, t_max=160.0, seed=None, device=None):
        """An observation made by the device source itself: one forward run at theta = (beta, gamma), observed at the
        increasing times `t_obs` (default 0, 5, ..., 155), on the predictive stream of particle 0, iteration 0 of `seed`.
        Returns (t_obs, I_obs) like `examples.sir_series_observation`."""
        from .api import simulate_outputs
        t_obs = np.arange(0.0, 160.0, 5.0) if t_obs is None else _segment(t_obs)
        model = cls(t_obs, np.zeros(len(t_obs)), S0=S0, I0=I0, R0=R0, t_max=t_max)
        out = simulate_outputs(model, np.asarray(theta, dtype=np.float64).reshape(1, 2), seed=seed, device=device)
        return t_obs, out[0, 0]

    def validate_data(self, segments):
        # the source reads I_obs[k] for every k < len(t_obs): a shorter I_obs would be read past its end on the device
        if len(segments) != 2 or len(segments[0]) != len(segments[1]) or len(segments[0]) < 1:
            raise ValueError("t_obs and I_obs hold the same number of values, at least one")
        if np.any(np.diff(segments[0]) <= 0):
            raise ValueError("t_obs must be increasing")


class GandKQuantiles(DeviceSource):
    """g-and-k -- x = A + B (1 + c tanh(g z / 2)) (1 + z^2)^k z, theta = (A, B, g, k) -- with real data shapes: any number of draws
    and any set of quantiles, where the built-in `GandK` sorts 128 draws at four ranks inside a kernel of its own.
    rho_j = |quantile(sort(x_1..n_draws), probs[j]) - q_obs[j]|, the quantile Julia's default (type 7; NumPy's "linear").
    `probs` and `q_obs` are two data segments (1 to 16 values each, as many as the model has statistics; another set of as
    many quantiles is another `SabcHandle.set_data` or `sabc(model, prior, probs=..., q_obs=...)`, never another compilation);
    `n_draws` and `c` are params.  `from_observations(y_obs)` takes `q_obs` from a sample with `np.quantile`.
    Source: device_sources/gk_quantiles.hip, which sorts the draws with `sabc::sort_ascending` -- n_draws is a compile-time constant
    of the source, up to 32 draws the sorting network runs on registers.  Outputs: the sorted sample (`posterior_predictive`
    gives [n, n_rep, n_draws], ascending along the last axis).
    `team_lanes` = 1, 4 or 16 (None: the above): the same model through `sabc::Sample<n_draws, W>` -- the sample spread over a team
    of lanes that draws, transforms and sorts it together, `team_lanes` lanes per particle on the launch chain and in the forward
    run (`DeviceSource`, the cooperative form).  The same statistics and outputs; the results are the default form's up to the
    order of the partial sums."""
    MAX_QUANTILES = 16
    MAX_DRAWS = 1024                 # the sample is 8 n_draws bytes of private memory per lane
    OCTILES = tuple(j / 8 for j in range(1, 8))

    def __init__(self, probs, q_obs, n_draws=128, c=0.8, data_names=("probs", "q_obs"), team_lanes=None):
        if isinstance(n_draws, bool) or int(n_draws) != n_draws or not 2 <= int(n_draws) <= self.MAX_DRAWS:
            raise ValueError(f"n_draws must be an integer in 2..{self.MAX_DRAWS}, got {n_draws!r}")
        probs, q_obs = _segment(probs), _segment(q_obs)
        if not 1 <= len(probs) <= self.MAX_QUANTILES:
            raise ValueError(f"1 to {self.MAX_QUANTILES} quantiles, got {len(probs)}")
        self.n_draws, self.c = int(n_draws), float(c)
        team = "" if team_lanes is None else "#define GKQ_TEAM 1\n"
        super().__init__(f"#define GKQ_N_DRAWS {self.n_draws}\n#define GKQ_N_STATS {len(probs)}\n" + team + device_source_text("gk_quantiles"),
                         4, len(probs), [self.n_draws, self.c], data=[probs, q_obs], data_names=data_names, n_outputs=self.n_draws,
                         team_lanes=team_lanes)

    @classmethod
    def from_observations(cls, y_obs, probs=OCTILES, n_draws=None, c=0.8, team_lanes=None):
        """The model for a sample `y_obs`: q_obs = np.quantile(y_obs, probs) and, unless given, as many draws per simulation as
        there are observations."""
        y_obs = _segment(y_obs)
        return cls(probs, np.quantile(y_obs, _segment(probs)), n_draws=len(y_obs) if n_draws is None else n_draws, c=c,
                   team_lanes=team_lanes)

    def validate_data(self, segments):
        # the source reads probs[j] and q_obs[j] and writes rho[j] for every j < n_stats
        if len(segments) != 2 or len(segments[0]) != len(segments[1]):
            raise ValueError("probs and q_obs hold the same number of values")
        if not 1 <= len(segments[0]) <= self.MAX_QUANTILES:
            raise ValueError(f"1 to {self.MAX_QUANTILES} quantiles, got {len(segments[0])}")
        if len(segments[0]) != self.n_stats:
            raise ValueError(f"this model was made for {self.n_stats} quantiles (its n_stats), got {len(segments[0])}")
        if not np.all((segments[0] >= 0.0) & (segments[0] <= 1.0)):
            raise ValueError("probs are probabilities: every value in [0, 1]")


class GandKSample(DeviceSource):
    """g-and-k -- the model of `GandKQuantiles`, theta = (A, B, g, k) -- compared with the observed sample as a whole, the
    usual ABC treatment of it: `distance` = "wasserstein" (rho = sum_i |x_(i) - y_(i)| / n between the sorted samples, the
    1-Wasserstein distance of two samples of one length), "ks" (Kolmogorov-Smirnov, sup_t |F_x(t) - F_y(t)|; any two lengths), or
    both names in a sequence: one statistic per name, in the order given.  `y_obs` is ONE data segment, kept sorted -- the
    class sorts what it is constructed with; another sample of the same length is another `SabcHandle.set_data` or
    `sabc(model, prior, y_obs=np.sort(y))`, never another compilation --; `n_draws` (default: len(y_obs); with "wasserstein" it
    must be) and `c` are params.  Source: device_sources/gk_sample.hip on csrc/sample_reduce.hpp: `sabc::tree_sum`, the sum as a
    balanced tree over the rank, and `sabc::count_less` / `sabc::count_less_equal`, branch-free binary searches in the observed
    sample.  `team_lanes` = 1, 4 or 16: the same through `sabc::Sample<n_draws, W>` (`wasserstein1`, `ks`) -- every lane compares
    the ranks it holds after the sort with the observations beside them; the results are the default form's bit for bit.
    Outputs: the sorted sample, as `GandKQuantiles`."""
    DISTANCES = ("wasserstein", "ks")
    MAX_DRAWS = 1024                 # the sample is 8 n_draws bytes of private memory per lane
    SOURCE = "gk_sample"             # device_sources/<SOURCE>.hip ...
    TEAM_DEFINE = "#define GKS_TEAM 1\n"      # ... and what selects its team-aware form

    def __init__(self, y_obs, distance=("wasserstein", "ks"), n_draws=None, c=0.8, team_lanes=None, data_names=("y_obs",)):
        names = (distance,) if isinstance(distance, str) else tuple(distance)
        if not names or len(set(names)) != len(names) or any(d not in self.DISTANCES for d in names):
            raise ValueError(f"distance is one of {self.DISTANCES!r} or both, each once, got {distance!r}")
        y_obs = np.sort(_segment(y_obs))
        if len(y_obs) < 1:
            raise ValueError("y_obs is one segment of at least one value")
        if n_draws is None:
            n_draws = len(y_obs)
        if isinstance(n_draws, bool) or int(n_draws) != n_draws or not 1 <= int(n_draws) <= self.MAX_DRAWS:
            raise ValueError(f"n_draws must be an integer in 1..{self.MAX_DRAWS}, got {n_draws!r}")
        self.distance, self.n_draws, self.c = names, int(n_draws), float(c)
        head = f"#define GKS_N_DRAWS {self.n_draws}\n" + "".join(f"#define GKS_{d.upper()} {j}\n" for j, d in enumerate(names))
        team = "" if team_lanes is None else self.TEAM_DEFINE
        super().__init__(head + team + device_source_text(self.SOURCE), 4, len(names), [self.n_draws, self.c], data=[y_obs],
                         data_names=data_names, n_outputs=self.n_draws, team_lanes=team_lanes)

    def validate_data(self, segments):
        # the source reads y[i] for every i < n_draws ("wasserstein") and searches an ascending y ("ks")
        if len(segments) != 1 or len(segments[0]) < 1:
            raise ValueError("y_obs is one segment of at least one value")
        y = segments[0]
        if not np.all(np.isfinite(y)):
            raise ValueError("y_obs must be finite")
        if np.any(np.diff(y) < 0):
            raise ValueError("y_obs must be ascending: give np.sort(y_obs) (the constructor sorts what it is given)")
        if "wasserstein" in self.distance and len(y) != self.n_draws:
            raise ValueError(f'distance "wasserstein" compares rank with rank: len(y_obs) = {len(y)} must equal n_draws = {self.n_draws}')
        if self.n_draws * len(y) >= 2 ** 53:
            raise ValueError(f"n_draws * len(y_obs) must stay below 2^53 (the Kolmogorov-Smirnov counts are exact up to there), got {self.n_draws} * {len(y)}")


class GandKSampleF32(GandKSample):
    """`GandKSample` with a binary32 sample (device_sources/gk_sample_f32.hip on `sabc::SampleF32<n_draws, W>`,
    csrc/team_sample_f32.hpp): the normals are the stream's binary32 draws, four per Philox block (|z| <= 6.7637, where the f64
    draws reach 8.57), the g-and-k transform is the f64 one applied to the widened normal, and its result is rounded to binary32
    once; the team keeps and sorts floats -- a register per slot, one word per cross-lane exchange -- and both distances
    accumulate in float64 against `y_obs`, which stays float64.  Another stream than `GandKSample`'s: the same model, not the
    same draws.  `team_lanes` = 1, 4 or 16 lanes per particle, the same bits for the three; the source has the team-aware form
    only, so None is refused (`GandKSample` has the plain-array form).  Arguments, their checks, data and outputs are
    `GandKSample`'s; the outputs are binary32 values."""
    SOURCE = "gk_sample_f32"
    TEAM_DEFINE = ""                 # the text is team-aware throughout

    def __init__(self, y_obs, distance=("wasserstein", "ks"), n_draws=None, c=0.8, team_lanes=4, data_names=("y_obs",)):
        if team_lanes is None:
            raise ValueError("team_lanes is 1, 4 or 16: GandKSampleF32 has the team-aware form only (sabc::SampleF32); the plain-array "
                             "form is GandKSample(..., team_lanes=None)")
        super().__init__(y_obs, distance=distance, n_draws=n_draws, c=c, team_lanes=team_lanes, data_names=data_names)


def _tree_sum(s):
    """The canonical sum of csrc/sample_reduce.hpp along the last axis: the balanced binary tree over the index, padded with
    +0.0 to a power of two, + 0.0 last."""
    a = np.asarray(s, dtype=np.float64)
    p = 1
    while p < a.shape[-1]:
        p *= 2
    a = np.concatenate([a, np.zeros(a.shape[:-1] + (p - a.shape[-1],))], axis=-1)
    while a.shape[-1] > 1:
        a = a.reshape(a.shape[:-1] + (-1, 2))
        a = a[..., 0] + a[..., 1]
    return a[..., 0] + 0.0


class MA2(DeviceSource):
    """MA(2) with autocovariance summaries, the canonical ABC benchmark (Marin, Pudlo, Robert, Ryder 2012): theta = (theta1,
    theta2), y_t = e_{t+2} + theta1 e_{t+1} + theta2 e_t for t = 0 .. n_obs-1 with e the next n_obs + 2 normals of the particle's
    stream, tau_j = sum_{t >= j} y_t y_{t-j} / n_obs for j = 0 .. n_lags (n_lags <= 7), rho_j = |tau_j - acov_obs[j]|: n_stats =
    n_lags + 1.  `acov_obs` is ONE data segment of n_lags + 1 finite values -- another series' autocovariances are another
    `SabcHandle.set_data` or `sabc(model, prior, acov_obs=...)`, never another compilation --; `n_obs` and `n_lags` are
    compile-time constants of the source.  `from_observations(y_obs)` computes `acov_obs` from a series with the device's own
    sum (`autocovariances`), `observe(theta)` lets the device source simulate a series.
    Source: device_sources/ma2.hip on `sabc::Series<n_obs + 2, W>` (csrc/team_series.hpp): the innovations in time order, y from
    `lag<1>`, `lag<2>` and two `zip`s with explicit fmas, the summaries `autocovariance<j>`.  `team_lanes` = 1, 4 or 16: the
    series spread over that many lanes per particle, lags through DPP; None (the default): the same text with a private array per
    lane.  All forms give the same bits.  Outputs: the series y (`posterior_predictive` gives [n, n_rep, n_obs])."""
    MAX_LAGS = 7
    MAX_OBS = 1022                   # the series is 8 (n_obs + 2) bytes of private memory per lane where it is not spread

    def __init__(self, acov_obs=None, n_obs=100, n_lags=2, team_lanes=None, data_names=("acov_obs",)):
        if isinstance(n_lags, bool) or int(n_lags) != n_lags or not 0 <= int(n_lags) <= self.MAX_LAGS:
            raise ValueError(f"n_lags must be an integer in 0..{self.MAX_LAGS}, got {n_lags!r}")
        if isinstance(n_obs, bool) or int(n_obs) != n_obs or not int(n_lags) < int(n_obs) <= self.MAX_OBS:
            raise ValueError(f"n_obs must be an integer above n_lags = {n_lags} and at most {self.MAX_OBS}, got {n_obs!r}")
        self.n_obs, self.n_lags = int(n_obs), int(n_lags)
        head = f"#define MA2_N_OBS {self.n_obs}\n#define MA2_N_LAGS {self.n_lags}\n" + ("" if team_lanes is None else "#define MA2_TEAM 1\n")
        super().__init__(head + device_source_text("ma2"), 2, self.n_lags + 1, [self.n_obs, self.n_lags],
                         data=None if acov_obs is None else [_segment(acov_obs)], data_names=data_names, n_outputs=self.n_obs,
                         team_lanes=team_lanes)

    @staticmethod
    def autocovariances(y, n_lags=2):
        """tau_0 .. tau_n_lags of a series (along the last axis) as the device computes them: every product rounded on its own,
        the canonical sum over the innovations' n_obs + 2 times -- two leading +0.0 terms, which the tree's shape depends on --,
        divided by n_obs."""
        y = np.asarray(y, dtype=np.float64)
        n = y.shape[-1]
        tau = []
        for j in range(int(n_lags) + 1):
            terms = np.zeros(y.shape[:-1] + (n + 2,))
            terms[..., 2 + j:] = y[..., j:] * y[..., :n - j]
            tau.append(_tree_sum(terms) / float(n))
        return np.stack(tau, axis=-1)

    @classmethod
    def from_observations(cls, y_obs, n_lags=2, team_lanes=None):
        """The model for an observed series `y_obs`: n_obs = len(y_obs), acov_obs = its autocovariances at lags 0 .. n_lags."""
        y_obs = _segment(y_obs)
        return cls(cls.autocovariances(y_obs, n_lags), n_obs=len(y_obs), n_lags=n_lags, team_lanes=team_lanes)

    @classmethod
    def observe(cls, theta, n_obs=100, seed=None, device=None):
        """A series of n_obs values made by the device source itself: one forward run at theta = (theta1, theta2) on the
        predictive stream of particle 0, iteration 0 of `seed`."""
        from .api import simulate_outputs
        model = cls(np.zeros(1), n_obs=n_obs, n_lags=0)
        return simulate_outputs(model, np.asarray(theta, dtype=np.float64).reshape(1, 2), seed=seed, device=device)[0, 0]

    def validate_data(self, segments):
        # the source reads acov_obs[j] and writes rho[j] for every j <= n_lags
        if len(segments) != 1 or len(segments[0]) != self.n_lags + 1:
            raise ValueError(f"acov_obs is one segment of n_lags + 1 = {self.n_lags + 1} values (the autocovariances at lags 0 .. {self.n_lags})")
        if not np.all(np.isfinite(segments[0])):
            raise ValueError("acov_obs must be finite")


class GARCH11(DeviceSource):
    """GARCH(1,1) (Bollerslev 1986), the model shipped on `sabc::Series::recur`: theta = (omega, alpha, beta), y_t = sigma_t z_t and
    sigma^2_{t+1} = omega + alpha y_t^2 + beta sigma^2_t for t = 0 .. n_obs-1, with z the next n_obs normals of the particle's
    stream and sigma^2_0 = `sigma2_0`, a positive number (`from_observations` sets it to the mean of y_obs^2).  Summaries of the
    squared returns r_t = y_t^2: their mean and their autocovariances about it at lags 0 .. n_lags (n_lags <= 7), rho_0 =
    |mean(r) - obs_0|, rho_{1+j} = |acov_j(r) - obs_{1+j}|: n_stats = n_lags + 2.  `summaries_obs` is ONE data segment of
    n_lags + 2 finite values -- another series' summaries are another `SabcHandle.set_data` or
    `sabc(model, prior, summaries_obs=...)`, never another compilation --; `n_obs` and `n_lags` are compile-time constants of the
    source, `sigma2_0` is one of its params.  `from_observations(y_obs)` computes `summaries_obs` from a series of returns with
    the device's own sums (`summaries`), `observe(theta)` lets the device source simulate one.
    Source: device_sources/garch11.hip on `sabc::Series<n_obs, W>` (csrc/team_series.hpp): one `recur` over the normals with the
    state sigma^2_t -- two products rounded on their own, two explicit fmas --, then `mean` and `autocovariance<j>`.
    `team_lanes` = 1, 4 or 16: the series spread over that many lanes per particle, the recurrence relayed from lane to lane in
    time order; None (the default): the same text with a private array per lane.  All forms give the same bits, those of the
    sequential loop.  Outputs: the returns y_t = copysign(sqrt(r_t), z_t) (`posterior_predictive` gives [n, n_rep, n_obs])."""
    MAX_LAGS = 7
    MAX_OBS = 1024                   # the series is 8 n_obs bytes of private memory per lane where it is not spread (twice: z and r)

    def __init__(self, summaries_obs=None, n_obs=100, n_lags=2, sigma2_0=1.0, team_lanes=None, data_names=("summaries_obs",)):
        if isinstance(n_lags, bool) or int(n_lags) != n_lags or not 0 <= int(n_lags) <= self.MAX_LAGS:
            raise ValueError(f"n_lags must be an integer in 0..{self.MAX_LAGS}, got {n_lags!r}")
        if isinstance(n_obs, bool) or int(n_obs) != n_obs or not int(n_lags) < int(n_obs) <= self.MAX_OBS:
            raise ValueError(f"n_obs must be an integer above n_lags = {n_lags} and at most {self.MAX_OBS}, got {n_obs!r}")
        if isinstance(sigma2_0, (bool, str)) or not (np.isfinite(float(sigma2_0)) and float(sigma2_0) > 0.0):
            raise ValueError(f"sigma2_0 must be a positive finite number, got {sigma2_0!r}")
        self.n_obs, self.n_lags, self.sigma2_0 = int(n_obs), int(n_lags), float(sigma2_0)
        head = f"#define GARCH11_N_OBS {self.n_obs}\n#define GARCH11_N_LAGS {self.n_lags}\n" + ("" if team_lanes is None else "#define GARCH11_TEAM 1\n")
        super().__init__(head + device_source_text("garch11"), 3, self.n_lags + 2, [self.n_obs, self.n_lags, self.sigma2_0],
                         data=None if summaries_obs is None else [_segment(summaries_obs)], data_names=data_names,
                         n_outputs=self.n_obs, team_lanes=team_lanes)

    @staticmethod
    def summaries(y, n_lags=2):
        """mean(r), acov_0(r) .. acov_n_lags(r) of r = y^2 for a series of returns y (along the last axis) as the device computes
        them: the canonical sum over the n_obs times, every product rounded on its own, the autocovariances about the mean and
        divided by n_obs."""
        y = np.asarray(y, dtype=np.float64)
        r = y * y
        n = r.shape[-1]
        mean = _tree_sum(r) / float(n)
        d = r - mean[..., None]
        out = [mean]
        for j in range(int(n_lags) + 1):
            terms = np.zeros(r.shape)
            terms[..., j:] = d[..., j:] * d[..., :n - j]
            out.append(_tree_sum(terms) / float(n))
        return np.stack(out, axis=-1)

    @classmethod
    def from_observations(cls, y_obs, n_lags=2, team_lanes=None):
        """The model for an observed series of returns `y_obs`: n_obs = len(y_obs), summaries_obs = `summaries(y_obs, n_lags)`,
        sigma2_0 = the mean of y_obs^2 (summaries_obs[0])."""
        y_obs = _segment(y_obs)
        obs = cls.summaries(y_obs, n_lags)
        return cls(obs, n_obs=len(y_obs), n_lags=n_lags, sigma2_0=float(obs[0]), team_lanes=team_lanes)

    @classmethod
    def observe(cls, theta, n_obs=100, seed=None, sigma2_0=1.0, device=None):
        """A series of n_obs returns made by the device source itself: one forward run at theta = (omega, alpha, beta) on the
        predictive stream of particle 0, iteration 0 of `seed`."""
        from .api import simulate_outputs
        model = cls(np.zeros(2), n_obs=n_obs, n_lags=0, sigma2_0=sigma2_0)
        return simulate_outputs(model, np.asarray(theta, dtype=np.float64).reshape(1, 3), seed=seed, device=device)[0, 0]

    def validate_data(self, segments):
        # the source reads summaries_obs[j] and writes rho[j] for every j < n_lags + 2
        if len(segments) != 1 or len(segments[0]) != self.n_lags + 2:
            raise ValueError(f"summaries_obs is one segment of n_lags + 2 = {self.n_lags + 2} values (the mean of the squared returns and "
                             f"their autocovariances at lags 0 .. {self.n_lags})")
        if not np.all(np.isfinite(segments[0])):
            raise ValueError("summaries_obs must be finite")


class Ricker(DeviceSource):
    """The Ricker map with Poisson observations (Wood 2010), the model shipped on count draws keyed by the time step
    (`sabc::CountDraws`, `sabc::Series::map_poisson`): theta = (log r, sigma, phi), N_{t+1} = r N_t exp(-N_t + sigma z_t) for
    t = 0 .. burn_in + n_obs - 1 from N_0 = `n0`, with z the next normals of the particle's stream, and y_t ~ Poisson(phi N_{t+1});
    the last n_obs counts are the observation.  Summaries of them: the mean, the number of zeros, and the autocovariances about
    the mean at lags 0 .. n_lags (n_lags <= 7): rho_0 = |mean(y) - obs_0|, rho_1 = |#{t: y_t = 0} - obs_1|, rho_{2+j} =
    |acov_j(y) - obs_{2+j}|: n_stats = n_lags + 3.  `summaries_obs` is ONE data segment of n_lags + 3 finite values -- another
    series' summaries are another `SabcHandle.set_data` or `sabc(model, prior, summaries_obs=...)`, never another compilation --;
    `n_obs`, `burn_in` and `n_lags` are compile-time constants of the source, `n0` is one of its params.
    `from_observations(y_obs)` computes `summaries_obs` from a series of counts with the device's own sums (`summaries`),
    `observe(theta)` lets the device source simulate one.
    Source: device_sources/ricker.hip on `sabc::Series<burn_in + n_obs, W>` (csrc/team_series.hpp): the noise sigma z_t, one
    `recur` with the state N_t (exp_tab and a product rounded on its own), `map_poisson(rng, phi)` -- the draw of time t owns 64
    blocks of the counter, so a lane of a team draws for the times it holds --, then the canonical sums over t >= burn_in.
    `team_lanes` = 1, 4 or 16: the series spread over that many lanes per particle; None (the default): the same text with a
    private array per lane.  All forms give the same bits.  Outputs: the counts y_t, t >= burn_in (`posterior_predictive` gives
    [n, n_rep, n_obs])."""
    MAX_LAGS = 7
    MAX_TIMES = 1024                 # burn_in + n_obs: the series is 8 bytes per time of private memory per lane where it is not spread (twice)

    def __init__(self, summaries_obs=None, n_obs=50, burn_in=50, n_lags=5, n0=1.0, team_lanes=None, data_names=("summaries_obs",)):
        if isinstance(n_lags, (bool, str)) or int(n_lags) != n_lags or not 0 <= int(n_lags) <= self.MAX_LAGS:
            raise ValueError(f"n_lags must be an integer in 0..{self.MAX_LAGS}, got {n_lags!r}")
        if isinstance(n_obs, (bool, str)) or int(n_obs) != n_obs or not int(n_lags) < int(n_obs) <= self.MAX_TIMES:
            raise ValueError(f"n_obs must be an integer above n_lags = {n_lags} and at most {self.MAX_TIMES}, got {n_obs!r}")
        if isinstance(burn_in, (bool, str)) or int(burn_in) != burn_in or not 0 <= int(burn_in) <= self.MAX_TIMES - int(n_obs):
            raise ValueError(f"burn_in must be a non-negative integer with burn_in + n_obs <= {self.MAX_TIMES}, got {burn_in!r}")
        if isinstance(n0, (bool, str)) or not (np.isfinite(float(n0)) and float(n0) > 0.0):
            raise ValueError(f"n0 must be a positive finite number, got {n0!r}")
        self.n_obs, self.burn_in, self.n_lags, self.n0 = int(n_obs), int(burn_in), int(n_lags), float(n0)
        head = (f"#define RICKER_N_OBS {self.n_obs}\n#define RICKER_BURN_IN {self.burn_in}\n#define RICKER_N_LAGS {self.n_lags}\n"
                + ("" if team_lanes is None else "#define RICKER_TEAM 1\n"))
        super().__init__(head + device_source_text("ricker"), 3, self.n_lags + 3, [self.n_obs, self.burn_in, self.n_lags, self.n0],
                         data=None if summaries_obs is None else [_segment(summaries_obs)], data_names=data_names,
                         n_outputs=self.n_obs, team_lanes=team_lanes)

    @staticmethod
    def summaries(y, n_lags=5, burn_in=0):
        """mean(y), #{t: y_t = 0}, acov_0(y) .. acov_n_lags(y) of a series of observed counts y (along the last axis) as the
        device computes them: the canonical sum over the burn_in + n_obs times of the simulated series, the burn-in's terms +0.0
        (the tree's shape, and with it the rounding of the autocovariances, depends on them; the sums of counts are exact
        integers in any shape), every product rounded on its own, the autocovariances about the mean and divided by n_obs."""
        y = np.asarray(y, dtype=np.float64)
        n, lead = y.shape[-1], np.zeros(y.shape[:-1] + (int(burn_in),))
        mean = _tree_sum(np.concatenate([lead, y], axis=-1)) / float(n)
        zeros = _tree_sum(np.concatenate([lead, (y == 0.0).astype(np.float64)], axis=-1))
        d = y - mean[..., None]
        out = [mean, zeros]
        for j in range(int(n_lags) + 1):
            terms = np.zeros(y.shape)
            terms[..., j:] = d[..., j:] * d[..., :n - j]
            out.append(_tree_sum(np.concatenate([lead, terms], axis=-1)) / float(n))
        return np.stack(out, axis=-1)

    @classmethod
    def from_observations(cls, y_obs, burn_in=50, n_lags=5, n0=1.0, team_lanes=None):
        """The model for an observed series of counts `y_obs`: n_obs = len(y_obs), summaries_obs = `summaries(y_obs, n_lags, burn_in)`."""
        y_obs = _segment(y_obs)
        if isinstance(burn_in, (bool, str)) or int(burn_in) != burn_in or int(burn_in) < 0:
            raise ValueError(f"burn_in must be a non-negative integer, got {burn_in!r}")
        return cls(cls.summaries(y_obs, n_lags, burn_in), n_obs=len(y_obs), burn_in=burn_in, n_lags=n_lags, n0=n0, team_lanes=team_lanes)

    @classmethod
    def observe(cls, theta, n_obs=50, burn_in=50, seed=None, n0=1.0, device=None):
        """A series of n_obs counts made by the device source itself: one forward run at theta = (log r, sigma, phi) on the
        predictive stream of particle 0, iteration 0 of `seed`."""
        from .api import simulate_outputs
        model = cls(np.zeros(3), n_obs=n_obs, burn_in=burn_in, n_lags=0, n0=n0)
        return simulate_outputs(model, np.asarray(theta, dtype=np.float64).reshape(1, 3), seed=seed, device=device)[0, 0]

    def validate_data(self, segments):
        # the source reads summaries_obs[j] and writes rho[j] for every j < n_lags + 3
        if len(segments) != 1 or len(segments[0]) != self.n_lags + 3:
            raise ValueError(f"summaries_obs is one segment of n_lags + 3 = {self.n_lags + 3} values (the mean of the counts, the number of "
                             f"zeros and the autocovariances at lags 0 .. {self.n_lags})")
        if not np.all(np.isfinite(segments[0])):
            raise ValueError("summaries_obs must be finite")
