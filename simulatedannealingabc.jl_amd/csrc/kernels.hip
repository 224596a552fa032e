// kernels.hip -- hand-written gfx950 (CDNA4) kernels of the SABC particle-population update loop.
//
// Design notes (DESIGN.md has the long form):
//  * one wavefront lane per particle; particle state is SoA ([row][cap]) so that the 64 lanes of a
//    wave read/write 512 contiguous bytes per row;
//  * no dense contraction anywhere -> MFMA deliberately unused; the kernel is bound by Philox
//    integer multiplies and f64 log/sqrt/sincospi, not by HBM (40 algorithmic bytes per
//    particle-simulation for d = s = 1);
//  * the reductions the reference does in separate passes (n_accept :334, mean(u) :353, column
//    means :369-370, cov(population) proposals.jl:47,59) are fused into the update kernel:
//    wave shuffles -> LDS across the 4 waves of a block -> one partial row per block, summed
//    later in a fixed order (bitwise reproducible for a given grid).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include "control.hpp"
#include "p2p.hpp"
#include "persistent_kernel.hpp"
#include "update_kernel.hpp"
// the kernels that exist in this unit only, one header per subsystem.  ONE translation unit on purpose: which kernels share a
// module changes the generated code of the hot ones ("kernels.hip stays one translation unit")
#include "gk_kernel.hpp"
#include "hostmode_kernel.hpp"
#include "p2p_kernel.hpp"
#include "control_kernel.hpp"
#include "resample_kernel.hpp"
#include "cdf_kernel.hpp"
#include "op_kernel.hpp"

namespace sabc {

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
#define SABC_LAUNCH_RC() ((int)hipGetLastError())

// launch of a kernel from the run-time compiled module of a user simulator (rtc.hpp): same argument list as the
// template it was instantiated from; timing events ride on the dispatch packet like hipExtLaunchKernelGGL's
template <class... A>
static int module_launch(hipFunction_t f, unsigned grid, unsigned block, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1,
                         A... a) {
  void *args[] = {(void *)&a...};
  if (ev0)
    return (int)hipExtModuleLaunchKernel(f, grid * block, 1, 1, block, 1, 1, 0, stream, args, nullptr, ev0, ev1, 0);
  return (int)hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, 0, stream, args, nullptr);
}

// The (model, d, s) combinations the per-particle kernels are instantiated for, written once: for_model calls
// f(ModelCase<M, D, S>{}) for the one that matches m and returns false when none does; for_proposal does the same for the
// proposal (an integral_constant).  The launchers pass generic lambdas and read the constants off the argument's type.
template <int M, int D, int S>
struct ModelCase { static constexpr int model = M, d = D, s = S; };

template <class F, int... M, int... D, int... S>
static bool for_model_in(const ModelDesc &m, F &&f, ModelCase<M, D, S>... c) {
  return ((m.model_id == M && m.d == D && m.s == S ? (f(c), true) : false) || ...);
}
template <class F>
static bool for_model(const ModelDesc &m, F &&f) {
  return for_model_in(m, f, ModelCase<SABC_MODEL_GAUSS_IID, 1, 1>{}, ModelCase<SABC_MODEL_GAUSS_IID, 1, 2>{},
                      ModelCase<SABC_MODEL_GAUSS_IID, 2, 1>{}, ModelCase<SABC_MODEL_GAUSS_IID, 2, 2>{},
                      ModelCase<SABC_MODEL_GAUSS2D, 2, 3>{}, ModelCase<SABC_MODEL_LV, 3, 4>{});
}
using GkCase = ModelCase<SABC_MODEL_GK, kGkD, kGkS>;     // has kernels of its own (gk_kernel.hpp); k_stats and the resample take it

template <int P> using Proposal = std::integral_constant<int, P>;
template <class F>
static bool for_proposal(int prop_kind, F &&f) {
  switch (prop_kind) {
    case SABC_PROP_RANDOMWALK: f(Proposal<SABC_PROP_RANDOMWALK>{}); return true;
    case SABC_PROP_DIFFEVO: f(Proposal<SABC_PROP_DIFFEVO>{}); return true;
    case SABC_PROP_STRETCH: f(Proposal<SABC_PROP_STRETCH>{}); return true;
    default: return false;
  }
}
// both levels: f(ModelCase, Proposal)
template <class F>
static bool for_model_and_proposal(const ModelDesc &m, int prop_kind, F &&f) {
  bool known = false;
  for_model(m, [&](auto mc) { known = for_proposal(prop_kind, [&](auto p) { f(mc, p); }); });
  return known;
}

// workgroup of the per-particle kernels of a simulator from source (the wide form: kWideBlock, update_kernel.hpp)
inline int source_block(const ModelDesc &m) { return source_wide(m.s) ? kWideBlock : kBlock; }
inline unsigned source_blocks(const ModelDesc &m, int64_t n) { return (unsigned)((n + source_block(m) - 1) / source_block(m)); }

inline unsigned gk_blocks(int64_t n) { return (unsigned)((n + kGkPerBlock - 1) / kGkPerBlock); }   // k_simulate_gk, k_update_gk

int launch_prior_simulate(const ModelDesc &m, PopPtrs pp, hipStream_t stream, const RtcKernels *rtc) {
  if (pp.n_local <= 0) return 0;
  if (m.model_id == SABC_MODEL_USER) {
    if (!rtc || !rtc->prior_simulate) return (int)hipErrorInvalidValue;
    return module_launch(rtc->prior_simulate, source_blocks(m, pp.n_local), source_block(m), stream, nullptr, nullptr, m, pp);
  }
  if (m.model_id == SABC_MODEL_GK) {
    hipLaunchKernelGGL(k_simulate_gk, dim3(gk_blocks(pp.n_local)), dim3(kBlock), 0, stream, m, (const double *)nullptr,
                       pp.n_local, pp.cap, (uint64_t)pp.gid0, (uint64_t)0, 1, pp.pop, pp.rho, pp.cap);
    return SABC_LAUNCH_RC();
  }
  const dim3 grid((unsigned)n_blocks(pp.n_local)), block(kBlock);
  const bool known = for_model(m, [&](auto mc) {
    using C = decltype(mc);
    hipLaunchKernelGGL((k_prior_simulate<C::model, C::d, C::s>), grid, block, 0, stream, m, pp);
  });
  return known ? SABC_LAUNCH_RC() : (int)hipErrorInvalidValue;
}

int launch_cdf_population(const ModelDesc &m, PopPtrs pp, CdfPtrs cdf, hipStream_t stream) {
  if (pp.n_local <= 0) return 0;
  hipLaunchKernelGGL(k_cdf_population, dim3((unsigned)n_blocks(pp.n_local)), dim3(kBlock), 0, stream, m.d, m.s, pp, cdf);
  return SABC_LAUNCH_RC();
}

// workgroups (= partial rows) of one k_update launch over act_n particles (k_update_team: the same number -- a workgroup takes
// its particles in several trips, update_kernel.hpp)
int64_t update_rows(const ModelDesc &m, int64_t act_n) {
  if (act_n <= 0) return 0;
  if (m.model_id == SABC_MODEL_USER && source_wide(m.s)) return source_blocks(m, act_n);   // k_update_wide
  return m.model_id == SABC_MODEL_GK ? (int64_t)gk_blocks(act_n)   // 4 waves x kGkParticlesPerWave particles per workgroup
                                     : (act_n + update_block_threads(m.s) - 1) / update_block_threads(m.s);   // one thread per particle
}

// the persistent form exists for the built-in simulators with one lane per particle.  Its workgroups must all be resident at
// once: at most 256 of them, one per CU (SABC_PERSISTENT_WG lowers that).  Measured against the launch chain, cfg2, us per
// population update (tools/sweep_small.sh): RandomWalk n = 1000: 16.3 | 22.6, 5000: 17.0 | 23.4, 10 000: 17.7 | 23.5, 16 384:
// 18.3 | 23.5, 32 768: 19.2 | 23.7, 62 500: 22.0 | 23.8; DifferentialEvolution 1000: 29.9 | 39.5, 16 384: 33.6 | 41.1, 62 500:
// 38.4 | 41.5.  (A first version fenced every barrier -- a write-back and an invalidate of the L2 per update -- and lost from
// 64 workgroups on: 25.8 us at n = 16 384, 50.6 at 62 500; what crosses between workgroups now goes past the caches.)
static int64_t persist_max_workgroups() {
  static const int64_t v = [] { const char *e = std::getenv("SABC_PERSISTENT_WG"); const long long x = e ? std::atoll(e) : 256; return x < 0 ? 0 : x > 256 ? 256 : x; }();
  return v;
}
// lanes per particle of the persistent form: a TEAM of 16 (a row of the wave) or 4 (a quad) shares a particle's generator work
// (update_kernel.hpp, LANES) while that many times the workgroups still fit the launch -- the device is then so empty that the
// extra waves run on idle SIMDs and a particle's serial chain is what an update waits for --, else 1.
// SABC_PERSISTENT_LANES = 1 | 4 | 16 overrides (a team: where it fits, else the next smaller).
static int persist_lanes_env() {                     // (read at every call: a process may run the forms side by side)
  const char *e = std::getenv("SABC_PERSISTENT_LANES");
  const int x = e ? std::atoi(e) : 0;
  return x == 1 || x == 4 || x == 16 ? x : 0;
}
static int64_t persist_team_max_particles(int lanes) {   // per launch (a half batch for DifferentialEvolution / StretchMove)
  const char *e = std::getenv(lanes == 16 ? "SABC_PERSISTENT_LANES16_MAX" : "SABC_PERSISTENT_LANES4_MAX");
  const long long x = e ? std::atoll(e) : (lanes == 16 ? 2048 : 16384);
  return x < 0 ? 0 : x;
}
int64_t persistent_workgroups(const ModelDesc &m, int prop_kind, int64_t act_n, const RtcKernels *rtc, int *lanes_out, int *active_out) {
  const int64_t B = update_block_threads(m.s);
  if (lanes_out) *lanes_out = 1;
  if (active_out) *active_out = (int)B;
  if (prop_kind < 0 || prop_kind > 2 || act_n < 2) return 0;
  const bool user = m.model_id == SABC_MODEL_USER;     // a simulator from source: compiled with it (rtc.cpp), where its shape fits
  if (user ? !rtc || !rtc->persistent[0][prop_kind]
           : !(m.model_id == SABC_MODEL_GAUSS_IID || m.model_id == SABC_MODEL_GAUSS2D || m.model_id == SABC_MODEL_LV))
    return 0;
  if (!persistent_fits(m.d, m.s)) return 0;
  const int64_t per_launch = prop_kind == SABC_PROP_RANDOMWALK ? act_n : act_n - act_n / 2;     // the larger half batch
  // a wave per SIMD at most, and one wave of the workgroup without particles: the control wave (persistent_kernel.hpp)
  const int64_t thin = B - 64 < 256 ? B - 64 : 256;
  const int want = persist_lanes_env();
  const bool may[3] = {true, want == 4 || want == 16 || (want == 0 && per_launch <= persist_team_max_particles(4)),
                       want == 16 || (want == 0 && per_launch <= persist_team_max_particles(16))};
  // the thinnest spread whose workgroups fit the launch: a row per particle before a quad before a lane, a wave per SIMD before
  // the whole block
  for (int team = 2; team >= 0; --team) {
    if (!may[team] || (user && !rtc->persistent[team][prop_kind])) continue;
    for (const int64_t active : {thin, B}) {
      const int64_t wg = (kPersistTeamLanes[team] * per_launch + active - 1) / active;
      if (wg > persist_max_workgroups()) continue;
      if (lanes_out) *lanes_out = kPersistTeamLanes[team];
      if (active_out) *active_out = (int)active;
      return wg;
    }
  }
  return 0;
}

#ifdef SABC_PERSIST_TRACE
extern "C" __attribute__((visibility("default"))) int sabc_debug_persist_trace(unsigned long long *out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_persist_trace), sizeof(unsigned long long) * 64 * 16);
}
#endif

// the most workgroups a persistent launch over a shard of at most `cap` particles can have (sizes the partial rows)
int64_t persistent_workgroups_bound(const ModelDesc &m, int64_t cap) {
  if (!persistent_fits(m.d, m.s)) return 0;
  const int64_t A = update_block_threads(m.s) - 64 < 256 ? update_block_threads(m.s) - 64 : 256, wg16 = (16 * cap + A - 1) / A;
  return wg16 < persist_max_workgroups() ? wg16 : persist_max_workgroups();
}

int launch_update_persistent(const ModelDesc &m, int prop_kind, const PersistArgs &pa_in, ControlBlock *cb, PopPtrs pp, CdfPtrs cdf,
                             PartnerView pv_a, PartnerView pv_b, double *partials, double *hist, Mailbox *mbox, double *stage,
                             hipStream_t stream, const RtcKernels *rtc) {
  int lanes = 1, active = 0;
  const int64_t wg = persistent_workgroups(m, prop_kind, pa_in.act_n, rtc, &lanes, &active);
  if (wg <= 0) return (int)hipErrorInvalidValue;
  PersistArgs pa = pa_in;
  pa.active = active;
  pa.ctrl_wave = active < (int)update_block_threads(m.s) ? active / 64 : -1;
  const dim3 grid((unsigned)wg), block((unsigned)update_block_threads(m.s));
  if (m.model_id == SABC_MODEL_USER)
    return module_launch(rtc->persistent[persist_team(lanes)][prop_kind], grid.x, block.x, stream, nullptr, nullptr, m, pa, cb, pp, cdf,
                         pv_a, pv_b, partials, hist, mbox, stage);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, m, pa, cb, pp, cdf, pv_a, pv_b, partials, hist, mbox, stage);
  };
  const bool known = for_model_and_proposal(m, prop_kind, [&](auto mc, auto p) {
    using C = decltype(mc);
    constexpr int P = decltype(p)::value;
    if (lanes == 16) launch(k_update_persistent<C::model, C::d, C::s, P, 16>);
    else if (lanes == 4) launch(k_update_persistent<C::model, C::d, C::s, P, 4>);
    else launch(k_update_persistent<C::model, C::d, C::s, P, 1>);
  });
  return known ? SABC_LAUNCH_RC() : (int)hipErrorInvalidValue;
}

int launch_update(const ModelDesc &m, const StepArgs &c, const ControlBlock *cb, PopPtrs pp, CdfPtrs cdf, PartnerView pv,
                  int64_t act_lo, int64_t act_n, double *partials, int64_t row0, hipStream_t stream, hipEvent_t ev0,
                  hipEvent_t ev1, const RtcKernels *rtc) {
  if (act_n <= 0) return 0;
  const dim3 grid((unsigned)update_rows(m, act_n)), block(m.model_id == SABC_MODEL_GK ? kBlock : update_block_threads(m.s));
  double *out = partials + row0 * n_partials(m.d, m.s);
  if (m.model_id == SABC_MODEL_USER) {
    if (!rtc || c.prop_kind < 0 || c.prop_kind > 2 || !rtc->update[c.prop_kind]) return (int)hipErrorInvalidValue;
    const unsigned b = source_wide(m.s) ? kWideBlock : update_block_threads(m.s);     // (k_update_wide | k_update)
    if (rtc->team_aware && rtc->chain_lanes > 1) {   // k_update_team: the same rows, a workgroup's particles in chain_lanes trips
      const hipFunction_t f = source_wide(m.s) ? nullptr : rtc->update_team[persist_team(rtc->chain_lanes) - 1][c.prop_kind];
      if (!f) return (int)hipErrorInvalidValue;
      return module_launch(f, grid.x, b, stream, ev0, ev1, m, c, cb, pp, cdf, pv, act_lo, act_n, out);
    }
    return module_launch(rtc->update[c.prop_kind], grid.x, b, stream, ev0, ev1, m, c, cb, pp, cdf, pv, act_lo, act_n, out);
  }
  // ev0 / ev1 (optional): timing events attached to the dispatch packet itself (hipExtLaunchKernel), so that
  // measuring the kernel does not put separate marker packets into the queue
  auto launch = [&](auto kernel) {
    if (ev0) hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, ev0, ev1, 0, m, c, cb, pp, cdf, pv, act_lo, act_n, out);
    else hipLaunchKernelGGL(kernel, grid, block, 0, stream, m, c, cb, pp, cdf, pv, act_lo, act_n, out);
  };
  if (m.model_id == SABC_MODEL_GK) {
    // wanted ranks that are all multiples of 16 (BASELINE config 4): FOUR particles at a time, one per row of 16 lanes, eight
    // values per lane -- 15 of the network's 24 steps stay inside the lane (device_models.hpp: gk_simulate_rows4)
    bool rows4 = true;
    for (int j = 0; j < kGkS; ++j) rows4 = rows4 && (((int)m.p[2 + j]) & 15) == 0 && (int)m.p[2 + j] >= 16 && (int)m.p[2 + j] <= 128;
    const bool known = for_proposal(c.prop_kind, [&](auto p) {
      constexpr int P = decltype(p)::value;
      if (rows4) launch(k_update_gk<P, true>);
      else launch(k_update_gk<P, false>);
    });
    return known ? SABC_LAUNCH_RC() : (int)hipErrorInvalidValue;
  }
  const bool known = for_model_and_proposal(m, c.prop_kind, [&](auto mc, auto p) {
    using C = decltype(mc);
    launch(k_update<C::model, C::d, C::s, decltype(p)::value>);
  });
  return known ? SABC_LAUNCH_RC() : (int)hipErrorInvalidValue;
}

int launch_host_prior(const ModelDesc &m, PopPtrs pp, hipStream_t stream) {
  if (pp.n_local <= 0) return 0;
  hipLaunchKernelGGL(k_host_prior, dim3((unsigned)n_blocks(pp.n_local)), dim3(kBlock), 0, stream, m, pp);
  return SABC_LAUNCH_RC();
}

int launch_host_propose(const ModelDesc &m, const StepArgs &c, const ControlBlock *cb, PopPtrs pp, PartnerView pv,
                        int64_t act_lo, int64_t act_n, double *thp, double *aux, double *thp_host, unsigned char *gate_host,
                        double *cur_out, unsigned int *done, unsigned long long *flag, unsigned long long seq, int64_t chunk,
                        hipStream_t stream) {
  if (act_n <= 0) return 0;
  HostSignal sig;
  sig.done = done; sig.flag = flag; sig.seq = seq; sig.chunk = chunk;
  hipLaunchKernelGGL(k_host_propose, dim3((unsigned)n_blocks(act_n)), dim3(kBlock), 0, stream, m, c, cb, pp, pv, act_lo, act_n,
                     thp, aux, thp_host, gate_host, cur_out, sig);
  return SABC_LAUNCH_RC();
}

int launch_host_accept(const ModelDesc &m, const StepArgs &c, const ControlBlock *cb, PopPtrs pp, CdfPtrs cdf, int64_t act_lo,
                       int64_t act_n, int64_t t_lo, int64_t t_n, const double *thp, const double *aux, const double *rho_prop,
                       const double *lp_host, unsigned long long *n_accept, hipStream_t stream) {
  if (t_n <= 0) return 0;
  hipLaunchKernelGGL(k_host_accept, dim3((unsigned)n_blocks(t_n)), dim3(kBlock), 0, stream, m, c, cb, pp, cdf, act_lo, act_n,
                     t_lo, t_n, thp, aux, rho_prop, lp_host, n_accept);
  return SABC_LAUNCH_RC();
}

int launch_stats_rt(const ModelDesc &m, const ControlBlock *cb, PopPtrs pp, double *partials, unsigned long long *n_accept,
                    hipStream_t stream) {
  if (pp.n_local <= 0) return 0;
  hipLaunchKernelGGL(k_stats_rt, dim3((unsigned)n_blocks(pp.n_local)), dim3(kBlock), 0, stream, m.d, m.s, cb, pp, partials,
                     n_accept);
  return SABC_LAUNCH_RC();
}

int launch_stats(const ModelDesc &m, const ControlBlock *cb, PopPtrs pp, double *partials, hipStream_t stream,
                 const RtcKernels *rtc) {
  if (pp.n_local <= 0) return 0;
  if (m.model_id == SABC_MODEL_HOST) return launch_stats_rt(m, cb, pp, partials, nullptr, stream);
  if (m.model_id == SABC_MODEL_USER) {
    if (!rtc || !rtc->stats) return (int)hipErrorInvalidValue;
    return module_launch(rtc->stats, (unsigned)n_blocks(pp.n_local), kBlock, stream, nullptr, nullptr, cb, pp, partials);
  }
  const dim3 grid((unsigned)n_blocks(pp.n_local)), block(kBlock);
  auto launch = [&](auto mc) {
    using C = decltype(mc);
    hipLaunchKernelGGL((k_stats<C::d, C::s>), grid, block, 0, stream, cb, pp, partials);
  };
  if (m.model_id == SABC_MODEL_GK) { launch(GkCase{}); return SABC_LAUNCH_RC(); }
  return for_model(m, launch) ? SABC_LAUNCH_RC() : (int)hipErrorInvalidValue;
}

int launch_reduce_partials(const double *partials, int64_t rows, int np, double *sums, const int *halt,
                           hipStream_t stream) {
  hipLaunchKernelGGL(k_reduce_partials, dim3((unsigned)np), dim3(kBlock), 0, stream, partials, rows, np, sums, halt);
  return SABC_LAUNCH_RC();
}

int launch_reduce_control(const double *partials, int64_t rows, int np, double *stage, ControlBlock *cb, const ControlArgs &a,
                          double *hist, Mailbox *mbox, hipStream_t stream, const P2PView *pv, uint32_t seq, bool do_control,
                          int silent) {
  XchgArgs x;
  std::memset(&x, 0, sizeof(x));
  x.do_control = do_control ? 1 : 0;
  // a short matrix of partial rows (a shard of an 8-GPU run: 489 rows at n = 1e6) takes 4 waves instead of 16: the waves of
  // one workgroup start one after the other and the launch waits for the last one's loads (seen with clock reads between the
  // phases in an instrumented build: DESIGN.md)
  static const int forced = [] { const char *e = std::getenv("SABC_RC_BLOCK"); const int v = e ? std::atoi(e) : 0; return (v == 256 || v == 1024) ? v : 0; }();
  // (np <= 256 threads' worth: the kernel gives every component of the row a lane)
  const int block = forced && np <= 256 ? forced : ((rows < 0 && np <= 256) || (np <= 64 && rows >= 0 && rows <= (int64_t)24 * (256 / np))) ? 256 : 1024;
  if (pv) {
    x.pv = *pv; x.seq = seq; x.silent = silent;
    hipLaunchKernelGGL(k_reduce_control<true>, dim3(1), dim3(block), 0, stream, partials, rows, np, stage, cb, a, hist, mbox, x);
  } else {
    hipLaunchKernelGGL(k_reduce_control<false>, dim3(1), dim3(block), 0, stream, partials, rows, np, stage, cb, a, hist, mbox, x);
  }
  return SABC_LAUNCH_RC();
}

int launch_p2p_barrier(const P2PView &pv, uint32_t seq, ControlBlock *cb, bool guarded, int silent, hipStream_t stream) {
  hipLaunchKernelGGL(k_p2p_barrier, dim3(1), dim3(64), 0, stream, pv, seq, cb, guarded ? 1 : 0, silent);
  return SABC_LAUNCH_RC();
}

int launch_p2p_commit(const P2PView &pv, uint32_t call, int status, bool wait, ControlBlock *cb, int silent, hipStream_t stream) {
  hipLaunchKernelGGL(k_p2p_commit, dim3(1), dim3(64), 0, stream, pv, call, status, wait ? 1 : 0, cb, silent);
  return SABC_LAUNCH_RC();
}

int launch_p2p_selftest(const P2PView &pv, uint32_t seq, int np, const double *in, double *out, int *failed, int silent,
                        hipStream_t stream) {
  hipLaunchKernelGGL(k_p2p_selftest, dim3(1), dim3(1024), 0, stream, pv, seq, np, in, out, failed, silent);
  return SABC_LAUNCH_RC();
}

int launch_p2p_leave(const P2PView &pv, uint32_t gen, hipStream_t stream) {
  hipLaunchKernelGGL(k_p2p_leave, dim3(1), dim3(64), 0, stream, pv, gen);
  return SABC_LAUNCH_RC();
}

static PatternBufs pattern_bufs(double *const buf[3], const int64_t len[3]) {
  PatternBufs g;
  for (int b = 0; b < 3; ++b) {
    g.buf[b] = reinterpret_cast<uint64_t *>(buf[b]);
    g.len[b] = len[b];
    g.count[b] = (int32_t)(len[b] < kPatternSamples ? len[b] : kPatternSamples);
  }
  return g;
}
int p2p_pattern_save_words() { return 3 * kPatternSamples; }
int launch_p2p_pattern_write(double *const buf[3], const int64_t len[3], double *save, uint32_t gen, int round, int rank, int mode,
                             hipStream_t stream) {
  hipLaunchKernelGGL(k_p2p_pattern_write, dim3(kPatternSamples / 256, 3), dim3(256), 0, stream, pattern_bufs(buf, len),
                     reinterpret_cast<uint64_t *>(save), gen, round, rank, mode);
  return SABC_LAUNCH_RC();
}
int launch_p2p_pattern_check(const double *const peer_buf[3][kMaxPeers], const int64_t len[3], uint32_t gen, int round, int world,
                             unsigned int *out, hipStream_t stream) {
  PatternPeers pp;
  for (int b = 0; b < 3; ++b)
    for (int r = 0; r < kMaxPeers; ++r) pp.buf[b][r] = reinterpret_cast<const uint64_t *>(peer_buf[b][r]);
  double *none[3] = {nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(k_p2p_pattern_check, dim3(kPatternSamples / 256, 3, world), dim3(256), 0, stream, pp, pattern_bufs(none, len), gen,
                     round, world, out);
  return SABC_LAUNCH_RC();
}

int launch_control(ControlBlock *cb, const ControlArgs &a, double *hist, Mailbox *mbox, const double *sums_in,
                   hipStream_t stream) {
  hipLaunchKernelGGL(k_control, dim3(1), dim3(64), 0, stream, cb, a, hist, mbox, sums_in);
  return SABC_LAUNCH_RC();
}

int launch_resample_weights(const ModelDesc &m, PopPtrs pp, const ControlBlock *cb, double n_global, double delta,
                            hipStream_t stream) {
  if (pp.n_local <= 0) return 0;
  hipLaunchKernelGGL(k_resample_weights, dim3((unsigned)n_blocks(pp.n_local)), dim3(kBlock), 0, stream, m.d, m.s, pp,
                     cb, n_global, delta);
  return SABC_LAUNCH_RC();
}

int launch_weight_scan(const ShardBlocks &gathered, int64_t n_global, double *block_sums,
                       double *cum, double *totals, double *totals_host, hipStream_t stream) {
  const int64_t nb = (n_global + kScanChunk - 1) / kScanChunk;
  double *bs = block_sums, *bq = block_sums + nb, *cm = block_sums + 2 * nb;
  WeightArgs wa;
  std::memset(&wa, 0, sizeof(wa));
  // blocks that live in other shards' memory are read ONCE: the first pass parks the weights in `cum`
  const int park = gathered.direct ? 1 : 0;
  hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)nb), dim3(kBlock), 0, stream, gathered, n_global, bs, bq, wa, park ? cum : (double *)nullptr);
  hipLaunchKernelGGL(k_scan_offsets, dim3(1), dim3(1024), 0, stream, bs, bq, nb, totals, totals_host);
  PackArgs none;
  std::memset(&none, 0, sizeof(none));
  hipLaunchKernelGGL(k_scan_final, dim3((unsigned)nb), dim3(kBlock), 0, stream, gathered, n_global, bs, cum, cm, none, park);
  return SABC_LAUNCH_RC();
}

// doubles of the packed-line scratch of launch_resample_local for a shard of n particles:
// packed lines | line ends (+ two of +inf, rounded up to a line) | the guide (n_lines + 2 int32)
static inline int64_t pack_ge_doubles(int64_t lines) { return ((lines + 8 + 15) / 16) * 16; }

int64_t resample_pack_doubles(int row_len, int64_t n) {
  const int per = 16 / (1 + row_len);
  const int pg = per >= 4 ? 4 : per >= 2 ? 2 : per >= 1 ? 1 : 0;
  if (pg == 0) return 0;
  const int64_t lines = (n + pg - 1) / pg;
  return lines * 16 + pack_ge_doubles(lines) + (lines + 2 + 1) / 2 + 32;
}

// One shard: weights (fused into the first scan pass), scan, staging copy, draw + gather (+ the moment sums of the
// resampled population when the model's (d, s) is one the kernels are instantiated for): 4 launches.
// *stats_rows = partial rows written, or -1 when the caller still has to run the stats pass.
int launch_resample_local(const ModelDesc &m, PopPtrs src, PopPtrs dst, const ControlBlock *cb, double delta, uint64_t iter,
                          double *block_sums, double *cum, double *totals, double *totals_host, double *pack,
                          double *partials, int64_t *stats_rows, hipStream_t stream) {
  const int64_t n = src.n_local, cap = src.cap;
  *stats_rows = -1;
  if (n <= 0) return 0;
  const int rows = m.d + m.s + 1, rl = m.d + m.s;
  const int per = 16 / (1 + rl);
  const int pg = per >= 4 ? 4 : per >= 2 ? 2 : per >= 1 ? 1 : 0;
  const int64_t nb = (n + kScanChunk - 1) / kScanChunk;
  double *bs = block_sums, *bq = block_sums + nb, *cm = block_sums + 2 * nb;
  WeightArgs wa;
  std::memset(&wa, 0, sizeof(wa));
  wa.fused = 1; wa.d = m.d; wa.s = m.s; wa.pp = src; wa.cb = cb; wa.n_global = (double)n; wa.delta = delta;
  PackArgs pa;
  std::memset(&pa, 0, sizeof(pa));
  if (pg > 0 && pack) {
    const int64_t lines = (n + pg - 1) / pg;
    pa.pk = pack; pa.ge = pack + lines * 16; pa.guide = reinterpret_cast<int32_t *>(pa.ge + pack_ge_doubles(lines));
    pa.totals = totals; pa.row_len = rl; pa.pg = pg;
  }
  const ShardBlocks own = flat_blocks(src.pop, rows, cap, 1);
  hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)nb), dim3(kBlock), 0, stream, own, n, bs, bq, wa, (double *)nullptr);
  hipLaunchKernelGGL(k_scan_offsets, dim3(1), dim3(1024), 0, stream, bs, bq, nb, totals, totals_host);
  hipLaunchKernelGGL(k_scan_final, dim3((unsigned)nb), dim3(kBlock), 0, stream, own, n, bs, cum, cm, pa, 0);
  const size_t lds = nb <= kGatherCoarseMax ? (size_t)nb * sizeof(double) : 0;
  const dim3 grid((unsigned)n_blocks(n)), block(kBlock);
  if (!pa.pk) {                      // a row does not fit a 128-byte line (d + s > 15): the unpacked gather, sums by the caller
    hipLaunchKernelGGL(k_resample_gather<true>, grid, block, lds, stream, m.seed, m.d, m.s, own, n,
                       (const double *)cum, (const double *)bs, (const double *)cm, nb, (const double *)totals, iter, dst,
                       (int64_t *)nullptr);
    return SABC_LAUNCH_RC();
  }
  auto launch_stats = [&](auto mc) {
    using C = decltype(mc);
    hipLaunchKernelGGL((k_resample_gather_stats<C::d, C::s>), grid, block, lds, stream, m.seed, (const double *)pa.pk,
                       (const double *)pa.ge, (const int32_t *)pa.guide, pg, n, (const double *)bs, nb,
                       (const double *)totals, iter, dst, cb, partials);
    *stats_rows = n_blocks(n);
  };
  if (m.model_id == SABC_MODEL_GK) { launch_stats(GkCase{}); return SABC_LAUNCH_RC(); }
  if (m.model_id == SABC_MODEL_HOST || m.model_id == SABC_MODEL_USER) {
    hipLaunchKernelGGL(k_resample_gather_packed, grid, block, lds, stream, m.seed, rl, (const double *)pa.pk,
                       (const double *)pa.ge, (const int32_t *)pa.guide, pg, n, (const double *)bs, nb, (const double *)totals, iter,
                       dst);
    return SABC_LAUNCH_RC();
  }
  return for_model(m, launch_stats) ? SABC_LAUNCH_RC() : (int)hipErrorInvalidValue;
}

int launch_resample_gather(const ModelDesc &m, const ShardBlocks &gathered, int64_t n_global,
                           const double *cum, const double *block_sums, const double *totals, uint64_t iter, PopPtrs dst,
                           hipStream_t stream) {
  if (dst.n_local <= 0) return 0;
  const int64_t nb = (n_global + kScanChunk - 1) / kScanChunk;
  const size_t lds = nb <= kGatherCoarseMax ? (size_t)nb * sizeof(double) : 0;
  hipLaunchKernelGGL(k_resample_gather<true>, dim3((unsigned)n_blocks(dst.n_local)), dim3(kBlock), lds, stream, m.seed, m.d,
                     m.s, gathered, n_global, cum, block_sums, block_sums + 2 * nb, nb, totals, iter, dst,
                     (int64_t *)nullptr);
  return SABC_LAUNCH_RC();
}

int launch_resample_select(const ModelDesc &m, int64_t cap, int64_t n_global, const double *cum, const double *block_sums,
                           const double *totals, uint64_t iter, PopPtrs dst, int64_t *idx_out, hipStream_t stream) {
  if (dst.n_local <= 0) return 0;
  const int64_t nb = (n_global + kScanChunk - 1) / kScanChunk;
  const size_t lds = nb <= kGatherCoarseMax ? (size_t)nb * sizeof(double) : 0;
  hipLaunchKernelGGL(k_resample_gather<false>, dim3((unsigned)n_blocks(dst.n_local)), dim3(kBlock), lds, stream, m.seed, m.d,
                     m.s, flat_blocks(nullptr, 0, cap, 1), n_global, cum, block_sums, block_sums + 2 * nb, nb, totals, iter,
                     dst, idx_out);
  return SABC_LAUNCH_RC();
}

int launch_bucket_count(const int64_t *idx, int64_t n_local, int64_t cap, unsigned long long *counts, hipStream_t stream) {
  if (n_local <= 0) return 0;
  hipLaunchKernelGGL(k_bucket_count, dim3((unsigned)n_blocks(n_local)), dim3(kBlock), 0, stream, idx, n_local, cap, counts);
  return SABC_LAUNCH_RC();
}

int launch_bucket_scatter(const int64_t *idx, int64_t n_local, int64_t cap, unsigned long long *cursor, double *req,
                          int64_t *slot, hipStream_t stream) {
  if (n_local <= 0) return 0;
  hipLaunchKernelGGL(k_bucket_scatter, dim3((unsigned)n_blocks(n_local)), dim3(kBlock), 0, stream, idx, n_local, cap, cursor,
                     req, slot);
  return SABC_LAUNCH_RC();
}

int launch_resample_serve(const double *req, int64_t m, int row_len, PopPtrs src, double *rows_out, hipStream_t stream) {
  if (m <= 0) return 0;
  hipLaunchKernelGGL(k_resample_serve, dim3((unsigned)n_blocks(m * row_len)), dim3(kBlock), 0, stream, req, m, row_len, src,
                     rows_out);
  return SABC_LAUNCH_RC();
}

int launch_resample_scatter(const double *rows_in, const int64_t *slot, int64_t n_local, int row_len, PopPtrs dst,
                            hipStream_t stream) {
  if (n_local <= 0) return 0;
  hipLaunchKernelGGL(k_resample_scatter, dim3((unsigned)n_blocks(n_local * row_len)), dim3(kBlock), 0, stream, rows_in, slot,
                     n_local, row_len, dst);
  return SABC_LAUNCH_RC();
}

int launch_cdf_knots(const double *sorted, int64_t n, double *knots, int64_t *meta, hipStream_t stream) {
  hipLaunchKernelGGL(k_cdf_meta, dim3(1), dim3(64), 0, stream, sorted, n, meta);
  hipLaunchKernelGGL(k_cdf_fill, dim3((unsigned)n_blocks(n > 0 ? n : 1)), dim3(kBlock), 0, stream, sorted, n, meta, knots);
  return SABC_LAUNCH_RC();
}

int launch_cdf_index(double *knots, int64_t len, int64_t stride, int shift, double *coarse, int n_coarse, double *mid,
                     int64_t mid_len, hipStream_t stream) {
  int64_t work = n_coarse;
  if (mid_len > work) work = mid_len;
  if (stride - len > work) work = stride - len;
  hipLaunchKernelGGL(k_cdf_index, dim3((unsigned)n_blocks(work)), dim3(kBlock), 0, stream, knots, len, stride, shift, coarse,
                     n_coarse, mid, mid_len);
  return SABC_LAUNCH_RC();
}

int launch_compact_column(const ShardBlocks &gathered, int stat, int64_t n_global, double *out, hipStream_t stream) {
  hipLaunchKernelGGL(k_compact_column, dim3((unsigned)n_blocks(n_global)), dim3(kBlock), 0, stream, gathered, stat, n_global, out);
  return SABC_LAUNCH_RC();
}

int launch_cdf_eval(const double *knots, int64_t len, const double *q, int64_t m, double *out, hipStream_t stream) {
  if (m <= 0) return 0;
  hipLaunchKernelGGL(k_cdf_eval, dim3((unsigned)n_blocks(m)), dim3(kBlock), 0, stream, knots, len, q, m, out);
  return SABC_LAUNCH_RC();
}

int launch_cdf_apply_matrix(CdfPtrs cdf, int s, const double *rho, int64_t m, double *u_out, hipStream_t stream) {
  if (m <= 0) return 0;
  hipLaunchKernelGGL(k_cdf_apply_matrix, dim3((unsigned)n_blocks(m)), dim3(kBlock), 0, stream, cdf, s, rho, m, u_out);
  return SABC_LAUNCH_RC();
}

static_assert(kPurposeSim == PURPOSE_SIM && kPurposePredict == PURPOSE_PREDICT, "kernels.hpp restates device_rng.hpp's purposes");
int launch_simulate_batch(const ModelDesc &m, const double *theta, int64_t n, uint64_t pid0, uint64_t iter,
                          double *rho_out, hipStream_t stream, const RtcKernels *rtc, const unsigned char *gate,
                          double *out, int64_t n_out, uint32_t purpose) {
  if (n <= 0) return 0;
  if (m.model_id == SABC_MODEL_USER) {
    if (!rtc || !rtc->simulate_batch) return (int)hipErrorInvalidValue;
    if (rtc->team_aware && rtc->chain_lanes > 1) {   // k_simulate_batch_team: chain_lanes threads per row
      const hipFunction_t f = source_wide(m.s) ? nullptr : rtc->simulate_batch_team[persist_team(rtc->chain_lanes) - 1];
      if (!f) return (int)hipErrorInvalidValue;
      return module_launch(f, (unsigned)n_blocks(n * rtc->chain_lanes), kBlock, stream, nullptr, nullptr, m, theta, n, pid0, iter, rho_out, gate,
                           out, n_out, purpose);
    }
    return module_launch(rtc->simulate_batch, source_blocks(m, n), source_block(m), stream, nullptr, nullptr, m, theta, n, pid0, iter,
                         rho_out, gate, out, n_out, purpose);
  }
  if (out || purpose != PURPOSE_SIM) return (int)hipErrorInvalidValue;      // outputs and other streams: simulators from source only
  if (m.model_id == SABC_MODEL_GK) {                  // (the gate is not looked at: the wave-cooperative simulator is a fixed
                                                      // amount of arithmetic for any theta, and gated-out rows are never read)
    hipLaunchKernelGGL(k_simulate_gk, dim3(gk_blocks(n)), dim3(kBlock), 0, stream, m, theta, n, n, pid0, iter, 0,
                       (double *)nullptr, rho_out, n);
    return SABC_LAUNCH_RC();
  }
  const dim3 grid((unsigned)n_blocks(n)), block(kBlock);
  const bool known = for_model(m, [&](auto mc) {
    using C = decltype(mc);
    hipLaunchKernelGGL((k_simulate_batch<C::model, C::d, C::s>), grid, block, 0, stream, m, theta, n, pid0, iter, rho_out, gate,
                       (double *)nullptr, (int64_t)0, (uint32_t)PURPOSE_SIM);
  });
  return known ? SABC_LAUNCH_RC() : (int)hipErrorInvalidValue;
}

int launch_prior_op(const ModelDesc &m, uint64_t pid0, int64_t n, double *theta, double *lp, hipStream_t stream,
                    const RtcKernels *rtc) {
  if (n <= 0) return 0;
  if (rtc) {                                   // a prior that lives in the run-time compiled unit
    if (!rtc->prior_op) return (int)hipErrorInvalidValue;
    return module_launch(rtc->prior_op, (unsigned)n_blocks(n), kBlock, stream, nullptr, nullptr, m, pid0, n, theta, lp);
  }
  hipLaunchKernelGGL(k_prior_op, dim3((unsigned)n_blocks(n)), dim3(kBlock), 0, stream, m, pid0, n, theta, lp);
  return SABC_LAUNCH_RC();
}

int launch_normal_pairs(uint64_t seed, uint64_t pid0, uint32_t purpose, uint64_t iter, uint32_t k, int64_t m, double *out,
                        hipStream_t stream) {
  if (m <= 0) return 0;
  hipLaunchKernelGGL(k_normal_pairs, dim3((unsigned)n_blocks(m)), dim3(kBlock), 0, stream, seed, pid0, purpose, iter, k, m, out);
  return SABC_LAUNCH_RC();
}

int launch_rng_peak(uint64_t seed, int pairs, int64_t n, double *out, hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_rng_peak, dim3((unsigned)n_blocks(n)), dim3(kBlock), 0, stream, seed, pairs, n, out);
  return SABC_LAUNCH_RC();
}

int launch_normal_quads_f32(uint64_t seed, uint64_t pid0, uint32_t purpose, uint64_t iter, uint32_t k, int64_t m, float *out,
                            hipStream_t stream) {
  if (m <= 0) return 0;
  hipLaunchKernelGGL(k_normal_quads_f32, dim3((unsigned)n_blocks(m)), dim3(kBlock), 0, stream, seed, pid0, purpose, iter, k, m, out);
  return SABC_LAUNCH_RC();
}

int launch_rng_peak_f32(uint64_t seed, int quads, int64_t n, float *out, hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_rng_peak_f32, dim3((unsigned)n_blocks(n)), dim3(kBlock), 0, stream, seed, quads, n, out);
  return SABC_LAUNCH_RC();
}

int launch_philox_debug(uint64_t seed, uint64_t pid, uint32_t purpose, uint64_t iter, uint32_t k, uint32_t *words,
                        double *normals, hipStream_t stream) {
  hipLaunchKernelGGL(k_philox_debug, dim3(1), dim3(64), 0, stream, seed, pid, purpose, iter, k, words, normals);
  return SABC_LAUNCH_RC();
}

}  // namespace sabc
