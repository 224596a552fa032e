// hip_backend_hostmode.hip -- HipBackend, host mode: f_dist and / or the prior are callbacks of the caller.
#include "hip_backend_internal.hpp"

#include <chrono>
#include <cmath>

namespace sabc {

// ---- host mode: f_dist (SABC_MODEL_HOST) and / or the prior (prior_joint = 2) are host callbacks ----
// A prior that lives in host callbacks next to a DEVICE-coded simulator (any Distribution of the reference next to a built-in
// or source-compiled f_dist) takes the same cut -- k_host_propose -> logpdf(prior, .) on the host -> the simulator as its own
// launch over the gated proposals (k_simulate_batch, the fused kernel's streams) -> k_host_accept -- with one chunk per half
// batch: the callback is the log density alone, there is no host simulation to overlap.
// f_dist is the caller's function (SimulatedAnnealingABC.jl:315), so every half batch is cut at the host:
//   k_host_propose (device) -> f_dist on the proposals inside the prior's support (host) -> k_host_accept (device).
// What the library adds around the callback is kept off the critical path:
//  * staging arrays are PINNED host memory MAPPED into the device, allocated once: the kernels write proposals and read
//    distances in place -- no hipMemcpy call, no pageable staging, no allocation per half batch; and only what the host
//    needs crosses PCIe: the proposals and ONE BYTE of prior gate go down, the distances come up; the proposals' second copy
//    and the log densities stay in device memory for the accept step;
//  * the propose kernel signals completion CHUNK by chunk into a pinned flag word the host polls (no stream sync): the
//    callback for chunk c runs while the accept kernel of chunk c - 1 executes and later chunks are still being proposed;
//  * nothing waits at the end of a half batch: the next kernel on the stream is ordered behind the accept kernels.
int HipBackend::ensure_host_buffers() {
  if (host_.buf.thp.host()) return 0;
  const size_t cap = (size_t)(sh_.cap > 0 ? sh_.cap : 1);
  HostMode::Staging b;                                   // (a failure below frees what it holds: the next call starts over)
  HB_CHECK(b.thp.alloc((size_t)m_.d * cap), "hipHostMalloc(host-mode staging)");
  HB_CHECK(b.rho.alloc((size_t)m_.s * cap), "hipHostMalloc(host-mode staging)");
  HB_CHECK(b.gate.alloc(cap), "hipHostMalloc(prior gate)");
  if (m_.prior_joint == 2) {
    HB_CHECK(b.cur.alloc((size_t)m_.d * cap), "hipHostMalloc(host-mode staging)");
    HB_CHECK(b.lp2.alloc(2 * cap), "hipHostMalloc(host-mode staging)");
  }
  // what only the device reads again: the proposals and (log prior, log factor) of the half batch in flight
  HB_CHECK(b.dev_thp.alloc((size_t)m_.d * cap), "hipMalloc(proposals)");
  HB_CHECK(b.dev_aux.alloc(2 * cap), "hipMalloc(log prior, log factor)");
  if (m_.model_id != SABC_MODEL_HOST)                    // a device-coded simulator next to a host prior: its distances stay on the device
    HB_CHECK(b.dev_rho_prop.alloc((size_t)m_.s * cap), "hipMalloc(proposals' distances)");
  HB_CHECK(b.flag.alloc(kHostMaxChunks), "hipHostMalloc(chunk flags)");
  for (int i = 0; i < kHostMaxChunks; ++i) b.flag.host()[i] = 0ull;
  HB_CHECK(b.done.alloc(kHostMaxChunks), "hipMalloc(chunk counters)");
  HB_CHECK(hipMemsetAsync(b.done.get(), 0, kHostMaxChunks * sizeof(unsigned int), stream_), "hipMemset");
  HB_CHECK(b.acc.alloc(1), "hipMalloc(host accept counter)");
  HB_CHECK(hipMemsetAsync(b.acc.get(), 0, sizeof(unsigned long long), stream_), "hipMemset");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  host_.buf = std::move(b);
  host_.ids.reserve(cap); host_.where.reserve(cap);
  return 0;
}

// particles per chunk of a half batch of cnt: whole workgroups, at most kHostMaxChunks chunks, and not so small that the
// fixed cost of one callback (a ctypes / ccall transition, ~10-50 us from Python) shows: >= 4096 unless asked otherwise
int64_t HipBackend::host_chunk_size(int64_t cnt) const {
  int64_t chunk = host_.chunk;
  if (chunk <= 0) {
    int64_t pieces = cnt / 4096;                         // automatic: equal pieces of >= 4096, at most 8
    pieces = pieces < 1 ? 1 : (pieces > 8 ? 8 : pieces);
    chunk = (cnt + pieces - 1) / pieces;
  }
  const int64_t least = (cnt + kHostMaxChunks - 1) / kHostMaxChunks;
  if (chunk < least) chunk = least;
  chunk = ((chunk + kBlock - 1) / kBlock) * kBlock;
  return chunk;
}

int HipBackend::wait_host_flag(int ch, unsigned long long seq) {
  volatile unsigned long long *f = host_.buf.flag.host() + ch;
  for (uint64_t spins = 1; *f != seq; ++spins) {
    __builtin_ia32_pause();
    if ((spins & 0x3FFF) == 0) {
      const hipError_t q = hipStreamQuery(stream_);
      if (q == hipSuccess) {
        if (*f == seq) break;
        err_ = "the proposal kernel did not signal a chunk although the stream is idle";
        return -1;
      }
      if (q != hipErrorNotReady) return check(q, "hipStreamQuery");
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return 0;
}

int HipBackend::host_prior_simulate() {
  const bool device_sim = m_.model_id != SABC_MODEL_HOST;
  if (!device_sim && !host_.fn) { err_ = "no host simulator set (sabc_set_host_simulator)"; return -1; }
  if (ensure_host_buffers()) return -1;
  const int d = m_.d, s = m_.s;
  const int64_t n = sh_.n_local;
  // the staging arrays double as theta [d][n] / rho [s][n] here (one-time, synchronous: n simulations on the host follow)
  double *th = host_.buf.thp.host(), *rho = host_.buf.rho.host();
  host_.ids.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) host_.ids[(size_t)i] = sh_.gid0 + i;
  const size_t w = (size_t)n * sizeof(double), pitch = (size_t)sh_.cap * sizeof(double);
  if (m_.prior_joint == 2) {                            // rand(prior) on the host (:174), theta uploaded
    if (!host_.prior_sample_fn) { err_ = "no host prior set (sabc_set_host_prior)"; return -1; }
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = n > 0 ? host_.prior_sample_fn(host_.prior_ctx, n, host_.ids.data(), th) : 0;
    host_.cb_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc) { err_ = "the host prior's sample callback failed"; return -1; }
    if (n > 0) HB_CHECK(hipMemcpy2DAsync(pop_[cur_].get(), pitch, th, w, w, (size_t)d, hipMemcpyHostToDevice, stream_), "upload theta");
    if (device_sim) {
      // f_dist on the device (:175), the streams of the fused initialisation kernel (particle id, iteration 0); the pinned
      // staging array is mapped into the device: the simulator reads theta [d][n] straight from it
      if (n > 0) {
        HB_LAUNCH(launch_simulate_batch(m_, host_.buf.thp.dev(), n, (uint64_t)sh_.gid0, 0, host_.buf.dev_rho_prop.get(), stream_, rtc()), "k_simulate_batch");
        HB_CHECK(hipMemcpy2DAsync(rho_.get(), pitch, host_.buf.dev_rho_prop.get(), w, w, (size_t)s, hipMemcpyDeviceToDevice, stream_), "rho");
      }
      HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
      return 0;
    }
  } else {
    HB_LAUNCH(launch_host_prior(m_, pop_ptrs(cur_), stream_), "k_host_prior");
    if (n > 0) HB_CHECK(hipMemcpy2DAsync(th, w, pop_[cur_].get(), pitch, w, (size_t)d, hipMemcpyDeviceToHost, stream_), "download theta");
  }
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  for (int64_t i = 0; i < (int64_t)s * n; ++i) rho[i] = 0.0;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = n > 0 ? host_.fn(host_.ctx, th, host_.ids.data(), n, 0, rho) : 0;
  host_.cb_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  host_.cb_calls += 1;
  if (rc) { err_ = "the host simulator (f_dist) failed"; return -1; }
  if (n > 0) HB_CHECK(hipMemcpy2DAsync(rho_.get(), pitch, rho, w, w, (size_t)s, hipMemcpyHostToDevice, stream_), "upload rho");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  return 0;
}

int HipBackend::host_update_range(const StepArgs &c, const PartnerView &pv, int64_t lo, int64_t cnt) {
  const bool device_sim = m_.model_id != SABC_MODEL_HOST;
  if (!device_sim && !host_.fn) { err_ = "no host simulator set (sabc_set_host_simulator)"; return -1; }
  if (lo < 0 || cnt < 0 || lo + cnt > sh_.n_local) { err_ = "host_update_range: range outside the shard"; return -1; }
  if (cnt == 0) return 0;
  if (ensure_host_buffers()) return -1;
  const int d = m_.d, s = m_.s;
  const bool host_prior = m_.prior_joint == 2;
  if (host_prior && !host_.prior_logpdf_fn) { err_ = "no host prior set (sabc_set_host_prior)"; return -1; }
  const int64_t chunk = device_sim ? ((cnt + kBlock - 1) / kBlock) * kBlock : host_chunk_size(cnt);
  const int n_chunks = (int)((cnt + chunk - 1) / chunk);
  const unsigned long long seq = ++host_.seq;
  // ONE launch proposes the whole half batch (:311-314); it signals its chunks as they complete
  HB_LAUNCH(launch_host_propose(m_, c, cb_dev_.get(), pop_ptrs(cur_), pv, lo, cnt, host_.buf.dev_thp.get(), host_.buf.dev_aux.get(), host_.buf.thp.dev(), host_.buf.gate.dev(),
                                host_prior ? host_.buf.cur.dev() : nullptr, host_.buf.done.get(), host_.buf.flag.dev(), seq, chunk, stream_),
            "k_host_propose");
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int64_t t0 = (int64_t)ch * chunk, tn = (t0 + chunk < cnt ? t0 + chunk : cnt) - t0;
    if (wait_host_flag(ch, seq)) return -1;
    if (host_prior) {
      // logpdf(prior, .) on the host (:314, :318): one call for the chunk's proposals followed by its current particles
      host_.both.resize((size_t)(2 * tn * d));
      host_.lp.assign((size_t)(2 * tn), -INFINITY);
      for (int k = 0; k < d; ++k)
        for (int64_t t = 0; t < tn; ++t) {
          host_.both[(size_t)(k * 2 * tn + t)] = host_.buf.thp.host()[(size_t)(k * cnt + t0 + t)];
          host_.both[(size_t)(k * 2 * tn + tn + t)] = host_.buf.cur.host()[(size_t)(k * cnt + t0 + t)];
        }
      const auto c0 = std::chrono::steady_clock::now();
      const int rc = host_.prior_logpdf_fn(host_.prior_ctx, 2 * tn, host_.both.data(), host_.lp.data());
      host_.cb_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
      if (rc) { err_ = "the host prior's logpdf callback failed"; return -1; }
      for (int64_t t = 0; t < tn; ++t) {
        const double l = host_.lp[(size_t)t];
        host_.buf.lp2.host()[(size_t)(t0 + t)] = l == l ? l : -INFINITY;             // NaN: outside the support
        host_.buf.lp2.host()[(size_t)(cnt + t0 + t)] = host_.lp[(size_t)(tn + t)];
        host_.buf.gate.host()[(size_t)(t0 + t)] = host_.buf.lp2.host()[(size_t)(t0 + t)] > -INFINITY ? 1 : 0;
      }
    }
    if (device_sim) {
      // the simulator on the device, over the proposals the host's gate bytes let through (mapped memory: read in place)
      prof_begin(SABC_KERNEL_UPDATE);
      HB_LAUNCH(launch_simulate_batch(m_, host_.buf.dev_thp.get(), cnt, (uint64_t)(sh_.gid0 + lo), c.iter, host_.buf.dev_rho_prop.get(), stream_, rtc(), host_.buf.gate.dev()),
                "k_simulate_batch");
      HB_LAUNCH(launch_host_accept(m_, c, cb_dev_.get(), pop_ptrs(cur_), cdf_ptrs(), lo, cnt, 0, cnt, host_.buf.dev_thp.get(), host_.buf.dev_aux.get(), host_.buf.dev_rho_prop.get(),
                                   host_.buf.lp2.dev(), host_.buf.acc.get(), stream_), "k_host_accept");
      prof_end(SABC_KERNEL_UPDATE);
      return 0;      // (nothing to wait for: the next half batch's proposal kernel is ordered behind these on the stream)
    }
    // only proposals inside the prior's support are simulated (:314-315): compact them for the callback
    host_.ids.resize((size_t)tn); host_.where.resize((size_t)tn);
    int64_t mv = 0;
    {
      const unsigned char *gate = host_.buf.gate.host() + t0;
      int64_t *ids = host_.ids.data(), *where = host_.where.data();
      const int64_t gid_first = sh_.gid0 + lo + t0;
      for (int64_t t = 0; t < tn; ++t)
        if (gate[t]) { ids[mv] = gid_first + t; where[mv] = t0 + t; ++mv; }
    }
    // every proposal of the chunk passed and the chunk's rows are contiguous (one parameter / statistic, or the chunk is the
    // whole half batch): f_dist reads the proposals and writes the distances IN the staging arrays, nothing is copied
    const bool direct = mv == tn && (d == 1 || tn == cnt) && (s == 1 || tn == cnt);
    const double *th_arg = host_.buf.thp.host() + t0;
    double *rho_arg = host_.buf.rho.host() + t0;
    if (!direct) {
      host_.thv.resize((size_t)(d * mv)); host_.rhov.assign((size_t)(s * mv), 0.0);
      for (int k = 0; k < d; ++k) {
        const double *src = host_.buf.thp.host() + (size_t)k * cnt;
        double *dst = host_.thv.data() + (size_t)k * mv;
        for (int64_t i = 0; i < mv; ++i) dst[i] = src[host_.where[(size_t)i]];
      }
      th_arg = host_.thv.data(); rho_arg = host_.rhov.data();
    }
    if (mv > 0) {
      const auto c0 = std::chrono::steady_clock::now();
      const int rc = host_.fn(host_.ctx, th_arg, host_.ids.data(), mv, c.iter, rho_arg);
      host_.cb_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
      host_.cb_calls += 1;
      if (rc) { err_ = "the host simulator (f_dist) failed"; return -1; }
    }
    if (!direct)
      for (int j = 0; j < s; ++j) {
        double *dst = host_.buf.rho.host() + (size_t)j * cnt;
        for (int64_t t = 0; t < tn; ++t) dst[t0 + t] = 0.0;
        const double *src = host_.rhov.data() + (size_t)j * mv;
        for (int64_t i = 0; i < mv; ++i) dst[host_.where[(size_t)i]] = src[i];
      }
    // the accept step of this chunk (:316-329) reads the distances in place; it runs while the host is in the next
    // chunk's callback.  (The launch orders the host's stores above before the kernel's loads.)
    if (ch == 0) prof_begin(SABC_KERNEL_UPDATE);
    HB_LAUNCH(launch_host_accept(m_, c, cb_dev_.get(), pop_ptrs(cur_), cdf_ptrs(), lo, cnt, t0, tn, host_.buf.dev_thp.get(), host_.buf.dev_aux.get(), host_.buf.rho.dev(),
                                 host_prior ? host_.buf.lp2.dev() : nullptr, host_.buf.acc.get(), stream_), "k_host_accept");
    if (ch == n_chunks - 1) prof_end(SABC_KERNEL_UPDATE);
  }
  return 0;
}

int HipBackend::host_stats(int64_t *rows_out) {
  if (ensure_host_buffers()) return -1;
  HB_LAUNCH(launch_stats_rt(m_, cb_dev_.get(), pop_ptrs(cur_), partials_.get(), host_.buf.acc.get(), stream_), "k_stats_rt");
  *rows_out = n_blocks(sh_.n_local);
  return 0;
}

}  // namespace sabc
