// hip_backend.hip -- HipBackend: owns the shard in HBM and launches the gfx950 kernels.
#include "hip_backend_internal.hpp"

#include <atomic>
#include <cmath>
#include <string>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace sabc {

namespace {
std::atomic<int64_t> g_parked_bytes{0};       // device memory kept because a peer had not released it when its owner went away
}

static double persist_timeout_ms() {                 // (read per launch: tests change it)
  const char *e = std::getenv("SABC_PERSISTENT_TIMEOUT_MS");
  const double v = e ? std::atof(e) : 0.0;
  return v > 0 ? v : 2000.0;
}

// Streams of closed handles are kept for the next handle on the same device: creating one costs ~0.4 ms, destroying one as much
// -- a tenth of a whole sabc() call at the sizes the reference's documentation works with (17 ms for n_particles = 1000,
// n_simulation = 1e6).  A stream goes back only after it has drained; streams the caller supplied (sabc_set_stream) are never
// pooled.  (The pool is never torn down: at process exit the runtime may already be gone.)
namespace {
std::mutex g_stream_pool_mutex;
std::vector<std::pair<int, hipStream_t>> *g_stream_pool = nullptr;       // (device, idle stream)
constexpr size_t kStreamPoolMax = 32;

hipStream_t pooled_stream_take(int device) {
  std::lock_guard<std::mutex> lock(g_stream_pool_mutex);
  if (!g_stream_pool) return nullptr;
  for (size_t i = 0; i < g_stream_pool->size(); ++i)
    if ((*g_stream_pool)[i].first == device) {
      hipStream_t s = (*g_stream_pool)[i].second;
      g_stream_pool->erase(g_stream_pool->begin() + (long)i);
      return s;
    }
  return nullptr;
}
void pooled_stream_give(int device, hipStream_t s) {
  if (hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamDestroy(s); return; }
  std::lock_guard<std::mutex> lock(g_stream_pool_mutex);
  if (!g_stream_pool) g_stream_pool = new std::vector<std::pair<int, hipStream_t>>();
  if (g_stream_pool->size() >= kStreamPoolMax) { (void)hipStreamDestroy(s); return; }
  g_stream_pool->emplace_back(device, s);
}
}  // namespace

static double persist_rendezvous_ms() {              // (the wait for every workgroup of a one-launch update to be resident)
  const char *e = std::getenv("SABC_PERSISTENT_RENDEZVOUS_MS");
  const double v = e ? std::atof(e) : 0.0;
  return v > 0 ? v : 20.0;
}

HipBackend::HipBackend(int device) : device_(device) {
  // shards up to this many particles run the population updates of a call in ONE launch (kernels.hip: k_update_persistent);
  // SABC_PERSISTENT=0 (or SABC_PERSISTENT_MAX=0) keeps the launch chain per update at every size
  if (const char *e = std::getenv("SABC_PERSISTENT_MAX")) persist_.max = std::atoll(e);
  if (const char *e = std::getenv("SABC_PERSISTENT")) { if (e[0] == '0') persist_.max = 0; }
  // (tests lower the limit to reach the two-launch form -- k_reduce_partials, then the control / exchange launch -- at small n)
  if (const char *e = std::getenv("SABC_FUSE_REDUCE_MAX")) {
    const long long v = std::atoll(e);
    if (v >= 0) fuse_reduce_max_ = v;
  }
}

// hipFree waits for EVERY stream of the process.  With several shards in one process (tests; a Julia host driving the GPUs
// of a node from threads) a peer's kernel may be spinning for this shard's next post, which the host cannot enqueue while
// it sits in hipFree: nothing is freed inside a call.  end_of_call() runs after the call's last exchange.
void HipBackend::free_later(void *p) {
  if (p) deferred_free_.push_back(p);
}

void HipBackend::end_of_call() {
  for (void *p : deferred_free_) (void)hipFree(p);
  deferred_free_.clear();
}

HipBackend::~HipBackend() {
  if (!stream_ && !pop_[0].get()) return;                // never allocated (e.g. create failed on a bad device ordinal)
  (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize(stream_);
  // the peer-to-peer group first (p2p.hpp "LEAVES"): what peers may have mapped -- both population buffers, rho, the slot
  // area -- is freed only when every one of them has recorded that it unmapped it; otherwise it is parked until the process
  // exits: a late reader meets stale particles, never an unmapped page
  if (!p2p_finish()) {
    g_parked_bytes += (int64_t)((pop_[0].count() + pop_[1].count() + rho_.count()) * sizeof(double) + p2p_.slots.count() * 8);
    (void)pop_[0].release(); (void)pop_[1].release(); (void)rho_.release(); (void)p2p_.slots.release();
  }
  end_of_call();
  for (auto &v : ev_)
    for (auto &e : v) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (auto &e : ev_pool_) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  // the members go in reverse order of declaration (hip_backend.hpp), device_ still current: every buffer, then the run-time
  // compiled kernels, and last of all the stream goes back to the pool
}

HipBackend::StreamReturn::~StreamReturn() {
  if (be->own_stream_ && be->stream_) pooled_stream_give(be->device_, be->stream_);
}

int HipBackend::check(hipError_t e, const char *what) {
  if (e == hipSuccess) return 0;
  char buf[256];
  std::snprintf(buf, sizeof(buf), "HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
  err_ = buf;
  return -1;
}

int HipBackend::set_stream(hipStream_t s) {
  HB_CHECK(hipSetDevice(device_), "hipSetDevice");
  if (stream_) HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  if (own_stream_ && stream_) pooled_stream_give(device_, stream_);
  stream_ = s;
  own_stream_ = false;
  return 0;
}

PopPtrs HipBackend::pop_ptrs(int which) const {
  PopPtrs pp;
  pp.pop = pop_[which].get();
  pp.rho = rho_.get();
  pp.cap = sh_.cap;
  pp.n_local = sh_.n_local;
  pp.gid0 = sh_.gid0;
  return pp;
}

CdfPtrs HipBackend::cdf_ptrs() const {
  CdfPtrs c;
  c.knots = knots_.get();
  c.stride = knot_stride_;
  c.coarse = coarse_.get();
  c.mid = mid_.get();
  c.mid_stride = mid_stride_;
  for (int j = 0; j < kMaxStats; ++j) { c.len[j] = cdf_len_[j]; c.shift[j] = cdf_shift_[j]; }
  return c;
}

int HipBackend::allocate(const ModelDesc &m, const Shard &sh) {
  m_ = m;
  sh_ = sh;
  np_ = n_partials(m.d, m.s);
  HB_CHECK(hipSetDevice(device_), "hipSetDevice");
  if (!stream_) {
    stream_ = pooled_stream_take(device_);
    if (!stream_) HB_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    own_stream_ = true;
  }
  const size_t cap = (size_t)sh.cap, N = (size_t)sh.n_global;
  const size_t rows = (size_t)(m.d + m.s + 1);
  // What peers read over the peer-to-peer transport (p2p.hpp): both population buffers and rho.  On a sharded handle they
  // live in FINE-GRAINED device memory -- coherent across devices at every access, so a peer's read never depends on what a
  // kernel boundary does to its caches.  On one GPU that costs nothing measurable (two processes sharing an MI355X, n = 1e6:
  // 5.48 / 4.99e9 sims/s RandomWalk / DE with plain hipMalloc, 5.49 / 5.03e9 fine-grained); what it
  // costs a REMOTE reader is unmeasured, its reads (partners, drawn rows: random; the weight rows: once) have little reuse to
  // lose.  SABC_P2P_FINEGRAINED=0 goes back to plain device memory, visible across devices at kernel boundaries only;
  // either way sabc_comm_p2p_selftest checks on first contact that peers read what the owners' kernels wrote.
  static const bool fine = [] { const char *e = std::getenv("SABC_P2P_FINEGRAINED"); return !(e && e[0] == '0'); }();
  const unsigned pop_flags = fine && sh.world > 1 ? hipDeviceMallocFinegrained : 0;
  for (int b = 0; b < 2; ++b) {
    HB_CHECK(pop_[b].alloc(rows * cap, pop_flags), "hipMalloc(pop)");
    HB_CHECK(hipMemsetAsync(pop_[b].get(), 0, rows * cap * sizeof(double), stream_), "hipMemset(pop)");
  }
  HB_CHECK(rho_.alloc((size_t)m.s * cap, pop_flags), "hipMalloc(rho)");
  HB_CHECK(hipMemsetAsync(rho_.get(), 0, (size_t)m.s * cap * sizeof(double), stream_), "hipMemset(rho)");
  HB_CHECK(coarse_.alloc((size_t)m.s * cdf_coarse_entries(m.s)), "hipMalloc(coarse)");
  // every table starts on a 128-byte line, and a whole line of +inf stays behind the longest one (N + 2 knots): the searches
  // read up to 15 knots past a table's last knot, which must never be the next statistic's first knots or past the allocation
  knot_stride_ = (((int64_t)N + 2 + 15) / 16) * 16 + 16;
  HB_CHECK(knots_.alloc((size_t)m.s * (size_t)knot_stride_), "hipMalloc(knots)");
  mid_stride_ = cdf_mid_stride(knot_stride_);
  HB_CHECK(mid_.alloc((size_t)m.s * (size_t)mid_stride_), "hipMalloc(mid)");
  {   // k_update writes one row per workgroup; its granularity depends on the model's kernel
    const int64_t per_half = update_rows(m, (sh.cap + 1) / 2) + 1, whole = update_rows(m, sh.cap);
    partial_rows_ = 2 * per_half > whole ? 2 * per_half : whole;
    if (partial_rows_ < n_blocks(sh.cap)) partial_rows_ = n_blocks(sh.cap);
    // (k_update_persistent double-buffers one row per workgroup by the update's parity)
    if (2 * persistent_workgroups_bound(m, sh.cap) > partial_rows_) partial_rows_ = 2 * persistent_workgroups_bound(m, sh.cap);
    partial_rows_ += 4;
  }
  HB_CHECK(partials_.alloc((size_t)partial_rows_ * np_), "hipMalloc(partials)");
  HB_CHECK(cb_dev_.alloc(1), "hipMalloc(control block)");
  HB_CHECK(hipMemsetAsync(cb_dev_.get(), 0, sizeof(ControlBlock), stream_), "hipMemset(control block)");
  {   // ONE pinned block for the control block's staging copy, the mailbox ring and the totals (hipHostFree is 0.2 ms apiece)
    const size_t off_mbox = (sizeof(ControlBlock) + 255) / 256 * 256, off_totals = off_mbox + (kMailboxRing * sizeof(Mailbox) + 255) / 256 * 256;
    HB_CHECK(pinned_.alloc(off_totals + 256), "hipHostMalloc(control block, mailbox, totals)");
    cb_host_ = reinterpret_cast<ControlBlock *>(pinned_.host());
    mbox_host_ = reinterpret_cast<Mailbox *>(pinned_.host() + off_mbox);
    mbox_dev_ = reinterpret_cast<Mailbox *>(pinned_.dev() + off_mbox);
    totals_host_ = reinterpret_cast<double *>(pinned_.host() + off_totals);
    totals_host_dev_ = reinterpret_cast<double *>(pinned_.dev() + off_totals);
  }
  HB_CHECK(sums_stage_.alloc(kMaxPartials), "hipMalloc(sums staging)");
  HB_CHECK(hipMemsetAsync(sums_stage_.get(), 0, kMaxPartials * sizeof(double), stream_), "hipMemset(sums staging)");
  for (int i = 0; i < kMailboxRing; ++i) { mbox_host_[i].w0 = kMailboxEmpty; mbox_host_[i].w1 = kMailboxEmpty; }
  HB_CHECK(cum_.alloc(N), "hipMalloc(cum)");
  HB_CHECK(block_sums_.alloc((size_t)weight_scan_doubles((int64_t)N)), "hipMalloc(block_sums)");
  HB_CHECK(totals_dev_.alloc(2), "hipMalloc(totals)");
  totals_host_[0] = totals_host_[1] = 0.0;
  HB_CHECK(meta_dev_.alloc(2 * kMaxStats), "hipMalloc(meta)");
  int khz = 0;                                          // rate of the constant wall clock every bounded wait counts in
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_) == hipSuccess && khz > 0) wall_clock_khz_ = khz;
  else (void)hipGetLastError();
  return 0;
}

double *HipBackend::gather_buffer(int64_t doubles) {
  if (doubles > (int64_t)gather_.count() && grow(gather_, (size_t)doubles) != hipSuccess) return nullptr;
  return gather_.get();
}

double *HipBackend::scratch_buffer(int which, int64_t doubles) {
  if (which < 0 || which >= 4) return nullptr;
  // head room: the request count of a resample varies from one to the next
  if (doubles > (int64_t)scratch_[which].count() && grow(scratch_[which], (size_t)(doubles + doubles / 4 + 64)) != hipSuccess) return nullptr;
  return scratch_[which].get();
}

int HipBackend::copy_rows(const double *src, int64_t src_pitch, double *dst, int64_t dst_pitch, int rows, int64_t count) {
  if (rows <= 0 || count <= 0) return 0;
  HB_CHECK(hipMemcpy2DAsync(dst, (size_t)dst_pitch * sizeof(double), src, (size_t)src_pitch * sizeof(double),
                            (size_t)count * sizeof(double), (size_t)rows, hipMemcpyDeviceToDevice, stream_), "copy_rows");
  return 0;
}

int HipBackend::to_backend(double *dst, const double *src_host, int64_t n) {
  if (n <= 0) return 0;
  HB_CHECK(hipMemcpyAsync(dst, src_host, (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream_), "to_backend");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  return 0;
}

int HipBackend::to_host(double *dst_host, const double *src, int64_t n) {
  if (n <= 0) return 0;
  HB_CHECK(hipMemcpyAsync(dst_host, src, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream_), "to_host");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  return 0;
}

// level 1: bracket only the dominant kernel (k_update) -- every hipEventRecord is a marker packet the
// queue has to drain, ~4 us of GPU time each, so the other kernels are bracketed only at level 2
void HipBackend::profile_enable(int level) {
  prof_ = level;
  prof_tick_ = 0;
  if (level)
    for (int k = 0; k < SABC_KERNEL_COUNT; ++k) { prof_ms_[k] = 0.0; prof_n_[k] = 0; prof_noop_[k] = 0; }
  while (level && ev_pool_.size() < 256) {       // created outside the timed region
    EvPair e;
    if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) break;
    ev_pool_.push_back(e);
  }
}

void HipBackend::prof_begin(int kernel) {
  if (!prof_ || (prof_ < 2 && kernel != SABC_KERNEL_UPDATE)) return;
  EvPair e;
  if (!ev_pool_.empty()) { e = ev_pool_.back(); ev_pool_.pop_back(); }
  else if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
  (void)hipEventRecord(e.a, stream_);
  ev_[kernel].push_back(e);
  prof_open_ = kernel;
}

void HipBackend::prof_end(int kernel) {
  if (prof_open_ != kernel || ev_[kernel].empty()) return;
  (void)hipEventRecord(ev_[kernel].back().b, stream_);
  prof_open_ = -1;
}

int HipBackend::profile_get(int kernel, double *total_ms, int64_t *launches) {
  if (kernel < 0 || kernel >= SABC_KERNEL_COUNT) return -1;
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  for (auto &e : ev_[kernel]) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
      // an update launch queued ahead of a resample test that fired returns at `if (cb->halt)`: not a sample of the kernel
      if (kernel == SABC_KERNEL_UPDATE && ms < 0.004f && sh_.n_local >= 4096) prof_noop_[kernel] += 1;
      else { prof_ms_[kernel] += ms; prof_n_[kernel] += 1; }
    }
    ev_pool_.push_back(e);
  }
  ev_[kernel].clear();
  if (total_ms) *total_ms = prof_ms_[kernel];
  if (launches) *launches = prof_n_[kernel];
  return 0;
}

int HipBackend::register_device_simulator(const char *hip_source, int chain_lanes) {
  if (m_.model_id != SABC_MODEL_USER) { err_ = "the handle was not created with SABC_MODEL_USER"; return -1; }
  const bool team_aware = chain_lanes != 0;
  if (team_aware && chain_lanes != 1 && chain_lanes != 4 && chain_lanes != 16) { err_ = "chain_lanes of a team-aware simulator is 1, 4 or 16"; return -1; }
  if (team_aware && source_wide(m_.s)) {
    err_ = "a team-aware simulator (sabc_user_simulate_team<W>) has no wide form: n_stats <= 16 (the kernels for 16 < n_stats <= 64 run a lane per particle)";
    return -1;
  }
  HB_CHECK(hipSetDevice(device_), "hipSetDevice");
  if (stream_) HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  rtc_release(&rtc_);
  std::string log;
  // (the one-launch form of small shards -- k_update_persistent -- is compiled only for handles that can take it)
  const bool small = persist_.max > 0 && sh_.world == 1 && sh_.n_local <= persist_.max && persistent_fits(m_.d, m_.s);
  RtcRequest rq{hip_source, m_.d, m_.s, rtc_default_csrc_dir(), /*user_prior=*/m_.prior_joint == 3, /*with_persistent=*/small, team_aware};
  if (rtc_compile(rq, &rtc_, &log)) {
    // the one-launch kernels are the largest of the unit (three team widths x three proposals): should the compiler give up on
    // them for this simulator, the launch chain alone still runs it -- only a source that fails there too is an error
    std::string log_chain;
    rq.with_persistent = false;
    if (!small || rtc_compile(rq, &rtc_, &log_chain)) {
      err_ = "compiling the device simulator failed:\n" + log;
      return -1;
    }
  }
  rtc_.chain_lanes = team_aware ? chain_lanes : 1;
  return push_data_desc();                                // a new module starts with an empty descriptor: the data are kept
}

static_assert(SABC_MAX_DATA_SEGMENTS == 8, "RtcDataDesc and the preamble of rtc.cpp hold 8 segments");

int HipBackend::push_data_desc() {
  if (!rtc()) return 0;                                   // no module yet: register_device_simulator writes it after the load
  hipDeviceptr_t sym = nullptr;
  size_t bytes = 0;
  HB_CHECK(hipModuleGetGlobal(&sym, &bytes, rtc_.module, rtc_data_symbol()), "hipModuleGetGlobal(sabc_data_desc)");
  if (bytes != sizeof(RtcDataDesc)) { err_ = "sabc_data_desc of the compiled simulator has another layout than this library's"; return -1; }
  HB_CHECK(hipMemcpyAsync(sym, &data_desc_, sizeof(RtcDataDesc), hipMemcpyHostToDevice, stream_), "hipMemcpy(sabc_data_desc)");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  return 0;
}

int HipBackend::set_device_data(const double *values, int64_t n, const int64_t *segment_len, int32_t n_segments) {
  if (m_.model_id != SABC_MODEL_USER) { err_ = "observed data are read by a simulator from source: the handle was not created with SABC_MODEL_USER"; return SABC_ERR_BAD_CONFIG; }
  if (n < 0 || n_segments < 0 || n_segments > SABC_MAX_DATA_SEGMENTS) { err_ = "sabc_set_device_data: n >= 0 and at most 8 segments"; return SABC_ERR_BAD_CONFIG; }
  if (n > 0 && (!values || !segment_len)) { err_ = "sabc_set_device_data: null argument"; return SABC_ERR_BAD_CONFIG; }
  RtcDataDesc desc;
  int64_t sum = 0;
  for (int k = 0; k < n_segments && n > 0; ++k) {
    if (segment_len[k] < 0 || segment_len[k] > n) { err_ = "sabc_set_device_data: a segment length is negative or larger than n"; return SABC_ERR_BAD_CONFIG; }
    desc.off[k] = sum;
    desc.len[k] = segment_len[k];
    sum += segment_len[k];
  }
  if (sum != n) { err_ = "sabc_set_device_data: the segment lengths do not sum to n"; return SABC_ERR_BAD_CONFIG; }
  if (check(hipSetDevice(device_), "hipSetDevice")) return SABC_ERR_HIP;
  // the host queues updates ahead: nothing of this handle may still be reading the old data or the old descriptor
  if (stream_ && check(hipStreamSynchronize(stream_), "hipStreamSynchronize")) return SABC_ERR_HIP;
  const size_t bytes = (size_t)n * sizeof(double);
  if ((size_t)n != data_.count()) {
    DeviceBuffer<double> fresh;
    if (n > 0 && check(fresh.alloc((size_t)n), "hipMalloc(observed data)")) return SABC_ERR_HIP;
    if (n > 0 && check(hipMemcpy(fresh.get(), values, bytes, hipMemcpyHostToDevice), "hipMemcpy(observed data)")) return SABC_ERR_HIP;
    data_ = std::move(fresh);                             // (the handle is idle: the old allocation is freed here)
  } else if (n > 0) {                                     // the same length again: the allocation is reused
    if (check(hipMemcpy(data_.get(), values, bytes, hipMemcpyHostToDevice), "hipMemcpy(observed data)")) return SABC_ERR_HIP;
  }
  desc.base = data_.get();
  desc.n_segments = n > 0 ? n_segments : 0;
  data_desc_ = desc;
  return push_data_desc() ? SABC_ERR_HIP : 0;
}

int HipBackend::prior_simulate() {
  if (m_.model_id == SABC_MODEL_USER && !rtc()) { err_ = "no device simulator registered (sabc_register_device_simulator)"; return -1; }
  prof_begin(SABC_KERNEL_INIT);
  HB_LAUNCH(launch_prior_simulate(m_, pop_ptrs(cur_), stream_, rtc()), "k_prior_simulate");
  prof_end(SABC_KERNEL_INIT);
  return 0;
}

int HipBackend::build_cdf(const double *gathered_rho, int64_t *len_out, int *any_negative) {
  return build_cdf_blocks(flat_blocks(gathered_rho, m_.s, sh_.cap, sh_.world), len_out, any_negative);
}

int HipBackend::build_cdf_blocks(const ShardBlocks &rho_blocks, int64_t *len_out, int *any_negative) {
  const int64_t N = sh_.n_global;
  if (!col_a_.get()) {
    HB_CHECK(col_a_.alloc((size_t)N), "hipMalloc(col_a)");
    HB_CHECK(col_b_.alloc((size_t)N), "hipMalloc(col_b)");
    size_t bytes = 0;
    HB_LAUNCH(sort_f64(col_a_.get(), col_b_.get(), N, nullptr, &bytes, stream_), "radix sort size query");
    sort_tmp_bytes_ = bytes ? bytes : 16;
    HB_CHECK(sort_tmp_.alloc(sort_tmp_bytes_), "hipMalloc(sort_tmp)");
  }
  for (int j = 0; j < m_.s; ++j) {
    HB_LAUNCH(launch_compact_column(rho_blocks, j, N, col_a_.get(), stream_), "k_compact_column");
    size_t bytes = sort_tmp_bytes_;
    HB_LAUNCH(sort_f64(col_a_.get(), col_b_.get(), N, sort_tmp_.get(), &bytes, stream_), "radix sort");
    launches_ += 31;                                   // 8 passes of 4 kernels
    HB_LAUNCH(launch_cdf_knots(col_b_.get(), N, knots_.get() + (int64_t)j * knot_stride_, meta_dev_.get() + 2 * j, stream_), "k_cdf_knots");
    launches_ += 1;
  }
  int64_t meta[2 * kMaxStats];
  HB_CHECK(hipMemcpyAsync(meta, meta_dev_.get(), 2 * (size_t)m_.s * sizeof(int64_t), hipMemcpyDeviceToHost, stream_), "memcpy(meta)");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  *any_negative = 0;
  for (int j = 0; j < m_.s; ++j) {
    const int64_t mpos = N - meta[2 * j];
    cdf_len_[j] = mpos > 0 ? mpos + 2 : 0;
    len_out[j] = cdf_len_[j];
    if (meta[2 * j + 1]) *any_negative = 1;
    if (cdf_len_[j] > 0 && build_coarse(j)) return -1;
  }
  // the sort scratch is only needed once per result
  free_later(col_a_.release()); free_later(col_b_.release()); free_later(sort_tmp_.release());
  return 0;
}

int HipBackend::cdf_population() {
  HB_LAUNCH(launch_cdf_population(m_, pop_ptrs(cur_), cdf_ptrs(), stream_), "k_cdf_population");
  return 0;
}

int HipBackend::update_range(const StepArgs &c, const PartnerView &pv, int64_t lo, int64_t cnt, int64_t row0,
                             int64_t *rows_out) {
  const int64_t rows = update_rows(m_, cnt);
  if (lo < 0 || cnt < 0 || lo + cnt > sh_.n_local || row0 + rows > partial_rows_) {
    err_ = "update_range: range outside the shard";
    return -1;
  }
  // the timing events ride on the kernel's own dispatch packet (no marker packets around it)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // level 1 times every SECOND launch of the update kernel (a timed dispatch packet costs ~4 us of queue time: sampling
  // halves what the measurement adds to the step); levels 2 and 3 time every launch
  if (prof_ && (prof_ != 1 || (prof_tick_++ & 1) == 0)) {
    EvPair e{nullptr, nullptr};
    if (!ev_pool_.empty()) { e = ev_pool_.back(); ev_pool_.pop_back(); }
    else if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) e = EvPair{nullptr, nullptr};
    if (e.a && e.b) { ev_[SABC_KERNEL_UPDATE].push_back(e); ev0 = e.a; ev1 = e.b; }
  }
  HB_LAUNCH(launch_update(m_, c, cb_dev_.get(), pop_ptrs(cur_), cdf_ptrs(), pv, lo, cnt, partials_.get(), row0, stream_, ev0, ev1, rtc()), "k_update");
  *rows_out = rows;
  return 0;
}

// Small shards: the updates of a call in one launch (persistent_kernel.hpp: k_update_persistent; for a simulator from source
// the run-time compiled instantiation).  Not under a profile level that wants every kernel bracketed (the launch chain is
// what such a run measures).
bool HipBackend::persistent_supported(int prop_kind) const {
  if (persist_.max <= 0 || sh_.world != 1 || sh_.n_local > persist_.max || prof_ >= 2) return false;
  const int64_t wg = persistent_workgroups(m_, prop_kind, sh_.n_local, rtc());
  return wg > 0 && 2 * wg <= partial_rows_;
}

int HipBackend::update_persistent(const StepArgs &c, const ControlArgs &ctrl, const PartnerView &pv_a, const PartnerView &pv_b, int64_t ix0,
                                  int64_t phase, int64_t cph, int64_t count, int64_t *done, int *halted, int *error) {
  if (pending_rows_ >= 0 && flush_reduce()) return -1;
  if (!persist_.sync.get()) HB_CHECK(persist_.sync.alloc(4), "hipMalloc(grid barrier)");
  HB_CHECK(hipMemsetAsync(persist_.sync.get(), 0, 4 * sizeof(unsigned long long), stream_), "hipMemset(grid barrier)");
  PersistArgs pa;
  std::memset(&pa, 0, sizeof(pa));
  pa.iter0 = c.iter;
  pa.ix0 = ix0; pa.phase = phase; pa.cph = cph;
  pa.act_n = sh_.n_local; pa.half = sh_.n_local / 2;
  pa.count = (int32_t)(count > (int64_t)1 << 30 ? (int64_t)1 << 30 : count);
  pa.prop_p0 = c.prop_p0; pa.prop_p1 = c.prop_p1;
  pa.ctrl = ctrl;
  pa.sync = persist_.sync.get();
  pa.timeout_ticks = (uint64_t)(persist_timeout_ms() * (double)wall_clock_khz_);
  pa.rendezvous_ticks = (uint64_t)(persist_rendezvous_ms() * (double)wall_clock_khz_);
  if (const char *e = std::getenv("SABC_PERSISTENT_TEST_ABSENT_WG")) pa.test_absent_wg = std::atoi(e);     // (tests/test_persistent.py)
  const int64_t wg = persistent_workgroups(m_, c.prop_kind, pa.act_n, rtc(), &persist_.lanes);
  if (wg <= 0) return check(hipErrorInvalidValue, "k_update_persistent: no one-launch form for this shard");
  // the rows travel as tagged words (two per value, two parities), zeroed before every launch: its tags start at 1
  const size_t row_words = (size_t)np_ * 2, row_bytes = row_words * sizeof(unsigned long long);
  if (persist_.rows_wg < wg) {
    const int64_t bound = persistent_workgroups_bound(m_, sh_.cap) > wg ? persistent_workgroups_bound(m_, sh_.cap) : wg;
    persist_.rows_wg = 0;
    HB_CHECK(grow(persist_.rows, 2 * (size_t)bound * row_words), "hipMalloc(partial rows of the one-launch form)");
    persist_.rows_wg = bound;
  }
  HB_CHECK(hipMemsetAsync(persist_.rows.get(), 0, 2 * (size_t)wg * row_bytes, stream_), "hipMemset(partial rows of the one-launch form)");
  prof_begin(SABC_KERNEL_UPDATE);
  HB_LAUNCH(launch_update_persistent(m_, c.prop_kind, pa, cb_dev_.get(), pop_ptrs(cur_), cdf_ptrs(), pv_a, pv_b, reinterpret_cast<double *>(persist_.rows.get()),
                                     hist_dev_.get(), mbox_dev_, sums_stage_.get(), stream_, rtc()), "k_update_persistent");
  prof_end(SABC_KERNEL_UPDATE);
  ControlBlock cb;
  if (read_control(&cb)) return -1;
  *done = cb.persist_done;
  *halted = cb.halt;
  *error = cb.error;
  return 0;
}

int HipBackend::stats(int64_t *rows_out) {
  HB_LAUNCH(launch_stats(m_, cb_dev_.get(), pop_ptrs(cur_), partials_.get(), stream_, rtc()), "k_stats");
  *rows_out = n_blocks(sh_.n_local);
  return 0;
}

// The reduction is deferred: if the next thing is the control step (one shard: no allreduce in
// between), both run as one launch (k_reduce_control); anything that needs the staged sums earlier
// (sums_buffer() for the allreduce) flushes it as its own kernel.
int HipBackend::reduce_partials(int64_t rows, bool guarded) {
  if (pending_rows_ >= 0 && flush_reduce()) return -1;
  pending_rows_ = rows;
  pending_guarded_ = guarded;
  return 0;
}

int HipBackend::flush_reduce() {
  if (pending_rows_ < 0) return 0;
  const int64_t rows = pending_rows_;
  pending_rows_ = -1;
  prof_begin(SABC_KERNEL_REDUCE);
  HB_LAUNCH(launch_reduce_partials(partials_.get(), rows, np_, sums_stage_.get(), pending_guarded_ ? &cb_dev_.get()->halt : nullptr, stream_),
            "k_reduce_partials");
  if (p2p_.pending_xchg) {          // somebody wants the GLOBAL sums in the staging buffer: the exchange without the control step
    p2p_.pending_xchg = false;
    ControlArgs none;
    std::memset(&none, 0, sizeof(none));
    none.mode = pending_guarded_ ? CTRL_GUARDED : 0;
    const P2PView pv = p2p_view();
    HB_LAUNCH(launch_reduce_control(partials_.get(), -1, np_, sums_stage_.get(), cb_dev_.get(), none, hist_dev_.get(), mbox_dev_, stream_, &pv,
                                    tag(++p2p_.xseq), /*do_control=*/false, take_silence()), "k_reduce_control (exchange)");
  }
  prof_end(SABC_KERNEL_REDUCE);
  return 0;
}

double *HipBackend::sums_buffer() {
  (void)flush_reduce();
  return sums_stage_.get();
}

int HipBackend::control(const ControlArgs &a) {
  const bool xchg = p2p_.pending_xchg && pending_rows_ >= 0;
  const P2PView pv = xchg ? p2p_view() : P2PView();
  if (pending_rows_ >= 0 && np_ <= 64 && pending_rows_ * np_ <= fuse_reduce_max_) {
    const int64_t rows = pending_rows_;
    pending_rows_ = -1;
    p2p_.pending_xchg = false;
    prof_begin(SABC_KERNEL_REDUCE);
    // several shards over the peer-to-peer slots: reduce -> exchange -> control step, ONE launch
    HB_LAUNCH(launch_reduce_control(partials_.get(), rows, np_, sums_stage_.get(), cb_dev_.get(), a, hist_dev_.get(), mbox_dev_, stream_,
                                    xchg ? &pv : nullptr, xchg ? tag(++p2p_.xseq) : 0, true, xchg ? take_silence() : 0),
              "k_reduce_control");
    prof_end(SABC_KERNEL_REDUCE);
    return 0;
  }
  if (xchg) {                   // a partial-row matrix too large for one workgroup: np workgroups reduce it first
    p2p_.pending_xchg = false;
    if (flush_reduce()) return -1;
    prof_begin(SABC_KERNEL_REDUCE);
    HB_LAUNCH(launch_reduce_control(partials_.get(), -1, np_, sums_stage_.get(), cb_dev_.get(), a, hist_dev_.get(), mbox_dev_, stream_, &pv,
                                    tag(++p2p_.xseq), true, take_silence()), "k_reduce_control (exchange)");
    prof_end(SABC_KERNEL_REDUCE);
    return 0;
  }
  if (flush_reduce()) return -1;
  HB_LAUNCH(launch_control(cb_dev_.get(), a, hist_dev_.get(), mbox_dev_, sums_stage_.get(), stream_), "k_control");
  return 0;
}

// Poll the mailbox.  A stream that has drained without the sequence word arriving means the
// control kernel never ran (a fault upstream): report instead of spinning forever.
int HipBackend::wait_notify(int64_t seq, int64_t *n_accept, int *error, int *halted) {
  Mailbox *mb = mbox_host_ + (seq % kMailboxRing);
  int32_t e = 0, hl = 0;
  for (uint64_t spins = 1;; ++spins) {
    if (mailbox_unpack(mb->w0, mb->w1, seq, n_accept, &e, &hl)) break;
    __builtin_ia32_pause();
    if ((spins & 0x3FFF) == 0) {
      const hipError_t q = hipStreamQuery(stream_);
      if (q == hipSuccess) {
        if (mailbox_unpack(mb->w0, mb->w1, seq, n_accept, &e, &hl)) break;
        err_ = "control step did not report back although the stream is idle";
        return -1;
      }
      if (q != hipErrorNotReady) return check(q, "hipStreamQuery");
    }
  }
  *error = (int)e;
  *halted = (int)hl;
  return 0;
}

int HipBackend::read_control(ControlBlock *out) {
  HB_CHECK(hipMemcpyAsync(cb_host_, cb_dev_.get(), sizeof(ControlBlock), hipMemcpyDeviceToHost, stream_), "memcpy(control block)");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  std::memcpy(out, cb_host_, sizeof(ControlBlock));
  return 0;
}

int HipBackend::write_control(const ControlBlock &in) {
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");     // the staging copy is reused
  std::memcpy(cb_host_, &in, sizeof(ControlBlock));
  HB_CHECK(hipMemcpyAsync(cb_dev_.get(), cb_host_, sizeof(ControlBlock), hipMemcpyHostToDevice, stream_), "memcpy(control block)");
  return 0;
}

int HipBackend::history_reserve(int64_t rows) {
  const int row_len = kMaxStats * 3;
  if (rows > hist_cap_) {
    // grow geometrically from 4096 rows (0.8 MB): a typical call never pays hipFree + hipMalloc inside update_population!
    int64_t cap = hist_cap_ > 0 ? 2 * hist_cap_ : 4096;
    if (cap < rows) cap = rows;
    HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    free_later(hist_dev_.release());
    HB_CHECK(hist_dev_.alloc((size_t)cap * row_len), "hipMalloc(history)");
    hist_cap_ = cap;
  }
  return 0;
}

int HipBackend::read_history(double *out, int64_t rows, int row_len) {
  if (rows > hist_cap_) { err_ = "read_history: more rows than reserved"; return -1; }
  HB_CHECK(hipMemcpyAsync(out, hist_dev_.get(), (size_t)rows * row_len * sizeof(double), hipMemcpyDeviceToHost, stream_), "memcpy(history)");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  return 0;
}

int HipBackend::resample_weights(double delta) {
  HB_LAUNCH(launch_resample_weights(m_, pop_ptrs(cur_), cb_dev_.get(), (double)sh_.n_global, delta, stream_), "k_resample_weights");
  return 0;
}

int HipBackend::resample_draw(const double *gathered_pop, uint64_t iter) {
  const int rows = m_.d + m_.s + 1;
  prof_begin(SABC_KERNEL_RESAMPLE);
  const ShardBlocks blocks = flat_blocks(gathered_pop, rows, sh_.cap, sh_.world);
  HB_LAUNCH(launch_weight_scan(blocks, sh_.n_global, block_sums_.get(), cum_.get(), totals_dev_.get(), totals_host_dev_, stream_), "weight scan");
  launches_ += 2;
  const int nxt = 1 - cur_;
  HB_LAUNCH(launch_resample_gather(m_, blocks, sh_.n_global, cum_.get(), block_sums_.get(), totals_dev_.get(), iter, pop_ptrs(nxt), stream_),
            "k_resample_gather");
  prof_end(SABC_KERNEL_RESAMPLE);
  flip_cur();
  return 0;
}

// one shard: the whole of :124-137 in four launches (kernels.hpp: launch_resample_local)
int HipBackend::resample_local(double delta, uint64_t iter, int64_t *stats_rows) {
  if (!pack_dev_.get()) {
    const int64_t doubles = resample_pack_doubles(m_.d + m_.s, sh_.cap > 0 ? sh_.cap : 1);
    if (doubles > 0) HB_CHECK(pack_dev_.alloc((size_t)doubles), "hipMalloc(packed resample lines)");
  }
  if (pending_rows_ >= 0 && flush_reduce()) return -1;      // the partial rows are about to be overwritten
  const int nxt = 1 - cur_;
  prof_begin(SABC_KERNEL_RESAMPLE);
  HB_LAUNCH(launch_resample_local(m_, pop_ptrs(cur_), pop_ptrs(nxt), cb_dev_.get(), delta, iter, block_sums_.get(), cum_.get(), totals_dev_.get(), totals_host_dev_,
                                  pack_dev_.get(), partials_.get(), stats_rows, stream_), "resample kernels");
  launches_ += 3;
  prof_end(SABC_KERNEL_RESAMPLE);
  flip_cur();
  return 0;
}

// ---- the sharded resample (engine.cpp: resample_exchange) -------------------------------------
int HipBackend::resample_select(const double *gathered_w, uint64_t iter) {
  if (!idx_dev_.get()) {
    const size_t cap = (size_t)(sh_.cap > 0 ? sh_.cap : 1);
    HB_CHECK(idx_dev_.alloc(cap), "hipMalloc(resample indices)");
    HB_CHECK(slot_dev_.alloc(cap), "hipMalloc(resample slots)");
    HB_CHECK(bucket_dev_.alloc(2 * (size_t)sh_.world), "hipMalloc(buckets)");
    HB_CHECK(bucket_host_.alloc(2 * (size_t)sh_.world), "hipHostMalloc(buckets)");
  }
  prof_begin(SABC_KERNEL_RESAMPLE);
  HB_LAUNCH(launch_weight_scan(flat_blocks(gathered_w, 1, sh_.cap, sh_.world), sh_.n_global, block_sums_.get(), cum_.get(), totals_dev_.get(), totals_host_dev_, stream_),
            "weight scan");
  launches_ += 2;
  HB_LAUNCH(launch_resample_select(m_, sh_.cap, sh_.n_global, cum_.get(), block_sums_.get(), totals_dev_.get(), iter, pop_ptrs(cur_), idx_dev_.get(), stream_),
            "k_resample_select");
  prof_end(SABC_KERNEL_RESAMPLE);
  return 0;
}

int HipBackend::resample_bucket(int64_t *counts_host, double *req_out) {
  const int W = sh_.world;
  const size_t bytes = (size_t)W * sizeof(unsigned long long);
  HB_CHECK(hipMemsetAsync(bucket_dev_.get(), 0, 2 * bytes, stream_), "hipMemset(buckets)");
  HB_LAUNCH(launch_bucket_count(idx_dev_.get(), sh_.n_local, sh_.cap, bucket_dev_.get(), stream_), "k_bucket_count");
  HB_CHECK(hipMemcpyAsync(bucket_host_.host(), bucket_dev_.get(), bytes, hipMemcpyDeviceToHost, stream_), "memcpy(bucket counts)");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  unsigned long long run = 0;
  for (int r = 0; r < W; ++r) {
    counts_host[r] = (int64_t)bucket_host_.host()[r];
    bucket_host_.host()[W + r] = run;                       // exclusive offsets = where each bucket's cursor starts
    run += bucket_host_.host()[r];
  }
  if ((int64_t)run != sh_.n_local) { err_ = "resample_bucket: the bucket counts do not add up to n_local"; return -1; }
  HB_CHECK(hipMemcpyAsync(bucket_dev_.get() + W, bucket_host_.host() + W, bytes, hipMemcpyHostToDevice, stream_), "memcpy(bucket cursors)");
  HB_LAUNCH(launch_bucket_scatter(idx_dev_.get(), sh_.n_local, sh_.cap, bucket_dev_.get() + W, req_out, slot_dev_.get(), stream_), "k_bucket_scatter");
  return 0;
}

int HipBackend::resample_serve(const double *req_in, int64_t m, double *rows_out) {
  HB_LAUNCH(launch_resample_serve(req_in, m, m_.d + m_.s, pop_ptrs(cur_), rows_out, stream_), "k_resample_serve");
  return 0;
}

int HipBackend::resample_scatter(const double *rows_in) {
  const int nxt = 1 - cur_;
  HB_LAUNCH(launch_resample_scatter(rows_in, slot_dev_.get(), sh_.n_local, m_.d + m_.s, pop_ptrs(nxt), stream_), "k_resample_scatter");
  flip_cur();
  return 0;
}

double HipBackend::last_ess() {
  if (stream_) (void)hipStreamSynchronize(stream_);
  return totals_host_ && totals_host_[1] > 0 ? totals_host_[0] * totals_host_[0] / totals_host_[1] : 0.0;   // :134
}

int HipBackend::download(double *theta, double *u, double *rho) {
  const size_t w = (size_t)sh_.n_local * sizeof(double), pitch = (size_t)sh_.cap * sizeof(double);
  if (sh_.n_local > 0) {
    if (theta) HB_CHECK(hipMemcpy2DAsync(theta, w, pop_[cur_].get(), pitch, w, (size_t)m_.d, hipMemcpyDeviceToHost, stream_), "download theta");
    if (u) HB_CHECK(hipMemcpy2DAsync(u, w, pop_[cur_].get() + (size_t)m_.d * sh_.cap, pitch, w, (size_t)m_.s, hipMemcpyDeviceToHost, stream_), "download u");
    if (rho) HB_CHECK(hipMemcpy2DAsync(rho, w, rho_.get(), pitch, w, (size_t)m_.s, hipMemcpyDeviceToHost, stream_), "download rho");
  }
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  return 0;
}

int HipBackend::upload(const double *theta, const double *u, const double *rho) {
  const size_t w = (size_t)sh_.n_local * sizeof(double), pitch = (size_t)sh_.cap * sizeof(double);
  if (sh_.n_local > 0) {
    if (theta) HB_CHECK(hipMemcpy2DAsync(pop_[cur_].get(), pitch, theta, w, w, (size_t)m_.d, hipMemcpyHostToDevice, stream_), "upload theta");
    if (u) HB_CHECK(hipMemcpy2DAsync(pop_[cur_].get() + (size_t)m_.d * sh_.cap, pitch, u, w, w, (size_t)m_.s, hipMemcpyHostToDevice, stream_), "upload u");
    if (rho) HB_CHECK(hipMemcpy2DAsync(rho_.get(), pitch, rho, w, w, (size_t)m_.s, hipMemcpyHostToDevice, stream_), "upload rho");
  }
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  return 0;
}

int HipBackend::get_knots(int stat, double *out, int64_t len) {
  if (stat < 0 || stat >= m_.s || len > cdf_len_[stat]) { err_ = "get_knots: bad statistic index or length"; return -1; }
  HB_CHECK(hipMemcpyAsync(out, knots_.get() + (int64_t)stat * knot_stride_, (size_t)len * sizeof(double), hipMemcpyDeviceToHost, stream_), "memcpy(knots)");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  return 0;
}

int HipBackend::set_knots(int stat, const double *knots, int64_t len) {
  if (stat < 0 || stat >= m_.s || len < 3 || len > knot_stride_ - 16) { err_ = "set_knots: bad statistic index or length"; return -1; }
  // every lookup assumes a sorted table of finite non-negative distances (a NaN breaks the search's predicate, +inf is the
  // padding behind the table): refuse anything else before the handle's table is touched
  for (int64_t i = 0; i < len; ++i) {
    if (!(std::isfinite(knots[i]) && knots[i] >= 0.0)) { err_ = "set_knots: knots must be finite and non-negative"; return -1; }
    if (i > 0 && knots[i] < knots[i - 1]) { err_ = "set_knots: knots must be non-decreasing"; return -1; }
  }
  HB_CHECK(hipMemcpyAsync(knots_.get() + (int64_t)stat * knot_stride_, knots, (size_t)len * sizeof(double), hipMemcpyHostToDevice, stream_), "memcpy(knots)");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  cdf_len_[stat] = len;
  return build_coarse(stat);
}

// index levels of the ECDF search (device_models.hpp): coarse = the smallest shift with ceil(len / 2^shift) <= cdf_coarse_entries(s)
int HipBackend::build_coarse(int stat) {
  int shift = 0;
  const int nc = cdf_coarse_entries(m_.s);
  while ((((int64_t)cdf_len_[stat] + ((int64_t)1 << shift) - 1) >> shift) > nc) ++shift;
  cdf_shift_[stat] = shift;
  HB_LAUNCH(launch_cdf_index(knots_.get() + (int64_t)stat * knot_stride_, cdf_len_[stat], knot_stride_, shift,
                             coarse_.get() + (int64_t)stat * nc, nc, mid_.get() + (int64_t)stat * mid_stride_, mid_stride_, stream_),
            "k_cdf_index");
  return 0;
}

int HipBackend::cdf_apply_host(const double *rho, int64_t m, double *u_out) {
  if (m <= 0) return 0;
  DeviceBuffer<double> d_in, d_out;
  const size_t bytes = (size_t)m * m_.s * sizeof(double);
  HB_CHECK(d_in.alloc((size_t)m * m_.s), "hipMalloc");
  HB_CHECK(d_out.alloc((size_t)m * m_.s), "hipMalloc");
  int rc = check(hipMemcpyAsync(d_in.get(), rho, bytes, hipMemcpyHostToDevice, stream_), "memcpy");
  if (!rc) rc = check((hipError_t)launch_cdf_apply_matrix(cdf_ptrs(), m_.s, d_in.get(), m, d_out.get(), stream_), "k_cdf_apply_matrix");
  if (!rc) rc = check(hipMemcpyAsync(u_out, d_out.get(), bytes, hipMemcpyDeviceToHost, stream_), "memcpy");
  if (!rc) rc = check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  return rc;
}

int HipBackend::prior_host(uint64_t pid0, int64_t n, double *theta_out, double *logpdf_out) {
  if (m_.prior_joint == 2) { err_ = "sabc_op_prior: the prior of this handle lives in host callbacks"; return -1; }
  if (m_.prior_joint == 3 && !(rtc() && rtc()->prior_op)) { err_ = "sabc_op_prior: no device simulator source (with its prior) registered"; return -1; }
  if (n <= 0) return 0;
  DeviceBuffer<double> d_th, d_lp;
  HB_CHECK(hipSetDevice(device_), "hipSetDevice");
  HB_CHECK(d_th.alloc((size_t)n * m_.d), "hipMalloc");
  HB_CHECK(d_lp.alloc((size_t)n), "hipMalloc");
  int rc = check((hipError_t)launch_prior_op(m_, pid0, n, d_th.get(), d_lp.get(), stream_, m_.prior_joint == 3 ? rtc() : nullptr), "k_prior_op");
  if (!rc) rc = check(hipMemcpyAsync(theta_out, d_th.get(), (size_t)n * m_.d * sizeof(double), hipMemcpyDeviceToHost, stream_), "memcpy");
  if (!rc) rc = check(hipMemcpyAsync(logpdf_out, d_lp.get(), (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream_), "memcpy");
  if (!rc) rc = check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  return rc;
}

int HipBackend::simulate_host(const double *theta, int64_t n, uint64_t pid0, uint64_t iter, double *rho_out) {
  if (n <= 0) return 0;
  DeviceBuffer<double> d_in, d_out;
  HB_CHECK(d_in.alloc((size_t)n * m_.d), "hipMalloc");
  HB_CHECK(d_out.alloc((size_t)n * m_.s), "hipMalloc");
  int rc = check(hipMemcpyAsync(d_in.get(), theta, (size_t)n * m_.d * sizeof(double), hipMemcpyHostToDevice, stream_), "memcpy");
  if (!rc) rc = check((hipError_t)launch_simulate_batch(m_, d_in.get(), n, pid0, iter, d_out.get(), stream_, rtc()), "k_simulate_batch");
  if (!rc) rc = check(hipMemcpyAsync(rho_out, d_out.get(), (size_t)n * m_.s * sizeof(double), hipMemcpyDeviceToHost, stream_), "memcpy");
  if (!rc) rc = check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  return rc;
}

// sabc_op_simulate_outputs: the forward run.  Row i is particle pid0 + i at iteration `iter` on the stream of `purpose`; what the
// simulator hands to sabc::emit arrives in out [n_out][n], the distances in rho_out [s][n] (either may be null).  No prior, no
// gate, nothing of the handle's state is read but the model, the module and the data; nothing is written.  Staging is
// DeviceBuffers of this call (freed on every way out), the outputs' pre-filled with NaN -- all bits set is one --, so that what
// a simulation never emits reads as NaN.  A launch stages at most kOutputStageBytes of outputs: a larger call is cut into
// chunks of rows, each copied into its columns of the caller's arrays (rows of the staging are chunk long, the caller's n).
int HipBackend::simulate_outputs_host(const double *theta, int64_t n, uint64_t pid0, uint64_t iter, uint32_t purpose,
                                      int32_t n_out, double *rho_out, double *out) {
  if (n_out < 0) { err_ = "sabc_op_simulate_outputs: n_out must not be negative"; return SABC_ERR_BAD_CONFIG; }
  if (purpose != kPurposeSim && purpose != kPurposePredict) { err_ = "sabc_op_simulate_outputs: stream is SABC_STREAM_UPDATE or SABC_STREAM_PREDICT"; return SABC_ERR_BAD_CONFIG; }
  if (m_.model_id != SABC_MODEL_USER && (n_out > 0 || purpose != kPurposeSim)) {
    err_ = "sabc_op_simulate_outputs: outputs and the predictive streams belong to a simulator from source, the handle was not created with SABC_MODEL_USER";
    return SABC_ERR_BAD_CONFIG;
  }
  if (m_.model_id == SABC_MODEL_USER && !rtc()) { err_ = "sabc_op_simulate_outputs: no device simulator registered (sabc_register_device_simulator)"; return SABC_ERR_BAD_CONFIG; }
  if (n < 0 || (n > 0 && (!theta || (n_out > 0 && !out)))) { err_ = "sabc_op_simulate_outputs: null argument or negative m"; return SABC_ERR_BAD_CONFIG; }
  if (n == 0) return 0;
  constexpr int64_t kOutputStageBytes = (int64_t)128 << 20;
  int64_t chunk = kOutputStageBytes / ((int64_t)sizeof(double) * (n_out > 0 ? n_out : 1));
  if (chunk > 256) chunk -= chunk % 256;                   // whole workgroups, aligned rows
  if (chunk < 1) chunk = 1;
  if (chunk > n) chunk = n;
  HB_CHECK(hipSetDevice(device_), "hipSetDevice");
  DeviceBuffer<double> d_in, d_rho, d_out;
  HB_CHECK(d_in.alloc((size_t)chunk * m_.d), "hipMalloc");
  HB_CHECK(d_rho.alloc((size_t)chunk * m_.s), "hipMalloc");
  if (n_out > 0) HB_CHECK(d_out.alloc((size_t)chunk * n_out), "hipMalloc");
  int rc = 0;
  for (int64_t lo = 0; lo < n && !rc; lo += chunk) {
    const int64_t cnt = n - lo < chunk ? n - lo : chunk;
    const size_t w = (size_t)cnt * sizeof(double), pitch = (size_t)n * sizeof(double);
    rc = check(hipMemcpy2DAsync(d_in.get(), w, theta + lo, pitch, w, (size_t)m_.d, hipMemcpyHostToDevice, stream_), "memcpy2D(theta)");
    if (!rc && n_out > 0) rc = check(hipMemsetAsync(d_out.get(), 0xFF, w * (size_t)n_out, stream_), "memset(outputs)");
    if (!rc) rc = check((hipError_t)launch_simulate_batch(m_, d_in.get(), cnt, pid0 + (uint64_t)lo, iter, d_rho.get(), stream_, rtc(), nullptr,
                                                          n_out > 0 ? d_out.get() : nullptr, n_out, purpose), "k_simulate_batch");
    if (!rc && rho_out) rc = check(hipMemcpy2DAsync(rho_out + lo, pitch, d_rho.get(), w, w, (size_t)m_.s, hipMemcpyDeviceToHost, stream_), "memcpy2D(rho)");
    if (!rc && n_out > 0) rc = check(hipMemcpy2DAsync(out + lo, pitch, d_out.get(), w, w, (size_t)n_out, hipMemcpyDeviceToHost, stream_), "memcpy2D(outputs)");
    // (the staging is reused by the next chunk: the copies out of it are complete before it is written again)
    const int rs = check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    if (!rc) rc = rs;
  }
  return rc;
}

// ---- peer-to-peer transport (p2p.hpp) ----------------------------------------------------------
int64_t HipBackend::parked_bytes() { return g_parked_bytes.load(); }

P2PView HipBackend::p2p_view() const {
  P2PView v;
  std::memset(&v, 0, sizeof(v));
  for (int r = 0; r < kMaxPeers; ++r) v.slots[r] = p2p_.peer_slots[r];
  v.rank = sh_.rank;
  v.world = sh_.world;
  v.timeout_ticks = (uint64_t)(p2p_.timeout_ms * (double)wall_clock_khz_);
  return v;
}


}  // namespace sabc
