// hip_backend.hpp -- the product Backend: particle shard resident in HBM, gfx950 kernels,
// one HIP stream.  There is no CPU path behind it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <string>
#include <mutex>
#include <utility>
#include <vector>
#include "engine.hpp"
#include "kernels.hpp"
#include "p2p_page.hpp"
#include "device_buffer.hpp"

namespace sabc {

class HipBackend : public Backend {
 public:
  explicit HipBackend(int device);
  ~HipBackend() override;

  int allocate(const ModelDesc &m, const Shard &sh) override;
  double *pop_block() override { return pop_[cur_].get(); }
  double *rho_block() override { return rho_.get(); }
  double *sums_buffer() override;
  double *gather_buffer(int64_t doubles) override;
  double *scratch_buffer(int which, int64_t doubles) override;
  int copy_rows(const double *src, int64_t src_pitch, double *dst, int64_t dst_pitch, int rows, int64_t count) override;
  int to_backend(double *dst, const double *src_host, int64_t n) override;
  int to_host(double *dst_host, const double *src, int64_t n) override;
  int set_host_simulator(sabc_simulate_fn fn, void *ctx) override { host_.fn = fn; host_.ctx = ctx; return 0; }
  int set_host_prior(sabc_prior_sample_fn sample, sabc_prior_logpdf_fn logpdf, void *ctx) override {
    host_.prior_sample_fn = sample; host_.prior_logpdf_fn = logpdf; host_.prior_ctx = ctx;
    return 0;
  }
  // SABC_MODEL_USER: compile the simulator source into the update kernels (rtc.hpp); the compiler log goes to error()
  // chain_lanes = 0: the source defines sabc_user_simulate; 1 | 4 | 16: it is team-aware (sabc_user_simulate_team<W>) and runs
  // with that many lanes per particle on the launch chain and in the forward run
  int register_device_simulator(const char *hip_source, int chain_lanes = 0);
  int chain_team_lanes() const { return rtc_.module && rtc_.team_aware ? rtc_.chain_lanes : 0; }
  // SABC_MODEL_USER: the observed data the source reads through sabc::data*() (rtc.hpp: RtcDataDesc).  0, or the SABC_ERR_*
  // code with the text in error(); on an error the old data stay in place
  int set_device_data(const double *values, int64_t n, const int64_t *segment_len, int32_t n_segments);
  int64_t device_data_len() const { return (int64_t)data_.count(); }
  int host_prior_simulate() override;
  int host_update_range(const StepArgs &c, const PartnerView &pv, int64_t lo, int64_t cnt) override;
  int host_stats(int64_t *rows_out) override;
  int prior_simulate() override;
  int build_cdf(const double *gathered_rho, int64_t *len_out, int *any_negative) override;
  int cdf_population() override;
  int update_range(const StepArgs &c, const PartnerView &pv, int64_t lo, int64_t cnt, int64_t row0,
                   int64_t *rows_out) override;
  bool persistent_supported(int prop_kind) const override;
  int persistent_lanes() const override { return persist_.lanes; }
  int update_persistent(const StepArgs &c, const ControlArgs &ctrl, const PartnerView &pv_a, const PartnerView &pv_b, int64_t ix0,
                        int64_t phase, int64_t cph, int64_t count, int64_t *done, int *halted, int *error) override;
  int stats(int64_t *rows_out) override;
  int reduce_partials(int64_t rows, bool guarded) override;
  int control(const ControlArgs &a) override;
  int wait_notify(int64_t seq, int64_t *n_accept, int *error, int *halted) override;
  int read_control(ControlBlock *out) override;
  int write_control(const ControlBlock &in) override;
  int history_reserve(int64_t rows) override;
  int read_history(double *out, int64_t rows, int row_len) override;
  int resample_weights(double delta) override;
  int resample_draw(const double *gathered_pop, uint64_t iter) override;
  int resample_local(double delta, uint64_t iter, int64_t *stats_rows) override;
  int resample_select(const double *gathered_w, uint64_t iter) override;
  int resample_bucket(int64_t *counts_host, double *req_out) override;
  int resample_serve(const double *req_in, int64_t m, double *rows_out) override;
  int resample_scatter(const double *rows_in) override;
  double last_ess() override;
  void end_of_call() override;
  void prof_begin(int kernel) override;
  void prof_end(int kernel) override;
  int64_t profile_noops(int kernel) const { return kernel >= 0 && kernel < SABC_KERNEL_COUNT ? prof_noop_[kernel] : 0; }
  int download(double *theta, double *u, double *rho) override;
  int upload(const double *theta, const double *u, const double *rho) override;
  int get_knots(int stat, double *out, int64_t len) override;
  int set_knots(int stat, const double *knots, int64_t len) override;

  // peer-to-peer transport (p2p.hpp)
  bool p2p_active() const override { return p2p_.on; }
  int p2p_exchange_pending() override { p2p_.pending_xchg = true; return 0; }
  int p2p_barrier(bool guarded) override;
  int p2p_commit(int status, bool wait) override;
  void p2p_disable() override { (void)p2p_leave(); }
  bool p2p_peers_present() override;                // every peer's host page still says `active` for this generation
  int build_cdf_p2p(int64_t *len_out, int *any_negative) override;
  int partner_view_p2p(PartnerView *pv) override;
  int resample_p2p(double delta, uint64_t iter) override;
  int snapshot() override;
  int restore_snapshot() override;
  int p2p_descriptor(P2PDesc *out);                 // allocates the slot area on first use
  int p2p_init(const P2PDesc *all);                 // maps every peer's slots, populations and rho; switches the transport on
  int p2p_selftest();
  int p2p_leave();                                  // p2p.hpp "LEAVES": leaving -> leave words -> drain -> unmap -> released
  // the group has agreed that every shard has left and unmapped (p2p_setup.hpp): nothing exported is mapped anywhere
  void p2p_forget_export() { if (!p2p_.mapped) p2p_.exported = false; }
  void p2p_set_destroy_wait(double ms) { p2p_.destroy_wait_ms = ms; }
  void p2p_inject_stale(int n) { p2p_.stale = n > 0 ? n : 0; }
  static int64_t parked_bytes();
  void p2p_set_timeout(double ms) { if (ms > 0) p2p_.timeout_ms = ms; }
  // test hook: n > 0: the next n posts are skipped; n < 0: -n more posts go out, then one is skipped
  void p2p_inject_silence(int n) { p2p_.loss = false; if (n >= 0) { p2p_.skip = 0; p2p_.silent = n; } else { p2p_.skip = -n; p2p_.silent = 1; } }
  // test hook: n more posts go out, then one reaches only this shard's OWN slots (a post lost on the wire: the shard itself
  // carries on with its peers' rows, they run into the bound)
  void p2p_inject_loss(int n) { p2p_.loss = true; p2p_.skip = n > 0 ? n : 0; p2p_.silent = 1; }
  int64_t kernel_launches() const { return launches_; }
  // host-simulator mode: seconds spent inside the caller's callbacks so far / calls of f_dist; particles per chunk
  double host_callback_seconds() const { return host_.cb_seconds; }
  int64_t host_callback_calls() const { return host_.cb_calls; }
  void set_host_chunk(int64_t particles) { host_.chunk = particles > 0 ? particles : 0; }

  // extras used by the C-ABI layer
  int set_stream(hipStream_t s);
  hipStream_t stream() const { return stream_; }
  void *stream_handle() const override { return (void *)stream_; }
  int device() const { return device_; }
  const std::string &error() const { return err_; }
  CdfPtrs cdf_ptrs() const;
  void set_cdf_len(int stat, int64_t len) { cdf_len_[stat] = len; }
  int cdf_apply_host(const double *rho, int64_t m, double *u_out);
  int simulate_host(const double *theta, int64_t n, uint64_t pid0, uint64_t iter, double *rho_out);
  int prior_host(uint64_t pid0, int64_t n, double *theta_out, double *logpdf_out);   // sabc_op_prior
  int simulate_outputs_host(const double *theta, int64_t n, uint64_t pid0, uint64_t iter, uint32_t purpose, int32_t n_out,
                            double *rho_out, double *out);                           // sabc_op_simulate_outputs
  void profile_enable(int level);
  int profile_get(int kernel, double *total_ms, int64_t *launches);

 private:
  int check(hipError_t e, const char *what);
  PopPtrs pop_ptrs(int which) const;

  // Declaration order is release order, backwards: after ~HipBackend() has left the group and drained the stream, the
  // buffers below are freed, then the run-time compiled kernels are released, and the stream goes back to the pool last.
  int device_ = 0;
  hipStream_t stream_ = nullptr;
  bool own_stream_ = false;
  struct StreamReturn { HipBackend *be; ~StreamReturn(); } stream_return_{this};
  struct Rtc : RtcKernels { ~Rtc() { rtc_release(this); } } rtc_;   // SABC_MODEL_USER: kernels compiled from the user's source
  const RtcKernels *rtc() const { return rtc_.module ? &rtc_ : nullptr; }
  std::string err_;
  ModelDesc m_{};
  Shard sh_{};
  int np_ = 0;
  DeviceBuffer<double> pop_[2];
  int cur_ = 0;
  DeviceBuffer<double> rho_, knots_, coarse_, mid_;
  DeviceBuffer<double> data_;                             // observed data of a simulator from source (set_device_data)
  RtcDataDesc data_desc_;                                 // ... and what the loaded module's sabc_data_desc holds about them
  int push_data_desc();                                   // writes data_desc_ into the module, if one is loaded
  int64_t mid_stride_ = 0;
  int32_t cdf_shift_[kMaxStats] = {0};
  int build_coarse(int stat);
  int64_t knot_stride_ = 0;
  int64_t cdf_len_[kMaxStats] = {0};
  DeviceBuffer<double> partials_;
  int64_t partial_rows_ = 0;
  // ONE pinned, mapped allocation (hipHostFree is 0.2 ms apiece) and the views into it: the control block's staging copy, the
  // mailbox ring the device posts to and the host polls, and where k_scan_offsets posts (sum w, sum w^2)
  MappedHostBuffer<char> pinned_;
  ControlBlock *cb_host_ = nullptr;
  Mailbox *mbox_host_ = nullptr, *mbox_dev_ = nullptr;
  double *totals_host_ = nullptr, *totals_host_dev_ = nullptr;
  DeviceBuffer<ControlBlock> cb_dev_;
  DeviceBuffer<double> hist_dev_;
  int flush_reduce();                                     // launch a deferred k_reduce_partials
  int64_t pending_rows_ = -1;                             // >= 0: a reduction waits to be fused into k_control
  int64_t fuse_reduce_max_ = kFuseReduceMaxDoubles;       // partial-row matrices up to this many doubles: reduced inside the control launch
  bool pending_guarded_ = false;
  DeviceBuffer<double> sums_stage_;                       // reduction / allreduce target, taken over by k_control
  int64_t hist_cap_ = 0;
  DeviceBuffer<double> gather_, scratch_[4];
  DeviceBuffer<int64_t> idx_dev_, slot_dev_;              // sharded resample: drawn source indices, reply -> destination
  DeviceBuffer<unsigned long long> bucket_dev_;           // [2][world]: counts, cursors
  MappedHostBuffer<unsigned long long> bucket_host_;      // pinned staging of the same
  DeviceBuffer<double> cum_, block_sums_, totals_dev_;
  DeviceBuffer<double> pack_dev_;                         // one shard: packed resample lines (kernels.hpp: launch_resample_local)
  DeviceBuffer<double> col_a_, col_b_;
  DeviceBuffer<char> sort_tmp_;
  size_t sort_tmp_bytes_ = 0;
  DeviceBuffer<int64_t> meta_dev_;
  void free_later(void *p);                               // device memory released by end_of_call(), never inside a call
  std::vector<void *> deferred_free_;
  // a buffer that has to grow inside a call: the old allocation goes to the deferred list, never to hipFree
  template <class T>
  hipError_t grow(DeviceBuffer<T> &b, size_t count) {
    if (stream_) (void)hipStreamSynchronize(stream_);
    free_later(b.release());
    return b.alloc(count);
  }

  // host-simulator mode (hip_backend_hostmode.hip)
  static constexpr int kHostMaxChunks = 64;
  struct HostMode {
    sabc_simulate_fn fn = nullptr;
    sabc_prior_sample_fn prior_sample_fn = nullptr;      // prior_joint = 2: rand(prior) / logpdf(prior, .) on the host
    sabc_prior_logpdf_fn prior_logpdf_fn = nullptr;
    void *prior_ctx = nullptr;
    void *ctx = nullptr;
    struct Staging {                                      // allocated once, all or nothing (ensure_host_buffers)
      // a half batch in pinned host arrays mapped into the device
      MappedHostBuffer<double> thp, rho, cur, lp2;
      MappedHostBuffer<unsigned char> gate;               // one byte per proposal: inside the prior's support?
      DeviceBuffer<double> dev_thp, dev_aux;              // device memory: proposals, (log prior, log factor)
      DeviceBuffer<double> dev_rho_prop;                  // ... and, for a device-coded simulator next to a host prior, their distances
      MappedHostBuffer<unsigned long long> flag;          // per chunk: the proposal kernel posts, the host polls
      DeviceBuffer<unsigned int> done;
      DeviceBuffer<unsigned long long> acc;
    } buf;
    unsigned long long seq = 0;
    int64_t chunk = 0;                                    // particles per chunk; 0 = automatic (host_chunk_size)
    std::vector<int64_t> ids, where;
    std::vector<double> thv, rhov, both, lp;
    double cb_seconds = 0.0;                              // time spent inside the caller's callbacks
    int64_t cb_calls = 0;
  } host_;
  int ensure_host_buffers();
  int64_t host_chunk_size(int64_t cnt) const;
  int wait_host_flag(int ch, unsigned long long seq);

  // peer-to-peer transport (hip_backend_p2p.hip)
  struct P2P {
    DeviceBuffer<uint64_t> slots;                         // this shard's slot area (fine-grained device memory)
    uint64_t *peer_slots[kMaxPeers] = {nullptr};
    double *peer_pop[2][kMaxPeers] = {{nullptr}};
    double *peer_rho[kMaxPeers] = {nullptr};
    int peer_cur0[kMaxPeers] = {0};                       // the owner's parity when the descriptors were written
    uint32_t flips = 0;                                   // buffer flips of THIS shard since then (in step on all shards)
    std::vector<void *> ipc_opened;                       // what hipIpcOpenMemHandle returned (closed when this shard leaves)
    P2PHostPage *page = nullptr;                          // this shard's host page (POSIX shared memory)
    char page_name[48] = {0};
    const P2PHostPage *peer_page[kMaxPeers] = {nullptr};
    bool peer_page_shm[kMaxPeers] = {false};              // opened by name (to be unmapped), not a pointer of this process
    uint32_t gen = 0;                                     // generation of the current (or last) set-up
    bool mapped = false;                                  // the peers' memory is mapped
    bool exported = false;                                // a descriptor has left: peers may have mapped this shard's memory
    double destroy_wait_ms = -1.0;                        // < 0: the bound of the waits
    int stale = 0;
    bool on = false, pending_xchg = false;
    uint32_t xseq = 0, bseq = 0, call = 0;                // exchange / barrier / call sequence numbers (the same on every shard)
    double timeout_ms = 5000.0;
    int silent = 0, skip = 0;
    bool loss = false;
    DeviceBuffer<double> test_dev;
    DeviceBuffer<double> snap_pop, snap_rho;              // device-side copy of the particles at the entry of a call
  } p2p_;
  int build_cdf_blocks(const ShardBlocks &rho_blocks, int64_t *len_out, int *any_negative);
  P2PView p2p_view() const;
  int take_silence() {                                    // 0 | 1 skipped | 2 own slots only
    if (p2p_.skip > 0) { --p2p_.skip; return 0; }
    if (p2p_.silent > 0) { --p2p_.silent; return p2p_.loss ? 2 : 1; }
    return 0;
  }
  bool p2p_finish();                                      // destructor: leave, wait for the peers' `released`; false = park
  void flip_cur() { cur_ = 1 - cur_; ++p2p_.flips; if (p2p_.page) p2p_.page->cur_parity.store((uint32_t)cur_, std::memory_order_relaxed); }
  // a peer's CURRENT population: indexed by the owner's parity at set-up + the flips since (p2p.hpp: P2PDesc::cur)
  double *peer_pop_cur(int r) const { return p2p_.peer_pop[(p2p_.peer_cur0[r] ^ (int)(p2p_.flips & 1u)) & 1][r]; }
  uint32_t tag(uint32_t seq) const { return p2p_tag(p2p_.gen, seq); }
  int selftest_patterns(const P2PView &pv);
  bool open_peer_page(int r, const P2PDesc &d);

  int wall_clock_khz_ = 100000;                           // s_memrealtime: 100 MHz unless the device says otherwise
  int64_t launches_ = 0;
  struct Persist {                                        // the one-launch form of small shards (persistent_kernel.hpp)
    int64_t max = 65536;                                  // shards up to this many particles run their updates in one launch (0: never)
    DeviceBuffer<unsigned long long> sync;                // the grid barrier's counter and abort flag
    DeviceBuffer<unsigned long long> rows;                // the workgroups' partial rows as tagged words, two parities
    int64_t rows_wg = 0;                                  // workgroups it holds rows for
    int lanes = 0;                                        // lanes per particle of the last one-launch update (0: none yet)
  } persist_;
  int prof_ = 0, prof_open_ = -1;
  unsigned prof_tick_ = 0;
  struct EvPair { hipEvent_t a, b; };
  std::vector<EvPair> ev_[SABC_KERNEL_COUNT];
  std::vector<EvPair> ev_pool_;
  double prof_ms_[SABC_KERNEL_COUNT] = {0};
  int64_t prof_n_[SABC_KERNEL_COUNT] = {0};
  int64_t prof_noop_[SABC_KERNEL_COUNT] = {0};
};

}  // namespace sabc
