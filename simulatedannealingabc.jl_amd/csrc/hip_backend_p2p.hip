// hip_backend_p2p.hip -- HipBackend, the peer-to-peer transport (p2p.hpp) and the snapshot a failed exchange falls back to.
#include "hip_backend_internal.hpp"

#include <unistd.h>
#include <chrono>
#include <cstdio>
#include <cstring>

namespace sabc {

int HipBackend::p2p_descriptor(P2PDesc *out) {
  std::memset(out, 0, sizeof(*out));
  if (sh_.world < 2 || sh_.world > kMaxPeers) { err_ = "the peer-to-peer transport takes 2..8 shards (one node)"; return -1; }
  HB_CHECK(hipSetDevice(device_), "hipSetDevice");
  // a new set-up (after a failed call switched the transport off, or on top of a live one): this shard LEAVES the old group
  // first -- its peers are unmapped and told so -- before anything of the new one is exported
  if (p2p_leave()) return -1;
  if (!p2p_.page) {
    p2p_.page = p2p_page_create(p2p_.page_name);
    if (!p2p_.page) { err_ = "the peer-to-peer transport needs POSIX shared memory for its host page (shm_open failed)"; return -1; }
  }
  if (!p2p_.slots.get()) {
    // fine-grained, uncached device memory: a peer's store is visible to this device's loads without a cache to go through
    hipError_t e = p2p_.slots.alloc(kP2PSlotWords, hipDeviceMallocUncached);
    if (e != hipSuccess) { (void)hipGetLastError(); e = p2p_.slots.alloc(kP2PSlotWords, hipDeviceMallocFinegrained); }
    if (e != hipSuccess) return check(e, "hipExtMallocWithFlags(slot area)");
    HB_CHECK(p2p_.test_dev.alloc((size_t)(2 * kMaxPartials + 2 + p2p_pattern_save_words() + 2)), "hipMalloc(self-test)");
  }
  // the slots are wiped and the running numbers start over.  (Correctness does not rest on the wipe: every word carries the
  // set-up generation, and a word of an earlier generation -- a status post still in flight from an old peer -- matches nothing.)
  HB_CHECK(hipMemsetAsync(p2p_.slots.get(), 0, (size_t)kP2PSlotWords * 8, stream_), "hipMemset(slot area)");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  p2p_.xseq = p2p_.bseq = p2p_.call = 0;
  out->magic = kP2PMagic;
  out->pid = (int32_t)getpid();
  out->device = device_;
  out->rank = sh_.rank; out->world = sh_.world;
  out->cap = sh_.cap; out->n_global = sh_.n_global;
  out->d = m_.d; out->s = m_.s;
  out->ptr_slots = (uint64_t)(uintptr_t)p2p_.slots.get();
  out->ptr_pop[0] = (uint64_t)(uintptr_t)pop_[0].get(); out->ptr_pop[1] = (uint64_t)(uintptr_t)pop_[1].get();
  out->ptr_rho = (uint64_t)(uintptr_t)rho_.get();
  out->cur = cur_;
  out->gen_proposal = p2p_.gen >= kP2PMaxGen ? 1u : p2p_.gen + 1u;
  out->ptr_page = (uint64_t)(uintptr_t)p2p_.page;
  std::memcpy(out->page_name, p2p_.page_name, sizeof(out->page_name));
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "P2PDesc holds 64-byte IPC handles");
  // the handles are only needed by shards in OTHER processes; a failure here surfaces there (all-zero handle)
  hipIpcMemHandle_t hd;
  void *what[4] = {p2p_.slots.get(), pop_[0].get(), pop_[1].get(), rho_.get()};
  unsigned char *where[4] = {out->ipc_slots, out->ipc_pop[0], out->ipc_pop[1], out->ipc_rho};
  for (int i = 0; i < 4; ++i) {
    if (hipIpcGetMemHandle(&hd, what[i]) == hipSuccess) std::memcpy(where[i], &hd, 64);
    else (void)hipGetLastError();
  }
  p2p_.exported = true;                                     // from here on a peer may hold a mapping of this shard's memory
  return 0;
}

int HipBackend::p2p_init(const P2PDesc *all) {
  if (!p2p_.slots.get() || !p2p_.page) { err_ = "sabc_comm_p2p_descriptor has to be called first"; return -1; }
  HB_CHECK(hipSetDevice(device_), "hipSetDevice");
  const int W = sh_.world;
  if (p2p_.mapped && p2p_leave()) return -1;                // (init twice without a new descriptor)
  p2p_.on = false;
  int khz = 0;                                          // rate of the constant wall clock the waits are bounded by
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_) == hipSuccess && khz > 0) wall_clock_khz_ = khz;
  else (void)hipGetLastError();
  uint32_t proposals[kMaxPeers] = {0};
  for (int r = 0; r < W; ++r) {
    const P2PDesc &d = all[r];
    if (d.magic != kP2PMagic || d.rank != r || d.world != W || d.cap != sh_.cap || d.n_global != sh_.n_global || d.d != m_.d || d.s != m_.s) {
      err_ = "peer-to-peer descriptor of a shard does not match this handle's configuration";
      return -1;
    }
    proposals[r] = d.gen_proposal;
  }
  // the group's generation: above every member's last one; from here on this shard counts as mapped -- whatever goes wrong
  // below is undone by p2p_leave(), which also tells the peers (through the host page) that nothing of theirs stays mapped
  p2p_.gen = p2p_agree_gen(proposals, W);
  p2p_.flips = 0;
  p2p_.page->gen.store(p2p_.gen, std::memory_order_relaxed);
  p2p_.page->cur_parity.store((uint32_t)cur_, std::memory_order_relaxed);
  p2p_.page->state.store(kP2PNone, std::memory_order_release);
  p2p_.mapped = true;
  auto fail = [&](const std::string &why) { (void)p2p_leave(); err_ = why; return -1; };
  for (int r = 0; r < W; ++r) {
    const P2PDesc &d = all[r];
    p2p_.peer_cur0[r] = d.cur & 1;
    if (r == sh_.rank) {
      p2p_.peer_slots[r] = p2p_.slots.get(); p2p_.peer_pop[0][r] = pop_[0].get(); p2p_.peer_pop[1][r] = pop_[1].get(); p2p_.peer_rho[r] = rho_.get();
      p2p_.peer_page[r] = p2p_.page; p2p_.peer_page_shm[r] = false;
      continue;
    }
    if (d.pid == (int32_t)getpid()) {                   // same process: the pointers themselves
      if (d.device != device_) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, device_, d.device) != hipSuccess || !can) return fail("no peer access between the devices of two shards");
        const hipError_t e = hipDeviceEnablePeerAccess(d.device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { (void)check(e, "hipDeviceEnablePeerAccess"); return fail(err_); }
        (void)hipGetLastError();
      }
      p2p_.peer_slots[r] = (uint64_t *)(uintptr_t)d.ptr_slots;
      p2p_.peer_pop[0][r] = (double *)(uintptr_t)d.ptr_pop[0]; p2p_.peer_pop[1][r] = (double *)(uintptr_t)d.ptr_pop[1];
      p2p_.peer_rho[r] = (double *)(uintptr_t)d.ptr_rho;
      // (the host page is opened by NAME even here: a mapping of this shard's own, which stays readable after the peer
      // has destroyed its handle and unmapped its side -- this shard may be polling it for `released` at that moment)
      if (!open_peer_page(r, d)) return fail("a peer shard's host page could not be opened (POSIX shared memory)");
      continue;
    }
    if (d.device != device_) {                          // another GPU of the node: kernels here must be able to reach it
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, device_, d.device) != hipSuccess || !can) {
        (void)hipGetLastError();
        return fail("no peer access between the devices of two shards (is the peer on this node?)");
      }
    }
    if (!open_peer_page(r, d)) return fail("a peer shard's host page could not be opened (POSIX shared memory; is the peer on this node?)");
    const unsigned char *from[4] = {d.ipc_slots, d.ipc_pop[0], d.ipc_pop[1], d.ipc_rho};
    void *got[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 4; ++i) {
      hipIpcMemHandle_t hd;
      std::memcpy(&hd, from[i], 64);
      const hipError_t e = hipIpcOpenMemHandle(&got[i], hd, hipIpcMemLazyEnablePeerAccess);
      if (e != hipSuccess) { (void)check(e, "hipIpcOpenMemHandle (a peer shard's memory)"); return fail(err_); }
      p2p_.ipc_opened.push_back(got[i]);
    }
    p2p_.peer_slots[r] = (uint64_t *)got[0];
    p2p_.peer_pop[0][r] = (double *)got[1]; p2p_.peer_pop[1][r] = (double *)got[2];
    p2p_.peer_rho[r] = (double *)got[3];
  }
  p2p_.page->state.store(kP2PActive, std::memory_order_release);
  p2p_.on = true;
  return 0;
}

bool HipBackend::open_peer_page(int r, const P2PDesc &d) {
  if (p2p_.peer_page_shm[r]) p2p_page_unmap(p2p_.peer_page[r]);           // (a page kept from an earlier set-up)
  char name[sizeof(d.page_name) + 1];
  std::memcpy(name, d.page_name, sizeof(d.page_name)); name[sizeof(d.page_name)] = 0;
  p2p_.peer_page[r] = p2p_page_open(name);
  p2p_.peer_page_shm[r] = p2p_.peer_page[r] != nullptr;
  return p2p_.peer_page[r] != nullptr;
}

// p2p.hpp "LEAVES".  Safe to call in any state and more than once; never frees anything a peer may have mapped.
int HipBackend::p2p_leave() {
  p2p_.pending_xchg = false;
  p2p_.on = false;
  if (!p2p_.mapped) return 0;
  (void)hipSetDevice(device_);
  p2p_.page->state.store(kP2PLeaving, std::memory_order_release);
  if (stream_) {
    // the peers' waits for this shard give up at once; then everything this shard has in flight -- it may be reading the
    // peers' populations -- is drained before their memory is unmapped
    const P2PView pv = p2p_view();
    (void)hipGetLastError();
    (void)launch_p2p_leave(pv, p2p_.gen, stream_);
    launches_ += 1;
    (void)hipStreamSynchronize(stream_);
    (void)hipGetLastError();
  }
  for (void *p : p2p_.ipc_opened) (void)hipIpcCloseMemHandle(p);
  p2p_.ipc_opened.clear();
  (void)hipGetLastError();
  for (int r = 0; r < kMaxPeers; ++r) {
    p2p_.peer_slots[r] = nullptr; p2p_.peer_pop[0][r] = p2p_.peer_pop[1][r] = nullptr; p2p_.peer_rho[r] = nullptr;
    p2p_.page->released[r].store(p2p_.gen, std::memory_order_release);          // "nothing of shard r's generation-p2p_.gen memory is mapped here"
  }
  p2p_.mapped = false;
  return 0;
}

bool HipBackend::p2p_peers_present() {
  if (!p2p_.mapped || !p2p_.on) return true;
  for (int r = 0; r < sh_.world; ++r) {
    const P2PHostPage *pg = p2p_.peer_page[r];
    if (r == sh_.rank || !pg) continue;
    if (pg->gen.load(std::memory_order_acquire) != p2p_.gen || pg->state.load(std::memory_order_acquire) != kP2PActive) return false;
  }
  return true;
}

// Destructor: leave, then wait (bounded) until every peer has recorded that it unmapped this shard's memory.  true: the
// memory peers could map may be freed; false: it has to be parked.
bool HipBackend::p2p_finish() {
  const P2PHostPage *pages[kMaxPeers];
  for (int r = 0; r < kMaxPeers; ++r) pages[r] = p2p_.peer_page[r];
  (void)p2p_leave();
  bool ok = true;
  if (p2p_.exported) {
    const double wait_ms = p2p_.destroy_wait_ms < 0 ? p2p_.timeout_ms : p2p_.destroy_wait_ms;
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < sh_.world && r < kMaxPeers; ++r) {
      if (r == sh_.rank) continue;
      // a peer this shard never got to know (set-up stopped before or inside sabc_comm_p2p_init) cannot acknowledge
      if (!pages[r] || p2p_.gen == 0) { ok = false; continue; }
      // acknowledged: the peer has unmapped this generation -- or has moved on to a later set-up, which begins by leaving
      while (pages[r]->released[sh_.rank].load(std::memory_order_acquire) != p2p_.gen && pages[r]->gen.load(std::memory_order_acquire) <= p2p_.gen) {
        if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > wait_ms) { ok = false; break; }
        usleep(50);
      }
    }
  }
  for (int r = 0; r < kMaxPeers; ++r) {
    if (p2p_.peer_page_shm[r]) p2p_page_unmap(p2p_.peer_page[r]);
    p2p_.peer_page[r] = nullptr; p2p_.peer_page_shm[r] = false;
  }
  if (p2p_.page) {
    p2p_.page->state.store(kP2PGone, std::memory_order_release);
    p2p_page_destroy(p2p_.page, p2p_.page_name);
    p2p_.page = nullptr;
  }
  return ok;
}

// First contact.  (1) a row of known values through the slots + one barrier, the host checks the sums; (2) what the
// transport READS: selftest_patterns().  Sequence numbers advance exactly as in a real exchange, so every shard has to call
// it the same number of times.
int HipBackend::p2p_selftest() {
  if (!p2p_.on) { err_ = "the peer-to-peer transport is not initialised"; return -1; }
  HB_CHECK(hipSetDevice(device_), "hipSetDevice");
  const int np = 7, W = sh_.world;
  double in[np], out[np];
  for (int q = 0; q < np; ++q) in[q] = (double)(sh_.rank + 1) * (q + 1) + (q == 3 ? 0.1 : 0.0);
  double *d_in = p2p_.test_dev.get(), *d_out = p2p_.test_dev.get() + kMaxPartials;
  int *d_failed = (int *)(p2p_.test_dev.get() + 2 * kMaxPartials);
  HB_CHECK(hipMemcpyAsync(d_in, in, sizeof(in), hipMemcpyHostToDevice, stream_), "memcpy");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  const P2PView pv = p2p_view();
  HB_LAUNCH(launch_p2p_selftest(pv, tag(++p2p_.xseq), np, d_in, d_out, d_failed, take_silence(), stream_), "k_p2p_selftest");
  HB_LAUNCH(launch_p2p_barrier(pv, tag(++p2p_.bseq), cb_dev_.get(), false, take_silence(), stream_), "k_p2p_barrier");
  int failed = 1;
  HB_CHECK(hipMemcpyAsync(out, d_out, sizeof(out), hipMemcpyDeviceToHost, stream_), "memcpy");
  HB_CHECK(hipMemcpyAsync(&failed, d_failed, sizeof(int), hipMemcpyDeviceToHost, stream_), "memcpy");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  ControlBlock cb;
  if (read_control(&cb)) return -1;
  bool slots_ok = !(failed || cb.error == SABC_ERR_COMM);
  std::string why = slots_ok ? "" : "peer-to-peer self-test: a shard did not post within the bound";
  for (int q = 0; slots_ok && q < np; ++q) {
    double want = 0.0;
    for (int r = 0; r < W; ++r) { const double x = (double)(r + 1) * (q + 1) + (q == 3 ? 0.1 : 0.0); want = r == 0 ? x : want + x; }
    if (out[q] != want) { slots_ok = false; why = "peer-to-peer self-test: wrong sums came back through the slots"; }
  }
  // the second half runs whatever the first said: the shards stay in step (its barriers return at once behind an error)
  const int prc = selftest_patterns(pv);
  if (!slots_ok) { err_ = why; p2p_.on = false; return -1; }
  if (prc) { p2p_.on = false; return -1; }
  return 0;
}

// What the transport reads (p2p_kernel.hpp: k_p2p_pattern_*): two rounds of write -> barrier -> read every shard's samples ->
// barrier, then the parked values go back.  Works on live populations (a set-up after sabc_initialize).
int HipBackend::selftest_patterns(const P2PView &pv) {
  const int64_t len[3] = {(int64_t)(m_.d + m_.s + 1) * sh_.cap, (int64_t)(m_.d + m_.s + 1) * sh_.cap, (int64_t)m_.s * sh_.cap};
  double *own[3] = {pop_[0].get(), pop_[1].get(), rho_.get()};
  const double *peers[3][kMaxPeers];
  for (int r = 0; r < kMaxPeers; ++r) { peers[0][r] = p2p_.peer_pop[0][r]; peers[1][r] = p2p_.peer_pop[1][r]; peers[2][r] = p2p_.peer_rho[r]; }
  double *save = p2p_.test_dev.get() + 2 * kMaxPartials + 2;
  unsigned int *d_out = (unsigned int *)(save + p2p_pattern_save_words());
  unsigned int res[2][2] = {{0, 0}, {0, 0}};
  for (int round = 1; round <= 2; ++round) {
    HB_LAUNCH(launch_p2p_pattern_write(own, len, save, p2p_.gen, round, sh_.rank, round == 1 ? 0 : 1, stream_), "k_p2p_pattern_write");
    HB_LAUNCH(launch_p2p_barrier(pv, tag(++p2p_.bseq), cb_dev_.get(), false, take_silence(), stream_), "k_p2p_barrier");   // every shard's pattern is written
    HB_CHECK(hipMemsetAsync(d_out, 0, 2 * sizeof(unsigned int), stream_), "memset");
    // (test hook: a shard told to see stale data compares the second round against a pattern nobody wrote)
    const int expect = (round == 2 && p2p_.stale > 0) ? 3 : round;
    HB_LAUNCH(launch_p2p_pattern_check(peers, len, p2p_.gen, expect, sh_.world, d_out, stream_), "k_p2p_pattern_check");
    HB_CHECK(hipMemcpyAsync(res[round - 1], d_out, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, stream_), "memcpy");
    HB_LAUNCH(launch_p2p_barrier(pv, tag(++p2p_.bseq), cb_dev_.get(), false, take_silence(), stream_), "k_p2p_barrier");   // every shard has read
  }
  if (p2p_.stale > 0) --p2p_.stale;
  HB_LAUNCH(launch_p2p_pattern_write(own, len, save, p2p_.gen, 0, sh_.rank, 2, stream_), "k_p2p_pattern_write (restore)");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  ControlBlock cb;
  if (read_control(&cb)) return -1;
  if (cb.error == SABC_ERR_COMM) { err_ = "peer-to-peer self-test: a shard did not reach a barrier within the bound"; return -1; }
  for (int round = 1; round <= 2; ++round)
    if (res[round - 1][0]) {
      static const char *what[3] = {"population buffer 0", "population buffer 1", "rho"};
      const unsigned w = res[round - 1][1];
      char buf[256];
      std::snprintf(buf, sizeof(buf), "peer-to-peer self-test: %u of the words read from the shards' memory were not what their owners wrote "
                    "(round %d; first: shard %u, %s, sample %u) -- a kernel boundary does not make a peer's plain device memory visible here",
                    res[round - 1][0], round, w >> 28, what[((w >> 24) & 15) % 3], w & 0xFFFFFFu);
      err_ = buf;
      return -1;
    }
  return 0;
}

int HipBackend::snapshot() {
  const size_t pop_bytes = (size_t)(m_.d + m_.s + 1) * (size_t)sh_.cap * sizeof(double), rho_bytes = (size_t)m_.s * (size_t)sh_.cap * sizeof(double);
  if (!p2p_.snap_pop.get()) {
    HB_CHECK(p2p_.snap_pop.alloc(pop_bytes / sizeof(double)), "hipMalloc(snapshot)");
    HB_CHECK(p2p_.snap_rho.alloc(rho_bytes / sizeof(double)), "hipMalloc(snapshot)");
  }
  HB_CHECK(hipMemcpyAsync(p2p_.snap_pop.get(), pop_[cur_].get(), pop_bytes, hipMemcpyDeviceToDevice, stream_), "snapshot");
  HB_CHECK(hipMemcpyAsync(p2p_.snap_rho.get(), rho_.get(), rho_bytes, hipMemcpyDeviceToDevice, stream_), "snapshot");
  return 0;
}

int HipBackend::restore_snapshot() {
  if (!p2p_.snap_pop.get()) { err_ = "no snapshot of the particles"; return -1; }
  const size_t pop_bytes = (size_t)(m_.d + m_.s + 1) * (size_t)sh_.cap * sizeof(double), rho_bytes = (size_t)m_.s * (size_t)sh_.cap * sizeof(double);
  pending_rows_ = -1;
  p2p_.pending_xchg = false;
  HB_CHECK(hipMemcpyAsync(pop_[cur_].get(), p2p_.snap_pop.get(), pop_bytes, hipMemcpyDeviceToDevice, stream_), "restore");
  HB_CHECK(hipMemcpyAsync(rho_.get(), p2p_.snap_rho.get(), rho_bytes, hipMemcpyDeviceToDevice, stream_), "restore");
  HB_CHECK(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  return 0;
}

int HipBackend::p2p_barrier(bool guarded) {
  if (!p2p_.on) { err_ = "the peer-to-peer transport is not initialised"; return -1; }
  HB_LAUNCH(launch_p2p_barrier(p2p_view(), tag(++p2p_.bseq), cb_dev_.get(), guarded, take_silence(), stream_), "k_p2p_barrier");
  return 0;
}

int HipBackend::p2p_commit(int status, bool wait) {
  if (!p2p_.on) { err_ = "the peer-to-peer transport is not initialised"; return -1; }
  if (pending_rows_ >= 0 && flush_reduce()) return -1;
  HB_LAUNCH(launch_p2p_commit(p2p_view(), tag(++p2p_.call), status, wait, cb_dev_.get(), take_silence(), stream_), "k_p2p_commit");
  return 0;
}

int HipBackend::build_cdf_p2p(int64_t *len_out, int *any_negative) {
  if (p2p_barrier(false)) return -1;                     // every shard's prior simulations are done
  ShardBlocks b = flat_blocks(nullptr, m_.s, sh_.cap, sh_.world);
  b.direct = 1;
  for (int r = 0; r < sh_.world; ++r) b.peer[r] = p2p_.peer_rho[r];
  return build_cdf_blocks(b, len_out, any_negative);
}

int HipBackend::partner_view_p2p(PartnerView *pv) {
  if (!p2p_.on) { err_ = "the peer-to-peer transport is not initialised"; return -1; }
  pv->direct = 1;
  pv->base = nullptr;
  pv->rank_stride = 0;
  pv->cap = sh_.cap;
  for (int r = 0; r < kMaxPeers; ++r) pv->peer[r] = r < sh_.world ? peer_pop_cur(r) : nullptr;   // the OWNER's current buffer
  return 0;
}

int HipBackend::resample_p2p(double delta, uint64_t iter) {
  if (!p2p_.on) { err_ = "the peer-to-peer transport is not initialised"; return -1; }
  if (pending_rows_ >= 0 && flush_reduce()) return -1;
  const int rows = m_.d + m_.s + 1;
  prof_begin(SABC_KERNEL_RESAMPLE);
  HB_LAUNCH(launch_resample_weights(m_, pop_ptrs(cur_), cb_dev_.get(), (double)sh_.n_global, delta, stream_), "k_resample_weights");   // :126-127
  if (p2p_barrier(false)) return -1;                     // every shard's weight row is written
  ShardBlocks b = flat_blocks(nullptr, rows, sh_.cap, sh_.world);
  b.direct = 1;
  for (int r = 0; r < sh_.world; ++r) b.peer[r] = peer_pop_cur(r);
  HB_LAUNCH(launch_weight_scan(b, sh_.n_global, block_sums_.get(), cum_.get(), totals_dev_.get(), totals_host_dev_, stream_), "weight scan");
  launches_ += 2;
  const int nxt = 1 - cur_;
  HB_LAUNCH(launch_resample_gather(m_, b, sh_.n_global, cum_.get(), block_sums_.get(), totals_dev_.get(), iter, pop_ptrs(nxt), stream_), "k_resample_gather");   // :129-132
  prof_end(SABC_KERNEL_RESAMPLE);
  flip_cur();
  return 0;
}

}  // namespace sabc
