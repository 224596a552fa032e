// capi_shared.hpp -- the backend-independent half of include/sabc_hip.h, written once: the handle, its error texts, the
// collectives over the caller's hooks, and every entry point that needs nothing of a backend beyond what both backends
// offer.  Included by exactly ONE translation unit per library -- capi.hip (libsabc_hip.so) and
// tests/cpu_engine/ref_backend.cpp (the CPU harness of the host engine) -- so that the tests without a GPU run the
// product's own C layer.  Plain C++17: no HIP header.  Before the #include the includer names, at file scope,
//   using CapiBackend = <its Backend>;        (HipBackend | RefBackend: next to sabc::Backend it has error(),
//                                              p2p_descriptor / _init / _selftest / _forget_export and the p2p_set_* /
//                                              p2p_inject_* knobs)
//   bool capi_make_current(CapiBackend *);    (the body of the prologue: make the handle's device the thread's current one)
// and, after it, the entry points that do depend on the backend (sabc_create and sabc_destroy among them).
// An includer with a device also defines SABC_CAPI_DEVICE_OPS before the #include and, after it, the device halves of the
// stand-alone operators declared below (device_op_*); without it those operators answer SABC_ERR_NO_DEVICE.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sabc_hip.h"
#include "engine.hpp"
#include "p2p.hpp"
#include "p2p_setup.hpp"

struct sabc_handle {
  sabc::Engine *eng = nullptr;
  CapiBackend *be = nullptr;
  sabc::Collectives *coll = nullptr;
  std::string err;
};

using namespace sabc;

namespace {

thread_local std::string g_err;

int hfail(sabc_handle *h, int code) {
  if (!h) return code;
  h->err = h->eng && !h->eng->error().empty() ? h->eng->error() : h->err;
  if (h->be && !h->be->error().empty()) { h->err += h->err.empty() ? "" : " | "; h->err += h->be->error(); }
  return code;
}
int hset(sabc_handle *h, int code, const char *msg) {
  if (h) h->err = msg;
  return code;
}

// The prologue of every entry point that can reach the device (it allocates, copies or enqueues there): a null handle is
// refused, and the handle's device becomes the calling thread's current one -- a handle may be used from a thread that
// last worked on another device.
int enter(sabc_handle *h) {
  if (!h) return SABC_ERR_STATE;
  return capi_make_current(h->be) ? 0 : hset(h, SABC_ERR_HIP, "hipSetDevice failed");
}

// world == 1
class NoCollectives : public Collectives {
 public:
  // only ever called with world > 1 (the engine skips collectives on one shard): no transport was installed
  int allreduce_sum(double *, int64_t) override { return -1; }
  int allgather(const double *, double *, int64_t) override { return -1; }
  bool usable() const override { return false; }
};

// user-supplied hooks (torch.distributed from Python, MPI/RCCL from Julia).  dev: the hooks take pointers into the
// backend's memory and its stream; otherwise every call is a round trip through host memory.
class CallbackCollectives : public Collectives {
 public:
  CallbackCollectives(Backend *be, int world, sabc_allreduce_fn ar, sabc_allgather_fn ag, void *ctx, bool dev)
      : be_(be), world_(world), ar_(ar), ag_(ag), ctx_(ctx), dev_(dev) {}
  void set_alltoallv(sabc_alltoallv_fn fn) { a2a_ = fn; }
  bool has_alltoallv() const override { return a2a_ != nullptr; }
  int alltoallv(const double *send, const int64_t *sc, double *recv, const int64_t *rc) override {
    if (!a2a_) return -1;
    if (dev_) return a2a_(ctx_, send, sc, recv, rc, world_, be_->stream_handle());
    int64_t ns = 0, nr = 0;
    for (int p = 0; p < world_; ++p) { ns += sc[p]; nr += rc[p]; }
    return staged(send, ns, recv, nr, [&](double *in, double *out) { return a2a_(ctx_, in, sc, out, rc, world_, nullptr); });
  }
  int allreduce_sum(double *buf, int64_t count) override {
    if (dev_) return ar_(ctx_, buf, count, be_->stream_handle());
    return staged(buf, count, buf, count, [&](double *in, double *) { return ar_(ctx_, in, count, nullptr); }, /*in_place=*/true);
  }
  int allgather(const double *send, double *recv, int64_t count) override {
    if (dev_) return ag_(ctx_, send, recv, count, be_->stream_handle());
    return staged(send, count, recv, count * world_, [&](double *in, double *out) { return ag_(ctx_, in, out, count, nullptr); });
  }

 private:
  // the host-staged round trip: n_in doubles of `src` to the host, the hook on the host copies (its result behind its
  // input, or in_place), n_out doubles of the result back to `dst`.  Each transfer has completed when it returns.
  template <class Hook>
  int staged(const double *src, int64_t n_in, double *dst, int64_t n_out, Hook hook, bool in_place = false) {
    if ((int64_t)stage_.size() < n_in + n_out + 2) stage_.resize((size_t)(n_in + n_out + 2));
    double *in = stage_.data(), *out = in_place ? in : in + n_in;
    if (be_->to_host(in, src, n_in)) return -1;
    if (hook(in, out)) return -1;
    return be_->to_backend(dst, out, n_out) ? -1 : 0;
  }

  Backend *be_;
  int world_;
  sabc_allreduce_fn ar_;
  sabc_allgather_fn ag_;
  sabc_alltoallv_fn a2a_ = nullptr;
  void *ctx_;
  bool dev_;
  std::vector<double> stage_;
};

#if defined(SABC_CAPI_DEVICE_OPS)
// the device halves: a usable device made current, the launch, the copy back; the error text in g_err
int device_op_normal_quads_f32(int32_t device, uint64_t seed, uint64_t pid0, uint32_t purpose, uint64_t iter, uint32_t k, int64_t m,
                               float *out_4m);
int device_op_rng_peak_f32(int32_t device, int64_t n_lanes, int32_t quads_per_lane, int32_t repeats, double *normals_per_s);
#endif

int no_device_op(const char *name) {
  g_err = std::string(name) + ": this library has no device";
  return SABC_ERR_NO_DEVICE;
}

}  // namespace

extern "C" {

int sabc_abi_version(void) { return SABC_ABI_VERSION; }
const char *sabc_last_global_error(void) { return g_err.c_str(); }
const char *sabc_last_error(const sabc_handle *h) { return h ? h->err.c_str() : g_err.c_str(); }

int sabc_set_collectives(sabc_handle *h, sabc_allreduce_fn ar, sabc_allgather_fn ag, void *ctx, int device_buffers) {
  if (!h || !ar || !ag) return hset(h, SABC_ERR_COMM, "null collective hook");
  Collectives *c = new CallbackCollectives(h->be, h->eng->shard().world, ar, ag, ctx, device_buffers != 0);
  delete h->coll;
  h->coll = c;
  h->eng->set_collectives(c);
  return 0;
}

int sabc_set_alltoallv(sabc_handle *h, sabc_alltoallv_fn fn) {
  if (!h || !fn) return hset(h, SABC_ERR_COMM, "null collective hook");
  CallbackCollectives *c = dynamic_cast<CallbackCollectives *>(h->coll);
  if (!c) return hset(h, SABC_ERR_COMM, "sabc_set_alltoallv needs the hooks of sabc_set_collectives to be installed first");
  c->set_alltoallv(fn);
  return 0;
}

int64_t sabc_comm_bytes(const sabc_handle *h) { return h ? h->eng->comm_bytes() : 0; }

// Exercise the installed collectives once and check the result on the host: an allgather of an odd-sized block (5
// doubles: not a multiple of any vector width), an allreduce, and -- when the transport has one -- a personalised
// exchange with a different segment length for every (sender, receiver) pair, as the resample issues it.
// Validates the transport before the first population update.
int sabc_comm_selftest(sabc_handle *h) {
  if (int rc = enter(h)) return rc;
  const Shard &sh = h->eng->shard();
  const int world = sh.world, B = 5;
  if (world == 1) return 0;
  double *g = h->be->gather_buffer((int64_t)(world + 1) * B);
  if (!g) return hset(h, SABC_ERR_HIP, "out of memory for the self-test buffer");
  double send[B] = {(double)(sh.rank + 1), 2.0, 3.0, (double)(100 + sh.rank), -1.5};
  std::vector<double> back((size_t)(world + 1) * B, 0.0);
  if (h->be->to_backend(g, send, B)) return hfail(h, SABC_ERR_HIP);
  if (h->coll->allgather(g, g + B, B)) return hset(h, SABC_ERR_COMM, "self-test allgather failed");
  if (h->coll->allreduce_sum(g, B)) return hset(h, SABC_ERR_COMM, "self-test allreduce failed");
  if (h->be->to_host(back.data(), g, (int64_t)back.size())) return hfail(h, SABC_ERR_HIP);
  if (back[0] != 0.5 * world * (world + 1) || back[1] != 2.0 * world || back[4] != -1.5 * world)
    return hset(h, SABC_ERR_COMM, "self-test allreduce gave a wrong sum");
  for (int r = 0; r < world; ++r)
    if (back[B + B * r] != (double)(r + 1) || back[B + B * r + 3] != (double)(100 + r) || back[B + B * r + 4] != -1.5)
      return hset(h, SABC_ERR_COMM, "self-test allgather gave wrong words");
  if (h->coll->has_alltoallv()) {
    // rank r sends (r + p + 1) doubles of value 1000 r + p to rank p
    std::vector<int64_t> sc((size_t)world), rc((size_t)world);
    int64_t ns = 0, nr = 0;
    for (int p = 0; p < world; ++p) { sc[(size_t)p] = rc[(size_t)p] = sh.rank + p + 1; ns += sc[(size_t)p]; nr += rc[(size_t)p]; }
    std::vector<double> out((size_t)ns), in((size_t)nr, 0.0);
    int64_t o = 0;
    for (int p = 0; p < world; ++p)
      for (int64_t k = 0; k < sc[(size_t)p]; ++k) out[(size_t)o++] = 1000.0 * sh.rank + p;
    double *ds = h->be->scratch_buffer(0, ns), *dr = h->be->scratch_buffer(1, nr);
    if (!ds || !dr) return hset(h, SABC_ERR_HIP, "out of memory for the self-test buffer");
    if (h->be->to_backend(ds, out.data(), ns)) return hfail(h, SABC_ERR_HIP);
    if (h->coll->alltoallv(ds, sc.data(), dr, rc.data())) return hset(h, SABC_ERR_COMM, "self-test alltoallv failed");
    if (h->be->to_host(in.data(), dr, nr)) return hfail(h, SABC_ERR_HIP);
    o = 0;
    for (int p = 0; p < world; ++p)
      for (int64_t k = 0; k < rc[(size_t)p]; ++k)
        if (in[(size_t)o++] != 1000.0 * p + sh.rank) return hset(h, SABC_ERR_COMM, "self-test alltoallv gave wrong words");
  }
  return 0;
}

// ---- peer-to-peer transport (csrc/p2p.hpp) ----
int sabc_comm_p2p_descriptor(sabc_handle *h, void *out_desc) {
  if (!out_desc) return SABC_ERR_STATE;
  if (int rc = enter(h)) return rc;
  return h->be->p2p_descriptor(reinterpret_cast<P2PDesc *>(out_desc)) ? hfail(h, SABC_ERR_COMM) : 0;
}

int sabc_comm_p2p_init(sabc_handle *h, const void *all_descs) {
  if (int rc = enter(h)) return rc;
  const Shard &sh = h->eng->shard();
  if (sh.world < 2 || sh.world > SABC_P2P_MAX_WORLD) return hset(h, SABC_ERR_COMM, "the peer-to-peer transport takes 2..8 shards (one node)");
  std::vector<P2PDesc> all((size_t)sh.world);
  if (all_descs) {
    std::memcpy(all.data(), all_descs, all.size() * sizeof(P2PDesc));
  } else {
    P2PDesc mine;
    if (h->be->p2p_descriptor(&mine)) return hfail(h, SABC_ERR_COMM);
    std::string why;
    if (int rc = p2p_gather_descriptors(h->be, h->coll, sh.world, mine, all, &why)) return hset(h, rc, why.c_str());
  }
  return h->be->p2p_init(all.data()) ? hfail(h, SABC_ERR_COMM) : 0;
}

// The whole set-up, with the shards agreeing after every step (csrc/p2p_setup.hpp).
int sabc_comm_p2p_setup(sabc_handle *h) {
  if (int rc = enter(h)) return rc;
  std::string note;
  const int rc = p2p_setup_sequence(h->be, h->coll, h->eng->shard(), h->eng->host_mode(), &note);
  h->err = note;
  return rc == 1 ? (h->eng->p2p() ? 1 : 0) : rc;
}

int sabc_comm_p2p_selftest(sabc_handle *h) {
  if (int rc = enter(h)) return rc;
  return h->be->p2p_selftest() ? hfail(h, SABC_ERR_COMM) : 0;
}

int sabc_comm_p2p_set_timeout(sabc_handle *h, double milliseconds) {
  if (!h || !(milliseconds > 0)) return hset(h, SABC_ERR_BAD_CONFIG, "the bound of a peer-to-peer wait must be positive");
  h->be->p2p_set_timeout(milliseconds);
  return 0;
}

int sabc_comm_p2p_disable(sabc_handle *h) {
  if (!h) return SABC_ERR_STATE;
  h->be->p2p_disable();
  return 0;
}

int sabc_comm_p2p_active(const sabc_handle *h) { return h && h->eng->p2p() ? 1 : 0; }
int64_t sabc_comm_p2p_fallbacks(const sabc_handle *h) { return h ? h->eng->p2p_fallbacks() : 0; }

int sabc_comm_p2p_inject_silence(sabc_handle *h, int32_t n) {
  if (!h) return SABC_ERR_STATE;
  h->be->p2p_inject_silence(n);
  return 0;
}

int sabc_comm_p2p_inject_loss(sabc_handle *h, int32_t n) {
  if (!h) return SABC_ERR_STATE;
  h->be->p2p_inject_loss(n);
  return 0;
}

int sabc_comm_p2p_inject_stale(sabc_handle *h, int32_t n) {
  if (!h) return SABC_ERR_STATE;
  h->be->p2p_inject_stale(n);
  return 0;
}

int sabc_comm_p2p_set_destroy_wait(sabc_handle *h, double milliseconds) {
  if (!h || !(milliseconds >= 0)) return hset(h, SABC_ERR_BAD_CONFIG, "the wait of sabc_destroy must not be negative");
  h->be->p2p_set_destroy_wait(milliseconds);
  return 0;
}

int64_t sabc_persistent_launches(const sabc_handle *h) { return h ? h->eng->persistent_launches() : 0; }
int32_t sabc_persistent_lanes(const sabc_handle *h) { return h ? h->eng->persistent_lanes() : 0; }
int64_t sabc_persistent_fallbacks(const sabc_handle *h) { return h ? h->eng->persistent_fallbacks() : 0; }

int sabc_initialize(sabc_handle *h, int64_t n_simulation) {
  if (int rc = enter(h)) return rc;
  const int rc = h->eng->initialize(n_simulation);
  return rc ? hfail(h, rc) : 0;
}

int sabc_update(sabc_handle *h, const sabc_update_args *args) {
  if (!args) return SABC_ERR_STATE;
  if (int rc = enter(h)) return rc;
  const int rc = h->eng->update(*args);
  return rc ? hfail(h, rc) : 0;
}

int64_t sabc_n_global(const sabc_handle *h) { return h ? h->eng->shard().n_global : 0; }
int64_t sabc_n_local(const sabc_handle *h) { return h ? h->eng->shard().n_local : 0; }
int64_t sabc_local_offset(const sabc_handle *h) { return h ? h->eng->shard().gid0 : 0; }

int sabc_get_population(sabc_handle *h, double *theta, double *u, double *rho) {
  if (int rc = enter(h)) return rc;
  return h->be->download(theta, u, rho) ? hfail(h, SABC_ERR_HIP) : 0;
}

int sabc_set_population(sabc_handle *h, const double *theta, const double *u, const double *rho) {
  if (int rc = enter(h)) return rc;
  if (h->be->upload(theta, u, rho)) return hfail(h, SABC_ERR_HIP);
  h->eng->mark_initialized();
  return 0;
}

int sabc_get_counters(const sabc_handle *h, int64_t out[4]) {
  if (!h) return SABC_ERR_STATE;
  h->eng->counters(out);
  return 0;
}
int sabc_set_counters(sabc_handle *h, const int64_t in[4]) {
  if (!h) return SABC_ERR_STATE;
  h->eng->set_counters(in);
  return 0;
}
int sabc_get_epsilon(const sabc_handle *h, double *eps, int32_t *len) {
  if (!h) return SABC_ERR_STATE;
  for (int i = 0; i < h->eng->eps_len(); ++i) eps[i] = h->eng->eps()[i];
  if (len) *len = h->eng->eps_len();
  return 0;
}
int sabc_set_epsilon(sabc_handle *h, const double *eps, int32_t len) {
  if (!h) return SABC_ERR_STATE;
  const int rc = h->eng->set_eps(eps, len);
  return rc ? hfail(h, rc) : 0;
}
int64_t sabc_history_len(const sabc_handle *h) { return h ? h->eng->history_len() : 0; }
int sabc_get_history(const sabc_handle *h, double *e, double *u, double *r) {
  if (!h) return SABC_ERR_STATE;
  h->eng->history(e, u, r);
  return 0;
}
int sabc_clear_history(sabc_handle *h) {
  if (!h) return SABC_ERR_STATE;
  h->eng->clear_history();
  return 0;
}

int64_t sabc_cdf_len(const sabc_handle *h, int32_t stat) {
  if (!h || stat < 0 || stat >= h->eng->model().s) return 0;
  return h->eng->cdf_len()[stat];
}
int sabc_get_cdf_knots(sabc_handle *h, int32_t stat, double *out) {
  if (int rc = enter(h)) return rc;
  return h->be->get_knots(stat, out, sabc_cdf_len(h, stat)) ? hfail(h, SABC_ERR_HIP) : 0;
}
int sabc_set_cdf_knots(sabc_handle *h, int32_t stat, const double *knots, int64_t len) {
  if (int rc = enter(h)) return rc;
  if (h->be->set_knots(stat, knots, len)) return hfail(h, SABC_ERR_BAD_CONFIG);
  h->eng->set_cdf_len(stat, len);
  return 0;
}
int sabc_get_proposal_sigma(const sabc_handle *h, double *sigma) {
  if (!h) return SABC_ERR_STATE;
  const int d = h->eng->model().d;
  for (int i = 0; i < d * d; ++i) sigma[i] = h->eng->sigma()[i];
  return 0;
}
double sabc_last_ess(const sabc_handle *h) { return enter(const_cast<sabc_handle *>(h)) ? 0.0 : h->be->last_ess(); }

// ---- stand-alone operators on the binary32 draws (csrc/device_rng.hpp, namespace f32) ----
int sabc_op_normal_quads_f32(int32_t device, uint64_t seed, uint64_t pid0, uint32_t purpose, uint64_t iter, uint32_t k, int64_t m,
                             float *out_4m) {
  if (m > 0 && !out_4m) { g_err = "sabc_op_normal_quads_f32: null output"; return SABC_ERR_BAD_CONFIG; }
#if defined(SABC_CAPI_DEVICE_OPS)
  return device_op_normal_quads_f32(device, seed, pid0, purpose, iter, k, m, out_4m);
#else
  (void)device; (void)seed; (void)pid0; (void)purpose; (void)iter; (void)k;
  return no_device_op("sabc_op_normal_quads_f32");
#endif
}

int sabc_op_rng_peak_f32(int32_t device, int64_t n_lanes, int32_t quads_per_lane, int32_t repeats, double *normals_per_s) {
  if (!normals_per_s || n_lanes < 1 || quads_per_lane < 1 || repeats < 1) { g_err = "sabc_op_rng_peak_f32: bad arguments"; return SABC_ERR_BAD_CONFIG; }
#if defined(SABC_CAPI_DEVICE_OPS)
  return device_op_rng_peak_f32(device, n_lanes, quads_per_lane, repeats, normals_per_s);
#else
  (void)device;
  return no_device_op("sabc_op_rng_peak_f32");
#endif
}

int64_t sabc_host_syncs(const sabc_handle *h) { return h ? h->eng->host_syncs() : 0; }
int64_t sabc_collective_calls(const sabc_handle *h) { return h ? h->eng->collective_calls() : 0; }

}  // extern "C"
