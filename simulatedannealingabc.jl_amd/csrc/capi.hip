// capi.hip -- the extern "C" surface of libsabc_hip.so (include/sabc_hip.h): what needs HIP, RCCL or HipBackend's own
// extras.  The backend-independent half (handle, errors, hook collectives, engine entry points, peer-to-peer set-up) is
// capi_shared.hpp, included below.  Plain pointers and sizes only; no exceptions cross this boundary.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/sabc_hip.h"
#include "engine.hpp"
#include "hip_backend.hpp"
#include "host_math.hpp"
#include "kernels.hpp"
#include "rtc.hpp"

using CapiBackend = sabc::HipBackend;
static bool capi_make_current(CapiBackend *be) { return hipSetDevice(be->device()) == hipSuccess; }
#define SABC_CAPI_DEVICE_OPS 1
#include "capi_shared.hpp"

namespace {

// RCCL over xGMI, bound at run time so that the library loads on hosts without librccl
// (and picks up the copy torch already mapped when there is one).
struct Id128 { char b[128]; };   // ncclUniqueId, passed by value
struct RcclApi {
  void *lib = nullptr;
  int (*GetUniqueId)(void *) = nullptr;
  int (*CommInitRank)(void **, int, Id128, int) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
};

RcclApi *rccl_api() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names) {
      api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
      if (api.lib) break;
    }
    if (api.lib) {
      api.GetUniqueId = (int (*)(void *))dlsym(api.lib, "ncclGetUniqueId");
      api.CommInitRank = (int (*)(void **, int, Id128, int))dlsym(api.lib, "ncclCommInitRank");
      api.CommDestroy = (int (*)(void *))dlsym(api.lib, "ncclCommDestroy");
      api.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(api.lib, "ncclAllReduce");
      api.AllGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(api.lib, "ncclAllGather");
      api.Send = (int (*)(const void *, size_t, int, int, void *, hipStream_t))dlsym(api.lib, "ncclSend");
      api.Recv = (int (*)(void *, size_t, int, int, void *, hipStream_t))dlsym(api.lib, "ncclRecv");
      api.GroupStart = (int (*)())dlsym(api.lib, "ncclGroupStart");
      api.GroupEnd = (int (*)())dlsym(api.lib, "ncclGroupEnd");
    }
  });
  return (api.lib && api.GetUniqueId && api.CommInitRank && api.AllReduce && api.AllGather) ? &api : nullptr;
}

class RcclCollectives : public Collectives {
 public:
  RcclCollectives(HipBackend *be, void *comm, int world) : be_(be), comm_(comm), world_(world) {}
  // The grouped send / recv exchange has not run between two GPUs yet (every box so far had one): it is OFF unless
  // SABC_RCCL_ALLTOALLV=1, and the sharded resample on this transport allgathers the whole population -- more bytes, but
  // nothing beyond ncclAllGather.  (Inside a node the peer-to-peer transport carries the resample anyway.)
  bool has_alltoallv() const override {
    static const bool allowed = [] { const char *e = std::getenv("SABC_RCCL_ALLTOALLV"); return e && e[0] == '1'; }();
    RcclApi *a = rccl_api();
    return allowed && a && a->Send && a->Recv && a->GroupStart && a->GroupEnd;
  }
  // grouped ncclSend / ncclRecv, one pair per peer with a non-empty segment (ncclFloat64 = 8)
  int alltoallv(const double *send, const int64_t *sc, double *recv, const int64_t *rc) override {
    RcclApi *a = rccl_api();
    if (a->GroupStart()) return -1;
    int bad = 0;
    int64_t so = 0, ro = 0;
    for (int p = 0; p < world_; ++p) {
      if (sc[p] > 0) bad |= a->Send(send + so, (size_t)sc[p], 8, p, comm_, be_->stream());
      if (rc[p] > 0) bad |= a->Recv(recv + ro, (size_t)rc[p], 8, p, comm_, be_->stream());
      so += sc[p]; ro += rc[p];
    }
    const int end = a->GroupEnd();
    return (bad || end) ? -1 : 0;
  }
  ~RcclCollectives() override {
    RcclApi *a = rccl_api();
    if (a && a->CommDestroy && comm_) a->CommDestroy(comm_);
  }
  int allreduce_sum(double *buf, int64_t count) override {   // ncclFloat64 = 8, ncclSum = 0
    return rccl_api()->AllReduce(buf, buf, (size_t)count, 8, 0, comm_, be_->stream());
  }
  int allgather(const double *send, double *recv, int64_t count) override {
    return rccl_api()->AllGather(send, recv, (size_t)count, 8, comm_, be_->stream());
  }

 private:
  HipBackend *be_;
  void *comm_;
  int world_;
};

// 0, or SABC_ERR_NO_DEVICE with the reason in the global error
int usable_device(int device) {
  (void)hipGetLastError();   // sticky: do not let an earlier failure leak into the launch checks below
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_err = "no usable HIP device (libsabc_hip.so has no CPU path): ";
    g_err += hipGetErrorString(e);
    return SABC_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= n) {
    g_err = "device ordinal out of range";
    return SABC_ERR_NO_DEVICE;
  }
  return 0;
}

// The opening of the stand-alone operators: a usable device, the operator's own argument check (bad_args: what is wrong
// with them, null when nothing is), the device made current.  0, or the code to return with the text in the global error.
int op_open(int32_t device, const char *bad_args = nullptr, int bad_rc = SABC_ERR_BAD_CONFIG) {
  if (int rc = usable_device(device)) return rc;
  if (bad_args) { g_err = bad_args; return bad_rc; }
  if (hipSetDevice(device) != hipSuccess) { g_err = "hipSetDevice failed"; return SABC_ERR_HIP; }
  return 0;
}

// the device halves of capi_shared.hpp's stand-alone operators
int device_op_normal_quads_f32(int32_t device, uint64_t seed, uint64_t pid0, uint32_t purpose, uint64_t iter, uint32_t k, int64_t m,
                               float *out_4m) {
  if (int rc = op_open(device)) return rc;
  if (m <= 0) return 0;
  DeviceBuffer<float> d;
  hipError_t e = d.alloc(4 * (size_t)m);
  if (e == hipSuccess) e = (hipError_t)launch_normal_quads_f32(seed, pid0, purpose, iter, k, m, d.get(), nullptr);
  if (e == hipSuccess) e = hipMemcpy(out_4m, d.get(), (size_t)m * 16, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { g_err = hipGetErrorString(e); return SABC_ERR_HIP; }
  return 0;
}

int device_op_rng_peak_f32(int32_t device, int64_t n_lanes, int32_t quads_per_lane, int32_t repeats, double *normals_per_s) {
  if (int rc = op_open(device)) return rc;
  DeviceBuffer<float> d;
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t e = d.alloc((size_t)n_lanes);
  if (e == hipSuccess) e = hipEventCreate(&a);
  if (e == hipSuccess) e = hipEventCreate(&b);
  if (e == hipSuccess) e = (hipError_t)launch_rng_peak_f32(1, quads_per_lane, n_lanes, d.get(), nullptr);   // warm-up
  if (e == hipSuccess) e = hipEventRecord(a, nullptr);
  for (int r = 0; r < repeats && e == hipSuccess; ++r) e = (hipError_t)launch_rng_peak_f32(2 + r, quads_per_lane, n_lanes, d.get(), nullptr);
  if (e == hipSuccess) e = hipEventRecord(b, nullptr);
  if (e == hipSuccess) e = hipEventSynchronize(b);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
  if (a) (void)hipEventDestroy(a);
  if (b) (void)hipEventDestroy(b);
  if (e != hipSuccess) { g_err = hipGetErrorString(e); return SABC_ERR_HIP; }
  *normals_per_s = 4.0 * (double)quads_per_lane * (double)n_lanes * (double)repeats / ((double)ms * 1e-3);
  return 0;
}

}  // namespace

extern "C" {

int sabc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int sabc_create(const sabc_config *cfg, sabc_handle **out) {
  if (!cfg || !out) { g_err = "null argument"; return SABC_ERR_BAD_CONFIG; }
  *out = nullptr;
  sabc_handle *h = new (std::nothrow) sabc_handle();
  if (!h) { g_err = "out of memory"; return SABC_ERR_BAD_CONFIG; }
  // configuration errors are reported even without a GPU (they are the reference's own errors)
  h->be = new HipBackend(cfg->device);
  h->coll = new NoCollectives();
  h->eng = new Engine(*cfg, h->be, h->coll);
  int rc = h->eng->validate();
  if (rc) { g_err = h->eng->error(); sabc_destroy(h); return rc; }
  rc = usable_device(cfg->device);
  if (rc) { sabc_destroy(h); return rc; }
  if (h->be->allocate(h->eng->model(), h->eng->shard())) {
    g_err = h->be->error();
    sabc_destroy(h);
    return SABC_ERR_HIP;
  }
  *out = h;
  return 0;
}

void sabc_destroy(sabc_handle *h) {
  if (!h) return;
  delete h->eng;
  delete h->coll;
  delete h->be;
  delete h;
}

int sabc_set_stream(sabc_handle *h, void *hip_stream) {
  if (!h) return SABC_ERR_STATE;
  return h->be->set_stream((hipStream_t)hip_stream) ? hfail(h, SABC_ERR_HIP) : 0;
}

static int compile_only(const char *hip_source, int32_t d, int32_t s, char *log_out, int64_t log_cap, bool user_prior, bool team_aware = false);

int sabc_op_compile_device_simulator(const char *hip_source, int32_t d, int32_t s, char *log_out, int64_t log_cap) {
  return compile_only(hip_source, d, s, log_out, log_cap, false);
}
int sabc_op_compile_device_simulator_with_prior(const char *hip_source, int32_t d, int32_t s, char *log_out, int64_t log_cap) {
  return compile_only(hip_source, d, s, log_out, log_cap, true);
}

int sabc_op_compile_device_simulator_team(const char *hip_source, int32_t d, int32_t s, char *log_out, int64_t log_cap) {
  return compile_only(hip_source, d, s, log_out, log_cap, false, true);
}
int sabc_op_compile_device_simulator_team_with_prior(const char *hip_source, int32_t d, int32_t s, char *log_out, int64_t log_cap) {
  return compile_only(hip_source, d, s, log_out, log_cap, true, true);
}

static int compile_only(const char *hip_source, int32_t d, int32_t s, char *log_out, int64_t log_cap, bool user_prior, bool team_aware) {
  if (!hip_source) { g_err = "null device simulator source"; return SABC_ERR_BAD_CONFIG; }
  std::string log;
  size_t cs = 0;
  const RtcRequest rq{hip_source, d, s, rtc_default_csrc_dir(), user_prior, /*with_persistent=*/persistent_fits(d, s), team_aware};
  const int rc = rtc_compile(rq, nullptr, &log, &cs);
  if (log_out && log_cap > 0) { std::snprintf(log_out, (size_t)log_cap, "%s", log.c_str()); }
  if (rc) { g_err = "compiling the device simulator failed:\n" + log; return SABC_ERR_BAD_CONFIG; }
  return 0;
}

int sabc_register_device_simulator(sabc_handle *h, const char *hip_source) {
  if (!h || !hip_source) return hset(h, SABC_ERR_BAD_CONFIG, "null device simulator source");
  if (h->eng->model().model_id != SABC_MODEL_USER) return hset(h, SABC_ERR_BAD_CONFIG, "the handle was not created with SABC_MODEL_USER");
  if (int rc = enter(h)) return rc;
  h->err.clear();
  return h->be->register_device_simulator(hip_source) ? hfail(h, SABC_ERR_BAD_CONFIG) : 0;
}

int sabc_register_device_simulator_team(sabc_handle *h, const char *hip_source, int32_t chain_lanes) {
  if (!h || !hip_source) return hset(h, SABC_ERR_BAD_CONFIG, "null device simulator source");
  if (h->eng->model().model_id != SABC_MODEL_USER) return hset(h, SABC_ERR_BAD_CONFIG, "the handle was not created with SABC_MODEL_USER");
  if (chain_lanes != 1 && chain_lanes != 4 && chain_lanes != 16) return hset(h, SABC_ERR_BAD_CONFIG, "chain_lanes of a team-aware simulator is 1, 4 or 16");
  if (int rc = enter(h)) return rc;
  h->err.clear();
  return h->be->register_device_simulator(hip_source, chain_lanes) ? hfail(h, SABC_ERR_BAD_CONFIG) : 0;
}
int32_t sabc_chain_team_lanes(const sabc_handle *h) { return h ? h->be->chain_team_lanes() : 0; }

int sabc_set_device_data(sabc_handle *h, const double *values, int64_t n, const int64_t *segment_len, int32_t n_segments) {
  if (int rc = enter(h)) return rc;
  h->err.clear();
  const int rc = h->be->set_device_data(values, n, segment_len, n_segments);
  return rc ? hfail(h, rc) : 0;
}
int64_t sabc_device_data_len(const sabc_handle *h) { return h ? h->be->device_data_len() : 0; }

int sabc_set_host_simulator(sabc_handle *h, sabc_simulate_fn fn, void *ctx) {
  if (!h || !fn) return hset(h, SABC_ERR_BAD_CONFIG, "null host simulator");
  if (h->eng->model().model_id != SABC_MODEL_HOST) return hset(h, SABC_ERR_BAD_CONFIG, "the handle was not created with SABC_MODEL_HOST");
  h->be->set_host_simulator(fn, ctx);
  return 0;
}

int sabc_set_host_prior(sabc_handle *h, sabc_prior_sample_fn sample, sabc_prior_logpdf_fn logpdf, void *ctx) {
  if (!h || !sample || !logpdf) return hset(h, SABC_ERR_BAD_CONFIG, "null host prior callback");
  if (h->eng->model().prior_joint != 2) return hset(h, SABC_ERR_BAD_CONFIG, "the handle was not created with prior_joint = 2");
  h->be->set_host_prior(sample, logpdf, ctx);
  return 0;
}

int sabc_set_host_chunk(sabc_handle *h, int64_t particles) {
  if (!h) return SABC_ERR_STATE;
  h->be->set_host_chunk(particles);
  return 0;
}
double sabc_host_callback_seconds(const sabc_handle *h) { return h ? h->be->host_callback_seconds() : 0.0; }
int64_t sabc_host_callback_calls(const sabc_handle *h) { return h ? h->be->host_callback_calls() : 0; }

int sabc_comm_unique_id(void *out_128b) {
  RcclApi *a = rccl_api();
  if (!a) { g_err = "librccl.so could not be loaded"; return SABC_ERR_COMM; }
  return a->GetUniqueId(out_128b) == 0 ? 0 : SABC_ERR_COMM;
}

int sabc_comm_init_rccl(sabc_handle *h, const void *unique_id_128b) {
  if (!h) return SABC_ERR_STATE;
  RcclApi *a = rccl_api();
  if (!a) return hset(h, SABC_ERR_COMM, "librccl.so could not be loaded");
  if (int rc = enter(h)) return rc;
  Id128 id;
  std::memcpy(id.b, unique_id_128b, 128);
  void *comm = nullptr;
  const Shard &sh = h->eng->shard();
  if (a->CommInitRank(&comm, sh.world, id, sh.rank) != 0) return hset(h, SABC_ERR_COMM, "ncclCommInitRank failed");
  delete h->coll;
  h->coll = new RcclCollectives(h->be, comm, sh.world);
  h->eng->set_collectives(h->coll);
  return 0;
}

int64_t sabc_comm_p2p_parked_bytes(void) { return HipBackend::parked_bytes(); }
// device and pinned bytes that DeviceBuffer / MappedHostBuffer own right now (device_buffer.hpp); parked memory is not among them
__attribute__((visibility("default"))) int sabc_debug_live_bytes(int64_t out[2]) {
  out[0] = g_live_bytes[0].load(); out[1] = g_live_bytes[1].load();
  return 0;
}

int sabc_cdf_apply(sabc_handle *h, const double *rho, int64_t m, double *u_out) {
  if (int rc = enter(h)) return rc;
  for (int j = 0; j < h->eng->model().s; ++j)
    if (h->eng->cdf_len()[j] < 3) return hset(h, SABC_ERR_STATE, "ECDF tables are not built yet");
  return h->be->cdf_apply_host(rho, m, u_out) ? hfail(h, SABC_ERR_HIP) : 0;
}

// ---- stand-alone operators -----------------------------------------------------------------
int sabc_op_build_cdf(int32_t device, const double *x, int64_t n, double *knots_out, int64_t *len_out) {
  if (int rc = op_open(device, n < 1 ? "empty input" : nullptr, SABC_ERR_EMPTY_CDF)) return rc;
  DeviceBuffer<double> a, b, k;
  DeviceBuffer<int64_t> meta;
  DeviceBuffer<char> tmp;
  size_t bytes = 0;
  hipError_t e = a.alloc((size_t)n);
  if (e == hipSuccess) e = b.alloc((size_t)n);
  if (e == hipSuccess) e = k.alloc((size_t)n + 2);
  if (e == hipSuccess) e = meta.alloc(2);
  if (e == hipSuccess) e = (hipError_t)sort_f64(a.get(), b.get(), n, nullptr, &bytes, nullptr);
  if (e == hipSuccess) e = tmp.alloc(bytes ? bytes : 16);
  if (e == hipSuccess) e = hipMemcpy(a.get(), x, (size_t)n * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = (hipError_t)sort_f64(a.get(), b.get(), n, tmp.get(), &bytes, nullptr);
  if (e == hipSuccess) e = (hipError_t)launch_cdf_knots(b.get(), n, k.get(), meta.get(), nullptr);
  int64_t hm[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpy(hm, meta.get(), 16, hipMemcpyDeviceToHost);
  int64_t len = 0;
  if (e == hipSuccess) {
    const int64_t mpos = n - hm[0];
    len = mpos > 0 ? mpos + 2 : 0;
    if (len) e = hipMemcpy(knots_out, k.get(), (size_t)len * 8, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) { g_err = hipGetErrorString(e); return SABC_ERR_HIP; }
  if (hm[1]) { g_err = "Negative distances are not allowed!"; return SABC_ERR_NEG_DISTANCE; }
  if (!len) { g_err = "no positive entry"; return SABC_ERR_EMPTY_CDF; }
  *len_out = len;
  return 0;
}

int sabc_op_sort(int32_t device, const double *x, int64_t n, double *out) {
  if (int rc = op_open(device)) return rc;
  if (n <= 0) return 0;
  DeviceBuffer<double> a, b;
  DeviceBuffer<char> tmp;
  size_t bytes = 0;
  hipError_t e = a.alloc((size_t)n);
  if (e == hipSuccess) e = b.alloc((size_t)n);
  if (e == hipSuccess) e = (hipError_t)sort_f64(a.get(), b.get(), n, nullptr, &bytes, nullptr);
  if (e == hipSuccess) e = tmp.alloc(bytes ? bytes : 16);
  if (e == hipSuccess) e = hipMemcpy(a.get(), x, (size_t)n * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = (hipError_t)sort_f64(a.get(), b.get(), n, tmp.get(), &bytes, nullptr);
  if (e == hipSuccess) e = hipMemcpy(out, b.get(), (size_t)n * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { g_err = hipGetErrorString(e); return SABC_ERR_HIP; }
  return 0;
}

int sabc_op_cdf_eval(int32_t device, const double *knots, int64_t len, const double *q, int64_t m, double *out) {
  if (int rc = op_open(device, len < 2 || m < 0 ? "bad length" : nullptr)) return rc;
  if (m == 0) return 0;
  DeviceBuffer<double> k, dq, dout;
  hipError_t e = k.alloc((size_t)len);
  if (e == hipSuccess) e = dq.alloc((size_t)m);
  if (e == hipSuccess) e = dout.alloc((size_t)m);
  if (e == hipSuccess) e = hipMemcpy(k.get(), knots, (size_t)len * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dq.get(), q, (size_t)m * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = (hipError_t)launch_cdf_eval(k.get(), len, dq.get(), m, dout.get(), nullptr);
  if (e == hipSuccess) e = hipMemcpy(out, dout.get(), (size_t)m * 8, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { g_err = hipGetErrorString(e); return SABC_ERR_HIP; }
  return 0;
}

int sabc_op_eps_single(double ubar, double v, double *eps_out) {
  *eps_out = hostmath::eps_single(ubar, v);
  return 0;
}

int sabc_op_eps_multi(const double *ubar, int32_t s, double v, double *eps_out) {
  if (s < 1 || s > SABC_MAX_STATS) return SABC_ERR_BAD_CONFIG;
  return hostmath::eps_multi(ubar, s, v, eps_out) ? 0 : SABC_ERR_ZERO_MEAN_U;
}

int sabc_op_simulate(sabc_handle *h, const double *theta, int64_t m, uint64_t pid0, uint64_t iter, double *rho_out) {
  if (int rc = enter(h)) return rc;
  return h->be->simulate_host(theta, m, pid0, iter, rho_out) ? hfail(h, SABC_ERR_HIP) : 0;
}

int sabc_op_simulate_outputs(sabc_handle *h, const double *theta, int64_t m, uint64_t pid0, uint64_t iter, int32_t stream,
                             int32_t n_out, double *rho_out, double *out) {
  if (int rc = enter(h)) return rc;
  if (stream != SABC_STREAM_UPDATE && stream != SABC_STREAM_PREDICT)
    return hset(h, SABC_ERR_BAD_CONFIG, "sabc_op_simulate_outputs: stream is SABC_STREAM_UPDATE or SABC_STREAM_PREDICT");
  const int rc = h->be->simulate_outputs_host(theta, m, pid0, iter, stream == SABC_STREAM_PREDICT ? kPurposePredict : kPurposeSim, n_out,
                                              rho_out, out);
  return rc ? hfail(h, rc == SABC_ERR_BAD_CONFIG ? SABC_ERR_BAD_CONFIG : SABC_ERR_HIP) : 0;
}

int sabc_op_prior(sabc_handle *h, uint64_t pid0, int64_t m, double *theta_out, double *logpdf_out) {
  if (!theta_out || !logpdf_out) return SABC_ERR_STATE;
  if (int rc = enter(h)) return rc;
  return h->be->prior_host(pid0, m, theta_out, logpdf_out) ? hfail(h, SABC_ERR_HIP) : 0;
}

int sabc_op_philox(int32_t device, uint64_t seed, uint64_t pid, uint32_t purpose, uint64_t iter, uint32_t k,
                   uint32_t out_words[4], double out_normals[2]) {
  if (int rc = op_open(device)) return rc;
  DeviceBuffer<uint32_t> w;
  DeviceBuffer<double> z;
  hipError_t e = w.alloc(4);
  if (e == hipSuccess) e = z.alloc(2);
  if (e == hipSuccess) e = (hipError_t)launch_philox_debug(seed, pid, purpose, iter, k, w.get(), z.get(), nullptr);
  if (e == hipSuccess) e = hipMemcpy(out_words, w.get(), 16, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_normals, z.get(), 16, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { g_err = hipGetErrorString(e); return SABC_ERR_HIP; }
  return 0;
}

int sabc_op_normal_pairs(int32_t device, uint64_t seed, uint64_t pid0, uint32_t purpose, uint64_t iter, uint32_t k,
                         int64_t m, double *out_2m) {
  if (int rc = op_open(device)) return rc;
  if (m <= 0) return 0;
  DeviceBuffer<double> d;
  hipError_t e = d.alloc(2 * (size_t)m);
  if (e == hipSuccess) e = (hipError_t)launch_normal_pairs(seed, pid0, purpose, iter, k, m, d.get(), nullptr);
  if (e == hipSuccess) e = hipMemcpy(out_2m, d.get(), (size_t)m * 16, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { g_err = hipGetErrorString(e); return SABC_ERR_HIP; }
  return 0;
}

int sabc_op_rng_peak(int32_t device, int64_t n_lanes, int32_t pairs_per_lane, int32_t repeats, double *normals_per_s) {
  if (int rc = op_open(device, n_lanes < 1 || pairs_per_lane < 1 || repeats < 1 ? "bad arguments" : nullptr)) return rc;
  DeviceBuffer<double> d;
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t e = d.alloc((size_t)n_lanes);
  if (e == hipSuccess) e = hipEventCreate(&a);
  if (e == hipSuccess) e = hipEventCreate(&b);
  if (e == hipSuccess) e = (hipError_t)launch_rng_peak(1, pairs_per_lane, n_lanes, d.get(), nullptr);   // warm-up
  if (e == hipSuccess) e = hipEventRecord(a, nullptr);
  for (int r = 0; r < repeats && e == hipSuccess; ++r) e = (hipError_t)launch_rng_peak(2 + r, pairs_per_lane, n_lanes, d.get(), nullptr);
  if (e == hipSuccess) e = hipEventRecord(b, nullptr);
  if (e == hipSuccess) e = hipEventSynchronize(b);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
  if (a) (void)hipEventDestroy(a);
  if (b) (void)hipEventDestroy(b);
  if (e != hipSuccess) { g_err = hipGetErrorString(e); return SABC_ERR_HIP; }
  *normals_per_s = 2.0 * (double)pairs_per_lane * (double)n_lanes * (double)repeats / ((double)ms * 1e-3);
  return 0;
}

int64_t sabc_kernel_launches(const sabc_handle *h) { return h ? h->be->kernel_launches() : 0; }

int sabc_profile_enable(sabc_handle *h, int32_t on) {
  if (int rc = enter(h)) return rc;
  h->be->profile_enable(on);
  return 0;
}

int64_t sabc_profile_noops(sabc_handle *h, int32_t kernel) { return h ? h->be->profile_noops(kernel) : 0; }

int sabc_profile_get(sabc_handle *h, int32_t kernel, double *total_ms, int64_t *launches) {
  if (int rc = enter(h)) return rc;
  return h->be->profile_get(kernel, total_ms, launches) ? hfail(h, SABC_ERR_HIP) : 0;
}

}  // extern "C"
