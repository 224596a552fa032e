// capi_probe.cpp -- TEST INFRASTRUCTURE.  The C ABI of the CPU harness (ref_backend.cpp: the product's own C layer,
// csrc/capi_shared.hpp, over the oracle-backed backend) from a plain C++ program: two shards on two threads, C hooks
// between them, host-staged collectives (device_buffers = 0) with the personalised exchange installed -- self-test, then
// initialisation and three DifferentialEvolution updates.  No Python in between, so the whole of it can also be built
// with -fsanitize=address,undefined and run as it is.  Links ref_backend.cpp, engine.cpp and the oracle.
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sabc_hip.h"

namespace {

constexpr int kWorld = 2, kUpdates = 3;
constexpr int64_t kParticles = 101;               // shards of 51 and 50

struct Group {                                    // what the hooks of all shards share
  std::mutex m;
  std::condition_variable cv;
  int waiting = 0;
  long generation = 0;
  std::vector<double> slot[kWorld];
  std::vector<int64_t> counts[kWorld];
  void barrier() {
    std::unique_lock<std::mutex> lock(m);
    const long g = generation;
    if (++waiting == kWorld) { waiting = 0; ++generation; cv.notify_all(); }
    else cv.wait(lock, [&] { return generation != g; });
  }
};
struct Ctx { Group *g; int rank; };

int allreduce(void *ctx, void *buf, int64_t count, void *) {
  Ctx *c = (Ctx *)ctx;
  double *b = (double *)buf;
  c->g->slot[c->rank].assign(b, b + count);
  c->g->barrier();
  std::vector<double> sum(c->g->slot[0]);
  for (int r = 1; r < kWorld; ++r)
    for (int64_t i = 0; i < count; ++i) sum[(size_t)i] += c->g->slot[r][(size_t)i];     // rank order on every shard
  c->g->barrier();
  if (count > 0) std::memcpy(b, sum.data(), (size_t)count * sizeof(double));
  return 0;
}

int allgather(void *ctx, const void *send, void *recv, int64_t count, void *) {
  Ctx *c = (Ctx *)ctx;
  const double *s = (const double *)send;
  c->g->slot[c->rank].assign(s, s + count);
  c->g->barrier();
  for (int r = 0; r < kWorld && count > 0; ++r) std::memcpy((double *)recv + r * count, c->g->slot[r].data(), (size_t)count * sizeof(double));
  c->g->barrier();
  return 0;
}

int alltoallv(void *ctx, const void *send, const int64_t *sc, void *recv, const int64_t *rc, int32_t world, void *) {
  Ctx *c = (Ctx *)ctx;
  if (world != kWorld) return -1;
  int64_t ns = 0;
  for (int p = 0; p < kWorld; ++p) ns += sc[p];
  const double *s = (const double *)send;
  if (ns > 0) c->g->slot[c->rank].assign(s, s + ns); else c->g->slot[c->rank].clear();
  c->g->counts[c->rank].assign(sc, sc + kWorld);
  c->g->barrier();
  int bad = 0;
  int64_t o = 0;
  for (int p = 0; p < kWorld; ++p) {
    int64_t off = 0;
    for (int q = 0; q < c->rank; ++q) off += c->g->counts[p][(size_t)q];
    if (c->g->counts[p][(size_t)c->rank] != rc[p]) bad = 1;
    else if (rc[p] > 0) std::memcpy((double *)recv + o, c->g->slot[p].data() + off, (size_t)rc[p] * sizeof(double));
    o += rc[p];
  }
  c->g->barrier();
  return bad ? -1 : 0;
}

struct Result { int rc = 0; const char *where = ""; std::string text; double eps = 0.0; int64_t counters[4] = {0}; int64_t calls = 0, n_local = 0; };

void shard(Group *g, int rank, Result *res) {
  sabc_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.abi_version = SABC_ABI_VERSION;
  cfg.n_particles = kParticles;
  cfg.n_para = 1; cfg.n_stats = 1;
  cfg.model_id = SABC_MODEL_GAUSS_IID;
  cfg.n_model_params = 4;
  cfg.model_params[0] = 100.0; cfg.model_params[1] = 1.0; cfg.model_params[2] = 1.5;   // n_obs, sd, observed mean
  cfg.prior_kind[0] = SABC_PRIOR_NORMAL; cfg.prior_a[0] = 0.0; cfg.prior_b[0] = 2.0;
  cfg.algorithm = SABC_ALG_SINGLE_EPS;
  cfg.rank = rank; cfg.world = kWorld;
  cfg.v = 1.0; cfg.delta = 0.1; cfg.seed = 20241220u;
  sabc_handle *h = nullptr;
  Ctx ctx{g, rank};
  auto step = [&](const char *where, int rc) {
    if (rc && !res->rc) { res->rc = rc; res->where = where; res->text = h ? sabc_last_error(h) : sabc_last_global_error(); }
    return rc;
  };
  // a step that fails on one shard fails on both (same configuration, same words): nobody is left waiting in a hook
  if (step("sabc_create", sabc_create(&cfg, &h))) return;
  if (!step("sabc_set_collectives", sabc_set_collectives(h, allreduce, allgather, &ctx, /*device_buffers=*/0)) &&
      !step("sabc_set_alltoallv", sabc_set_alltoallv(h, alltoallv)) &&
      !step("sabc_comm_selftest", sabc_comm_selftest(h)) &&
      !step("sabc_initialize", sabc_initialize(h, (kUpdates + 1) * kParticles))) {
    sabc_update_args a;
    std::memset(&a, 0, sizeof(a));
    a.n_simulation = kParticles; a.v = 1.0; a.delta = 0.1; a.resample = (double)(kParticles / 4); a.checkpoint_history = 1;
    a.proposal_kind = SABC_PROP_DIFFEVO; a.proposal_p0 = 2.38 / 1.4142135623730951; a.proposal_p1 = 1e-5;
    for (int k = 0; k < kUpdates; ++k)
      if (step("sabc_update", sabc_update(h, &a))) break;
  }
  if (!res->rc) {
    int32_t len = 0;
    double eps[SABC_MAX_STATS];
    step("sabc_get_epsilon", sabc_get_epsilon(h, eps, &len));
    step("sabc_get_counters", sabc_get_counters(h, res->counters));
    res->eps = eps[0];
    res->calls = sabc_collective_calls(h);
    res->n_local = sabc_n_local(h);
  }
  sabc_destroy(h);
}

}  // namespace

int main() {
  Group g;
  Result res[kWorld];
  std::thread t[kWorld];
  for (int r = 0; r < kWorld; ++r) t[r] = std::thread(shard, &g, r, &res[r]);
  for (int r = 0; r < kWorld; ++r) t[r].join();
  int bad = 0;
  for (int r = 0; r < kWorld; ++r)
    if (res[r].rc) { std::printf("shard %d: %s returned %d: %s\n", r, res[r].where, res[r].rc, res[r].text.c_str()); bad = 1; }
  if (bad) return 1;
  // the control step runs on rank-ordered sums: bitwise the same state on both shards
  if (res[0].eps != res[1].eps || !(res[0].eps > 0.0) || std::memcmp(res[0].counters, res[1].counters, sizeof(res[0].counters)) != 0 ||
      res[0].counters[3] != kUpdates || res[0].n_local + res[1].n_local != kParticles || res[0].calls <= 0 || res[0].calls != res[1].calls) {
    std::printf("shards disagree: eps %.17g / %.17g, updates %lld / %lld, collective calls %lld / %lld\n", res[0].eps, res[1].eps,
                (long long)res[0].counters[3], (long long)res[1].counters[3], (long long)res[0].calls, (long long)res[1].calls);
    return 1;
  }
  std::printf("capi_probe ok: 2 shards (%lld + %lld), %d updates, %lld resamples, eps %.17g, %lld collective calls per shard\n",
              (long long)res[0].n_local, (long long)res[1].n_local, kUpdates, (long long)res[0].counters[2], res[0].eps,
              (long long)res[0].calls);
  return 0;
}
