// rtc.hpp -- a simulator supplied as HIP source (SABC_MODEL_USER): compiled at run time with hipRTC into the same
// fused update kernel the built-in simulators use (update_kernel.hpp), loaded as a code-object module.
// rtc.cpp keeps ONE table of the unit's kernels (name expression and slot of RtcKernels, in the order code objects and cache
// files depend on), ONE loader of a code object for the three ways to one (this process's cache, the disk's, the compiler),
// and finds the headers whose text keys the disk cache by following the unit's #include "..." lines.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <string>
#include <vector>

namespace sabc {

// lanes per particle of the one-launch form (update_kernel.hpp, LANES): a lane, a quad, a row of the wave
constexpr int kPersistTeamLanes[3] = {1, 4, 16};
constexpr int persist_team(int lanes) { return (lanes >= kPersistTeamLanes[1]) + (lanes >= kPersistTeamLanes[2]); }

struct RtcKernels {
  hipModule_t module = nullptr;
  hipFunction_t prior_simulate = nullptr;      // k_prior_simulate<USER, D, S>
  hipFunction_t update[3] = {};                // k_update<USER, D, S, PROP>
  hipFunction_t simulate_batch = nullptr;      // k_simulate_batch<USER, D, S>
  hipFunction_t stats = nullptr;               // k_stats<D, S>
  hipFunction_t prior_op = nullptr;            // k_prior_op_t<D>
  hipFunction_t persistent[3][3] = {};         // [team][PROP]: k_update_persistent<USER, D, S, PROP, kPersistTeamLanes[team]> (persistent_kernel.hpp)
  // a team-aware unit only (RtcRequest::team_aware), [team - 1] = a quad | a row of 16 lanes per particle:
  hipFunction_t update_team[2][3] = {};        // [team - 1][PROP]: k_update_team<USER, D, S, PROP, kPersistTeamLanes[team]>
  hipFunction_t simulate_batch_team[2] = {};   // [team - 1]: k_simulate_batch_team<USER, D, S, kPersistTeamLanes[team]>
  bool team_aware = false;                     // the unit was compiled from a source that defines sabc_user_simulate_team<W>
  int chain_lanes = 1;                         // ... and its handle runs it with this many lanes per particle on the launch chain and in the
                                               // forward run (1 | 4 | 16; set by the backend at registration, not by rtc_compile)
};

// `source` must define
//     __device__ void sabc_user_simulate(const double *theta, const double *params, sabc::NormalStream &rng, double *rho_out);
// or, team_aware (the storage of sabc::Sample<N, W> depends on the lanes W = 1 | 4 | 16 that run a particle side by side, so the
// simulator gets W as a template argument instead of reading rng.coop),
//     template <int W> __device__ void sabc_user_simulate_team(const double *theta, const double *params, sabc::NormalStream &rng, double *rho_out);
// All lanes of a team see the same data and must make the same requests of rng and of a Sample, in the same order.  Such a unit
// also holds k_update_team and k_simulate_batch_team for 4 and 16 lanes (one compilation serves every choice of width); it has
// no wide form: s <= kNarrowStats.
// `csrc_dir` holds update_kernel.hpp and what it includes.
// user_prior: the source also defines sabc_user_prior_sample / sabc_user_prior_logpdf (sabc_config::prior_joint = 3).
// with_persistent: also compile k_update_persistent<USER, D, S, PROP, LANES> (small shards: the updates of a call in one launch;
// it multiplies the compile time, so only handles that can take the form ask for it; ignored where source_wide(s))
struct RtcRequest {
  const char *source = nullptr;
  int d = 0, s = 0;
  std::string csrc_dir;
  bool user_prior = false, with_persistent = false;
  bool team_aware = false;
};

// Compiles the request for gfx950 and loads its kernels into `out`.  Returns 0 or -1 with the compiler log / error text in `log`.
// out == nullptr stops after the compiler (no device needed): a syntax / interface check of a source.
// code_size (optional) receives the size of the code object.
int rtc_compile(const RtcRequest &request, RtcKernels *out, std::string *log, size_t *code_size = nullptr);
void rtc_release(RtcKernels *k);
// read-only views of what rtc_compile works from (tests/rtc_host): the name expressions of the unit's kernels in table order,
// and the files whose names and text the disk cache's key covers (hash, optional: what the key takes of them)
// team_aware: behind them, in this order, k_update_team for 4 lanes x three proposals, for 16 lanes x three proposals,
// k_simulate_batch_team for 4 and for 16 lanes
std::vector<std::string> rtc_kernel_names(int d, int s, bool with_persistent, bool team_aware = false);
std::vector<std::string> rtc_unit_headers(const std::string &csrc_dir, uint64_t *hash = nullptr);
// Observed data (sabc_set_device_data): every source-compiled unit defines one module-scope __constant__ variable of this
// layout ahead of the user's text (rtc.cpp: kDataPreamble, which declares the same struct to the device compiler); the
// backend writes it through hipModuleGetGlobal(rtc_data_symbol()).
struct RtcDataDesc {
  const double *base = nullptr;
  int32_t n_segments = 0, reserved = 0;
  long long off[8] = {0}, len[8] = {0};
};
const char *rtc_data_symbol();
// directory of this shared library + "/csrc" (the headers ship next to the library)
std::string rtc_default_csrc_dir();

}  // namespace sabc
