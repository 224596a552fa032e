// rtc.cpp -- see rtc.hpp.  hipRTC is bound with dlopen at first use: a host without libhiprtc can still load the
// library and run the built-in simulators.
#include "rtc.hpp"

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/sabc_hip.h"
#include "kernels.hpp"

namespace sabc {

namespace {

struct HiprtcApi {
  void *lib = nullptr;
  int (*CreateProgram)(void **, const char *, const char *, int, const char **, const char **) = nullptr;
  int (*DestroyProgram)(void **) = nullptr;
  int (*CompileProgram)(void *, int, const char **) = nullptr;
  int (*GetProgramLogSize)(void *, size_t *) = nullptr;
  int (*GetProgramLog)(void *, char *) = nullptr;
  int (*GetCodeSize)(void *, size_t *) = nullptr;
  int (*GetCode)(void *, char *) = nullptr;
  int (*AddNameExpression)(void *, const char *) = nullptr;
  int (*GetLoweredName)(void *, const char *, const char **) = nullptr;
};

HiprtcApi *hiprtc_api() {
  static HiprtcApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    const char *names[] = {"libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"};
    for (const char *n : names) {
      api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
      if (api.lib) break;
    }
    if (api.lib) {
#define SABC_RTC_SYM(field, sym) api.field = (decltype(api.field))dlsym(api.lib, sym)
      SABC_RTC_SYM(CreateProgram, "hiprtcCreateProgram");
      SABC_RTC_SYM(DestroyProgram, "hiprtcDestroyProgram");
      SABC_RTC_SYM(CompileProgram, "hiprtcCompileProgram");
      SABC_RTC_SYM(GetProgramLogSize, "hiprtcGetProgramLogSize");
      SABC_RTC_SYM(GetProgramLog, "hiprtcGetProgramLog");
      SABC_RTC_SYM(GetCodeSize, "hiprtcGetCodeSize");
      SABC_RTC_SYM(GetCode, "hiprtcGetCode");
      SABC_RTC_SYM(AddNameExpression, "hiprtcAddNameExpression");
      SABC_RTC_SYM(GetLoweredName, "hiprtcGetLoweredName");
#undef SABC_RTC_SYM
    }
  });
  const bool ok = api.lib && api.CreateProgram && api.DestroyProgram && api.CompileProgram && api.GetProgramLogSize &&
                  api.GetProgramLog && api.GetCodeSize && api.GetCode && api.AddNameExpression && api.GetLoweredName;
  return ok ? &api : nullptr;
}

void anchor() {}

// compiled code objects of this process, keyed by (source, d, s): a second handle with the same simulator (every
// sabc() call makes one) loads the module without paying the ~2 s of compilation again
struct CachedModule {
  std::vector<char> code;
  std::vector<std::string> lowered;                    // one per entry of kernel_table()
};
std::mutex g_cache_mutex;
std::map<std::string, CachedModule> g_cache;

// ---- the same across processes: code objects on disk ----
// Compiling a simulator costs 2-5 s (the fused kernels with the user's code inlined, x 3 proposals, + the one-launch form of
// small shards) -- every sabc() of every process paid it again.  The code object and the kernels' lowered names are kept
// under $SABC_RTC_CACHE_DIR | $XDG_CACHE_HOME/sabc_hip | ~/.cache/sabc_hip, keyed by a hash of EVERYTHING that goes into the
// compilation: the in-process cache key (shape, flags, the user's source), the text of every header of csrc/ the unit
// includes (a rebuilt or different library never finds another one's code) and this library's ABI version.
// SABC_RTC_CACHE=0 switches it off.  A file that does not parse (truncated, foreign) is ignored and overwritten.
uint64_t fnv1a(const void *data, size_t n, uint64_t h) {
  const unsigned char *p = static_cast<const unsigned char *>(data);
  for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

// The headers of the unit are FOUND, not listed: from the two the unit names, every file an #include "..." line names, looked
// for next to the including file and then in csrc_dir; depth first in order of appearance, each file once, its name as written
// and then its text into the hash.  Conditionals are not evaluated: a superset of what the compiler reads (rtc.hpp comes in
// through kernels.hpp), never less -- text that moves into a new header is covered without anybody remembering a list.
// <...> includes (ROCm, the C++ library) are not followed.  A file that cannot be opened contributes its name only.
struct UnitHeaders {
  std::vector<std::string> paths;                      // in order of the visit
  std::vector<std::pair<dev_t, ino_t>> files;          // those that opened: each once, by whichever route it is reached
  uint64_t hash = 14695981039346656037ull;
};

void scan_header(const std::string &name, const std::string &from_dir, const std::string &csrc_dir, UnitHeaders *u) {
  std::string path = from_dir + "/" + name;
  FILE *fp = std::fopen(path.c_str(), "rb");
  if (!fp) { path = csrc_dir + "/" + name; fp = std::fopen(path.c_str(), "rb"); }
  struct stat st = {};
  if (fp) (void)::fstat(fileno(fp), &st);
  const std::pair<dev_t, ino_t> id(st.st_dev, st.st_ino);
  if (fp ? std::count(u->files.begin(), u->files.end(), id) : std::count(u->paths.begin(), u->paths.end(), path)) {
    if (fp) std::fclose(fp);
    return;
  }
  u->paths.push_back(path);
  u->hash = fnv1a(name.data(), name.size(), u->hash);
  if (!fp) return;
  u->files.push_back(id);
  std::string text((size_t)st.st_size, '\0');
  text.resize(std::fread(&text[0], 1, text.size(), fp));
  std::fclose(fp);
  u->hash = fnv1a(text.data(), text.size(), u->hash);
  const std::string dir = path.substr(0, path.rfind('/'));
  const auto blank = [&](size_t i) { return text[i] == ' ' || text[i] == '\t'; };
  for (size_t at = text.find('#'); at != std::string::npos; at = text.find('#', at + 1)) {
    size_t i = at;                                     // # include "name", with nothing but blanks ahead of it on its line
    while (i > 0 && blank(i - 1)) --i;
    if (i > 0 && text[i - 1] != '\n') continue;
    size_t q = text.find_first_not_of(" \t", at + 1);
    if (q == std::string::npos || text.compare(q, 7, "include") != 0) continue;
    q = text.find_first_not_of(" \t", q + 7);
    const size_t e = q == std::string::npos ? q : text.find_first_of("\"\n", q + 1);
    if (e != std::string::npos && text[q] == '"' && text[e] == '"') scan_header(text.substr(q + 1, e - q - 1), dir, csrc_dir, u);
  }
}

const UnitHeaders &unit_headers(const std::string &csrc_dir) {
  static std::mutex m;
  static std::map<std::string, UnitHeaders> memo;
  std::lock_guard<std::mutex> lock(m);
  auto hit = memo.find(csrc_dir);
  if (hit != memo.end()) return hit->second;
  UnitHeaders u;
  for (const char *root : {"update_kernel.hpp", "persistent_kernel.hpp"}) scan_header(root, csrc_dir, csrc_dir, &u);
  return memo.emplace(csrc_dir, std::move(u)).first->second;
}

std::string disk_cache_dir() {
  if (const char *e = std::getenv("SABC_RTC_CACHE")) { if (e[0] == '0') return std::string(); }
  std::string dir;
  if (const char *e = std::getenv("SABC_RTC_CACHE_DIR")) dir = e;
  else if (const char *x = std::getenv("XDG_CACHE_HOME")) dir = std::string(x) + "/sabc_hip";
  else if (const char *home = std::getenv("HOME")) dir = std::string(home) + "/.cache/sabc_hip";
  if (dir.empty()) return dir;
  for (size_t i = 1; i <= dir.size(); ++i)             // mkdir -p
    if (i == dir.size() || dir[i] == '/') (void)::mkdir(dir.substr(0, i).c_str(), 0700);
  return dir;
}

std::string disk_cache_path(const std::string &cache_key, const std::string &csrc_dir) {
  const std::string dir = disk_cache_dir();
  if (dir.empty()) return dir;
  uint64_t h = fnv1a(cache_key.data(), cache_key.size(), 14695981039346656037ull);
  const uint64_t hh = unit_headers(csrc_dir).hash;
  const int abi = SABC_ABI_VERSION;
  h = fnv1a(&hh, sizeof(hh), h);
  h = fnv1a(&abi, sizeof(abi), h);
  uint64_t h2 = fnv1a(cache_key.data(), cache_key.size(), 0x9E3779B97F4A7C15ull ^ hh);      // 128 bits in the name
  char name[64];
  std::snprintf(name, sizeof(name), "/%016llx%016llx.sabcrtc", (unsigned long long)h, (unsigned long long)h2);
  return dir + name;
}

constexpr uint64_t kDiskMagic = 0x5341424352544331ull;   // "SABCRTC1"

bool disk_cache_load(const std::string &path, int n_kernels, CachedModule *out) {
  FILE *fp = std::fopen(path.c_str(), "rb");
  if (!fp) return false;
  bool ok = false;
  uint64_t head[3] = {0, 0, 0};                        // magic, kernels, code bytes
  out->lowered.assign((size_t)n_kernels, std::string());
  if (std::fread(head, sizeof(head), 1, fp) == 1 && head[0] == kDiskMagic && head[1] == (uint64_t)n_kernels && head[2] > 0 &&
      head[2] < ((uint64_t)1 << 30)) {
    ok = true;
    for (int i = 0; ok && i < n_kernels; ++i) {
      uint32_t len = 0;
      ok = std::fread(&len, sizeof(len), 1, fp) == 1 && len > 0 && len < 4096;
      if (ok) { out->lowered[i].assign(len, '\0'); ok = std::fread(&out->lowered[i][0], 1, len, fp) == len; }
    }
    if (ok) { out->code.resize((size_t)head[2]); ok = std::fread(out->code.data(), 1, out->code.size(), fp) == out->code.size(); }
    uint64_t tail = 0;                                 // the file was written to its end
    ok = ok && std::fread(&tail, sizeof(tail), 1, fp) == 1 && tail == (kDiskMagic ^ head[2]);
  }
  std::fclose(fp);
  return ok;
}

void disk_cache_store(const std::string &path, const CachedModule &m) {
  char tmp[32];
  std::snprintf(tmp, sizeof(tmp), ".%d.tmp", (int)getpid());
  const std::string t = path + tmp;
  FILE *fp = std::fopen(t.c_str(), "wb");
  if (!fp) return;
  const uint64_t head[3] = {kDiskMagic, (uint64_t)m.lowered.size(), (uint64_t)m.code.size()};
  bool ok = std::fwrite(head, sizeof(head), 1, fp) == 1;
  for (const std::string &name : m.lowered) {
    const uint32_t len = (uint32_t)name.size();
    ok = ok && std::fwrite(&len, sizeof(len), 1, fp) == 1 && std::fwrite(name.data(), 1, len, fp) == len;
  }
  ok = ok && std::fwrite(m.code.data(), 1, m.code.size(), fp) == m.code.size();
  const uint64_t tail = kDiskMagic ^ head[2];
  ok = ok && std::fwrite(&tail, sizeof(tail), 1, fp) == 1;
  ok = (std::fclose(fp) == 0) && ok;
  if (ok) ok = std::rename(t.c_str(), path.c_str()) == 0;       // (a reader never sees a partial file)
  if (!ok) (void)std::remove(t.c_str());
}

// ---- observed data (sabc_set_device_data): what every source-compiled unit sees ahead of the user's text ----
// The carrier is ONE module-scope __constant__ variable, sabc_data_desc (struct RtcDataDesc of rtc.hpp): base pointer, segment
// count, offsets and lengths.  HipBackend writes it through hipModuleGetGlobal after each module load and after each
// sabc_set_device_data; every handle loads a module of its own, so every handle has a descriptor of its own.  No kernel
// signature changes, and all sixteen kernels of the unit -- and the user's prior functions -- read it.
// This text is part of the cache key below (in memory and, through it, on disk): a code object compiled before the symbols
// existed, or with another layout of the descriptor, is never loaded in place of this one.
const char kDataPreamble[] = R"SABC(
struct SabcDataDesc {
  const double *base;
  int n_segments, reserved;
  long long off[8], len[8];
};
extern "C" { __constant__ SabcDataDesc sabc_data_desc = {}; }
namespace sabc {
__device__ __forceinline__ int data_segments() { return sabc_data_desc.n_segments; }
__device__ __forceinline__ long long data_len(int segment = 0) { return sabc_data_desc.len[segment]; }
__device__ __forceinline__ const double *data(int segment = 0) {
  return sabc_data_desc.base ? sabc_data_desc.base + sabc_data_desc.off[segment] : nullptr;
}
// The read goes through the constant address space.  The data are immutable during a launch: they are replaced only on an
// idle handle (sabc_set_device_data synchronises the stream first), so no kernel runs while they change.  A later launch may
// find the new values at the old address (a set of the same length reuses the allocation): what keeps the scalar cache from
// serving the old ones there is the cache invalidation every kernel dispatch begins with (its acquire), not the host's
// synchronise.  An index that is uniform in the wave becomes a scalar load (one per wave), a divergent one a global vector load.
__device__ __forceinline__ double data_at(long long i, int segment = 0) {
  typedef const double __attribute__((address_space(4))) *const_ptr;
  return ((const_ptr)(sabc_data_desc.base + sabc_data_desc.off[segment]))[i];
}
}  // namespace sabc
// The simulator is the body of every kernel's loop over particles: it is inlined wherever it is called, whatever its size.
// Left to the inliner's cost estimate, a simulator near the threshold becomes a CALL when the estimate moves -- a member more
// in NormalStream did that to normal_moments.hip: the stream in scratch (192 bytes), 132 instead of 71 registers in k_update --
// and only then can what depends on the stream's constants (its coop mode; a null destination of sabc::emit) be folded away.
// The definition in the user's text inherits the attribute from this declaration.
__device__ __attribute__((always_inline)) void sabc_user_simulate(const double *theta, const double *params,
                                                                  sabc::NormalStream &rng, double *rho_out);
)SABC";

// ... and behind it: the simulator the kernel templates of the unit are instantiated with
const char kUserSimTail[] = R"SABC(
namespace sabc {
template <int D, int S>
struct Sim<SABC_MODEL_USER, D, S> {
  static __device__ __forceinline__ void run(const ModelDesc &m, const double *th, uint64_t pid, uint64_t iter,
                                             double *rho, int coop = 0) {
    NormalStream ns(m.seed, pid, PURPOSE_SIM, iter, coop);
    ::sabc_user_simulate(th, m.p, ns, rho);
  }
  // the forward run (k_simulate_batch with an output buffer): a lane per simulation, the stream of `purpose`, and on it the
  // destination of sabc::emit -- output i of this simulation at out[i * stride]
  static __device__ __forceinline__ void run_out(const ModelDesc &m, const double *th, uint64_t pid, uint32_t purpose,
                                                 uint64_t iter, double *rho, double *out, long long stride, long long n_out) {
    NormalStream ns(m.seed, pid, purpose, iter, 0);
    ns.set_outputs(out, stride, n_out);
    ::sabc_user_simulate(th, m.p, ns, rho);
  }
};
}  // namespace sabc
)SABC";

// ---- a team-aware source (RtcRequest::team_aware): the entry point is a template over the lanes that run the particle ----
// Declared in place of sabc_user_simulate, with the same attribute for the same reason; Sim dispatches on its coop, which is a
// constant after inlining in every kernel (0 and kCoopPlainLoop: a lane per particle), so each kernel keeps one instantiation.
const char kTeamDecl[] = R"SABC(
template <int W>
__device__ __attribute__((always_inline)) void sabc_user_simulate_team(const double *theta, const double *params,
                                                                       sabc::NormalStream &rng, double *rho_out);
)SABC";

const char kTeamSimTail[] = R"SABC(
namespace sabc {
template <int D, int S>
struct Sim<SABC_MODEL_USER, D, S> {
  static __device__ __forceinline__ void dispatch(const double *th, const double *p, NormalStream &ns, double *rho) {
    if (ns.coop == 16) ::sabc_user_simulate_team<16>(th, p, ns, rho);
    else if (ns.coop == 4) ::sabc_user_simulate_team<4>(th, p, ns, rho);
    else ::sabc_user_simulate_team<1>(th, p, ns, rho);
  }
  static __device__ __forceinline__ void run(const ModelDesc &m, const double *th, uint64_t pid, uint64_t iter,
                                             double *rho, int coop = 0) {
    NormalStream ns(m.seed, pid, PURPOSE_SIM, iter, coop);
    dispatch(th, m.p, ns, rho);
  }
  // the forward run: the stream of `purpose` with the destination of sabc::emit on it; coop = 4 | 16: k_simulate_batch_team
  static __device__ __forceinline__ void run_out(const ModelDesc &m, const double *th, uint64_t pid, uint32_t purpose,
                                                 uint64_t iter, double *rho, double *out, long long stride, long long n_out,
                                                 int coop = 0) {
    NormalStream ns(m.seed, pid, purpose, iter, coop);
    ns.set_outputs(out, stride, n_out);
    dispatch(th, m.p, ns, rho);
  }
};
}  // namespace sabc
)SABC";

// ---- the kernels of a unit: THE table ----
// Name expression (what hipRTC instantiates) and slot of `k` per kernel.  Everything that walks the kernels -- the name
// expressions, the lowered names of a cached module, the resolution of the slots, their number -- walks this, in this order;
// cache files and code objects depend on it.  More than kNarrowStats statistics: the wide kernels in the slots of the narrow
// ones and the launch chain only (persistent_fits is false there).  A team-aware unit APPENDS k_update_team for 4 lanes x three
// proposals, for 16 lanes x three proposals, then k_simulate_batch_team for 4 and for 16 lanes; every other unit's table is
// what it was.
struct KernelEntry {
  std::string name;
  hipFunction_t *slot;
};

bool one_launch(int s, bool with_persistent) { return with_persistent && !source_wide(s); }

std::vector<KernelEntry> kernel_table(int d, int s, bool with_persistent, RtcKernels *k, bool team_aware = false) {
  const std::string w = source_wide(s) ? "_wide" : "", ds = std::to_string(d) + ", " + std::to_string(s);
  const std::string mds = std::to_string((int)SABC_MODEL_USER) + ", " + ds;
  std::vector<KernelEntry> t;
  t.push_back({"sabc::k_prior_simulate" + w + "<" + mds + ">", &k->prior_simulate});
  for (int p = 0; p < 3; ++p) t.push_back({"sabc::k_update" + w + "<" + mds + ", " + std::to_string(p) + ">", &k->update[p]});
  t.push_back({"sabc::k_simulate_batch" + w + "<" + mds + ">", &k->simulate_batch});
  t.push_back({"sabc::k_stats" + w + "<" + ds + ">", &k->stats});
  t.push_back({"sabc::k_prior_op_t<" + std::to_string(d) + ">", &k->prior_op});
  if (one_launch(s, with_persistent))
    for (int team = 0; team < 3; ++team) {             // (a lane per particle is the template's default: named without it, as ever)
      const std::string lanes = team ? ", " + std::to_string(kPersistTeamLanes[team]) : "";
      for (int p = 0; p < 3; ++p)
        t.push_back({"sabc::k_update_persistent<" + mds + ", " + std::to_string(p) + lanes + ">", &k->persistent[team][p]});
    }
  if (team_aware && !source_wide(s)) {
    for (int team = 1; team < 3; ++team)
      for (int p = 0; p < 3; ++p)
        t.push_back({"sabc::k_update_team<" + mds + ", " + std::to_string(p) + ", " + std::to_string(kPersistTeamLanes[team]) + ">", &k->update_team[team - 1][p]});
    for (int team = 1; team < 3; ++team)
      t.push_back({"sabc::k_simulate_batch_team<" + mds + ", " + std::to_string(kPersistTeamLanes[team]) + ">", &k->simulate_batch_team[team - 1]});
  }
  return t;
}

// a code object into a module of its own with every slot of the table resolved, or nothing loaded and the reason in `log`
bool load_kernels(const CachedModule &m, const RtcRequest &rq, RtcKernels *out, std::string *log) {
  RtcKernels k;
  if (hipModuleLoadData(&k.module, m.code.data()) != hipSuccess) { *log = "hipModuleLoadData of the simulator's code object failed"; return false; }
  const std::vector<KernelEntry> table = kernel_table(rq.d, rq.s, rq.with_persistent, &k, rq.team_aware);
  k.team_aware = rq.team_aware;
  for (size_t i = 0; i < table.size(); ++i)
    if (i >= m.lowered.size() || hipModuleGetFunction(table[i].slot, k.module, m.lowered[i].c_str()) != hipSuccess) {
      *log = "kernel not found in the simulator's module: " + table[i].name;
      rtc_release(&k);
      return false;
    }
  *out = k;
  return true;
}

// The launch geometry the host library was built with (launch_update, build_coarse) must be the one the kernels are compiled
// for: a variant library (tools/build_variants.sh) forwards its -D overrides to the run-time compiler.  The same strings are
// part of the cache key: a variant library must not find another's code.
#define SABC_RTC_STR2(x) #x
#define SABC_RTC_STR(x) SABC_RTC_STR2(x)
#define SABC_RTC_DEFINE(x) "-D" #x "=" SABC_RTC_STR(x)
const char *const kGeometry[6] = {SABC_RTC_DEFINE(SABC_UPDATE_BLOCK),  SABC_RTC_DEFINE(SABC_UPDATE_BLOCK_MS),  SABC_RTC_DEFINE(SABC_CDF_COARSE),
                                  SABC_RTC_DEFINE(SABC_CDF_COARSE_MS), SABC_RTC_DEFINE(SABC_UPDATE_MIN_WAVES), SABC_RTC_DEFINE(SABC_UPDATE_MIN_WAVES_MS)};
#undef SABC_RTC_DEFINE
#undef SABC_RTC_STR
#undef SABC_RTC_STR2

struct Program {                                       // the hipRTC program, destroyed on every way out
  HiprtcApi *api;
  void *p = nullptr;
  ~Program() { if (p) api->DestroyProgram(&p); }
};

}  // namespace

const char *rtc_data_symbol() { return "sabc_data_desc"; }

std::string rtc_default_csrc_dir() {
  Dl_info info;
  if (dladdr((void *)&anchor, &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    const size_t slash = p.rfind('/');
    return (slash == std::string::npos ? std::string(".") : p.substr(0, slash)) + "/csrc";
  }
  return "csrc";
}

void rtc_release(RtcKernels *k) {
  if (k && k->module) (void)hipModuleUnload(k->module);
  if (k) *k = RtcKernels();
}

std::vector<std::string> rtc_kernel_names(int d, int s, bool with_persistent, bool team_aware) {
  RtcKernels unused;
  std::vector<std::string> names;
  for (const KernelEntry &e : kernel_table(d, s, with_persistent, &unused, team_aware)) names.push_back(e.name);
  return names;
}

std::vector<std::string> rtc_unit_headers(const std::string &csrc_dir, uint64_t *hash) {
  const UnitHeaders &u = unit_headers(csrc_dir);
  if (hash) *hash = u.hash;
  return u.paths;
}

int rtc_compile(const RtcRequest &rq, RtcKernels *out, std::string *log, size_t *code_size) {
  HiprtcApi *api = hiprtc_api();
  if (!api) { *log = "libhiprtc.so could not be loaded: simulators from source need the hipRTC of ROCm"; return -1; }
  if (rq.d < 1 || rq.d > SABC_MAX_PARA || rq.s < 1 || rq.s > SABC_MAX_SOURCE_STATS) { *log = "n_para / n_stats out of range (a simulator from source: d <= 16, s <= 64)"; return -1; }
  if (rq.team_aware && source_wide(rq.s)) {
    *log = "a team-aware simulator (sabc_user_simulate_team<W>) has no wide form: n_stats <= 16 (the kernels for 16 < n_stats <= 64 run a lane per particle)";
    return -1;
  }
  const bool persistent = one_launch(rq.s, rq.with_persistent);
  std::string src = std::string("#include \"update_kernel.hpp\"\n") + (persistent ? "#include \"persistent_kernel.hpp\"\n" : "") + kDataPreamble +
                    (rq.team_aware ? kTeamDecl : "") + "#line 1 \"f_dist.hip\"\n";
  src += rq.source;
  src += rq.team_aware ? kTeamSimTail : kUserSimTail;
  RtcKernels unused;
  const std::vector<KernelEntry> table = kernel_table(rq.d, rq.s, persistent, &unused, rq.team_aware);
  // extra compiler flags (e.g. -DSABC_NO_BITOP3: the two-instruction form of the Philox round's three-input XOR)
  const char *extra_env = std::getenv("SABC_RTC_EXTRA_FLAGS");
  const std::string extra = extra_env ? extra_env : "";
  std::string cache_key = std::to_string(rq.d) + "," + std::to_string(rq.s) + (rq.user_prior ? ",P" : "") + (persistent ? ",1L4L16" : "") + "," + extra;
  for (const char *g : kGeometry) cache_key += std::string(",") + g;
  if (rq.team_aware) cache_key += std::string(",TEAM\n") + kTeamDecl + "\n" + kTeamSimTail;   // (a plain unit's key is what it was)
  cache_key += std::string("\n") + kDataPreamble + "\n" + kUserSimTail + "\n" + rq.source;

  if (out) {                                           // this process has compiled it: a failure here is an error
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    auto hit = g_cache.find(cache_key);
    if (hit != g_cache.end()) {
      if (!load_kernels(hit->second, rq, out, log)) return -1;
      if (code_size) *code_size = hit->second.code.size();
      return 0;
    }
  }
  const std::string disk_path = out ? disk_cache_path(cache_key, rq.csrc_dir) : std::string();
  CachedModule entry;
  if (!disk_path.empty() && disk_cache_load(disk_path, (int)table.size(), &entry)) {
    std::string refused;
    if (load_kernels(entry, rq, out, &refused)) {
      if (code_size) *code_size = entry.code.size();
      std::lock_guard<std::mutex> lock(g_cache_mutex);
      g_cache.emplace(cache_key, std::move(entry));
      return 0;
    }
    (void)hipGetLastError();                           // a code object this device does not take: compile afresh, overwrite
  }

  Program prog{api};
  if (api->CreateProgram(&prog.p, src.c_str(), "sabc_user_simulator.hip", 0, nullptr, nullptr)) { *log = "hiprtcCreateProgram failed"; return -1; }
  for (const KernelEntry &e : table) api->AddNameExpression(prog.p, e.name.c_str());
  const char *rocm = std::getenv("ROCM_PATH");
  const std::string inc_rocm = std::string("-I") + (rocm && *rocm ? rocm : "/opt/rocm") + "/include";
  const std::string inc_csrc = "-I" + rq.csrc_dir;
  std::vector<const char *> opts = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", inc_csrc.c_str(), inc_rocm.c_str()};
  opts.insert(opts.end(), std::begin(kGeometry), std::end(kGeometry));
  if (rq.user_prior) opts.push_back("-DSABC_USER_PRIOR=1");
  std::vector<std::string> extra_words;
  for (size_t i = 0; i < extra.size();) {
    while (i < extra.size() && extra[i] == ' ') ++i;
    size_t j = i;
    while (j < extra.size() && extra[j] != ' ') ++j;
    if (j > i) extra_words.push_back(extra.substr(i, j - i));
    i = j;
  }
  for (const std::string &w : extra_words) opts.push_back(w.c_str());
  const int rc = api->CompileProgram(prog.p, (int)opts.size(), opts.data());
  size_t ls = 0;
  api->GetProgramLogSize(prog.p, &ls);
  if (ls > 1) { log->assign(ls, '\0'); api->GetProgramLog(prog.p, &(*log)[0]); }
  if (rc) {
    if (log->empty()) *log = "hiprtcCompileProgram failed";
    return -1;
  }
  size_t cs = 0;
  api->GetCodeSize(prog.p, &cs);
  if (code_size) *code_size = cs;
  entry.code.resize(cs);
  api->GetCode(prog.p, entry.code.data());
  // $SABC_RTC_CODE_OUT, compile only: the code object is also written to that file (its metadata -- registers, LDS, scratch --
  // can be read there without a device: tests/test_source_many_stats.py)
  const char *dump = out ? nullptr : std::getenv("SABC_RTC_CODE_OUT");
  if (dump) {
    FILE *fp = std::fopen(dump, "wb");
    const bool ok = fp && std::fwrite(entry.code.data(), 1, cs, fp) == cs;
    if (fp) std::fclose(fp);
    if (!ok) { *log = std::string("could not write the code object to ") + dump; return -1; }
  }
  entry.lowered.clear();
  for (const KernelEntry &e : table) {                 // every kernel must be there by name
    const char *lowered = nullptr;
    if (api->GetLoweredName(prog.p, e.name.c_str(), &lowered) || !lowered) { *log = "kernel missing from the compiled module: " + e.name; return -1; }
    entry.lowered.push_back(lowered);
  }
  if (!out) return 0;                                  // the compile-only check ends here
  if (!load_kernels(entry, rq, out, log)) return -1;
  if (!disk_path.empty()) disk_cache_store(disk_path, entry);
  std::lock_guard<std::mutex> lock(g_cache_mutex);
  g_cache.emplace(cache_key, std::move(entry));
  return 0;
}

}  // namespace sabc
