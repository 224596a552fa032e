// rtc_check -- the host side of csrc/rtc.cpp from a plain C++ program, no device needed (tests/test_rtc_host.py):
//   rtc_check headers CSRC_DIR                      the hash of the unit's headers, then the files it covers, one per line
//   rtc_check names D S WITH_PERSISTENT             the name expressions of the unit's kernels, in table order
//   rtc_check compile CSRC_DIR D S PRIOR WITH_PERSISTENT SOURCE_FILE [TEAM_AWARE]      the compiler stage alone ($SABC_RTC_CODE_OUT keeps
//                                                   the code object); TEAM_AWARE 1: a source that defines sabc_user_simulate_team<W>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../simulatedannealingabc.jl_amd/csrc/rtc.hpp"

int main(int argc, char **argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "headers" && argc == 3) {
    uint64_t hash = 0;
    const std::vector<std::string> paths = sabc::rtc_unit_headers(argv[2], &hash);
    std::printf("%016llx\n", (unsigned long long)hash);
    for (const std::string &p : paths) std::printf("%s\n", p.c_str());
    return 0;
  }
  if (cmd == "names" && argc == 5) {
    for (const std::string &n : sabc::rtc_kernel_names(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]) != 0)) std::printf("%s\n", n.c_str());
    return 0;
  }
  if (cmd == "compile" && (argc == 8 || argc == 9)) {
    std::ifstream in(argv[7]);
    std::stringstream text;
    text << in.rdbuf();
    const std::string source = text.str();
    const sabc::RtcRequest rq{source.c_str(), std::atoi(argv[3]), std::atoi(argv[4]), argv[2], std::atoi(argv[5]) != 0, std::atoi(argv[6]) != 0,
                               argc == 9 && std::atoi(argv[8]) != 0};
    std::string log;
    size_t code_size = 0;
    const int rc = sabc::rtc_compile(rq, nullptr, &log, &code_size);
    std::printf("rc %d, code object %zu bytes\n%s\n", rc, code_size, log.c_str());
    return rc ? 1 : 0;
  }
  std::fprintf(stderr, "usage: rtc_check headers CSRC_DIR | names D S WITH_PERSISTENT | compile CSRC_DIR D S PRIOR WITH_PERSISTENT SOURCE_FILE [TEAM_AWARE]\n");
  return 2;
}
