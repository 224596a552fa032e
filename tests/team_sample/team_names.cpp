// team_names -- the kernel table of csrc/rtc.cpp for a team-aware unit, from a plain C++ program (tests/test_team_sample_host.py;
// built like tests/rtc_host/rtc_check.cpp, against rtc.cpp alone):
//   team_names D S WITH_PERSISTENT TEAM_AWARE       the name expressions of the unit's kernels, in table order
// TEAM_AWARE = 0 goes through the three-argument call every caller made before there were team-aware units.
#include <cstdio>
#include <cstdlib>

#include "../../simulatedannealingabc.jl_amd/csrc/rtc.hpp"

int main(int argc, char **argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: team_names D S WITH_PERSISTENT TEAM_AWARE\n");
    return 2;
  }
  const int d = std::atoi(argv[1]), s = std::atoi(argv[2]);
  const bool with_persistent = std::atoi(argv[3]) != 0;
  const std::vector<std::string> names =
      std::atoi(argv[4]) != 0 ? sabc::rtc_kernel_names(d, s, with_persistent, true) : sabc::rtc_kernel_names(d, s, with_persistent);
  for (const std::string &n : names) std::printf("%s\n", n.c_str());
  return 0;
}
