// sabc::SampleF32<128, W> on its own, for tests/test_team_sample_f32_isa.py: tests/team_sample/team_sort_probe.hip with the
// binary32 sample -- a team of W lanes fills it from a counter that is a kernel argument (nothing folds away), sorts it and reads
// ONE quantile whose probability is a kernel argument, a rank the compiler cannot know.  The fill is the f64 probe's generator with
// its top 24 bits as the value (the f64 probe converts 53), so the difference in registers and instructions is the sample's.
#include "device_rng.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

template <int W>
__device__ __forceinline__ void probe(const uint64_t counter, const double p, const int64_t teams, double *__restrict__ out) {
  const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) / W;
  if (t >= teams) return;                              // (uniform over a team)
  sabc::SampleF32<128, W> x;
  x.fill([&](const int i) {
    const uint64_t c = (counter + (uint64_t)t * 128u + (uint64_t)i) * 6364136223846793005ull + 1442695040888963407ull;
    return (float)(int32_t)(c >> 40);                 // 24 bits: exact in binary32, one v_cvt_f32_i32
  });
  x.sort();
  const double q = x.quantile(p);
  if ((threadIdx.x & (W - 1)) == 0) out[t] = q;
}

extern "C" __global__ void __launch_bounds__(256)
k_team_sort_probe_f32_16(const uint64_t counter, const double p, const int64_t teams, double *__restrict__ out) {
  probe<16>(counter, p, teams, out);
}

extern "C" __global__ void __launch_bounds__(256)
k_team_sort_probe_f32_4(const uint64_t counter, const double p, const int64_t teams, double *__restrict__ out) {
  probe<4>(counter, p, teams, out);
}
