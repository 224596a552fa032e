// sabc::Series<128, W>::recur on its own, for tests/test_series_recur_isa.py: a team of W lanes fills the series from a counter
// that is a kernel argument (fill(g): no generator, so no LDS tables), runs cumsum(), then the AR(2) recurrence with a Carry<2>
// whose coefficients are kernel arguments, then sum().  The relay hands the state on with DPP moves alone: no LDS memory, no
// barrier, and the slots must not leave the registers.
#include "device_rng.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

template <int W>
__device__ __forceinline__ void probe(const uint64_t counter, const double phi1, const double phi2, const int64_t teams, double *__restrict__ out) {
  const int64_t team = ((int64_t)blockIdx.x * 256 + threadIdx.x) / W;
  if (team >= teams) return;                           // (uniform over a team)
  sabc::Series<128, W> x;
  x.fill([&](const int t) {
    const uint64_t c = (counter + (uint64_t)team * 128u + (uint64_t)t) * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(c >> 11) * 0x1p-52;
  });
  x.cumsum();
  const sabc::series::Carry<2> end = x.recur(sabc::series::Carry<2>{{0.25, -0.5}}, [&](const int, sabc::series::Carry<2> &s, const double v) {
    const double o = fma(phi1, s.v[0], fma(phi2, s.v[1], v));
    s.v[1] = s.v[0];
    s.v[0] = o;
    return o;
  });
  const double sum = x.sum();
  if ((threadIdx.x & (W - 1)) == 0) {
    out[3 * team] = sum;
    out[3 * team + 1] = end.v[0];
    out[3 * team + 2] = end.v[1];
  }
}

extern "C" __global__ void __launch_bounds__(256)
k_series_recur_probe_16(const uint64_t counter, const double phi1, const double phi2, const int64_t teams, double *__restrict__ out) {
  probe<16>(counter, phi1, phi2, teams, out);
}

extern "C" __global__ void __launch_bounds__(256)
k_series_recur_probe_4(const uint64_t counter, const double phi1, const double phi2, const int64_t teams, double *__restrict__ out) {
  probe<4>(counter, phi1, phi2, teams, out);
}
