// cdf_kernel.hpp -- K2 and K3: the ECDF knots, their index levels and the column gather of the build, and u = cdf(rho) over
// the shard.  Device code only, included by kernels.hip alone; the launchers are in kernels.hip.
#pragma once
#include "update_kernel.hpp"

namespace sabc {

// K3 over the shard: u = cdf(rho)  (:190-192)
__global__ void __launch_bounds__(kBlock) k_cdf_population(const int d, const int s, const PopPtrs pp, const CdfPtrs cdf) {
  const int64_t li = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (li >= pp.n_local) return;
  // mid level (every 16th knot, L2-resident) -> one line of the table: same rank as the plain search, ~7 instead of ~20
  // distinct lines per lookup
  for (int j = 0; j < s; ++j)
    pp.pop[(int64_t)(d + j) * pp.cap + li] = cdf_apply_mid(cdf.knots + (int64_t)j * cdf.stride, cdf.len[j],
                                                           cdf.mid + (int64_t)j * cdf.mid_stride, pp.rho[(int64_t)j * pp.cap + li]);
}

// ------------------------------------------------------------------------------------------
// K2: ECDF knots from a sorted column (cdf_estimators.jl:29-33)
// ------------------------------------------------------------------------------------------
__global__ void k_cdf_meta(const double *__restrict__ sorted, const int64_t n, int64_t *__restrict__ meta) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t lo = 0, hi = n;             // first index with sorted[i] > 0
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (sorted[mid] > 0.0) hi = mid; else lo = mid + 1;
  }
  meta[0] = lo;
  meta[1] = (n > 0 && sorted[0] < 0.0) ? 1 : 0;
}

__global__ void __launch_bounds__(kBlock)
k_cdf_fill(const double *__restrict__ sorted, const int64_t n, const int64_t *__restrict__ meta,
           double *__restrict__ knots) {
  const int64_t z = meta[0], mpos = n - z;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < mpos) knots[1 + i] = sorted[z + i];
  if (i == 0) {
    knots[0] = 0.0;
    if (mpos > 0) knots[mpos + 1] = sorted[n - 1] * 1.5;
  }
}

__global__ void __launch_bounds__(kBlock)
k_cdf_index(double *__restrict__ knots, const int64_t len, const int64_t stride, const int shift, double *__restrict__ coarse,
            const int n_coarse, double *__restrict__ mid, const int64_t mid_len) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k < n_coarse) {
    const int64_t p = k << shift;
    coarse[k] = p < len ? knots[p] : INFINITY;
  }
  if (k < mid_len) {
    const int64_t p = k << kCdfLineShift;
    mid[k] = p < len ? knots[p] : INFINITY;
  }
  if (len + k < stride) knots[len + k] = INFINITY;       // the searches read up to 15 knots past the last one
}

__global__ void __launch_bounds__(kBlock)
k_compact_column(const ShardBlocks g, const int stat, const int64_t n, double *__restrict__ out) {
  const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (gid >= n) return;
  int64_t r, o;
  split_index(gid, g.cap, r, o);
  out[gid] = shard_block(g, r)[(int64_t)stat * g.cap + o];
}

}  // namespace sabc
