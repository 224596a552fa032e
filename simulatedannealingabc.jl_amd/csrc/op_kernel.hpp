// op_kernel.hpp -- the kernels behind the operators exposed on their own (sabc_op_*) and the generator's debug / peak-rate
// kernels.  Device code only, included by kernels.hip alone; the launchers are in kernels.hip.
#pragma once
#include "hostmode_kernel.hpp"

namespace sabc {

// ------------------------------------------------------------------------------------------
// operators exposed on their own
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_cdf_eval(const double *__restrict__ knots, const int64_t len, const double *__restrict__ q, const int64_t m,
           double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < m) out[i] = cdf_apply(knots, len, q[i]);
}

__global__ void __launch_bounds__(kBlock)
k_cdf_apply_matrix(const CdfPtrs cdf, const int s, const double *__restrict__ rho, const int64_t m,
                   double *__restrict__ u) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  for (int j = 0; j < s; ++j)
    u[(int64_t)j * m + i] = cdf_apply(cdf.knots + (int64_t)j * cdf.stride, cdf.len[j], rho[(int64_t)j * m + i]);
}

// rand(prior) and its log density for particle ids pid0.. (sabc_op_prior)
__global__ void __launch_bounds__(kBlock)
k_prior_op(const ModelDesc m, const uint64_t pid0, const int64_t n, double *__restrict__ theta, double *__restrict__ lp) {
  rng_tables_init();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double th[kMaxPara];
  if (m.prior_joint) mvnormal_sample(m, m.d, pid0 + (uint64_t)i, th);
  else
    for (int k = 0; k < m.d; ++k) th[k] = prior_sample_dim(m, k, pid0 + (uint64_t)i);
  for (int k = 0; k < m.d; ++k) theta[(int64_t)k * n + i] = th[k];
  lp[i] = prior_logpdf_rt(m, th);
}

__global__ void k_philox_debug(uint64_t seed, uint64_t pid, uint32_t purpose, uint64_t iter, uint32_t k,
                               uint32_t *words, double *normals) {
  rng_tables_init();
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const u32x4 w = stream_block(seed, pid, purpose, iter, k);
  words[0] = w.x; words[1] = w.y; words[2] = w.z; words[3] = w.w;
  box_muller(w, normals[0], normals[1]);
}

// Pure generator loop: `pairs` Philox blocks + Box-Muller pairs per lane, nothing else (one store at the
// end keeps it alive).  Its rate is the VALU ceiling for any simulator that consumes normals from this
// generator; bench.py quotes k_update's in-kernel normal rate against it.
__global__ void __launch_bounds__(kBlock)
k_rng_peak(const uint64_t seed, const int pairs, const int64_t n, double *__restrict__ out) {
  rng_tables_init();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double acc = 0.0;
  NormalStream ns(seed, (uint64_t)i, PURPOSE_SIM, 0);      // the simulators' own loop (for_pairs), not a copy of it
  ns.for_pairs(pairs, [&](const double z0, const double z1) {
    acc += z0;
    acc += z1;
  });
  out[i] = acc;
}

__global__ void __launch_bounds__(kBlock)
k_normal_pairs(uint64_t seed, uint64_t pid0, uint32_t purpose, uint64_t iter, uint32_t k, int64_t m, double *out) {
  rng_tables_init();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  double z0, z1;
  box_muller(stream_block(seed, pid0 + (uint64_t)i, purpose, iter, k), z0, z1);
  out[2 * i] = z0;
  out[2 * i + 1] = z1;
}

// the binary32 twins: the four normals of block k per particle (sabc_op_normal_quads_f32) ...
__global__ void __launch_bounds__(kBlock)
k_normal_quads_f32(uint64_t seed, uint64_t pid0, uint32_t purpose, uint64_t iter, uint32_t k, int64_t m, float *out) {
  rng_tables_init();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  float z0, z1, z2, z3;
  f32::box_muller_quad(stream_block(seed, pid0 + (uint64_t)i, purpose, iter, k), z0, z1, z2, z3);
  out[4 * i] = z0;
  out[4 * i + 1] = z1;
  out[4 * i + 2] = z2;
  out[4 * i + 3] = z3;
}

// ... and the bare loop of for_quads_f32, `quads` blocks of four normals per lane (sabc_op_rng_peak_f32)
__global__ void __launch_bounds__(kBlock)
k_rng_peak_f32(const uint64_t seed, const int quads, const int64_t n, float *__restrict__ out) {
  rng_tables_init();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float acc = 0.0f;
  NormalStream ns(seed, (uint64_t)i, PURPOSE_SIM, 0);
  ns.for_quads_f32(quads, [&](const float z0, const float z1, const float z2, const float z3) {
    acc += z0;
    acc += z1;
    acc += z2;
    acc += z3;
  });
  out[i] = acc;
}

}  // namespace sabc
