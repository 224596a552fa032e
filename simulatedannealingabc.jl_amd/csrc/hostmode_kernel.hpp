// hostmode_kernel.hpp -- the kernels of the host-simulator mode (SABC_MODEL_HOST): prior draws, proposal step, accept step and
// moment sums with d and s at run time.  Device code only, included by kernels.hip alone; the launchers are in kernels.hip.
#pragma once
#include "update_kernel.hpp"

namespace sabc {

// ------------------------------------------------------------------------------------------
// Host-simulator mode (SABC_MODEL_HOST): f_dist is a host callable, so the per-particle
// body (:308-331) is cut at the simulator.  k_host_propose does :311-314 (proposal, prior gate),
// the host evaluates f_dist for the proposals that passed the gate, k_host_accept does :316-329
// (ECDF, annealed MH test, store).  d and s are run-time values here (any model within the
// maxima); these kernels are host-bound by construction, so they are written for generality.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double prior_logpdf_rt(const ModelDesc &m, const double *th) {
  if (m.prior_joint == 2) return 0.0;                  // host-callback prior: the host overwrites this (hip_backend.hip)
  if (m.prior_joint) return mvnormal_logpdf(m, m.d, th);
  double lp = 0.0;
  for (int k = 0; k < m.d; ++k) {
    const double l = prior_logpdf_dim(m, k, th[k]);
    lp = (l > -INFINITY && lp > -INFINITY) ? lp + l : -INFINITY;
  }
  return lp;
}

// rand(prior) for the shard (:174); theta goes to the population rows
__global__ void __launch_bounds__(kBlock) k_host_prior(const ModelDesc m, const PopPtrs pp) {
  rng_tables_init();
  const int64_t li = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (li >= pp.n_local) return;
  const uint64_t gid = (uint64_t)(pp.gid0 + li);
  if (m.prior_joint) {
    double th[kMaxPara];
    mvnormal_sample(m, m.d, gid, th);
    for (int k = 0; k < m.d; ++k) pp.pop[(int64_t)k * pp.cap + li] = th[k];
    return;
  }
  for (int k = 0; k < m.d; ++k)
    pp.pop[(int64_t)k * pp.cap + li] = prior_sample_dim(m, k, gid);
}

// one particle of the host-mode proposal step (:311-314)
__device__ __forceinline__ void host_propose_one(const ModelDesc &m, const StepArgs &c, const ControlBlock *__restrict__ cb,
                                                 const PopPtrs &pp, const PartnerView &pv, const int64_t act_lo, const int64_t act_n,
                                                 double *__restrict__ thp_out, double *__restrict__ aux,
                                                 double *__restrict__ thp_host, unsigned char *__restrict__ gate_host,
                                                 double *__restrict__ cur_out, const int64_t t) {
  const int d = m.d;
  const int64_t li = act_lo + t;
  const uint64_t gid = (uint64_t)(pp.gid0 + li);
  double th[kMaxPara], thp[kMaxPara];
  for (int k = 0; k < d; ++k) th[k] = pp.pop[(int64_t)k * pp.cap + li];
  double logf = 0.0;
  if (c.prop_kind == SABC_PROP_RANDOMWALK) {
    NormalStream ns(m.seed, gid, PURPOSE_PROP, c.iter);
    double z[kMaxPara];
    for (int k = 0; k < d; ++k) z[k] = ns.next();
    for (int k = 0; k < d; ++k) {
      double a = 0.0;
      for (int l = 0; l <= k; ++l) a += cb->chol[k * d + l] * z[l];
      thp[k] = th[k] + a;
    }
  } else if (c.prop_kind == SABC_PROP_DIFFEVO) {
    uint64_t i1 = 0, i2 = 0;
    for (uint32_t a = 0;; ++a) {
      const u32x4 w = stream_block(m.seed, gid, PURPOSE_PROP, c.iter, a);
      i1 = mulhi64(pack64(w.x, w.y), (uint64_t)pv.m_total);
      i2 = mulhi64(pack64(w.z, w.w), (uint64_t)pv.m_total);
      if (i1 != i2 || a > 64u) break;
    }
    double z0, z1;
    box_muller(stream_block(m.seed, gid, PURPOSE_PROP2, c.iter, 0), z0, z1);
    const double gamma = c.prop_p0 * (1.0 + c.prop_p1 * z0);
    const double *p1 = partner_ptr(pv, i1), *p2 = partner_ptr(pv, i2);
    for (int k = 0; k < d; ++k) thp[k] = th[k] + gamma * (p1[(int64_t)k * pv.cap] - p2[(int64_t)k * pv.cap]);
  } else {
    const u32x4 w = stream_block(m.seed, gid, PURPOSE_PROP, c.iter, 0);
    const uint64_t ip = mulhi64(pack64(w.x, w.y), (uint64_t)pv.m_total);
    const double U = u52(w.z, w.w);
    const double a = c.prop_p0;
    const double tt = (a - 1.0) * U + 1.0;
    const double z = tt * tt / a;
    const double *p = partner_ptr(pv, ip);
    for (int k = 0; k < d; ++k) {
      const double pk = p[(int64_t)k * pv.cap];
      thp[k] = pk + z * (th[k] - pk);
    }
    logf = log(z) * (double)(d - 1);
  }
  // the proposal stays in device memory for the accept step AND goes to the host for f_dist; of the prior gate the host
  // needs one byte (simulate or not), the log densities stay on the device
  const double lpp = prior_logpdf_rt(m, thp);
  for (int k = 0; k < d; ++k) { thp_out[(int64_t)k * act_n + t] = thp[k]; thp_host[(int64_t)k * act_n + t] = thp[k]; }
  aux[t] = lpp;
  aux[act_n + t] = logf;
  gate_host[t] = lpp > -INFINITY ? 1 : 0;
  if (cur_out)
    for (int k = 0; k < d; ++k) cur_out[(int64_t)k * act_n + t] = th[k];
}

// thp [d][act_n] = proposals, aux [2][act_n] = (log prior of the proposal or -inf, log_factor): device memory, read again by
// k_host_accept.  What the HOST needs goes to pinned host memory mapped into the device (zero copy, no D2H call follows):
// thp_host = the proposals, gate_host [act_n] = one byte per proposal (inside the prior's support?), cur_out (optional,
// [d][act_n]) = the current particles (a host-callback prior needs their log density too).  The half batch is cut into chunks of `sig.chunk`
// particles; the LAST workgroup of a chunk to finish posts `sig.seq` into the chunk's flag word in host memory, which the
// host polls -- it starts f_dist on chunk c while the later chunks are still being proposed, without a stream sync.
struct HostSignal {
  unsigned int *done;            // device: workgroups of each chunk that have finished
  unsigned long long *flag;      // mapped host memory: one word per chunk
  unsigned long long seq;
  int64_t chunk;                 // particles per chunk (a multiple of kBlock)
};

__global__ void __launch_bounds__(kBlock)
k_host_propose(const ModelDesc m, const StepArgs c, const ControlBlock *__restrict__ cb, const PopPtrs pp,
               const PartnerView pv, const int64_t act_lo, const int64_t act_n, double *__restrict__ thp_out,
               double *__restrict__ aux, double *__restrict__ thp_host, unsigned char *__restrict__ gate_host,
               double *__restrict__ cur_out, const HostSignal sig) {
  rng_tables_init();
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t < act_n) host_propose_one(m, c, cb, pp, pv, act_lo, act_n, thp_out, aux, thp_host, gate_host, cur_out, t);
  __threadfence_system();                     // this lane's stores to host memory are out ...
  __syncthreads();                            // ... for every lane of the workgroup
  if (threadIdx.x == 0) {
    const int64_t ch = ((int64_t)blockIdx.x * kBlock) / sig.chunk;
    const int64_t first = ch * sig.chunk, last = first + sig.chunk < act_n ? first + sig.chunk : act_n;
    const unsigned int groups = (unsigned int)((last - first + kBlock - 1) / kBlock);
    if (atomicAdd(&sig.done[ch], 1u) == groups - 1u) {
      sig.done[ch] = 0u;                      // ready for the next half batch
      __threadfence_system();
      __hip_atomic_store(&sig.flag[ch], sig.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// rho_prop [s][act_n] from the host; n_accept is counted with an integer atomic (exact, order-free)
__global__ void __launch_bounds__(kBlock)
k_host_accept(const ModelDesc m, const StepArgs c, const ControlBlock *__restrict__ cb, const PopPtrs pp, const CdfPtrs cdf,
              const int64_t act_lo, const int64_t act_n, const int64_t t_lo, const int64_t t_n,
              const double *__restrict__ thp_in,
              const double *__restrict__ aux, const double *__restrict__ rho_prop, const double *__restrict__ lp_host,
              unsigned long long *n_accept) {
  // one chunk [t_lo, t_lo + t_n) of the half batch; thp / aux: device memory (k_host_propose); rho_prop: the host's mapped
  // staging array; lp_host (a host-callback prior only, mapped): [2][act_n] = log prior of the proposals | of the current particles
  const int64_t t = t_lo + (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool accepted = false;
  if (t < t_lo + t_n) {
    const int d = m.d, s = m.s;
    const int64_t li = act_lo + t;
    const uint64_t gid = (uint64_t)(pp.gid0 + li);
    const double lpp = lp_host ? lp_host[t] : aux[t], logf = aux[act_n + t];
    double log_accept = -INFINITY;
    double up[kMaxStats];
    if (lpp > -INFINITY) {
      double th[kMaxPara];
      for (int k = 0; k < d; ++k) th[k] = pp.pop[(int64_t)k * pp.cap + li];
      double a = 0.0;
      for (int j = 0; j < s; ++j) {
        up[j] = cdf_apply_mid(cdf.knots + (int64_t)j * cdf.stride, cdf.len[j], cdf.mid + (int64_t)j * cdf.mid_stride,
                              rho_prop[(int64_t)j * act_n + t]);
        const double e = (cb->eps_len == 1) ? cb->eps[0] : cb->eps[j];
        a += (pp.pop[(int64_t)(d + j) * pp.cap + li] - up[j]) / e;
      }
      log_accept = lpp - (lp_host ? lp_host[act_n + t] : prior_logpdf_rt(m, th)) + a + logf;   // (lp_host: host-callback prior)
    }
    const u32x4 wa = stream_block(m.seed, gid, PURPOSE_ACCEPT, c.iter, 0);
    accepted = log_fast(u52(wa.x, wa.y)) < log_accept;
    if (accepted) {
      for (int k = 0; k < d; ++k) pp.pop[(int64_t)k * pp.cap + li] = thp_in[(int64_t)k * act_n + t];
      for (int j = 0; j < s; ++j) {
        pp.pop[(int64_t)(d + j) * pp.cap + li] = up[j];
        pp.rho[(int64_t)j * pp.cap + li] = rho_prop[(int64_t)j * act_n + t];
      }
    }
  }
  const unsigned long long votes = __ballot(accepted);
  if ((threadIdx.x & 63) == 0 && votes) atomicAdd(n_accept, (unsigned long long)__popcll(votes));
}

// moment sums with run-time d and s (same partial-row layout as k_stats); block 0 also folds the
// accept counter of the host-mode update into component 0 and clears it
__global__ void __launch_bounds__(kBlock)
k_stats_rt(const int d, const int s, const ControlBlock *__restrict__ cb, const PopPtrs pp, double *__restrict__ partials,
           unsigned long long *n_accept) {
  __shared__ double sm[kBlock / 64];
  const int np = n_partials(d, s);
  const int64_t li = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = li < pp.n_local;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double dk[kMaxPara];
  for (int k = 0; k < d; ++k) dk[k] = live ? pp.pop[(int64_t)k * pp.cap + li] - cb->pivot[k] : 0.0;
  for (int q = 0; q < np; ++q) {
    double v = 0.0;
    if (live) {
      if (q == 0) v = 0.0;
      else if (q < 1 + s) v = pp.pop[(int64_t)(d + q - 1) * pp.cap + li];
      else if (q < 1 + 2 * s) v = pp.rho[(int64_t)(q - 1 - s) * pp.cap + li];
      else if (q < 1 + 2 * s + d) v = dk[q - 1 - 2 * s];
      else {
        int r = q - (1 + 2 * s + d), kk = 0;          // row-major lower index -> (kk, ll)
        while (r > kk) { r -= kk + 1; ++kk; }
        v = dk[kk] * dk[r];
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      double tot = ((sm[0] + sm[1]) + sm[2]) + sm[3];
      if (q == 0 && blockIdx.x == 0 && n_accept) { tot = (double)*n_accept; *n_accept = 0ull; }
      partials[(int64_t)blockIdx.x * np + q] = tot;
    }
    __syncthreads();
  }
}

}  // namespace sabc
