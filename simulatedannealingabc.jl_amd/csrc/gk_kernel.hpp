// gk_kernel.hpp -- the g-and-k model's own kernels (BASELINE config 4): K4 `k_update_gk` and `k_simulate_gk`, with the
// simulation wave-per-particle (device_models.hpp: gk_simulate_rows4 / gk_simulate_wave_ranks*).  Device code only, included by
// kernels.hip alone (never by the headers hipRTC compiles for a user simulator); the launchers are in kernels.hip.
#pragma once
#include "update_kernel.hpp"

namespace sabc {

// ------------------------------------------------------------------------------------------
// g-and-k (BASELINE config 4): the SIMULATION is wave-per-particle (128 draws sorted across the lanes); a wave owns
// kGkParticlesPerWave consecutive particles (a block of 4 waves 4 x that), does their proposals, prior gates, ECDF
// lookups and accept steps one particle per lane, and simulates them one after the other in between.
// k_update_gk: every wave takes ONE group of kGkParticlesPerWave particles and the workgroup writes one partial row for all
// of them (several groups per wave in turn lost: DESIGN.md section 3).
// ------------------------------------------------------------------------------------------
constexpr int kGkD = 4, kGkS = 4;
constexpr int kGkPerBlock = (kBlock / 64) * kGkParticlesPerWave;

// per-wave staging of what phase 1 (propose + simulate) hands to phase 2 (ECDF) and 3 (accept)
struct GkStage {
  double thp[kGkParticlesPerWave][kGkD];
  double rp[kGkParticlesPerWave][kGkS];
  double up[kGkParticlesPerWave][kGkS];
  double lpp[kGkParticlesPerWave];
  double logf[kGkParticlesPerWave];
};

// 4 workgroups per CU (<= 128 VGPRs, 68 B of scratch outside the sort): 850 -> 755 us at n = 1e6 against 3 per CU (144 VGPRs,
// no scratch) -- the sort waits on lane exchanges, so the extra wave pays; 5 per CU spills inside the loop (1030 us).
// (The figures of the kernel as it was then; as it stands: 102 VGPRs with ROWS4, 105 without, no scratch -- DESIGN.md.)
// ROWS4: every wanted rank is a multiple of 16 (the host looks: launch_update) -- the simulations run four particles at a time
// on the network of gk_simulate_rows4 only; the two-values-per-lane network stays out of this instantiation (and its
// registers with it)
template <int PROP, bool ROWS4>
__global__ void __launch_bounds__(kBlock, 4)
k_update_gk(const ModelDesc m, const StepArgs c, const ControlBlock *__restrict__ cb, const PopPtrs pp, const CdfPtrs cdf,
            const PartnerView pv, const int64_t act_lo, const int64_t act_n, double *__restrict__ partials) {
  constexpr int D = kGkD, S = kGkS, NP = n_partials(D, S), PW = kGkParticlesPerWave;
  static_assert(S == 4 && (PW * S) % 64 == 0 && PW <= 64, "phase 2 maps one (particle, statistic) pair to each lane, PW S / 64 times");
  if (cb->halt) return;                    // queued ahead of a resample decision that fired (uniform)
  rng_tables_init();
  __shared__ GkStage stage[kBlock / 64];
  __shared__ double red[kBlock / 64][NP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  GkStage &st = stage[wave];
  if (lane < NP) red[wave][lane] = 0.0;
  const int64_t t0 = (int64_t)blockIdx.x * kGkPerBlock + wave * PW;
  if (t0 < act_n) {                        // uniform over the wave; a wave without particles goes straight to the block's sum
    // the wave owns particles t0 .. t0+PW-1; in the scalar phases (1a, 3) lane i < PW handles particle t0+i
    const int64_t t_mine = t0 + lane;
    const bool mine = lane < PW && t_mine < act_n;
    const int64_t li = act_lo + t_mine;
    const uint64_t gid = (uint64_t)(pp.gid0 + li);

    // ---- phase 1a, lane-parallel over the wave's particles: proposal (:311) and prior gate (:314)
    // -- the narrow form's draft without its simulation, the very code k_update runs (update_kernel.hpp: kDraftOnly)
    if (mine) {
      ParticleDraft<D, 1> q;               // (q.th, q.u, q.rp: unused)
      update_particle_draft<kDraftOnly, D, 1, PROP, false, 1>(m, c.iter, c.prop_p0, c.prop_p1, cb, pp, pv, li, gid, q);
#pragma unroll
      for (int k = 0; k < D; ++k) st.thp[lane][k] = q.thp[k];
      st.lpp[lane] = q.lpp;
      st.logf[lane] = q.logf;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- phase 1b, the whole wave on the simulations (:315), lane l draws 2 of a particle's 128; TWO particles at a time
    // (one at a time was the slower A/B arm): their sorting networks are independent, so the lane exchanges of one overlap
    // the selects of the other.  Particles outside the prior's support are not simulated (:314): the wave walks the set
    // bits of `todo`.
    {
      unsigned long long todo = __ballot(mine && st.lpp[lane] > -INFINITY);
      // wanted ranks that are all multiples of 16 (BASELINE config 4): FOUR particles at a time, one per row of 16 lanes, eight
      // values per lane -- 15 of the network's 24 steps stay inside the lane (device_models.hpp: gk_simulate_rows4)
      while (ROWS4 && todo) {
        int idx[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (todo) { idx[q] = __ffsll((long long)todo) - 1; todo &= todo - 1; }
          else idx[q] = idx[q - 1 < 0 ? 0 : q - 1];        // fewer than four left: the last one again (it writes the same values)
        }
        const int row = lane >> 4;
        const int my = row == 0 ? idx[0] : row == 1 ? idx[1] : row == 2 ? idx[2] : idx[3];
        gk_simulate_rows4<S>(m, st.thp, st.rp, my, (uint64_t)(pp.gid0 + act_lo + t0 + my), c.iter);
      }
      while (!ROWS4 && todo) {                             // uniform over the wave
        const int ia = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        int ib = ia;                                       // an odd one out is paired with itself
        if (todo) { ib = __ffsll((long long)todo) - 1; todo &= todo - 1; }
        double tha[D], thb[D], ra[S], rb[S];
#pragma unroll
        for (int k = 0; k < D; ++k) { tha[k] = st.thp[ia][k]; thb[k] = st.thp[ib][k]; }
        // the wanted order statistics of the normals where the quantile function is increasing (phase 2 maps them), else rho
        gk_simulate_wave_ranks_x2<S>(m, tha, thb, (uint64_t)(pp.gid0 + act_lo + t0 + ia), (uint64_t)(pp.gid0 + act_lo + t0 + ib),
                                     c.iter, ra, rb);
        if (lane == 0) {
#pragma unroll
          for (int j = 0; j < S; ++j) { st.rp[ia][j] = ra[j]; st.rp[ib][j] = rb[j]; }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- phase 2: the PW x 4 (particle, statistic) pairs of the wave, PW S / 64 per lane -- all with the lane's statistic
    // j = lane & 3: quantile function of the order statistic of the normals -> distance (device_models.hpp: gk_increasing),
    // then the lane's ECDF lookups (:316) in lockstep on the one table they share
    {
      constexpr int NPASS = PW * S / 64;
      const int j = lane & 3;
      int64_t len = cdf.len[0];
      double obs = m.p[2 + S];
#pragma unroll
      for (int q = 1; q < S; ++q)
        if (j == q) { len = cdf.len[q]; obs = m.p[2 + S + q]; }
      double r[NPASS], upv[NPASS];
      bool live[NPASS];
#pragma unroll
      for (int pass = 0; pass < NPASS; ++pass) {
        const int it = pass * (64 / S) + (lane >> 2);
        live[pass] = t0 + it < act_n && st.lpp[it] > -INFINITY;
        r[pass] = 0.0;
        if (live[pass]) {
          double thp[D];
#pragma unroll
          for (int k = 0; k < D; ++k) thp[k] = st.thp[it][k];
          r[pass] = st.rp[it][j];
          if (gk_increasing(thp, m.p[1])) {
            r[pass] = gk_rho_of_normal(thp, m.p[1], r[pass], obs);
            st.rp[it][j] = r[pass];
          }
        }
      }
      cdf_apply_mid_lockstep<NPASS>(cdf.knots + (int64_t)j * cdf.stride, len, cdf.mid + (int64_t)j * cdf.mid_stride, r, upv);
#pragma unroll
      for (int pass = 0; pass < NPASS; ++pass) st.up[pass * (64 / S) + (lane >> 2)][j] = live[pass] ? upv[pass] : 0.0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- phase 3, lane-parallel again: acceptance (:318-329), store, and the particle's moment terms
    double term[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) term[q] = 0.0;
    if (mine) {
      double th[D], u[S], drho[S], thp[D], up[S], rp[S];
#pragma unroll
      for (int k = 0; k < D; ++k) { th[k] = pp.pop[(int64_t)k * pp.cap + li]; thp[k] = st.thp[lane][k]; }
#pragma unroll
      for (int j = 0; j < S; ++j) {
        u[j] = pp.pop[(int64_t)(D + j) * pp.cap + li];
        drho[j] = 0.0;                                         // the change of sum(rho), see k_update
        up[j] = st.up[lane][j];
        rp[j] = st.rp[lane][j];
      }
      const double lpp = st.lpp[lane];
      double log_accept = -INFINITY;
      if (lpp > -INFINITY) {
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < S; ++j) {
          const double e = (cb->eps_len == 1) ? cb->eps[0] : cb->eps[j];
          a += (u[j] - up[j]) / e;
        }
        log_accept = lpp - prior_logpdf<D>(m, th) + a + st.logf[lane];
      }
      const u32x4 wa = stream_block(m.seed, gid, PURPOSE_ACCEPT, c.iter, 0);
      const bool accepted = -0.5 * neg2_log_tab(u52(wa.x, wa.y)) < log_accept;      // log(U) < log alpha, :324
      if (accepted) {
#pragma unroll
        for (int k = 0; k < D; ++k) { th[k] = thp[k]; pp.pop[(int64_t)k * pp.cap + li] = thp[k]; }
#pragma unroll
        for (int j = 0; j < S; ++j) {
          u[j] = up[j];
          drho[j] = rp[j] - pp.rho[(int64_t)j * pp.cap + li];
          pp.pop[(int64_t)(D + j) * pp.cap + li] = up[j];
          pp.rho[(int64_t)j * pp.cap + li] = rp[j];
        }
      }
      moment_terms<D, S>(cb->pivot, accepted, th, u, drho, term);
    }
    // sum the moment terms over the wave's PW particle lanes (lanes >= PW hold zeros) into the wave's row, ...
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      double v = term[q];
#pragma unroll
      for (int off = PW / 2; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) red[wave][q] += v;
    }
  }
  // ... then over the 4 waves
  __syncthreads();
  if (threadIdx.x < NP) {
    const int q = threadIdx.x;
    partials[(int64_t)blockIdx.x * NP + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
  }
}

// one wave per row of theta: used for the prior sample at initialization and for sabc_op_simulate.
// Same phase structure as k_update_gk: one lane per particle draws / loads the parameters of the wave's particles in parallel
// (the prior draw is four Philox blocks + Box-Muller pairs per particle: done by all 64 lanes for one particle at a
// time it cost more than the simulation itself -- 1.8 ms for the 1e6 simulations k_update_gk does in 0.7 ms), the whole
// wave then simulates them one after the other, the particles' lanes store.
__global__ void __launch_bounds__(kBlock)
k_simulate_gk(const ModelDesc m, const double *__restrict__ theta_in, const int64_t n, const int64_t stride,
              const uint64_t pid0, const uint64_t iter, const int sample_prior, double *__restrict__ theta_out,
              double *__restrict__ rho_out, const int64_t out_stride) {
  constexpr int D = kGkD, S = kGkS, PW = kGkParticlesPerWave;
  rng_tables_init();
  __shared__ double sth[kBlock / 64][PW][D];
  __shared__ double srho[kBlock / 64][PW][S];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * kGkPerBlock + wave * PW;
  const int64_t i_mine = i0 + lane;
  const bool mine = lane < PW && i_mine < n;
  if (mine) {
    double th[D];
    if (sample_prior) {
      prior_sample<D>(m, pid0 + (uint64_t)i_mine, th);
    } else {
#pragma unroll
      for (int k = 0; k < D; ++k) th[k] = theta_in[(int64_t)k * stride + i_mine];
    }
#pragma unroll
    for (int k = 0; k < D; ++k) sth[wave][lane][k] = th[k];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int it = 0; it < PW; ++it) {
    if (i0 + it >= n) break;                          // uniform over the wave
    double th[D], rho[S];
#pragma unroll
    for (int k = 0; k < D; ++k) th[k] = sth[wave][it][k];
    gk_simulate_wave_ranks<S>(m, th, pid0 + (uint64_t)(i0 + it), iter, rho);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < S; ++j) srho[wave][it][j] = rho[j];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // order statistics of the normals -> distances, 16 x 4 (particle, statistic) pairs of the wave at once (gk_increasing)
  static_assert(S == 4 && (PW * S) % 64 == 0 && PW <= 64, "one (particle, statistic) pair per lane, PW S / 64 times");
  for (int pass = 0; pass < PW * S / 64; ++pass) {
    const int it = pass * (64 / S) + (lane >> 2), j = lane & 3;
    if (i0 + it < n) {
      double th[D];
#pragma unroll
      for (int k = 0; k < D; ++k) th[k] = sth[wave][it][k];
      double obs = m.p[2 + S];
#pragma unroll
      for (int q = 1; q < S; ++q)
        if (j == q) obs = m.p[2 + S + q];
      if (gk_increasing(th, m.p[1])) srho[wave][it][j] = gk_rho_of_normal(th, m.p[1], srho[wave][it][j], obs);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (mine) {
    if (theta_out) {
#pragma unroll
      for (int k = 0; k < D; ++k) theta_out[(int64_t)k * out_stride + i_mine] = sth[wave][lane][k];
    }
#pragma unroll
    for (int j = 0; j < S; ++j) rho_out[(int64_t)j * out_stride + i_mine] = srho[wave][lane][j];
  }
}

}  // namespace sabc
