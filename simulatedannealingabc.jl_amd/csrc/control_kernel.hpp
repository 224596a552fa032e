// control_kernel.hpp -- the launches between two population updates: the fixed-order sum of the partial rows
// (k_reduce_partials), the control step on an LDS copy of the control block (control_on_copy, k_control) and the two in one
// launch, with the sum over the shards in between (k_reduce_control).  Device code only, included by kernels.hip alone;
// the launchers are in kernels.hip.
#pragma once
#include "persistent_kernel.hpp"
#include "p2p_kernel.hpp"

namespace sabc {

// fixed-order sum of the per-block partial rows: block c reduces component c
__global__ void __launch_bounds__(kBlock)
k_reduce_partials(const double *__restrict__ partials, const int64_t rows, const int np, double *__restrict__ sums,
                  const int *__restrict__ halt) {
  __shared__ double sm[kBlock / 64];
  if (halt && *halt) return;               // guarded: part of a step queued ahead of a fired resample test
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x;
  double v = 0.0;
#pragma unroll 4
  for (int64_t r = threadIdx.x; r < rows; r += kBlock) v += partials[r * np + c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) sums[c] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

__device__ __forceinline__ void control_on_copy(ControlBlock &lcb, int &ran, ControlBlock *cb, const ControlArgs &a,
                                                double *hist, Mailbox *ring, const double *sums, double *stage) {
  // the multi-eps schedule (:100-117): one lane per statistic computes its epsilon from the sums the step is about to take
  // over -- s^2 divisions and square roots plus s root solves on ONE lane are 12 us per update at s = 3 and over a
  // millisecond at s = 48; lane 0 then applies the candidates inside control_step(), in order
  __shared__ EpsCandidates cand;
  __shared__ double ubar_s[kMaxStats];
  const bool noop = (a.mode & CTRL_GUARDED) && lcb.halt;                  // uniform; nobody has written lcb.halt yet
  ControlArgs a_step = a;
  if (!noop && !(a.mode & CTRL_KEEP_SUMS)) {
    // the sums are taken over by one lane per component; the step then works on them as they stand
    for (int q = threadIdx.x; q < n_partials(a.d, a.s); q += blockDim.x) control_take_sum(lcb, a, sums, q);
    a_step.mode |= CTRL_KEEP_SUMS;
    __syncthreads();
  }
  const bool multi = !noop && (a.mode & CTRL_EPSILON) && a.algorithm == SABC_ALG_MULTI_EPS;
  if (multi) {
    if ((int)threadIdx.x < a.s) ubar_s[threadIdx.x] = lcb.sums[1 + threadIdx.x] / a.n_global;
    __syncthreads();
    if ((int)threadIdx.x < a.s) {
      const int i = threadIdx.x;
      cand.ok[i] = hostmath::eps_multi_one(ubar_s, a.s, a.v, hostmath::eps_multi_cn(a.s), i, &cand.eps[i]) ? 1 : 0;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) ran = control_step(lcb, a_step, hist, sums, &cand, multi) ? 1 : 0;
  __syncthreads();
  if (!ran) {                               // guarded and halted: nothing changed
    // ... and nothing is posted, unless the halt is a peer-to-peer wait that gave up (p2p.hpp): the host is waiting for
    // this step's sequence word and has to learn of the error
    if (threadIdx.x == 0 && a.notify_seq != 0 && lcb.error == SABC_ERR_COMM) mailbox_post(ring, a, lcb);
    return;
  }
  for (int i = threadIdx.x; i < kControlWords; i += blockDim.x)
    reinterpret_cast<uint64_t *>(cb)[i] = reinterpret_cast<const uint64_t *>(&lcb)[i];
  if (stage)
    for (int q = threadIdx.x; q < n_partials(a.d, a.s); q += blockDim.x) stage[q] = sums[q];
  if (threadIdx.x == 0 && a.notify_seq != 0) mailbox_post(ring, a, lcb);
}

__global__ void __launch_bounds__(64)
k_control(ControlBlock *cb, const ControlArgs a, double *hist, Mailbox *ring, const double *sums_in) {
  __shared__ ControlBlock lcb;
  __shared__ int ran;
  __shared__ double sums[kMaxPartials];
  const int np = n_partials(a.d, a.s);
  control_load(lcb, cb);
  for (int i = threadIdx.x; i < np; i += blockDim.x) sums[i] = sums_in[i];
  __syncthreads();
  control_on_copy(lcb, ran, cb, a, hist, ring, sums, nullptr);
}

// k_reduce_partials + [the sum over the shards] + k_control in ONE launch.
//  XCHG = false: one shard, no collective in between.
//  XCHG = true : several shards over the peer-to-peer slots -- what was k_reduce_partials -> ncclAllReduce -> k_control.
// 1024 threads: thread (g, c) sums rows g, g+G, ... of column c (consecutive threads read consecutive addresses), LDS
// combines the G row groups in a fixed order, lane 0 runs the control step on the sums.  The loads of the control block
// and of the partial rows are issued together (one round trip); the staging buffer is written only by a step that runs.
// rows < 0: the shard's sums are already in `stage` (k_reduce_partials ran: a partial matrix too large for one workgroup).
// do_control == 0: only the (global) sums, into `stage` (whoever asked for sums_buffer()).
struct XchgArgs {
  P2PView pv;
  uint32_t seq;
  int32_t do_control, silent, reserved;
};

// lane i of every row of 16 receives the value of lane i - k of its row (0.0 where there is none): v_mov_b32 dpp row_shr:k x 2
template <int CTRL>
__device__ __forceinline__ double dpp_row_shr(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

template <bool XCHG>
__global__ void __launch_bounds__(1024)
k_reduce_control(const double *__restrict__ partials, const int64_t rows, const int np, double *__restrict__ stage,
                 ControlBlock *cb, const ControlArgs a, double *hist, Mailbox *ring, const XchgArgs x) {
  __shared__ ControlBlock lcb;
  __shared__ int ran;
  __shared__ int failed;
  __shared__ double sm[1024];
  __shared__ double sums[kMaxPartials];
  __shared__ uint32_t words[XCHG ? kMaxPeers * kP2PWords : 1];
  const int B = blockDim.x;                         // 1024, or 256 for a short matrix of partial rows (launch_reduce_control)
  const int G = B / np;
  const int g = threadIdx.x / np, c = threadIdx.x - g * np;
  // the rows first (they come from the other XCDs' blocks, i.e. from memory: the longest latency of this launch), then the
  // control block; all of a lane's rows in ONE round trip where they fit (20 at n = 1e6: 3906 rows over 204 row groups),
  // masked so that there is no tail of dependent single loads (each a trip to the L2: 3-4 of them were ~3 us of this
  // kernel); the additions stay in row order, a masked slot adds +0
  constexpr int kInFlight = 24;
  double xx[kInFlight];
  if (rows >= 0 && g < G) {
#pragma unroll
    for (int e = 0; e < kInFlight; ++e) {
      const int64_t r = g + (int64_t)e * G;
      xx[e] = r < rows ? partials[r * np + c] : 0.0;
    }
  }
  control_load(lcb, cb);
  if (threadIdx.x == 0) failed = 0;
  if (rows >= 0) {
    double v = 0.0;
    if (g < G) {
#pragma unroll
      for (int e = 0; e < kInFlight; ++e) v += xx[e];
      for (int64_t r0 = g + (int64_t)kInFlight * G; r0 < rows; r0 += (int64_t)kInFlight * G) {
#pragma unroll
        for (int e = 0; e < kInFlight; ++e) {
          const int64_t r = r0 + (int64_t)e * G;
          xx[e] = r < rows ? partials[r * np + c] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < kInFlight; ++e) v += xx[e];
      }
    }
    sm[threadIdx.x] = v;
    __syncthreads();
    const int n_waves = B >> 6;
    if (np <= 16) {
      // one WAVE per column: lane l adds the groups l, l + 64, ... (<= 4 LDS reads), the 64 lane sums are added inside the
      // wave -- DPP row shifts, then the four row totals in order -- without another barrier or LDS round (the 8-level LDS
      // tree below was 1.2 us of this launch, by thread 0's clock reads between the phases in an instrumented build)
      const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
      for (int col = w; col < np; col += n_waves) {
        double t = 0.0;
        for (int gg = l; gg < G; gg += 64) t += sm[gg * np + col];
        t += dpp_row_shr<0x111>(t);
        t += dpp_row_shr<0x112>(t);
        t += dpp_row_shr<0x114>(t);
        t += dpp_row_shr<0x118>(t);                 // lane 16 r + 15 now holds the sum of row r
        const double total = ((read_lane(t, 15) + read_lane(t, 31)) + read_lane(t, 47)) + read_lane(t, 63);
        if (l == 0) sums[col] = total;
      }
    } else {
      // fixed-shape tree over the G row groups (a serial sum by np lanes would be G dependent LDS reads: 6 us at G = 204)
      int top = 1;
      while (top * 2 < G) top *= 2;
      for (int stride = top; stride >= 1; stride >>= 1) {
        if (g < stride && g + stride < G) sm[threadIdx.x] += sm[threadIdx.x + stride * np];
        __syncthreads();
      }
      if ((int)threadIdx.x < np) sums[threadIdx.x] = sm[threadIdx.x];
    }
  } else if ((int)threadIdx.x < np) {
    sums[threadIdx.x] = stage[threadIdx.x];
  }
  __syncthreads();
  if (XCHG) {
    // every shard takes the same decision here (the halt flag follows from sums all shards share), so a step that is a
    // no-op posts nothing on ANY shard and nobody waits for it
    const bool noop = ((a.mode & CTRL_GUARDED) && lcb.halt) || lcb.error == SABC_ERR_COMM;
    if (noop) {
      if (threadIdx.x == 0 && x.do_control && a.notify_seq != 0 && lcb.error == SABC_ERR_COMM) mailbox_post(ring, a, lcb);
      return;
    }
    if (!p2p_allreduce_rows(x.pv, x.seq, np, sums, words, &failed, x.silent)) {
      if (threadIdx.x == 0) p2p_fail(cb, &lcb, x.do_control ? &a : nullptr, ring, 1, failed, x.seq);
      return;
    }
    if (!x.do_control) {
      if ((int)threadIdx.x < np) stage[threadIdx.x] = sums[threadIdx.x];
      return;
    }
  }
  control_on_copy(lcb, ran, cb, a, hist, ring, sums, stage);
}

}  // namespace sabc
