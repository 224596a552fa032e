// p2p_kernel.hpp -- the peer-to-peer transport's device side (p2p.hpp has the slot layout): the word store / load / wait
// helpers, the sum of the shards' rows (p2p_allreduce_rows, also called by k_reduce_control: control_kernel.hpp comes after
// this header), the barrier / commit / leave kernels and the self-tests.  Device code only, included by kernels.hip alone;
// the launchers are in kernels.hip.
#pragma once
#include "p2p.hpp"
#include "persistent_kernel.hpp"

namespace sabc {

// ------------------------------------------------------------------------------------------
// peer-to-peer exchange over mapped slots (p2p.hpp)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void p2p_store(uint64_t *p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);        // one 8-byte store, past the caches
}
__device__ __forceinline__ uint64_t p2p_load(const uint64_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint64_t p2p_clock() { return (uint64_t)wall_clock64(); }

// spin until the word's upper half is the tag `seq`; gives up after `ticks`, as soon as another lane of the workgroup has,
// or as soon as the awaited shard has LEFT the group (its leave word in this shard's slots carries the tag's generation:
// p2p.hpp) -- *failed = 1 + peer, + 16 when the peer left
__device__ __forceinline__ uint64_t p2p_wait_word(const uint64_t *src, uint32_t seq, uint64_t t0, uint64_t ticks, volatile int *failed,
                                                  int peer, const uint64_t *my_slots) {
  uint64_t w = p2p_load(src);
  for (uint32_t polls = 1; (uint32_t)(w >> 32) != seq; ++polls) {
    if ((polls & 15u) == 0) {
      if (*failed) break;
      if (p2p_clock() - t0 > ticks) { *failed = 1 + peer; break; }
      const uint64_t lw = p2p_load(my_slots + kP2PLeaveOff + peer);
      if ((uint32_t)(lw >> 32) == p2p_tag_gen(seq) && (uint32_t)lw == 1u) {
        w = p2p_load(src);                                   // (what it posted before it left still counts)
        if ((uint32_t)(w >> 32) != seq) *failed = 17 + peer;
        break;
      }
    }
    __builtin_amdgcn_s_sleep(2);
    w = p2p_load(src);
  }
  return w;
}

// a wait gave up: the error goes into the control block together with the halt flag (everything queued behind becomes a
// no-op) and, if the host is waiting for this step, into the mailbox
__device__ __forceinline__ void p2p_fail(ControlBlock *cb, ControlBlock *lcb, const ControlArgs *a, Mailbox *ring, int kind, int failed,
                                         uint32_t seq) {
  cb->error = SABC_ERR_COMM;
  cb->halt = 1;
  // kind: 1 sums exchange | 2 barrier | 3 end-of-call status; + 4 when the shard waited for has left the group
  cb->comm_where = ((kind + (failed > 16 ? 4 : 0)) << 24) | (((failed - 1) & 15) << 20) | (int)(seq & kP2PSeqMask);
  if (lcb) { lcb->error = SABC_ERR_COMM; lcb->halt = 1; lcb->comm_where = cb->comm_where; }
  __threadfence();
  if (lcb && a && ring && a->notify_seq != 0) mailbox_post(ring, *a, *lcb);
}

// sum of the shards' rows of `np` doubles: `mine` (LDS) goes to every peer's slots in the LL form, the peers' rows are
// awaited in this shard's slots, and the rows are added in RANK order (every shard gets bitwise the same sums).
// All threads of the workgroup call it; returns false when a wait gave up.  words: LDS, world * 2 np.
__device__ __forceinline__ bool p2p_allreduce_rows(const P2PView &pv, const uint32_t seq, const int np, double *mine,
                                                   uint32_t *words, volatile int *failed, const int silent) {
  const int W = pv.world, nw = 2 * np, ring = (int)(seq % kP2PRing);
  const uint32_t *half = reinterpret_cast<const uint32_t *>(mine);
  if (silent != 1)                                   // test hook: 1 = nothing is posted, 2 = the post reaches this shard's own slots only
    for (int i = threadIdx.x; i < W * nw; i += blockDim.x) {
      const int p = i / nw, t = i - p * nw;
      if (silent == 2 && p != pv.rank) continue;
      p2p_store(pv.slots[p] + kP2PSumsOff + ((int64_t)ring * kMaxPeers + pv.rank) * kP2PWords + t, ((uint64_t)seq << 32) | half[t]);
    }
  const uint64_t t0 = p2p_clock();
  for (int i = threadIdx.x; i < W * nw; i += blockDim.x) {
    const int r = i / nw, t = i - r * nw;
    const uint64_t w = p2p_wait_word(pv.slots[pv.rank] + kP2PSumsOff + ((int64_t)ring * kMaxPeers + r) * kP2PWords + t, seq, t0,
                                     pv.timeout_ticks, failed, r, pv.slots[pv.rank]);
    words[i] = (uint32_t)w;
  }
  __syncthreads();
  if (*failed) return false;
  if ((int)threadIdx.x < np) {
    const int q = threadIdx.x;
    double a = 0.0;
    for (int r = 0; r < W; ++r) {
      const double x = __hiloint2double((int)words[r * nw + 2 * q + 1], (int)words[r * nw + 2 * q]);
      a = r == 0 ? x : a + x;
    }
    mine[q] = a;
  }
  __syncthreads();
  return true;
}

// Flag barrier between the shards' streams: everything every shard has enqueued before its barrier `seq` has completed
// (kernel boundary) before anything enqueued behind it starts.  Lane r posts to / waits for shard r.
__global__ void __launch_bounds__(64)
k_p2p_barrier(const P2PView pv, const uint32_t seq, ControlBlock *cb, const int guarded, const int silent) {
  __shared__ int failed;
  if (threadIdx.x == 0) failed = 0;
  __syncthreads();
  if ((guarded && cb->halt) || cb->error == SABC_ERR_COMM) return;        // the same on every shard (see k_reduce_control)
  const int r = threadIdx.x, ring = (int)(seq % kP2PRing);
  __threadfence_system();
  if (r < pv.world && silent != 1 && (silent != 2 || r == pv.rank)) p2p_store(pv.slots[r] + kP2PBarOff + (int64_t)ring * kMaxPeers + pv.rank, ((uint64_t)seq << 32) | 1u);
  if (r < pv.world)
    (void)p2p_wait_word(pv.slots[pv.rank] + kP2PBarOff + (int64_t)ring * kMaxPeers + r, seq, p2p_clock(), pv.timeout_ticks, &failed, r,
                        pv.slots[pv.rank]);
  __syncthreads();
  if (threadIdx.x == 0 && failed) p2p_fail(cb, nullptr, nullptr, nullptr, 2, failed, seq);
  __threadfence_system();
}

// End of a sabc_initialize / sabc_update call over the peer-to-peer transport: every shard tells the others how the call
// went (status 0 = fine) and -- on the success path -- learns the same of them, so that a shard whose peer gave up in the
// call's LAST exchange does not return success on its own.  A shard that failed posts without waiting.
__global__ void __launch_bounds__(64)
k_p2p_commit(const P2PView pv, const uint32_t call, const int status, const int wait, ControlBlock *cb, const int silent) {
  __shared__ int failed;
  if (threadIdx.x == 0) failed = 0;
  __syncthreads();
  const int r = threadIdx.x;
  const int mine = (status != 0 || cb->error != 0) ? 1 : 0;
  if (r < pv.world && silent != 1 && (silent != 2 || r == pv.rank)) p2p_store(pv.slots[r] + kP2PCommitOff + pv.rank, ((uint64_t)call << 32) | (uint32_t)mine);
  if (!wait) return;
  if (r < pv.world) {
    const uint64_t w = p2p_wait_word(pv.slots[pv.rank] + kP2PCommitOff + r, call, p2p_clock(), pv.timeout_ticks, &failed, r,
                                     pv.slots[pv.rank]);
    if ((uint32_t)w != 0u && !failed) failed = 1 + r;                     // the peer's call failed
  }
  __syncthreads();
  if (threadIdx.x == 0 && failed && cb->error == 0) p2p_fail(cb, nullptr, nullptr, nullptr, 3, failed, call);
}

// rows of known values through the slots, for sabc_comm_p2p_selftest: out[q] = sum over shards of in[q]
__global__ void __launch_bounds__(1024)
k_p2p_selftest(const P2PView pv, const uint32_t seq, const int np, const double *__restrict__ in, double *__restrict__ out,
               int *__restrict__ failed_out, const int silent) {
  __shared__ int failed;
  __shared__ double sums[kMaxPartials];
  __shared__ uint32_t words[kMaxPeers * kP2PWords];
  if (threadIdx.x == 0) failed = 0;
  if ((int)threadIdx.x < np) sums[threadIdx.x] = in[threadIdx.x];
  __syncthreads();
  const bool ok = p2p_allreduce_rows(pv, seq, np, sums, words, &failed, silent);
  if (ok && (int)threadIdx.x < np) out[threadIdx.x] = sums[threadIdx.x];
  if (threadIdx.x == 0) *failed_out = ok ? 0 : failed;
}

// This shard leaves the group of generation `gen`: one word into every peer's slots (p2p.hpp); lane r tells shard r.
__global__ void __launch_bounds__(64) k_p2p_leave(const P2PView pv, const uint32_t gen) {
  const int r = threadIdx.x;
  if (r < pv.world && pv.slots[r]) p2p_store(pv.slots[r] + kP2PLeaveOff + pv.rank, ((uint64_t)gen << 32) | 1u);
}

// First contact, second half (sabc_comm_p2p_selftest): what the transport READS.  Partners, resampled rows and the ECDF
// build read a peer's populations and rho -- plain device memory, written by the owner's kernels, made visible by nothing but
// a kernel boundary on each side of a flag (p2p.hpp).  Every shard writes a pattern tagged with (generation, round, rank,
// buffer, sample) into `count` doubles spread evenly over each of its three buffers (mode 0: after parking what was there
// in `save`; mode 1: the second round), a barrier, every shard reads every shard's samples through its mappings and counts
// what is not the pattern; mode 2 puts the parked values back.
struct PatternBufs {
  uint64_t *buf[3];              // population buffer 0, population buffer 1, rho (as 64-bit words)
  int64_t len[3];                // doubles in each
  int32_t count[3];              // samples in each (<= kPatternSamples)
};
constexpr int kPatternSamples = 1024;
__device__ __forceinline__ uint64_t pattern_word(uint32_t gen, int round, int rank, int b, int k) {
  return 0x5AB0000000000000ull | ((uint64_t)(gen & 0xFFFu) << 40) | ((uint64_t)(round & 0xFF) << 32) | ((uint64_t)(rank & 0xFF) << 24) |
         ((uint64_t)(b & 0xF) << 20) | (uint64_t)(k & 0xFFFFF);
}
__device__ __forceinline__ int64_t pattern_index(int64_t len, int count, int k) { return (int64_t)k * (len / count); }

__global__ void __launch_bounds__(256)
k_p2p_pattern_write(const PatternBufs own, uint64_t *__restrict__ save, const uint32_t gen, const int round, const int rank, const int mode) {
  const int b = blockIdx.y;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < own.count[b]; k += gridDim.x * blockDim.x) {
    uint64_t *p = own.buf[b] + pattern_index(own.len[b], own.count[b], k);
    if (mode == 2) { *p = save[b * kPatternSamples + k]; continue; }
    if (mode == 0) save[b * kPatternSamples + k] = *p;
    *p = pattern_word(gen, round, rank, b, k);
  }
}

struct PatternPeers {
  const uint64_t *buf[3][kMaxPeers];
};
// out[0] = mismatches, out[1] = first mismatch as rank << 28 | buffer << 24 | sample (valid when out[0] > 0)
__global__ void __launch_bounds__(256)
k_p2p_pattern_check(const PatternPeers peers, const PatternBufs geo, const uint32_t gen, const int round, const int world,
                    unsigned int *__restrict__ out) {
  const int b = blockIdx.y, r = blockIdx.z;
  if (r >= world || !peers.buf[b][r]) return;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < geo.count[b]; k += gridDim.x * blockDim.x) {
    const uint64_t got = peers.buf[b][r][pattern_index(geo.len[b], geo.count[b], k)];    // a plain load, like the transport's
    if (got != pattern_word(gen, round, r, b, k)) {
      if (atomicAdd(&out[0], 1u) == 0u) out[1] = ((unsigned)r << 28) | ((unsigned)b << 24) | (unsigned)k;
    }
  }
}

}  // namespace sabc
