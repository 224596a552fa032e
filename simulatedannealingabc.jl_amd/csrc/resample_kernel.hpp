// resample_kernel.hpp -- K5, the resample (SimulatedAnnealingABC.jl:124-137): weights, the three-pass weight scan, the draws
// with their gather (plain, packed lines, packed with the moment sums) and the sharded form (requests grouped by owner).
// Device code only, included by kernels.hip alone; the launchers are in kernels.hip.
#pragma once
#include "update_kernel.hpp"

namespace sabc {

// ------------------------------------------------------------------------------------------
// K5: resample (SimulatedAnnealingABC.jl:124-137)
// ------------------------------------------------------------------------------------------
// w_i = exp(-sum_j u_ij delta / ubar_j), :126-127
__device__ __forceinline__ double particle_weight(const int d, const int s, const PopPtrs &pp, const ControlBlock *__restrict__ cb,
                                                  const double n_global, const double delta, const int64_t li) {
  double a = 0.0;
  for (int j = 0; j < s; ++j) {
    const double ubar = cb->sums[1 + j] / n_global;                                         // :126
    a += pp.pop[(int64_t)(d + j) * pp.cap + li] * delta / ubar;                             // :127
  }
  return exp(-a);
}

__global__ void __launch_bounds__(kBlock)
k_resample_weights(const int d, const int s, const PopPtrs pp, const ControlBlock *__restrict__ cb,
                   const double n_global, const double delta) {
  const int64_t li = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (li >= pp.n_local) return;
  pp.pop[(int64_t)(d + s) * pp.cap + li] = particle_weight(d, s, pp, cb, n_global, delta, li);
}

__device__ __forceinline__ double gathered_weight(const ShardBlocks &g, int64_t gid) {
  int64_t r, o;
  split_index(gid, g.cap, r, o);
  return shard_block(g, r)[(int64_t)(g.rows - 1) * g.cap + o];
}

// pass 1: per-chunk sums of w and w^2.  One shard (wargs.fused): the weights are computed here from the u rows and
// written to the weight row on the way (no separate k_resample_weights launch); same arithmetic, same values.
struct WeightArgs {
  int fused, d, s, reserved;
  PopPtrs pp;
  const ControlBlock *cb;
  double n_global, delta;
};

__global__ void __launch_bounds__(kBlock)
k_scan_sums(const ShardBlocks g, const int64_t n, double *__restrict__ bs, double *__restrict__ bq, const WeightArgs wa,
            double *__restrict__ wcopy) {
  __shared__ double sm[2][kBlock / 64];
  const int64_t base = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * 4;
  double s = 0.0, q = 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t i = base + e;
    double w = 0.0;
    if (i < n) {
      if (wa.fused) {
        w = particle_weight(wa.d, wa.s, wa.pp, wa.cb, wa.n_global, wa.delta, i);
        wa.pp.pop[(int64_t)(wa.d + wa.s) * wa.pp.cap + i] = w;
      } else {
        w = gathered_weight(g, i);
        if (wcopy) wcopy[i] = w;       // weights read from their owners (peer-mapped): the last pass finds them here, not over xGMI again
      }
    }
    s += w; q += w * w;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { s += __shfl_down(s, off, 64); q += __shfl_down(q, off, 64); }
  if (lane == 0) { sm[0][wave] = s; sm[1][wave] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    bs[blockIdx.x] = ((sm[0][0] + sm[0][1]) + sm[0][2]) + sm[0][3];
    bq[blockIdx.x] = ((sm[1][0] + sm[1][1]) + sm[1][2]) + sm[1][3];
  }
}

// pass 2 (single block of 1024): exclusive scan of the chunk sums in place; totals.  Thread t owns
// `per` consecutive chunks; the 1024 thread totals are scanned in LDS by a fixed-shape
// Hillis-Steele network (same result on every run and every shard).
__global__ void __launch_bounds__(1024)
k_scan_offsets(double *__restrict__ bs, const double *__restrict__ bq, const int64_t nb, double *__restrict__ totals,
               double *__restrict__ totals_host) {
  __shared__ double sa[2][1024];
  __shared__ double sq[1024];
  const int t = threadIdx.x;
  const int64_t per = (nb + 1023) / 1024;
  const int64_t lo = (int64_t)t * per, hi = (lo + per < nb) ? lo + per : nb;
  double s = 0.0, q = 0.0;
  for (int64_t b = lo; b < hi; ++b) { s += bs[b]; q += bq[b]; }
  sa[0][t] = s; sq[t] = q;
  __syncthreads();
  int cur = 0;
  for (int off = 1; off < 1024; off <<= 1) {          // inclusive scan of the thread totals
    sa[1 - cur][t] = t >= off ? sa[cur][t] + sa[cur][t - off] : sa[cur][t];
    cur = 1 - cur;
    __syncthreads();
  }
  for (int off = 512; off > 0; off >>= 1) {           // tree sum of the squares
    if (t < off) sq[t] += sq[t + off];
    __syncthreads();
  }
  if (t == 0) {
    totals[0] = sa[cur][1023]; totals[1] = sq[0];
    if (totals_host) { totals_host[0] = sa[cur][1023]; totals_host[1] = sq[0]; }   // pinned + mapped: the ESS of :134, no memcpy
  }
  double run = t > 0 ? sa[cur][t - 1] : 0.0;          // exclusive offset of this thread's first chunk
  for (int64_t b = lo; b < hi; ++b) { const double v = bs[b]; bs[b] = run; run += v; }
}

// pass 3: inclusive scan inside each chunk + chunk offset
// Packed lines (one shard): particle i's running sum AND its (theta, u) row sit together, `pg` particles to a 128-byte
// line (pg = 4, 2 or 1: the largest power of two with pg (1 + row_len) <= 16, so that a line never straddles a scan chunk
// and every particle's slot starts on a 16 / pg-double boundary):
//   pk[(i / pg) * 16 + (i % pg) * (16 / pg)] = { cum_i, theta_i..., u_i... }
//   ge[i / pg]  = cum at the line's last particle                      (kScanChunk / pg per chunk)
//   guide[b]    = a line whose running sums reach bucket b of [0, total), n_lines + 2 buckets (guide_bucket)
// A draw then costs THREE dependent fetches (the guide entry, two line ends, the packed line) instead of ~10 (binary
// search through `cm` and `cum`, one line per gathered row).  The running sums are the same numbers, so the drawn index
// is the same.
struct PackArgs {
  double *pk, *ge;       // pk == nullptr: no packing (the sharded path gathers rows by request)
  int32_t *guide;        // guide[b]: a line whose running sums reach bucket b of [0, total) -- where a draw starts looking
  const double *totals;  // totals[0] = sum of the weights (written by k_scan_offsets)
  int row_len, pg;
};

// bucket of a running sum t: n_lines equal buckets over [0, total).  The SAME expression places the lines in
// k_scan_final and the draws in the gather; it only has to be monotone -- the guide is a starting point, the search
// around it decides (packed_search).
__device__ __forceinline__ int64_t guide_bucket(const double t, const double total, const int64_t n_lines) {
  const double x = t * ((double)n_lines / total);
  const int64_t b = x > 0.0 ? (int64_t)x : 0;             // (NaN -> 0)
  return b <= n_lines + 1 ? b : n_lines + 1;
}

// pass 3: inclusive scan inside each chunk + chunk offset
__global__ void __launch_bounds__(kBlock)
k_scan_final(const ShardBlocks g, const int64_t n, const double *__restrict__ bs, double *__restrict__ cum,
             double *__restrict__ cm, const PackArgs pa, const int w_in_cum) {
  __shared__ double sm[kBlock];
  __shared__ double scum[kScanChunk];
  const int64_t base = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * 4;
  double w[4];
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t i = base + e;
    // w_in_cum: the first pass left the weights in `cum` (each element is read here before this thread overwrites it below)
    w[e] = i < n ? (w_in_cum ? cum[i] : gathered_weight(g, i)) : 0.0;
    s += w[e];
  }
  sm[threadIdx.x] = s;
  __syncthreads();
  // Exclusive scan of the 256 thread totals in the FIXED sequential order 0, 1, 2, ... (part of the summation order the
  // oracle shares).  One lane walking the LDS array paid a dependent LDS round trip per element (~12 us of the kernel);
  // here the first wave holds the totals in registers (4 per lane) and the running sum visits them in the same order
  // through v_readlane: the same 256 additions, in registers.
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const double a[4] = {sm[4 * lane], sm[4 * lane + 1], sm[4 * lane + 2], sm[4 * lane + 3]};
    double ex[4] = {0.0, 0.0, 0.0, 0.0};
    double run = 0.0;
    for (int l = 0; l < 64; ++l) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double b = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(a[e]), l),
                                          __builtin_amdgcn_readlane(__double2loint(a[e]), l));
        if (lane == l) ex[e] = run;
        run += b;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sm[4 * lane + e] = ex[e];
  }
  __syncthreads();
  double run = bs[blockIdx.x] + sm[threadIdx.x];
  const bool packed = pa.pk != nullptr;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t i = base + e;
    run += w[e];
    if (packed) { scum[threadIdx.x * 4 + e] = run; continue; }       // the packed gather reads neither cum nor cm
    if (i < n) cum[i] = run;
    // mid level of the resample search: cm[g] = cum at the end of 16-element group g (one 128-byte line of `cum`);
    // weights behind n are 0, so `run` is the total there; groups entirely behind n get +inf
    if ((i & 15) == 15) cm[i >> 4] = (i - 15 < n) ? run : INFINITY;
  }
  if (!packed) return;
  __syncthreads();
  // consecutive lanes take consecutive particles here (not 4 each, as in the scan): coalesced row reads, and the pg lanes
  // of a line write its 128 bytes with 16-byte stores
  const int stride = 16 / pa.pg;
  const int64_t n_lines = (n + pa.pg - 1) / pa.pg;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int loc = threadIdx.x + e * kBlock;
    const int64_t i = (int64_t)blockIdx.x * kScanChunk + loc;
    const int64_t line = i / pa.pg;
    if (line >= n_lines) continue;
    const int slot = (int)(i - line * pa.pg);
    double v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = 0.0;
    v[0] = i < n ? scum[loc] : INFINITY;                             // empty slots of the last line never win a search
    if (i < n)
      for (int row = 0; row < pa.row_len; ++row) v[1 + row] = g.flat[(int64_t)row * g.cap + i];   // packing: one shard, its own block
    double2 *dst = reinterpret_cast<double2 *>(pa.pk + line * 16 + slot * stride);
    // (only the slot's used part: the padding behind 1 + row_len doubles is never read)
    for (int q = 0; 2 * q < stride && 2 * q < 1 + pa.row_len; ++q) dst[q] = make_double2(v[2 * q], v[2 * q + 1]);
    // the line's end value: its last particle, or the last particle of the population (scum is flat behind n)
    if (i < n && (slot == pa.pg - 1 || i == n - 1)) {
      const double e1 = scum[loc];
      pa.ge[line] = e1;
      // the buckets this line's running sums reach: from the end of the line before it (the chunk's offset for the chunk's
      // first line, inclusive there so that rounding between the offset and the previous chunk's end leaves no bucket
      // unwritten) to its own end; the population's last line takes the rest
      const int first_loc = loc - slot;                              // the line's first particle, inside this chunk
      const double total = pa.totals[0];
      int64_t b0 = first_loc > 0 ? guide_bucket(scum[first_loc - 1], total, n_lines) + 1 : guide_bucket(bs[blockIdx.x], total, n_lines);
      int64_t b1 = i == n - 1 ? n_lines + 1 : guide_bucket(e1, total, n_lines);
      for (int64_t b = b0; b <= b1; ++b) pa.guide[b] = (int32_t)line;
      if (i == n - 1) { pa.ge[line + 1] = INFINITY; pa.ge[line + 2] = INFINITY; }
    }
  }
}

// n_local categorical draws + gather of theta and u rows (rho is NOT permuted, :131-132).
// Inverse CDF by a three-level search, one line of `cum` per draw: the exclusive chunk offsets `bs` of the
// weight scan (one per 1024 weights, in LDS) -> `cm`, the running sum at the end of every 16-element group
// (64 per chunk, 0.5 MB at n = 1e6: L2-resident) -> the 16 elements of that group (one 128-byte line).
constexpr int kGatherCoarseMax = 4096;     // chunks held in LDS (n <= 4.2e6); beyond that bs is searched in global memory
constexpr int kGroupsPerChunk = kScanChunk / 16;
// the chunk offsets into LDS, four reads in flight per thread (nb <= 4096 and 256 threads: at most 4 trips to memory at the
// front of every workgroup of a latency-bound kernel instead of 16); the caller's __syncthreads() publishes them
__device__ __forceinline__ void stage_chunk_offsets(const double *__restrict__ bs, const int64_t nb, double *lds) {
  for (int64_t i0 = threadIdx.x; i0 < nb; i0 += 4 * kBlock) {
    double t[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { const int64_t i = i0 + (int64_t)e * kBlock; t[e] = i < nb ? bs[i] : 0.0; }
#pragma unroll
    for (int e = 0; e < 4; ++e) { const int64_t i = i0 + (int64_t)e * kBlock; if (i < nb) lds[i] = t[e]; }
  }
}
// first index k with cum[k] > t, by the three levels described above (B = the chunk offsets, in LDS or global memory)
__device__ __forceinline__ int64_t resample_search(const double t, const double *B, const int64_t nb,
                                                   const double *__restrict__ cm, const double *__restrict__ cum,
                                                   const int64_t n) {
  int64_t blo = 0, bhi = nb;              // first chunk whose offset exceeds t; bs[0] = 0 <= t
  while (blo < bhi) {
    const int64_t mid = blo + ((bhi - blo) >> 1);
    if (B[mid] > t) bhi = mid; else blo = mid + 1;
  }
  const int64_t chunk = blo - 1;
  // first group of the chunk whose end value exceeds t (count form over the chunk's 64 group ends)
  int64_t grp = chunk * kGroupsPerChunk;
#pragma unroll
  for (int step = kGroupsPerChunk >> 1; step >= 1; step >>= 1)
    if (cm[grp + step - 1] <= t) grp += step;
  if (cm[grp] <= t) grp += 1;             // 64 of 64: t is not below the chunk's own end (rounding of bs vs cum)
  int64_t lo = grp << 4, hi = lo + 16;    // first k in the group with cum[k] > t
  if (grp == (chunk + 1) * kGroupsPerChunk) hi = lo;
  if (hi > n) hi = n;
  if (lo > n) lo = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (cum[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo < n ? lo : n - 1;
}

// One shard: the draw and the gather of its rows in one kernel.  Several shards (k_resample_select): the draws only,
// as global source indices; the rows are fetched from their owners afterwards (k_resample_serve / _scatter).
template <bool GATHER>
__global__ void __launch_bounds__(kBlock)
k_resample_gather(const uint64_t seed, const int d, const int s, const ShardBlocks g, const int64_t n,
                  const double *__restrict__ cum, const double *__restrict__ bs,
                  const double *__restrict__ cm, const int64_t nb, const double *__restrict__ totals, const uint64_t iter,
                  const PopPtrs dst, int64_t *__restrict__ idx_out) {
  extern __shared__ double bs_lds[];
  const bool in_lds = nb <= kGatherCoarseMax;
  if (in_lds) {
    stage_chunk_offsets(bs, nb, bs_lds);
    __syncthreads();
  }
  const double *B = in_lds ? bs_lds : bs;
  const int64_t li = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (li >= dst.n_local) return;
  const uint64_t gid = (uint64_t)(dst.gid0 + li);
  const u32x4 w = stream_block(seed, gid, PURPOSE_RESAMPLE, iter, 0);
  const double t = u52(w.x, w.y) * totals[0];
  const int64_t idx = resample_search(t, B, nb, cm, cum, n);
  if (!GATHER) { idx_out[li] = idx; return; }
  int64_t r, o;
  split_index(idx, g.cap, r, o);
  const double *src = shard_block(g, r) + o;               // the drawn particle, in a gathered copy or in its owner's HBM
  for (int row = 0; row < d + s; ++row)
    dst.pop[(int64_t)row * dst.cap + li] = src[(int64_t)row * g.cap];
}

// The draw on packed lines.  Chunk by the offsets `B` (as resample_search: the oracle's answer is defined per chunk); inside
// the chunk the first line whose end value exceeds t is found AROUND a guess: guide[bucket of t] (k_scan_final) is a line
// whose running sums reach t's bucket -- with n_lines buckets usually the line itself or a neighbour --, the ends of that
// line and of the one before it are read together, and the search walks from there in whichever direction they say
// (the ends are non-decreasing inside a chunk, so the walk is the search).  Then the packed line: the running sums of its
// first PG - 1 slots pick the slot, and the caller reads that slot's row.  Per draw: the guide entry, two line ends, PG - 1
// running sums, the row -- ~8 load instructions in 4 dependent trips, the last two to one line (the binary search through
// two index levels was ~27 in ~11; the kernel is bound by the number of divergent-address loads).  Same decisions as resample_search on the same
// numbers: if no running sum of the chunk exceeds t (rounding of the offsets against the sums) the next chunk's first
// particle is taken, the last particle at the end of the population.  `row` receives the address of the drawn particle's row.
template <int PG>
__device__ __forceinline__ int64_t packed_search(const double t, const double total, const double *B, const int64_t nb,
                                                 const int32_t *__restrict__ guide, const double *__restrict__ ge,
                                                 const double *__restrict__ pk, const int64_t n, const double *&row) {
  constexpr int kStride = 16 / PG;
  constexpr int64_t kLinesPerChunk = kScanChunk / PG;
  const int64_t n_lines = (n + PG - 1) / PG;
  int64_t s = guide[guide_bucket(t, total, n_lines)];     // in flight during the search of the offsets
  int64_t blo = 0, bhi = nb;
  while (blo < bhi) {
    const int64_t mid = blo + ((bhi - blo) >> 1);
    if (B[mid] > t) bhi = mid; else blo = mid + 1;
  }
  const int64_t chunk = blo - 1;
  const int64_t l0 = chunk * kLinesPerChunk;
  int64_t end = l0 + kLinesPerChunk;
  if (end > n_lines) end = n_lines;
  s = s < l0 ? l0 : (s > end - 1 ? end - 1 : s);
  const double e_prev = s > l0 ? ge[s - 1] : -INFINITY;
  double e_s = ge[s];
  if (e_prev > t) {                                       // the guess lies behind the line: walk back
    s -= 1;
    while (s > l0 && ge[s - 1] > t) s -= 1;
  } else {
    int walked = 0;
    while (!(e_s > t) && s + 1 < end) {
      if (++walked > 8) {                                 // a bucket full of all-but-weightless lines: bisect the rest of the chunk
        int64_t lo = s + 1, hi = end;                     // first line in [lo, hi) whose end exceeds t, or `end`
        while (lo < hi) {
          const int64_t mid = lo + ((hi - lo) >> 1);
          if (ge[mid] > t) hi = mid; else lo = mid + 1;
        }
        s = lo;
        e_s = s < end ? INFINITY : -INFINITY;
        break;
      }
      s += 1;
      e_s = ge[s];
    }
    if (!(e_s > t)) s = end;                              // no line of the chunk exceeds t
  }
  int64_t idx;
  if (s < end) {
    // the slot: the COUNT of the running sums of the line's first PG - 1 slots that do not exceed t (independent reads;
    // the line's end exceeds t, so its last slot needs no test)
    double cw[PG > 1 ? PG - 1 : 1];
#pragma unroll
    for (int q = 0; q < PG - 1; ++q) cw[q] = pk[s * 16 + q * kStride];
    int slot = 0;
#pragma unroll
    for (int q = 0; q < PG - 1; ++q) slot += !(cw[q] > t) ? 1 : 0;
    idx = s * PG + slot;
    if (idx >= n) idx = n - 1;                            // (the last line; its empty slots hold +inf)
  } else {
    idx = (chunk + 1) * (int64_t)kScanChunk;
    if (idx >= n) idx = n - 1;
  }
  const int64_t line = idx / PG;
  row = pk + line * 16 + (idx - line * PG) * kStride + 1;
  return idx;
}

constexpr int packed_per_line(int row_len) {
  return 16 / (1 + row_len) >= 4 ? 4 : 16 / (1 + row_len) >= 2 ? 2 : 1;
}

// One shard, packed: the draw and its (theta, u) row come from one line, and -- with D, S known at compile time -- the
// moment sums of the RESAMPLED population (what k_stats would compute in a pass of its own: Sigma, eps and the history
// row are taken from the resampled population, :348-353) come out of the same kernel, in the same per-workgroup order.
template <int D, int S>
__global__ void __launch_bounds__(kBlock)
k_resample_gather_stats(const uint64_t seed, const double *__restrict__ pk, const double *__restrict__ ge,
                        const int32_t *__restrict__ guide, const int pg, const int64_t n, const double *__restrict__ bs, const int64_t nb, const double *__restrict__ totals,
                        const uint64_t iter, const PopPtrs dst, const ControlBlock *__restrict__ cb,
                        double *__restrict__ partials) {
  constexpr int NP = n_partials(D, S);
  extern __shared__ double bs_lds[];
  const bool in_lds = nb <= kGatherCoarseMax;
  if (in_lds) {
    stage_chunk_offsets(bs, nb, bs_lds);
    __syncthreads();
  }
  const double *B = in_lds ? bs_lds : bs;
  double acc[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) acc[q] = 0.0;
  const int64_t li = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (li < dst.n_local) {
    const uint64_t gid = (uint64_t)(dst.gid0 + li);
    const u32x4 w = stream_block(seed, gid, PURPOSE_RESAMPLE, iter, 0);
    const double total = totals[0];
    const double t = u52(w.x, w.y) * total;
    constexpr int PG = packed_per_line(D + S);
    const double *row;
    (void)packed_search<PG>(t, total, B, nb, guide, ge, pk, n, row);
    double th[D], u[S], rho[S];
#pragma unroll
    for (int k = 0; k < D; ++k) { th[k] = row[k]; dst.pop[(int64_t)k * dst.cap + li] = th[k]; }
#pragma unroll
    for (int j = 0; j < S; ++j) {
      u[j] = row[D + j];
      dst.pop[(int64_t)(D + j) * dst.cap + li] = u[j];
      rho[j] = dst.rho[(int64_t)j * dst.cap + li];                        // rho stays where it is (:131-132)
    }
    moment_terms<D, S>(cb->pivot, false, th, u, rho, acc);
  }
  block_reduce_store<NP>(acc, partials + (int64_t)blockIdx.x * NP);
}

// the same without the sums, d and s at run time (host-callback and source-compiled simulators)
__global__ void __launch_bounds__(kBlock)
k_resample_gather_packed(const uint64_t seed, const int row_len, const double *__restrict__ pk, const double *__restrict__ ge,
                         const int32_t *__restrict__ guide, const int pg, const int64_t n, const double *__restrict__ bs, const int64_t nb,
                         const double *__restrict__ totals, const uint64_t iter, const PopPtrs dst) {
  extern __shared__ double bs_lds[];
  const bool in_lds = nb <= kGatherCoarseMax;
  if (in_lds) {
    stage_chunk_offsets(bs, nb, bs_lds);
    __syncthreads();
  }
  const double *B = in_lds ? bs_lds : bs;
  const int64_t li = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (li >= dst.n_local) return;
  const u32x4 w = stream_block(seed, (uint64_t)(dst.gid0 + li), PURPOSE_RESAMPLE, iter, 0);
  const double total = totals[0];
  const double t = u52(w.x, w.y) * total;
  const double *row;
  if (pg == 4) (void)packed_search<4>(t, total, B, nb, guide, ge, pk, n, row);
  else if (pg == 2) (void)packed_search<2>(t, total, B, nb, guide, ge, pk, n, row);
  else (void)packed_search<1>(t, total, B, nb, guide, ge, pk, n, row);
  for (int r = 0; r < row_len; ++r) dst.pop[(int64_t)r * dst.cap + li] = row[r];
}

// ---- the sharded resample: requests grouped by owner, served by the owner, scattered by the requester ----
// counts[r] += number of draws whose source lives on shard r (wave-aggregated integer atomics)
__global__ void __launch_bounds__(kBlock)
k_bucket_count(const int64_t *__restrict__ idx, const int64_t n_local, const int64_t cap, unsigned long long *counts) {
  const int64_t li = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = li < n_local;
  int64_t r = 0, o = 0;
  if (live) split_index(idx[li], cap, r, o);
  unsigned long long todo = __ballot(live);
  const int lane = threadIdx.x & 63;
  while (todo) {                                   // one trip per distinct owner in the wave (<= world)
    const int leader = __ffsll((long long)todo) - 1;
    const int64_t r0 = __shfl(r, leader, 64);
    const unsigned long long same = __ballot(live && r == r0);
    if (lane == leader) atomicAdd(&counts[r0], (unsigned long long)__popcll(same));
    todo &= ~same;
  }
}

// cursor[r] starts at the exclusive offset of bucket r; req[pos] = offset inside the owner (exact as a double),
// slot[pos] = the local destination the reply belongs to.  The order inside a bucket is arbitrary (atomics); it only
// pairs a request with its reply.
__global__ void __launch_bounds__(kBlock)
k_bucket_scatter(const int64_t *__restrict__ idx, const int64_t n_local, const int64_t cap, unsigned long long *cursor,
                 double *__restrict__ req, int64_t *__restrict__ slot) {
  const int64_t li = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = li < n_local;
  int64_t r = 0, o = 0;
  if (live) split_index(idx[li], cap, r, o);
  unsigned long long todo = __ballot(live);
  const int lane = threadIdx.x & 63;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int64_t r0 = __shfl(r, leader, 64);
    const unsigned long long same = __ballot(live && r == r0);
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(&cursor[r0], (unsigned long long)__popcll(same));
    base = __shfl(base, leader, 64);
    if (live && r == r0) {
      const int64_t pos = (int64_t)base + __popcll(same & below);
      req[pos] = (double)o;
      slot[pos] = li;
    }
    todo &= ~same;
  }
}

// owner side: rows_out[q][row] = pop[row][offset_q] for the m requested offsets (AoS: one contiguous row per request)
__global__ void __launch_bounds__(kBlock)
k_resample_serve(const double *__restrict__ req, const int64_t m, const int row_len, const PopPtrs src,
                 double *__restrict__ rows_out) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= m * row_len) return;
  const int64_t q = e / row_len;
  const int row = (int)(e - q * row_len);
  int64_t o = (int64_t)req[q];
  o = o < 0 ? 0 : (o >= src.n_local ? src.n_local - 1 : o);      // a corrupt request must not fault
  rows_out[e] = src.pop[(int64_t)row * src.cap + o];
}

// requester side: rows_in is in the bucket order of k_bucket_scatter
__global__ void __launch_bounds__(kBlock)
k_resample_scatter(const double *__restrict__ rows_in, const int64_t *__restrict__ slot, const int64_t n_local,
                   const int row_len, const PopPtrs dst) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_local * row_len) return;
  const int64_t pos = e / row_len;
  const int row = (int)(e - pos * row_len);
  dst.pop[(int64_t)row * dst.cap + slot[pos]] = rows_in[e];
}

}  // namespace sabc
