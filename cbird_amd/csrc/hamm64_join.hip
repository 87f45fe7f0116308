// hamm64_join.hip -- the 64-bit Hamming threshold search as a bucketed join (multi-index hashing) for small thresholds.
//
// The same predicate as hamm64_scan.hip / hamm64_mfma.hip (DctHashIndex::find, src/dcthashindex.cpp:193-220:
// hamm64(q, hash[i]) < thresh && id[i] != 0, q != 0), the same records -- but not every pair is looked at.  Two 64-bit
// words that differ in at most d = thresh - 1 bits agree on at least one of any m > d disjoint chunks of their bits
// (pigeonhole), so with m = max(4, thresh) chunks of 64 / m bits a needle has to be compared only with the slots that share
// one of its m chunk values.  On hashes whose bits are close to independent (the bench's 10^6 image hashes, NOTES 15) that is
// 1 / 10 000 of the all-pairs scan at thresholds <= 4 and 1 / 28 at threshold 8; on a library of near-identical hashes it is
// MORE work than the scan -- the launcher counts the candidate pairs exactly (sum over chunk values of slots x needles, from
// the two histograms) before it commits, and hands the call back (CBH_E_UNSUPPORTED) when the matrix-core scan is cheaper.
//
//   k_join_hist        a histogram of every chunk's values, one global atomic per item and chunk: the 16-bit chunks of
//                      thresholds <= 4, and every n / 16384-th item for the sampled pre-check (k_join_pairs_only adds up
//                      its pairs)
//   k_join_hist_lds    the same for chunks of <= 13 bits (thresholds 5..8), privatised in LDS
//   k_join_scan1       per chunk, one side: the exclusive scan -> where each value's slots / needles start
//   k_join_jobs        per chunk, from the two sides' starts: the jobs of the wide join (one per 512 slots x 2048 needles of
//                      a value) and their prefix; the chunk's candidate pairs, exactly
//   k_join_scatter     slots (hash, id) and needles (hash, needle index) in chunk-value order, one copy per chunk
//   k_join_pairs       chunks of <= 11 bits: a workgroup per job, two slots per lane, the value's needles through the scalar
//                      cache eight at a time, one min-test per block and the exact look only behind it
//   k_join_narrow      chunks of 12-13 bits (threshold 5): a lane per slot walks its value's needles
//   k_join_by_needle   four 16-bit chunks (thresholds <= 4): only the slots' side is prepared; a lane per NEEDLE walks the
//                      ~15 slots of each of its four values
// A pair that also agrees on an EARLIER chunk is that chunk's to report; records are parked per wave in LDS and appended with
// one atomic per flush.
//
// The slots' side (histogram, scans, the m chunk-ordered copies) depends on the index contents alone.  A handle that asks
// for it (cbh_idx64_join_prepare, or "join_resident" 1) keeps it: JoinCache / JoinTables in cbh_internal.h -- built once per
// plan under the cache's mutex, reference counted, dropped by every mutation, bounded by "join_resident_mb".  Such a handle
// stands for the reference's tree, built once at load / the first find and queried many times (buildTree, src/dcthashindex.cpp:61-68,
// called at :110, searched at :208).  A launch without a handle behind it (cbh_idx64_scan_dev on the caller's stream, which nobody waits for) or
// whose tables could not be had prepares the slots per call from the stream-ordered arena, as every launch used to.
// The needles' side of thresholds 5..8 is prepared per call -- once per device for the shards of a sharded handle.
#include "cbh_internal.h"

#include <atomic>

namespace cbh {
namespace {

constexpr int kJT = 256;        // threads
constexpr uint32_t kJH = 2 * kJT;  // slots per job of the wide join (two per lane)
constexpr uint32_t kJQ = 2048;  // needles per job (a value's needles beyond that make further jobs)
constexpr int kMaxChunks = kJoinMaxThresh;  // chunks: max(4, thresh)
constexpr uint32_t kOutCap = 96;  // records a wave parks before it appends them

struct JoinPlan {
  int m;                       // chunks
  int lo[kMaxChunks + 1];      // chunk j = bits [lo[j], lo[j + 1])
  uint32_t voff[kMaxChunks + 1];  // chunk j's values start at voff[j] in the per-value arrays (+ j for the "+1" slots)
};

__device__ __forceinline__ uint32_t chunk_of(uint64_t h, int lo, int hi) {
  return (uint32_t)((h >> lo) & ((1ull << (hi - lo)) - 1ull));
}

// hist[voff[j] + j + value] += 1 for every item and chunk (the arrays carry one extra entry per chunk for the scans' ends).
// One global atomic per item and chunk: the 16-bit chunks of plan 4 (slots only, and with resident tables only when they
// are built) and the sampled pre-check (stride > 1).
__global__ __launch_bounds__(256) void k_join_hist(const uint64_t* __restrict__ x, uint32_t n, uint32_t stride, JoinPlan P,
                                                   uint32_t* __restrict__ hist) {
  const uint32_t i = (blockIdx.x * 256u + threadIdx.x) * stride;  // (stride > 1: the sampled pre-check)
  if (i >= n) return;
  const uint64_t h = x[i];
#pragma unroll 1
  for (int j = 0; j < P.m; ++j) atomicAdd(&hist[P.voff[j] + (uint32_t)j + chunk_of(h, P.lo[j], P.lo[j + 1])], 1u);
}

// The same histogram for chunks of <= 13 bits (every chunk of plans 5..8), privatised in LDS: a workgroup per (span of
// items, chunk) counts into 2^bits bins of its own (32 KB at 13 bits: five workgroups fit a CU's 160 KB) and adds every
// non-empty bin to the global array once.  A span is at least eight items per bin, so the global adds are at most an
// eighth of the items (k_join_hist: one per item), and a million equal hashes meet in LDS, not on one global word.
constexpr int kHistLdsBits = 13;
constexpr uint32_t kHistSpan = 16384;  // items per workgroup at <= 11 bits; 8 << bits above
__global__ __launch_bounds__(256) void k_join_hist_lds(const uint64_t* __restrict__ x, uint32_t n, JoinPlan P,
                                                       uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[1u << kHistLdsBits];
  const int j = blockIdx.y;
  const int bits = P.lo[j + 1] - P.lo[j];
  const uint32_t nv = 1u << bits, span = max(kHistSpan, 8u << bits);
  const uint64_t i0 = (uint64_t)blockIdx.x * span;  // (the grid is sized for the shortest span: the rest leave, as one)
  if (i0 >= n) return;
  const uint32_t i1 = (uint32_t)min((uint64_t)n, i0 + span);
  for (uint32_t v = threadIdx.x; v < nv; v += 256u) bins[v] = 0u;
  __syncthreads();
  for (uint32_t i = (uint32_t)i0 + threadIdx.x; i < i1; i += 256u) atomicAdd(&bins[chunk_of(x[i], P.lo[j], P.lo[j + 1])], 1u);
  __syncthreads();
  const uint32_t off = P.voff[j] + (uint32_t)j;
  for (uint32_t v = threadIdx.x; v < nv; v += 256u) {
    const uint32_t c = bins[v];
    if (c) atomicAdd(&hist[off + v], c);
  }
}

// One workgroup per chunk, one side: start = the exclusive scan of hist (nv + 1 entries per chunk).  `zero`: hist is left
// zeroed -- it becomes the scatter's cursors.  (At build time for the slots, per call for the needles.)
__global__ __launch_bounds__(1024) void k_join_scan1(JoinPlan P, uint32_t* hist, uint32_t* __restrict__ start, uint32_t zero) {
  const int j = blockIdx.x;
  const uint32_t nv = 1u << (P.lo[j + 1] - P.lo[j]);
  const uint32_t off = P.voff[j] + (uint32_t)j;
  __shared__ uint32_t sa[1024];
  const uint32_t per = (nv + 1023u) / 1024u, v0 = min(nv, threadIdx.x * per), v1 = min(nv, v0 + per);
  uint32_t a = 0;
  for (uint32_t v = v0; v < v1; ++v) a += hist[off + v];
  sa[threadIdx.x] = a;
  __syncthreads();
  for (uint32_t d = 1; d < 1024u; d <<= 1) {  // inclusive scan of the per-thread sums
    const uint32_t ta = threadIdx.x >= d ? sa[threadIdx.x - d] : 0u;
    __syncthreads();
    sa[threadIdx.x] += ta;
    __syncthreads();
  }
  uint32_t ea = sa[threadIdx.x] - a;
  for (uint32_t v = v0; v < v1; ++v) {
    const uint32_t c = hist[off + v];
    start[off + v] = ea;
    ea += c;
    if (zero) hist[off + v] = 0u;
  }
  if (threadIdx.x == 1023) start[off + nv] = sa[1023];
}

// One workgroup per chunk, per call.  In: the slots' starts (resident, or this call's) and the call's needle starts.  Out:
// jobstart (exclusive scan of ceil(nh / kJH) * ceil(nq / kJQ) per value, nv + 1 entries), stats[2 j] = the chunk's jobs,
// stats[2 j + 1] = its candidate pairs, exactly (sum over the values of slots x needles).
__global__ __launch_bounds__(1024) void k_join_jobs(JoinPlan P, const uint32_t* __restrict__ start_h,
                                                    const uint32_t* __restrict__ start_q, uint32_t* __restrict__ jobstart,
                                                    unsigned long long* __restrict__ stats) {
  const int j = blockIdx.x;
  const uint32_t nv = 1u << (P.lo[j + 1] - P.lo[j]);
  const uint32_t off = P.voff[j] + (uint32_t)j;
  __shared__ unsigned long long sc[1024], sp[1024];  // (64-bit job sums: the launcher refuses more than 2^31 - 1)
  const uint32_t per = (nv + 1023u) / 1024u, v0 = min(nv, threadIdx.x * per), v1 = min(nv, v0 + per);
  unsigned long long c = 0, p = 0;
  for (uint32_t v = v0; v < v1; ++v) {
    const uint32_t nh = start_h[off + v + 1] - start_h[off + v], nq = start_q[off + v + 1] - start_q[off + v];
    c += (nh && nq) ? (unsigned long long)((nh + kJH - 1u) / kJH) * ((nq + kJQ - 1u) / kJQ) : 0ull;
    p += (unsigned long long)nh * nq;
  }
  sc[threadIdx.x] = c, sp[threadIdx.x] = p;
  __syncthreads();
  for (uint32_t d = 1; d < 1024u; d <<= 1) {
    const unsigned long long tc = threadIdx.x >= d ? sc[threadIdx.x - d] : 0ull, tp_ = threadIdx.x >= d ? sp[threadIdx.x - d] : 0ull;
    __syncthreads();
    sc[threadIdx.x] += tc, sp[threadIdx.x] += tp_;
    __syncthreads();
  }
  unsigned long long ec = sc[threadIdx.x] - c;
  for (uint32_t v = v0; v < v1; ++v) {
    const uint32_t nh = start_h[off + v + 1] - start_h[off + v], nq = start_q[off + v + 1] - start_q[off + v];
    jobstart[off + v] = (uint32_t)ec;  // (only read when the chunk's jobs fit a grid)
    ec += (nh && nq) ? (unsigned long long)((nh + kJH - 1u) / kJH) * ((nq + kJQ - 1u) / kJQ) : 0ull;
  }
  if (threadIdx.x == 1023) {
    jobstart[off + nv] = (uint32_t)sc[1023];
    stats[2 * j] = sc[1023];
    stats[2 * j + 1] = sp[1023];
  }
}

// the pre-check needs the candidate pairs only: stats[2 j + 1] = sum over chunk j's values of slots x needles
__global__ __launch_bounds__(1024) void k_join_pairs_only(JoinPlan P, const uint32_t* __restrict__ hist_h,
                                                          const uint32_t* __restrict__ hist_q,
                                                          unsigned long long* __restrict__ stats) {
  const int j = blockIdx.x;
  const uint32_t nv = 1u << (P.lo[j + 1] - P.lo[j]), off = P.voff[j] + (uint32_t)j;
  __shared__ unsigned long long sp[1024];
  unsigned long long p = 0;
  for (uint32_t v = threadIdx.x; v < nv; v += 1024u) p += (unsigned long long)hist_h[off + v] * hist_q[off + v];
  sp[threadIdx.x] = p;
  __syncthreads();
  for (uint32_t d = 512; d > 0; d >>= 1) {
    if (threadIdx.x < d) sp[threadIdx.x] += sp[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) stats[2 * j] = 0ull, stats[2 * j + 1] = sp[0];
}

// item i of x goes to position start[value] + (its turn among the value's items) of chunk j's copy; aux = ids (slots) or
// nullptr (needles: the item's own index)
__global__ __launch_bounds__(256) void k_join_scatter(const uint64_t* __restrict__ x, const uint32_t* __restrict__ aux,
                                                      uint32_t n, JoinPlan P, const uint32_t* __restrict__ start,
                                                      uint32_t* __restrict__ cursor, uint64_t* __restrict__ out_x,
                                                      uint32_t* __restrict__ out_aux) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t h = x[i];
  const uint32_t a = aux ? aux[i] : i;
#pragma unroll 1
  for (int j = 0; j < P.m; ++j) {
    const uint32_t v = P.voff[j] + (uint32_t)j + chunk_of(h, P.lo[j], P.lo[j + 1]);
    const uint32_t pos = start[v] + atomicAdd(&cursor[v], 1u);
    out_x[(size_t)j * n + pos] = h;
    out_aux[(size_t)j * n + pos] = a;
  }
}

// per-wave record buffer in LDS: `has` lanes append {needle, dist, id}; one atomic per flush
__device__ __forceinline__ void join_flush(uint64_t* __restrict__ buf, uint32_t& cnt, cbh_record* __restrict__ rec,
                                           unsigned long long cap, unsigned long long* __restrict__ total) {
  if (cnt == 0) return;
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(total, (unsigned long long)cnt);
  base = __shfl(base, 0);
  for (uint32_t k = lane; k < cnt; k += 64u)
    if (base + k < cap) rec[base + k] = buf[k];
  cnt = 0;
}

// one candidate pair that passed the distance test: is it this chunk's to report, and what is the slot's id?
__device__ __forceinline__ bool join_mine(const JoinPlan& P, int j, uint32_t x0, uint32_t x1, uint64_t qq,
                                          const uint32_t* __restrict__ hay_id, size_t at, uint32_t keep0, uint32_t* id) {
  const uint64_t x = ((uint64_t)x1 << 32) | x0;
  bool mine = qq != 0;  // null needles never match
  for (int e = 0; e < j; ++e) mine = mine && chunk_of(x, P.lo[e], P.lo[e + 1]) != 0u;  // an earlier chunk's pair
  if (mine) {
    *id = hay_id[at];
    mine = *id != 0 || keep0;  // removed slots only where the caller asked for them
  }
  return mine;
}

// `hit` lanes park {needle, dist, id}; wave-uniform count, flushed with one atomic
__device__ __forceinline__ void join_push(uint64_t* __restrict__ buf, uint32_t& cnt, bool hit, uint32_t qidx, uint32_t d,
                                          uint32_t id, cbh_record* __restrict__ rec, unsigned long long cap,
                                          unsigned long long* __restrict__ total) {
  const unsigned long long bm = __builtin_amdgcn_ballot_w64(hit);
  if (bm == 0) return;
  if (hit) {
    const uint32_t k = cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
    buf[k] = ((cbh_record)qidx << 39) | ((cbh_record)d << 32) | id;
  }
  cnt += (uint32_t)__popcll(bm);
  if (cnt >= kOutCap) join_flush(buf, cnt, rec, cap, total);
}

// chunk j's join, wide buckets (chunks of <= 11 bits: hundreds to thousands of slots and needles per value): blockIdx.x = a
// job = (value, tile of 2 x 256 of its slots, block of kJQ of its needles).  A lane holds two slots, the needles stream
// through the scalar cache eight at a time; one test per eight needles and two slots, the exact look only behind it.
__global__ __launch_bounds__(kJT) void k_join_pairs(int j, JoinPlan P, uint32_t n, uint32_t nq,
                                                    const uint64_t* __restrict__ hay_x, const uint32_t* __restrict__ hay_id,
                                                    const uint64_t* __restrict__ q_x, const uint32_t* __restrict__ q_idx,
                                                    const uint32_t* __restrict__ start_h, const uint32_t* __restrict__ start_q,
                                                    const uint32_t* __restrict__ jobstart, uint32_t thresh,
                                                    cbh_record* __restrict__ rec, unsigned long long cap,
                                                    unsigned long long* __restrict__ total, uint32_t keep0) {
  __shared__ uint64_t s_out[kJT / 64][kOutCap + 64];
  const uint32_t off = P.voff[j] + (uint32_t)j, nv = 1u << (P.lo[j + 1] - P.lo[j]);
  // the value whose jobs hold this one: the last v with jobstart[v] <= job (uniform: scalar loads)
  const uint32_t job = blockIdx.x;
  uint32_t lo = 0, hi = nv;  // jobstart[lo] <= job < jobstart[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (jobstart[off + mid] <= job) lo = mid; else hi = mid;
  }
  const uint32_t v = lo, rel = job - jobstart[off + v];
  const uint32_t hs = start_h[off + v], he = start_h[off + v + 1], qs = start_q[off + v], qe = start_q[off + v + 1];
  const uint32_t ht = (he - hs + kJH - 1u) / kJH;  // slot tiles of the value
  const uint32_t it = rel % ht, iq = rel / ht;
  const uint32_t i0 = hs + it * kJH + threadIdx.x, i1 = i0 + (uint32_t)kJT;
  const bool live0 = i0 < he, live1 = i1 < he;
  const uint64_t* __restrict__ hxp = hay_x + (size_t)j * n;
  const uint64_t a0 = hxp[live0 ? i0 : hs], a1 = hxp[live1 ? i1 : hs];
  const uint32_t a0l = (uint32_t)a0, a0h = (uint32_t)(a0 >> 32), a1l = (uint32_t)a1, a1h = (uint32_t)(a1 >> 32);
  const uint32_t q0 = qs + iq * kJQ, q1 = min(qe, q0 + kJQ);
  uint64_t* buf = s_out[threadIdx.x >> 6];
  uint32_t cnt = 0;  // (wave-uniform)
  const uint64_t* __restrict__ qx = q_x + (size_t)j * nq;
  const uint32_t* __restrict__ qix = q_idx + (size_t)j * nq;
  auto exact = [&](uint32_t qi) {  // one needle against the lane's two slots
    const uint64_t qq = qx[qi];
    const uint32_t ql = (uint32_t)qq, qh = (uint32_t)(qq >> 32);
    {
      const uint32_t x0 = a0l ^ ql, x1 = a0h ^ qh, d = __popc(x0) + __popc(x1);
      uint32_t id = 0;
      const bool hit = live0 && d < thresh && join_mine(P, j, x0, x1, qq, hay_id, (size_t)j * n + i0, keep0, &id);
      join_push(buf, cnt, hit, hit ? qix[qi] : 0u, d, id, rec, cap, total);
    }
    {
      const uint32_t x0 = a1l ^ ql, x1 = a1h ^ qh, d = __popc(x0) + __popc(x1);
      uint32_t id = 0;
      const bool hit = live1 && d < thresh && join_mine(P, j, x0, x1, qq, hay_id, (size_t)j * n + i1, keep0, &id);
      join_push(buf, cnt, hit, hit ? qix[qi] : 0u, d, id, rec, cap, total);
    }
  };
  uint32_t qi = q0;
  // (a 64-bit pointer bump keeps the eight loads of a block at constant offsets from one SGPR base -- wave-uniform, so they
  // are scalar loads; the next block is fetched while this one is compared: hamm64_scan.hip's loop)
  const uint2* __restrict__ qp = reinterpret_cast<const uint2*>(qx) + q0;
  uint2 cur[8];
  if (qi + 8u <= q1) {
#pragma unroll
    for (int k = 0; k < 8; ++k) cur[k] = qp[k];
  }
  for (; qi + 8u <= q1; qi += 8u) {
    uint2 nxt[8];
    qp += 8;
    if (qi + 16u <= q1) {
#pragma unroll
      for (int k = 0; k < 8; ++k) nxt[k] = qp[k];
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) nxt[k] = make_uint2(0u, 0u);
    }
    uint32_t m0 = 64u, m1 = 64u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      m0 = min(m0, (uint32_t)__popc(a0l ^ cur[k].x) + (uint32_t)__popc(a0h ^ cur[k].y));
      m1 = min(m1, (uint32_t)__popc(a1l ^ cur[k].x) + (uint32_t)__popc(a1h ^ cur[k].y));
    }
    if (__builtin_amdgcn_ballot_w64((live0 && m0 < thresh) || (live1 && m1 < thresh)) != 0) {  // (one block in 10^2 .. 10^4)
#pragma unroll 1
      for (uint32_t k = 0; k < 8u; ++k) exact(qi + k);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) cur[k] = nxt[k];
  }
#pragma unroll 1
  for (; qi < q1; ++qi) exact(qi);
  join_flush(buf, cnt, rec, cap, total);
}

// chunk j's join, narrow buckets (chunks of >= 12 bits: a handful of slots and needles per value): a lane takes one slot of
// the chunk's order and walks ITS value's needles (the lanes of a wave walk different lists: per-lane loads, a uniform loop
// until the longest is done) -- 10^8 .. 10^9 pairs in all, where a workgroup per value would be a million launches of
// fifteen lanes.
__global__ __launch_bounds__(kJT) void k_join_narrow(int j, JoinPlan P, uint32_t n, uint32_t nq,
                                                     const uint64_t* __restrict__ hay_x, const uint32_t* __restrict__ hay_id,
                                                     const uint64_t* __restrict__ q_x, const uint32_t* __restrict__ q_idx,
                                                     const uint32_t* __restrict__ start_q, uint32_t thresh,
                                                     cbh_record* __restrict__ rec, unsigned long long cap,
                                                     unsigned long long* __restrict__ total, uint32_t keep0) {
  __shared__ uint64_t s_out[kJT / 64][kOutCap + 64];
  const uint32_t off = P.voff[j] + (uint32_t)j;
  const uint32_t i = blockIdx.x * (uint32_t)kJT + threadIdx.x;
  const bool live = i < n;
  const uint64_t a = hay_x[(size_t)j * n + (live ? i : 0u)];
  const uint32_t al = (uint32_t)a, ah = (uint32_t)(a >> 32);
  const uint32_t v = chunk_of(a, P.lo[j], P.lo[j + 1]);
  uint32_t qi = live ? start_q[off + v] : 0u;
  const uint32_t qe = live ? start_q[off + v + 1] : 0u;
  uint64_t* buf = s_out[threadIdx.x >> 6];
  uint32_t cnt = 0;
  const uint64_t* __restrict__ qx = q_x + (size_t)j * nq;
  while (__builtin_amdgcn_ballot_w64(qi < qe) != 0) {
    const bool act = qi < qe;
    const uint64_t qq = act ? qx[qi] : 0ull;
    const uint32_t x0 = al ^ (uint32_t)qq, x1 = ah ^ (uint32_t)(qq >> 32), d = __popc(x0) + __popc(x1);
    bool hit = act && d < thresh;
    if (__builtin_amdgcn_ballot_w64(hit) != 0) {
      uint32_t id = 0;
      hit = hit && join_mine(P, j, x0, x1, qq, hay_id, (size_t)j * n + i, keep0, &id);
      join_push(buf, cnt, hit, hit ? q_idx[(size_t)j * nq + qi] : 0u, d, id, rec, cap, total);
    }
    ++qi;
  }
  join_flush(buf, cnt, rec, cap, total);
}

// four chunks of 16 bits (thresholds <= 4): the needles need no order at all -- a lane takes a NEEDLE
// and, chunk after chunk, walks the slots that share its value (the slots' side alone is histogrammed, scanned and
// scattered: half the bookkeeping of a call whose join proper is a tenth of a millisecond)
__global__ __launch_bounds__(kJT) void k_join_by_needle(JoinPlan P, uint32_t n, uint32_t nq, const uint64_t* __restrict__ hay_x,
                                                        const uint32_t* __restrict__ hay_id, const uint64_t* __restrict__ q,
                                                        const uint32_t* __restrict__ start_h, uint32_t thresh,
                                                        cbh_record* __restrict__ rec, unsigned long long cap,
                                                        unsigned long long* __restrict__ total, uint32_t keep0) {
  __shared__ uint64_t s_out[kJT / 64][kOutCap + 64];
  const uint32_t i = blockIdx.x * (uint32_t)kJT + threadIdx.x;
  const uint64_t qq = i < nq ? q[i] : 0ull;
  const bool live = qq != 0;  // (null needles never match)
  const uint32_t ql = (uint32_t)qq, qh = (uint32_t)(qq >> 32);
  uint64_t* buf = s_out[threadIdx.x >> 6];
  uint32_t cnt = 0;
#pragma unroll 1
  for (int j = 0; j < P.m; ++j) {
    const uint32_t off = P.voff[j] + (uint32_t)j + chunk_of(qq, P.lo[j], P.lo[j + 1]);
    uint32_t hi_ = live ? start_h[off] : 0u;
    const uint32_t he = live ? start_h[off + 1] : 0u;
    const uint64_t* __restrict__ hx = hay_x + (size_t)j * n;
    while (__builtin_amdgcn_ballot_w64(hi_ < he) != 0) {
      const bool act = hi_ < he;
      const uint64_t a = act ? hx[hi_] : 0ull;
      const uint32_t x0 = (uint32_t)a ^ ql, x1 = (uint32_t)(a >> 32) ^ qh, d = __popc(x0) + __popc(x1);
      bool hit = act && d < thresh;
      if (__builtin_amdgcn_ballot_w64(hit) != 0) {
        uint32_t id = 0;
        hit = hit && join_mine(P, j, x0, x1, qq, hay_id, (size_t)j * n + hi_, keep0, &id);
        join_push(buf, cnt, hit, i, d, id, rec, cap, total);
      }
      ++hi_;
    }
  }
  join_flush(buf, cnt, rec, cap, total);
}

constexpr int g_join_model_ps_e3 = 250;  // the launcher's cost model: 0.25 ns of ONE SIMD lane... i.e. 2.5e-13 s of the
                                         // machine per candidate pair (measured 2.8e-13 at threshold 8)

std::atomic<long long> g_n_join{0}, g_n_needle_preps{0};
std::atomic<int> g_join_resident{0}, g_join_resident_mb{2048};

JoinPlan make_plan(int thresh) {
  JoinPlan P;
  memset(&P, 0, sizeof P);
  P.m = std::max(4, thresh);
  uint32_t nvals = 0;
  for (int j = 0; j <= P.m; ++j) P.lo[j] = (64 * j + P.m / 2) / P.m;
  for (int j = 0; j < P.m; ++j) {
    P.voff[j] = nvals;
    nvals += 1u << (P.lo[j + 1] - P.lo[j]);
  }
  P.voff[P.m] = nvals;
  return P;
}
size_t plan_entries(const JoinPlan& P) { return (size_t)P.voff[P.m] + (size_t)P.m; }  // one extra entry per chunk

// the full histogram of n items into the zeroed `hist`: privatised in LDS where every chunk fits (plans 5..8)
void launch_hist(const uint64_t* x, size_t n, const JoinPlan& P, uint32_t* hist, hipStream_t stream) {
  if (P.m >= 5)
    hipLaunchKernelGGL(k_join_hist_lds, dim3((unsigned)((n + kHistSpan - 1) / kHistSpan), (unsigned)P.m), dim3(256), 0, stream,
                       x, (uint32_t)n, P, hist);
  else
    hipLaunchKernelGGL(k_join_hist, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, (uint32_t)n, 1u, P, hist);
}

// the needles' side in two steps, so that a launch can count its candidate pairs before it orders anything
int needles_alloc(const JoinPlan& P, size_t nq, hipStream_t stream, JoinNeedles* N) {
  N->m = P.m, N->nq = nq, N->stream = stream;
  CBH_HIP(malloc_async((void**)&N->start_q, plan_entries(P) * 4, stream));
  CBH_HIP(malloc_async((void**)&N->qx, (size_t)P.m * nq * 8, stream));
  CBH_HIP(malloc_async((void**)&N->qidx, (size_t)P.m * nq * 4, stream));
  return CBH_OK;
}
int needles_count(const uint64_t* d_q, size_t nq, const JoinPlan& P, uint32_t* cursor, hipStream_t stream, JoinNeedles* N) {
  CBH_HIP(hipMemsetAsync(cursor, 0, plan_entries(P) * 4, stream));
  launch_hist(d_q, nq, P, cursor, stream);
  hipLaunchKernelGGL(k_join_scan1, dim3((unsigned)P.m), dim3(1024), 0, stream, P, cursor, N->start_q, 1u);
  CBH_HIP(hipGetLastError());
  g_n_needle_preps++;
  return CBH_OK;
}
void needles_scatter(const uint64_t* d_q, size_t nq, const JoinPlan& P, uint32_t* cursor, hipStream_t stream, JoinNeedles* N) {
  hipLaunchKernelGGL(k_join_scatter, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, d_q, (const uint32_t*)nullptr,
                     (uint32_t)nq, P, N->start_q, cursor, N->qx, N->qidx);
}

}  // namespace

long long get_scan_joins() { return g_n_join.load(); }
long long get_join_needle_preps() { return g_n_needle_preps.load(); }
int set_join_resident(int v) {
  if (v != 0 && v != 1) return CBH_E_INVAL;
  g_join_resident = v;
  return CBH_OK;
}
int set_join_resident_mb(int v) {
  if (v < 0) return CBH_E_INVAL;
  g_join_resident_mb = v;
  return CBH_OK;
}
int get_join_resident() { return g_join_resident.load(); }
int get_join_resident_mb() { return g_join_resident_mb.load(); }

// ---- the resident slot tables --------------------------------------------------------------------------------------------

JoinTables::~JoinTables() {
  int prev = -1;
  if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  if (prev != device) (void)hipSetDevice(device);
  if (hist_h) (void)hipFree(hist_h);
  if (start_h) (void)hipFree(start_h);
  if (hx) (void)hipFree(hx);
  if (hid) (void)hipFree(hid);
  if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
}

std::shared_ptr<const JoinTables> JoinCache::current(int m) {
  std::lock_guard<std::mutex> lk(mu);
  return plan[m];
}

uint32_t JoinCache::plans() {
  std::lock_guard<std::mutex> lk(mu);
  uint32_t b = 0;
  for (int m = 4; m <= kJoinMaxThresh; ++m)
    if (plan[m]) b |= 1u << m;
  return b;
}

void JoinCache::drop_all() {
  std::lock_guard<std::mutex> lk(mu);
  for (int m = 4; m <= kJoinMaxThresh; ++m)
    if (plan[m]) {
      bytes -= plan[m]->bytes;
      plan[m].reset();  // (the memory goes when the last launch that reads it has let go)
      drops++;
    }
}

std::shared_ptr<const JoinTables> JoinCache::get_or_build(int m, const uint64_t* d_hashes, const uint32_t* d_ids, size_t n,
                                                          int device, hipStream_t stream, int* rc) {
  std::lock_guard<std::mutex> lk(mu);
  *rc = CBH_OK;
  if (plan[m] && plan[m]->n == n) return plan[m];  // a concurrent first call has built it
  if (plan[m]) {  // (of another size: no mutation path leaves one behind, and a table never outlives its contents)
    bytes -= plan[m]->bytes;
    plan[m].reset();
    drops++;
  }
  const JoinPlan P = make_plan(m);
  const size_t entries = plan_entries(P), cost = (size_t)12 * P.m * n + 2 * entries * 4;
  auto give_up = [&](int code) -> std::shared_ptr<const JoinTables> {
    failed_builds++;
    *rc = code;
    return nullptr;
  };
  if (bytes.load() + cost > ((uint64_t)(unsigned)g_join_resident_mb.load() << 20)) {
    set_last_error_text("join tables: over the \"join_resident_mb\" budget");
    return give_up(CBH_E_NOMEM);
  }
  std::shared_ptr<JoinTables> T(new (std::nothrow) JoinTables);
  if (!T) return give_up(CBH_E_NOMEM);
  T->m = P.m, T->n = n, T->bytes = cost, T->device = device;
  // everything is allocated before anything is written, let alone published (a failure frees what T holds)
  Scratch scratch(stream);
  uint32_t* cursor = nullptr;
  hipError_t e;
  if ((e = hipMalloc(&T->hist_h, entries * 4)) != hipSuccess || (e = hipMalloc(&T->start_h, entries * 4)) != hipSuccess ||
      (e = hipMalloc(&T->hx, (size_t)P.m * n * 8)) != hipSuccess || (e = hipMalloc(&T->hid, (size_t)P.m * n * 4)) != hipSuccess ||
      (e = scratch.get(&cursor, entries * 4)) != hipSuccess) {
    return give_up(fail("join tables", e));
  }
  if ((e = hipMemsetAsync(T->hist_h, 0, entries * 4, stream)) == hipSuccess && (e = hipMemsetAsync(cursor, 0, entries * 4, stream)) == hipSuccess) {
    launch_hist(d_hashes, n, P, T->hist_h, stream);
    hipLaunchKernelGGL(k_join_scan1, dim3((unsigned)P.m), dim3(1024), 0, stream, P, T->hist_h, T->start_h, 0u);
    hipLaunchKernelGGL(k_join_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_hashes, d_ids, (uint32_t)n, P,
                       T->start_h, cursor, T->hx, T->hid);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(stream);  // complete before any other stream may read them
  if (e != hipSuccess) {
    set_last_error("join tables build", e);
    return give_up(CBH_E_HIP);
  }
  plan[m] = T;
  bytes += cost;
  builds++;
  return T;
}

void JoinNeedles::free() {
  if (start_q) (void)free_async(start_q, stream);
  if (qx) (void)free_async(qx, stream);
  if (qidx) (void)free_async(qidx, stream);
  start_q = nullptr, qidx = nullptr, qx = nullptr;
}

int join_prepare_needles(const uint64_t* d_q, size_t nq, int thresh, hipStream_t stream, JoinNeedles* out) {
  const JoinPlan P = make_plan(thresh);
  if (P.m < 5 || P.m > kMaxChunks || nq == 0) return CBH_E_INVAL;
  Scratch scratch(stream);
  uint32_t* cursor = nullptr;
  int rc = needles_alloc(P, nq, stream, out);
  if (!rc) {
    hipError_t e = scratch.get(&cursor, plan_entries(P) * 4);
    if (e != hipSuccess) rc = fail("join needles", e);
  }
  if (!rc) rc = needles_count(d_q, nq, P, cursor, stream, out);
  if (!rc) {
    needles_scatter(d_q, nq, P, cursor, stream, out);
    if (hipGetLastError() != hipSuccess) rc = CBH_E_HIP;
  }
  if (rc) out->free();
  return rc;
}

// CBH_OK: done (records appended, *d_total advanced like the scans do); CBH_E_UNSUPPORTED: the caller's scan is cheaper
// (or `force` is false and the call is too small to be worth the bookkeeping) -- nothing has been written.
int launch_hamm64_join(const uint64_t* d_hashes, const uint32_t* d_ids, size_t n, const uint64_t* d_q, size_t nq,
                       int thresh, cbh_record* d_rec, size_t cap, unsigned long long* d_total, hipStream_t stream,
                       const ScanOpts& o, bool force, double scan_ms_estimate) {
  const JoinPlan P = make_plan(thresh);
  const size_t entries = plan_entries(P);
  const bool keep_id0 = o.keep_id0;
  // (16-bit chunks only: ~15 slots a value.  At five chunks of 12-13 bits a needle walks 5 x 122 slots by per-lane loads: 5.8 ms
  // against the 2.9 of sorting both sides)
  const bool by_needle = P.m == 4;
  JoinCache* jc = o.join && o.join_hold && o.join->enabled() ? o.join : nullptr;
  std::shared_ptr<const JoinTables> T;
  if (jc) T = jc->current(P.m);
  if (T && T->n != n) T.reset();
  const bool reused = (bool)T;
  Scratch scratch(stream);
  unsigned long long* stats = nullptr;
  CBH_HIP(scratch.get(&stats, 2 * kMaxChunks * 8));
  unsigned long long h_stats[2 * kMaxChunks];
  uint32_t *hist_h = nullptr, *hist_q = nullptr;  // this call's histograms, then its scatters' cursors
  auto read_stats = [&]() -> int {
    CBH_HIP(hipGetLastError());
    CBH_HIP(hipMemcpyAsync(h_stats, stats, (size_t)2 * P.m * 8, hipMemcpyDeviceToHost, stream));
    CBH_HIP(hipStreamSynchronize(stream));
    return CBH_OK;
  };
  int rc;
  if (!force) {
    // a library of near-identical hashes makes the full histogram itself expensive (10^6 atomics on one counter): look at
    // 16 384 of each side first and leave if THEIR candidate pairs, scaled up, already say the scan is cheaper.  Resident
    // tables have the slots' FULL histogram: only the needles are sampled, and plans 5..8 skip the look altogether (their
    // exact count below costs a needle histogram in LDS and one kernel).
    const uint32_t sh = T ? 1u : (uint32_t)std::max<size_t>(1, n / 16384), sq = (uint32_t)std::max<size_t>(1, nq / 16384);
    if (T ? by_needle : (sh > 1 || sq > 1 || by_needle)) {
      CBH_HIP(scratch.get(&hist_q, entries * 4));
      CBH_HIP(hipMemsetAsync(hist_q, 0, entries * 4, stream));
      const uint32_t* hh = T ? T->hist_h : nullptr;
      if (!T) {
        CBH_HIP(scratch.get(&hist_h, entries * 4));
        CBH_HIP(hipMemsetAsync(hist_h, 0, entries * 4, stream));
        hipLaunchKernelGGL(k_join_hist, dim3((unsigned)(((n + sh - 1) / sh + 255) / 256)), dim3(256), 0, stream, d_hashes,
                           (uint32_t)n, sh, P, hist_h);
        hh = hist_h;
      }
      hipLaunchKernelGGL(k_join_hist, dim3((unsigned)(((nq + sq - 1) / sq + 255) / 256)), dim3(256), 0, stream, d_q, (uint32_t)nq,
                         sq, P, hist_q);
      hipLaunchKernelGGL(k_join_pairs_only, dim3((unsigned)P.m), dim3(1024), 0, stream, P, hh, hist_q, stats);
      if ((rc = read_stats())) return rc;
      double sp = 0;
      for (int j = 0; j < P.m; ++j) sp += (double)h_stats[2 * j + 1];
      // (sampling thins the occupied values' pairs by sh x sq on average; a generous factor keeps borderline calls in --
      // the by-needle form has no exact count behind this one: there the estimate decides, with less slack)
      const double est_ms = sp * (double)sh * (double)sq * (double)g_join_model_ps_e3 * 1e-12;
      if (est_ms > (by_needle ? 0.6 : 4.0) * scan_ms_estimate) return CBH_E_UNSUPPORTED;
    }
  }
  // the slots' side: resident (built now if this is the handle's first call at this plan), or made for this call alone
  if (!T && jc) {
    int device = 0, brc = CBH_OK;
    CBH_HIP(hipGetDevice(&device));
    T = jc->get_or_build(P.m, d_hashes, d_ids, n, device, stream, &brc);
    if (!T) cbh_clear_error();  // (no memory, over budget: not an error of the search, which goes on as it always has)
  }
  uint32_t *own_start_h = nullptr, *own_hid = nullptr, *jobstart = nullptr;
  uint64_t* own_hx = nullptr;
  if (T) {
    *o.join_hold = T;  // (the caller lets go once the stream has finished what is queued below)
    if (reused) jc->hits++;
  } else {
    if (!hist_h) CBH_HIP(scratch.get(&hist_h, entries * 4));
    CBH_HIP(scratch.get(&own_start_h, entries * 4));
    CBH_HIP(scratch.get(&own_hx, (size_t)P.m * n * 8));
    CBH_HIP(scratch.get(&own_hid, (size_t)P.m * n * 4));
  }
  const uint32_t* start_h = T ? T->start_h : own_start_h;
  const uint64_t* hx = T ? T->hx : own_hx;
  const uint32_t* hid = T ? T->hid : own_hid;
  // the needles' side (plans 5..8): the caller's, prepared once for several launches, or this call's own
  struct OwnNeedles : JoinNeedles {
    ~OwnNeedles() { free(); }
  } own_needles;
  const JoinNeedles* N = nullptr;
  if (!by_needle) {
    CBH_HIP(scratch.get(&jobstart, entries * 4));
    if (o.join_needles && o.join_needles->m == P.m && o.join_needles->nq == nq) {
      N = o.join_needles;
    } else {
      if (!hist_q) CBH_HIP(scratch.get(&hist_q, entries * 4));
      if ((rc = needles_alloc(P, nq, stream, &own_needles))) return rc;
      N = &own_needles;
    }
  }
  // ---- every block is taken: from here on nothing fails for lack of memory, and no record has been written yet
  auto scatter_slots = [&] {
    hipLaunchKernelGGL(k_join_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_hashes, d_ids, (uint32_t)n, P,
                       own_start_h, hist_h, own_hx, own_hid);
  };
  if (!T) {
    CBH_HIP(hipMemsetAsync(hist_h, 0, entries * 4, stream));
    launch_hist(d_hashes, n, P, hist_h, stream);
    hipLaunchKernelGGL(k_join_scan1, dim3((unsigned)P.m), dim3(1024), 0, stream, P, hist_h, own_start_h, 1u);
  }
  if (by_needle) {  // (with resident tables: this kernel and nothing else)
    if (!T) scatter_slots();
    hipLaunchKernelGGL(k_join_by_needle, dim3((unsigned)((nq + kJT - 1) / kJT)), dim3(kJT), 0, stream, P, (uint32_t)n,
                       (uint32_t)nq, hx, hid, d_q, start_h, (uint32_t)thresh, d_rec, (unsigned long long)cap, d_total,
                       (uint32_t)keep_id0);
    CBH_HIP(hipGetLastError());
    g_n_join++;
    return CBH_OK;
  }
  if (N == &own_needles && (rc = needles_count(d_q, nq, P, hist_q, stream, &own_needles))) return rc;
  hipLaunchKernelGGL(k_join_jobs, dim3((unsigned)P.m), dim3(1024), 0, stream, P, start_h, N->start_q, jobstart, stats);
  if ((rc = read_stats())) return rc;
  double pairs = 0;
  unsigned long long jobs_max = 0;
  for (int j = 0; j < P.m; ++j) {
    pairs += (double)h_stats[2 * j + 1];
    jobs_max = std::max(jobs_max, h_stats[2 * j]);
  }
  if (jobs_max > 0x7fffffffull) return CBH_E_UNSUPPORTED;
  if (!force) {
    const double join_ms = pairs * (double)g_join_model_ps_e3 * 1e-12 + 0.1 * P.m + 0.2;
    if (join_ms > 0.9 * scan_ms_estimate) return CBH_E_UNSUPPORTED;
  }
  if (!T) scatter_slots();
  if (N == &own_needles) needles_scatter(d_q, nq, P, hist_q, stream, &own_needles);
  for (int j = 0; j < P.m; ++j) {
    if (h_stats[2 * j] == 0) continue;
    if (P.lo[j + 1] - P.lo[j] >= 12)
      hipLaunchKernelGGL(k_join_narrow, dim3((unsigned)((n + kJT - 1) / kJT)), dim3(kJT), 0, stream, j, P, (uint32_t)n,
                         (uint32_t)nq, hx, hid, N->qx, N->qidx, N->start_q, (uint32_t)thresh, d_rec, (unsigned long long)cap,
                         d_total, (uint32_t)keep_id0);
    else
      hipLaunchKernelGGL(k_join_pairs, dim3((unsigned)h_stats[2 * j]), dim3(kJT), 0, stream, j, P, (uint32_t)n, (uint32_t)nq,
                         hx, hid, N->qx, N->qidx, start_h, N->start_q, jobstart, (uint32_t)thresh, d_rec,
                         (unsigned long long)cap, d_total, (uint32_t)keep_id0);
  }
  CBH_HIP(hipGetLastError());
  g_n_join++;
  return CBH_OK;
}

}  // namespace cbh
