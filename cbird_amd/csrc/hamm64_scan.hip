// hamm64_scan.hip -- K3: all-pairs 64-bit Hamming threshold scan for gfx950 (CDNA4).
//
// Replaces the per-needle tree walk behind DctHashIndex::find (src/dcthashindex.cpp:193-220;
// VpTree::thresholdSearch src/tree/vptree.h:228-255) with the exact brute-force predicate the
// reference states at dcthashindex.cpp:210-217:  hamm64(q, hash[i]) < thresh  &&  id[i] != 0
// (hamm64 = popcountll(a ^ b), src/hamm.h:24-26), evaluated for a whole batch of needles.
//
// Mapping to the machine (see NOTES.md "k_hamm64_scan")
//  * haystack slots live in VGPRs: each lane owns H=8 slots (16 VGPRs), a 256-thread workgroup
//    owns a tile of 2048 slots, loaded once with coalesced 8-B loads;
//  * needles are wave-uniform: they stream through the scalar cache (s_load_dwordx16 = 8 needles)
//    and feed the VALU as SGPR operands, so the inner loop has no vector memory traffic at all;
//  * per (needle, slot): v_xor_b32 + v_bcnt_u32_b32 on the low word (plus xor+bcnt-accumulate on
//    the high word in the FULL variant); two needles fold into one v_min3_u32 against a running
//    per-slot minimum.  After QB=8 needles one compare decides whether anything in the
//    8x8x64 block can be under threshold; only then the exact 64-bit distances are recomputed
//    and records are appended (wave-aggregated atomic).  PRE (low-word prefilter) is exact
//    because popc(lo) <= popc(lo)+popc(hi): a pair whose low-word distance is already >= thresh
//    cannot match.  It is used for small thresholds where the low word alone rejects almost
//    every block; FULL is used otherwise.
//  * grid = (slot tiles) x (needle chunks); consecutive blockIdx.x share a needle chunk, so the
//    workgroups resident at one time stream the same few needle chunks out of L2.
// The end of the file: launch_hamm64_scan, the entry of every 64-bit threshold search, and the one place that decides
// which path a search takes.
#include <atomic>

#include "cbh_internal.h"

namespace cbh {
namespace {

constexpr int kThreads = 256;
constexpr int kH = 8;   // haystack slots per lane
constexpr int kQB = 8;  // needles per check block (one s_load_dwordx16)

__device__ __forceinline__ uint32_t min3u(uint32_t a, uint32_t b, uint32_t c) {
  return min(min(a, b), c);  // -> v_min3_u32
}

__device__ __forceinline__ void emit(cbh_record* __restrict__ rec, unsigned long long cap,
                                     unsigned long long* __restrict__ total, uint32_t qidx,
                                     uint32_t dist, uint32_t id) {
  unsigned long long slot = atomicAdd(total, 1ull);  // compiler aggregates per wave
  if (slot < cap) rec[slot] = ((cbh_record)qidx << 39) | ((cbh_record)dist << 32) | id;
}

// exact evaluation of needles [qa, qb) (read back from memory) against this lane's H slots
template <int H>
__device__ __forceinline__ void exact_block(const uint2 (&h)[H], uint32_t base_idx, uint32_t n,
                                            const uint32_t* __restrict__ ids,
                                            const uint64_t* __restrict__ q, uint32_t qa,
                                            uint32_t qb, uint32_t thresh,
                                            cbh_record* __restrict__ rec, unsigned long long cap,
                                            unsigned long long* __restrict__ total,
                                            uint32_t keep0, const uint2* __restrict__ qmask) {
#pragma unroll 1
  for (uint32_t qi = qa; qi < qb; ++qi) {
    const uint64_t qq = q[qi];
    if (qq == 0) continue;  // null needle: DctHashIndex::find returns nothing (:196-200)
    const uint32_t ql = (uint32_t)qq, qh = (uint32_t)(qq >> 32);
    const uint2 mk = qmask ? qmask[qi] : make_uint2(0u, 0u);  // bits that must be equal (tree/bucket modes)
#pragma unroll
    for (int j = 0; j < H; ++j) {
      const uint32_t d = __popc(h[j].x ^ ql) + __popc(h[j].y ^ qh);
      if (d < thresh && (((h[j].x ^ ql) & mk.x) | ((h[j].y ^ qh) & mk.y)) == 0) {
        const uint32_t idx = base_idx + (uint32_t)j * kThreads;
        if (idx < n) {
          const uint32_t id = ids[idx];
          if (id != 0 || keep0) emit(rec, cap, total, qi, d, id);
        }
      }
    }
  }
}

// second level of the filter: only slots whose running minimum fell under the threshold are
// re-evaluated exactly against the QB needles of the block.  The needles are still in SGPRs
// (cur[]), so this costs ~5 VALU ops per needle and no memory access; the media id is fetched
// only for a pair that really matches (about one in 10^6 on distinct images).
template <int H, int QB>
__device__ __forceinline__ void refine_block(const uint2 (&h)[H], const uint32_t (&acc)[H],
                                             const uint2 (&cur)[QB], uint32_t base_idx, uint32_t n,
                                             const uint32_t* __restrict__ ids, uint32_t qb,
                                             uint32_t thresh, cbh_record* __restrict__ rec,
                                             unsigned long long cap,
                                             unsigned long long* __restrict__ total,
                                             uint32_t keep0, const uint2* __restrict__ qmask) {
#pragma unroll
  for (int j = 0; j < H; ++j) {
    if (acc[j] < thresh) {
      const uint32_t idx = base_idx + (uint32_t)j * kThreads;
      // exact distances of the QB needles to slot j; one branch for the (rare) real match
      uint32_t d[QB];
#pragma unroll
      for (int i = 0; i < QB; ++i) d[i] = __popc(h[j].x ^ cur[i].x) + __popc(h[j].y ^ cur[i].y);
      uint32_t m = d[0];
#pragma unroll
      for (int i = 1; i + 1 < QB; i += 2) m = min3u(m, d[i], d[i + 1]);
      if (QB % 2 == 0) m = min(m, d[QB - 1]);
      if (m < thresh && idx < n) {
        const uint32_t id = ids[idx];
        if (id != 0 || keep0) {
#pragma unroll
          for (int i = 0; i < QB; ++i)
            if (d[i] < thresh && (cur[i].x | cur[i].y) != 0) {
              const uint2 mk = qmask ? qmask[qb + (uint32_t)i] : make_uint2(0u, 0u);
              if ((((h[j].x ^ cur[i].x) & mk.x) | ((h[j].y ^ cur[i].y) & mk.y)) == 0)
                emit(rec, cap, total, qb + (uint32_t)i, d[i], id);
            }
        }
      }
    }
  }
}

enum { MODE_PRE = 0, MODE_FULL = 1, MODE_EQ = 2 };

template <int H, int QB, int MODE>
__global__ __launch_bounds__(kThreads) void k_hamm64_scan(
    const uint2* __restrict__ hay, const uint32_t* __restrict__ ids, uint32_t n,
    const uint64_t* __restrict__ q, uint32_t nq, uint32_t q_chunk, uint32_t thresh,
    cbh_record* __restrict__ rec, unsigned long long cap, unsigned long long* __restrict__ total,
    uint32_t keep0, const uint2* __restrict__ qmask) {
  const uint32_t base_idx = blockIdx.x * (uint32_t)(kThreads * H) + threadIdx.x;
  uint2 h[H];
#pragma unroll
  for (int j = 0; j < H; ++j) {
    const uint32_t idx = base_idx + (uint32_t)j * kThreads;
    h[j] = idx < n ? hay[idx] : make_uint2(0u, 0u);
  }
  const uint32_t q0 = blockIdx.y * q_chunk;
  const uint32_t q1 = min(nq, q0 + q_chunk);
  uint32_t qb = q0;
  // needles as (lo,hi) dword pairs; 64-bit pointer bump keeps the 8 loads of a block at constant
  // offsets from one SGPR base (wave-uniform -> SMEM)
  const uint2* __restrict__ qp = reinterpret_cast<const uint2*>(q) + (size_t)q0;

  uint2 cur[QB];
  if (qb + QB <= q1) {
#pragma unroll
    for (int i = 0; i < QB; ++i) cur[i] = qp[i];
  }
  for (; qb + QB <= q1; qb += QB) {
    // prefetch the next block of needles while this one is being compared
    uint2 nxt[QB];
    qp += QB;
    if (qb + 2 * QB <= q1) {
#pragma unroll
      for (int i = 0; i < QB; ++i) nxt[i] = qp[i];
    } else {
#pragma unroll
      for (int i = 0; i < QB; ++i) nxt[i] = make_uint2(0u, 0u);
    }
    if (MODE == MODE_EQ) {
      // dht == 1: distance < 1 is equality -- one v_cmp_eq_u64 per pair, OR-ed on the scalar unit
      unsigned long long any = 0;
#pragma unroll
      for (int i = 0; i < QB; ++i) {
        const unsigned long long qq = ((unsigned long long)cur[i].y << 32) | cur[i].x;
#pragma unroll
        for (int j = 0; j < H; ++j) {
          const unsigned long long hh = ((unsigned long long)h[j].y << 32) | h[j].x;
          any |= __ballot(hh == qq);
        }
      }
      if (any) exact_block<H>(h, base_idx, n, ids, q, qb, qb + QB, thresh, rec, cap, total, keep0, qmask);
    } else {
      uint32_t acc[H];
#pragma unroll
      for (int j = 0; j < H; ++j) acc[j] = 0xffu;
      // Issue-rate shaping (tools/ubench/valu_rate.hip): VGPR-only v_xor_b32 runs at 32 lanes/clk
      // only inside long runs of such ops, while v_bcnt/v_min3 (and any op with an SGPR source)
      // run at 16 lanes/clk and cost a ~25-cycle mode switch when interleaved.  So: broadcast
      // the needles into VGPRs, do all QB*H xors back to back, then all the popcounts/minima.
      uint32_t ql[QB], qh[QB];
#pragma unroll
      for (int i = 0; i < QB; ++i) {
        asm volatile("v_mov_b32 %0, %1" : "=v"(ql[i]) : "s"(cur[i].x));
        if (MODE == MODE_FULL) asm volatile("v_mov_b32 %0, %1" : "=v"(qh[i]) : "s"(cur[i].y));
      }
      uint32_t x[QB][H];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < QB; ++i)
#pragma unroll
        for (int j = 0; j < H; ++j) x[i][j] = h[j].x ^ ql[i];
      __builtin_amdgcn_sched_barrier(0);
      if (MODE == MODE_FULL) {
#pragma unroll
        for (int i = 0; i < QB; ++i)
#pragma unroll
          for (int j = 0; j < H; ++j) x[i][j] = (uint32_t)__popc(x[i][j]);
        uint32_t y[QB][H];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < QB; ++i)
#pragma unroll
          for (int j = 0; j < H; ++j) y[i][j] = h[j].y ^ qh[i];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < QB; i += 2)
#pragma unroll
          for (int j = 0; j < H; ++j)
            acc[j] = min3u(acc[j], x[i][j] + (uint32_t)__popc(y[i][j]),
                           x[i + 1][j] + (uint32_t)__popc(y[i + 1][j]));
      } else {
#pragma unroll
        for (int i = 0; i < QB; i += 2)
#pragma unroll
          for (int j = 0; j < H; ++j)
            acc[j] = min3u(acc[j], (uint32_t)__popc(x[i][j]), (uint32_t)__popc(x[i + 1][j]));
      }
      __builtin_amdgcn_sched_barrier(0);
      uint32_t m = acc[0];
#pragma unroll
      for (int j = 1; j + 1 < H; j += 2) m = min3u(m, acc[j], acc[j + 1]);
      if (H % 2 == 0) m = min(m, acc[H - 1]);
      if (m < thresh) refine_block<H, QB>(h, acc, cur, base_idx, n, ids, qb, thresh, rec, cap, total, keep0, qmask);
    }
#pragma unroll
    for (int i = 0; i < QB; ++i) cur[i] = nxt[i];
  }
  if (qb < q1) exact_block<H>(h, base_idx, n, ids, q, qb, q1, thresh, rec, cap, total, keep0, qmask);
}

// ScanOpts::zero_needles: the records of the needles whose hash is 0, which every scan kernel skips.  Such needles are rare
// (a black frame of a needle video, a flat keypoint patch) and the slots within `thresh` of 0 rarer still, so this is two
// small launches behind the scan: the zero needles into list[1..], their number into list[0] (zeroed by the caller); then
// one lane per slot, which leaves at once unless popcount(slot) < thresh.
__global__ __launch_bounds__(256) void k_zero_needle_list(const uint64_t* __restrict__ q, uint32_t nq,
                                                          uint32_t* __restrict__ list /* nq + 1 */) {
  const uint32_t qi = blockIdx.x * 256u + threadIdx.x;
  if (qi < nq && q[qi] == 0) list[1u + atomicAdd(&list[0], 1u)] = qi;
}

__global__ __launch_bounds__(256) void k_zero_needle_scan(const uint2* __restrict__ hay, const uint32_t* __restrict__ ids,
                                                          uint32_t n, const uint32_t* __restrict__ list, uint32_t thresh,
                                                          cbh_record* __restrict__ rec, unsigned long long cap,
                                                          unsigned long long* __restrict__ total, uint32_t keep0,
                                                          const uint2* __restrict__ qmask) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t nz = list[0];
  if (i >= n || nz == 0) return;
  const uint2 h = hay[i];
  const uint32_t d = (uint32_t)__popc(h.x) + (uint32_t)__popc(h.y);
  if (d >= thresh) return;
  const uint32_t id = ids[i];
  if (id == 0 && !keep0) return;
  for (uint32_t k = 0; k < nz; ++k) {
    const uint32_t qi = list[1u + k];
    const uint2 mk = qmask ? qmask[qi] : make_uint2(0u, 0u);
    if (((h.x & mk.x) | (h.y & mk.y)) == 0) emit(rec, cap, total, qi, d, id);
  }
}

// the lone needle: see cbh_internal.h.  A thread takes 8 slots 256 apart (coalesced 8-byte loads).
constexpr unsigned kLoneSlots = 8;
__global__ __launch_bounds__(256) void k_find_one(const uint2* __restrict__ hay, const uint32_t* __restrict__ ids,
                                                  uint32_t n, uint32_t qlo, uint32_t qhi, uint32_t thresh,
                                                  unsigned* __restrict__ d_state, LoneBlock* __restrict__ host,
                                                  unsigned long long seq) {
  const uint32_t base = blockIdx.x * (256u * kLoneSlots) + threadIdx.x;
  bool wrote = false;
#pragma unroll
  for (unsigned k = 0; k < kLoneSlots; ++k) {
    const uint32_t i = base + k * 256u;
    if (i >= n) break;
    const uint2 hv = hay[i];
    const uint32_t d = (uint32_t)__popc(hv.x ^ qlo) + (uint32_t)__popc(hv.y ^ qhi);
    if (d < thresh) {
      const uint32_t id = ids[i];
      if (id != 0) {
        const unsigned slot = atomicAdd(&d_state[0], 1u);
        if (slot < LoneBlock::kRecs) {
          host->recs[slot] = ((cbh_record)d << 32) | id;
          wrote = true;
        }
      }
    }
  }
  if (wrote) __threadfence_system();  // this lane's records are in host memory before its workgroup reports
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(&d_state[1], 1u) == gridDim.x - 1u) {  // the last workgroup: everyone's matches are counted and written
      __threadfence();
      host->count = atomicExch(&d_state[0], 0u);
      d_state[1] = 0u;
      __threadfence_system();
      __hip_atomic_store(const_cast<unsigned long long*>(&host->done), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

}  // namespace

int launch_find_one(const uint64_t* d_hashes, const uint32_t* d_ids, size_t n, uint64_t q, int thresh, unsigned* d_state,
                    LoneBlock* h_block, unsigned long long seq, hipStream_t stream) {
  if (n == 0 || n > 0xfffffff0ull || !d_state || !h_block || thresh <= 0) return CBH_E_INVAL;
  const unsigned per_wg = 256u * kLoneSlots;
  hipLaunchKernelGGL(k_find_one, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(256), 0, stream,
                     reinterpret_cast<const uint2*>(d_hashes), d_ids, (uint32_t)n, (uint32_t)q, (uint32_t)(q >> 32),
                     (uint32_t)thresh, d_state, h_block, seq);
  CBH_HIP(hipGetLastError());
  return CBH_OK;
}

int wait_find_one(const LoneBlock* h_block, unsigned long long seq, hipStream_t stream) {
  const unsigned long long* flag = const_cast<const unsigned long long*>(&h_block->done);
  for (unsigned spins = 0;; ++spins) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return CBH_OK;
    if ((spins & 0xfffu) == 0xfffu) {  // every 4096 polls: is the stream still busy at all?
      const hipError_t q = hipStreamQuery(stream);
      if (q == hipSuccess) {  // the kernel has retired: its last store is visible by now, or something went wrong
        return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq ? CBH_OK : CBH_E_HIP;
      }
      if (q != hipErrorNotReady) {
        set_last_error("k_find_one", q);
        return CBH_E_HIP;
      }
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
}

// ---- which path a 64-bit search takes: the bucketed join, the popcount kernel above (EQ / PRE / FULL) or the matrix-core
// scan (prefilter / three-field / two-field).  The knobs and constants below are read nowhere else; the data enter only
// through the probe's rates and the join's own candidate count, which can still hand a call back.
namespace {

constexpr int kPreMax = 7;            // largest threshold served by the popcount kernel's low-word PRE form (r01: wins up to 7)
constexpr size_t kMfmaMinNq = 256;    // below this the needle expansion + tile padding is not worth it
constexpr size_t kMfmaMinN = 4096;
// The prefilter kernel is twice as fast as the three-field kernel while its candidates are rare and loses to it when
// they are not: every candidate costs a descriptor and one lane's walk of its chain's rows (~22 SIMD cycles).
// How many there are is a property of the data -- r_cand(t) = P[popc(fold(a) ^ fold(b)) < t] over the launch's
// needle x slot pairs: 5.8e-5 at t = 6, 2.7e-4 at t = 7 and 1.04e-3 at t = 8 for unrelated hashes, but anything for a
// library of scans of one form, blank frames or a video against itself.  The three-field kernel in turn pays for every
// TRUE match (a flagged group goes through three passes of sixteen ballots, 2.7e5 ms per unit of r_true against the
// prefilter's 0.7e5): where the candidates are mostly true matches -- a dense cluster of near-identical hashes -- the
// prefilter wins again, at any rate.  Measured per 10^12 pairs (tools/ab/adaptive_ab.py, profiles/r07_adaptive_ab_*.jsonl):
//   T_pre = 8.55 ms + 1.0e4 ms x r_cand  (8.8 / 8.9 / 9.5 / 11.3 ms at thresholds 4..7 of image hashes; the slope was 2.4e4
//   while the drain took one descriptor per lane instead of one candidate field, NOTES 23, and 1.3e4 while it walked a
//   chain's rows on all 64 bits instead of on their fold first -- re-fitted at threshold 7 of profiles/r12_lib_ab.json,
//   (11.315 - 8.55) / 2.7e-4, with the floor held; the true-match weights below are round 7's),
//   T_full = 15.75 ms + 2.7e5 ms x r_true.
// The probe counts both rates on a sample of the launch's pairs -- a few microseconds and one host round trip, against
// launches of milliseconds -- and the prefilter is taken while
//   r_cand - kTrueWeight x r_true <= "scan_pre_rate_e9" x 1e-9      (3.0e-4: where the prefilter tied with the three-field
//   kernel at the slope of 2.4e4, kTrueWeight = (2.7e5 - 0.7e5) / 2.4e4; at today's it reaches 11.6 ms there, 2.4 ms
//   short of the 48-bit prefilter below -- the kernel that takes the launches beyond it; the knob keeps its value, no
//   data set between the two was measured),
// which puts threshold 7 of unrelated hashes on the prefilter (11.3 ms against 13.8-17.0) and leaves 8 to the others.  Launches too small to pay for the round trip, and a probe that cannot run, take the fixed rule
// (thresholds <= 6: at 7 the prefilter's margin is 7 % on unrelated hashes and gone on anything denser).
//
// The 48-bit prefilter (PRE48: 16 folds + 32 plain bits, three MFMAs per four needle tiles = 3/4 of the three-field
// kernel's matrix work) sits between the two.  Its candidates are the pairs whose 48-bit distance h is <= t, a hundred
// times rarer than the fold's, plus the fields that wrap (h > 32 + t, its flag rule: hamm64_mfma.hip): 2.0e-6 per pair
// at thresholds 7 and 8 of unrelated hashes, but 3.1e-5 / 1.1e-4 / 3.6e-4 at 5 / 4 / 3, where it loses.  The probe counts
// that rate r48 in the same sample.  Fitted on tools/ab/adaptive_ab.py's five data sets (profiles/r08_adaptive_ab_fit.jsonl,
// ms per 10^12 pairs):
//   T_48 = 14.0 + 2.8e4 x r48 + 1.0e5 x r_true
// (floor 13.96-14.3 on image hashes at 7 / 8; 15.0 / 17.4 / 23.4 at thresholds 5 / 4 / 3 give the slope; the 2 % of equal
// hashes of "flat", 3.3e-4 true matches per pair, cost it 46.3 against the prefilter's 42.2 at threshold 7).
// It replaces the three-field kernel wherever T_48 is the smaller -- everywhere measured, by 14-17 % -- and the 32-bit
// prefilter only where T_48 < kPre48Margin x T_pre: T_pre is not good to better than 15 %.  A candidate costs the
// prefilter one descriptor per hit LANE, so candidates that come in runs of neighbouring rows (the frames of a video)
// are cheaper than their rate says: at threshold 7 the video set runs 12.4 ms on the prefilter where the model says
// 14.8, and 13.7 on PRE48, while image hashes with the same r_cand run 15.1 and 14.0.  The probe samples rows at
// random and cannot tell the two apart; the margin leaves threshold 7 where it was (on the prefilter) in both.
// "scan_pre48": -1 = routed like this, 0 = never, 1 = always for thresholds <= 16 (its bias 32 + t leaves a 6-bit field
// that much room).  Launches on the fixed rule never take it.
//
// The 16-bit prefilter (PRE16: fold16, ONE MFMA per four needle tiles = half of the 32-bit prefilter's matrix work) sits
// under it.  Its candidates are the pairs whose fold16 distance is < t, at the rate of uniform 16-bit words on unrelated
// hashes: 1.5e-5 per pair at t = 1, 2.6e-4 at 2, 2.1e-3 at 3 -- the probe counts that rate r16 in the same sample -- and a
// candidate costs it what it costs the 32-bit prefilter (the events, the drain and the re-check are the same code):
//   T_16 = 5.85 + 1.0e4 x r16 + 0.7e5 x r_true
// (6.09 ms per 10^12 pairs at threshold 1 of image hashes, r16 = 1.8e-5, against the 32-bit prefilter's 8.78 on the same
// box, profiles/r10_lib_ab.json; the issue model 24 M + 4 V gave 6.2 + 0.24).
// It is taken where T_16 < kPre16Margin x T_pre, at thresholds <= 8 (its bias 24 + t): threshold 1 of unrelated hashes;
// at 2 the model has the candidates at 2.6 ms, 8.45 against 0.9 x 8.55 = 7.7 (measured, forced: 8.15 against the 32-bit
// prefilter's 8.74 on the same box, profiles/r12_pre16_forced_t2.json -- inside the margin).  "scan_pre16": -1 = routed
// like this, 0 = never, 1 = always for thresholds <= 8 (larger thresholds are routed as if it were -1).  Launches on the
// fixed rule never take it.
constexpr int kPreStatic = 6;
constexpr double kTrueWeight = 8.0;
constexpr double kSlopePre = 1.0e4, kBaseFull = 15.75, kTrueFull = 2.7e5, kTruePre = 0.7e5;  // ms per 10^12 pairs
constexpr double kBasePre = 8.55, kBase48 = 14.0, kSlope48 = 2.8e4, kTrue48 = 1.0e5, kPre48Margin = 0.9;
constexpr double kBase16 = 5.85, kPre16Margin = 0.9;
constexpr uint64_t kProbeMinPairs = 1ull << 31;  // ~20 us of scan: below this the probe's round trip is not worth it

int g_scan_mfma = 1;             // "scan_mfma"
int g_pre_max_thresh = -1;       // "scan_mfma_pre_max"
int g_pre_rate_max_e9 = 300000;  // "scan_pre_rate_e9"
int g_pre48 = -1;                // "scan_pre48"
int g_pre16 = -1;                // "scan_pre16"
std::atomic<uint64_t> g_variant_mask[4];    // by ScanVariant; bit t: the most recent matrix-core launch at threshold t took it
std::atomic<uint64_t> g_n_probe{0};         // probes run
std::atomic<long long> g_last_rate_e9{-1};  // candidate rate x 1e9 the last probe found for its threshold
std::atomic<long long> g_last_true_e9{-1};  // ... and the rate of true (64-bit) matches
std::atomic<long long> g_last_rate48_e9{-1};  // ... and of the 48-bit prefilter's candidates
std::atomic<long long> g_last_rate16_e9{-1};  // ... and of the 16-bit prefilter's

enum class Join { None, IfCheaper, Forced };
enum class Kernel { PopcEq, PopcPre, PopcFull, Mfma };
struct Route {
  Join join;
  Kernel kernel;   // the scan: the whole call, or what a join that hands the call back leaves
  double scan_ms;  // the scan's modelled time, which the join has to beat
};

// the route of one launch of n slots x nq needles (n, nq >= 1, n <= 0xfffffff0, thresh >= 1)
Route route(size_t n, size_t nq, int thresh, bool masked) {
  Route r;
  // (the 16-bit prefilter at threshold 1; the 32-bit one at thresholds <= 5, at 6 and at 7 on unrelated hashes; the
  // three-field kernel)
  const double pairs = (double)n * (double)nq;
  const double pre_ms = pairs * (thresh <= 5 ? 8.7e-12 : thresh == 6 ? 9.5e-12 : thresh == 7 ? 11.3e-12 : 15.8e-12);
  r.scan_ms = thresh == 1 ? pairs * 6.1e-12 : pre_ms;
  // thresholds <= 8, "scan_mfma" 3: the join when its candidate count says it is cheaper than looking at every pair (only
  // asked where a scan on the 32-bit prefilter or the three-field kernel would take >= 1 ms: the bound weighs the call's
  // size against the fixed cost of the join's count, which a faster scan at threshold 1 did not change -- it keeps its
  // reach in pairs; what the join then has to beat is scan_ms); 4: whenever it can represent the call (the parity suite).
  // As shipped (1) every pair is compared: the join avoids comparisons, it does not make them faster.
  const bool joinable = thresh <= kJoinMaxThresh && !masked && n < 0xfffffff0ull;
  r.join = !joinable ? Join::None : g_scan_mfma == 4 ? Join::Forced
           : g_scan_mfma == 3 && pre_ms >= 1.0 ? Join::IfCheaper : Join::None;
  // "scan_mfma" 2 and 4 force the matrix cores for any size (tests); 3 sizes like 1
  const bool mfma = thresh <= 65 && (g_scan_mfma == 2 || g_scan_mfma == 4 ||
                                     (g_scan_mfma != 0 && nq >= kMfmaMinNq && n >= kMfmaMinN));
  r.kernel = mfma ? Kernel::Mfma : thresh == 1 ? Kernel::PopcEq : thresh <= kPreMax ? Kernel::PopcPre : Kernel::PopcFull;
  return r;
}

// which variant the launch at `thresh` took, behind the read-backs "scan_pre_mask" / "scan_pre48_mask" / "scan_pre16_mask".
// "scan_pre_mask" (get_scan_pre_mask) is the launches on the 32-bit prefilter OR those on the 16-bit one, and NOT those on
// the 48-bit one: bench.py prices the thresholds of that mask at the 32-bit prefilter's 64 flop per pair and the rest at
// 128.  With the 48-bit prefilter's launches in it the mask would cover every threshold of the sweep, 1..8, and bench.py
// then falls back to pricing ALL of them at 128: the 9 ms launches of thresholds 1..5 would read 1.4 x the peak.  Left
// with the three-field kernel's thresholds, a 14 ms launch reads 0.91 of the peak at 128 flop per pair; it issues 96
// (NOTES 18).  Without the 16-bit prefilter's launches bench.py would price their 6 ms at 128 flop per pair, twice the
// FP4 peak; inside, roofline_pre averages them in at 64 flop per pair where they issue 32 (NOTES 24).
void note_variant(int thresh, ScanVariant v) {
  for (int i = 1; i < 4; ++i)  // (Full keeps none)
    if (i == (int)v) g_variant_mask[i] |= 1ull << thresh; else g_variant_mask[i] &= ~(1ull << thresh);
}

int launch_popc(Kernel kernel, const uint64_t* d_hashes, const uint32_t* d_ids, size_t n, const uint64_t* d_q, size_t nq,
                int thresh, cbh_record* d_rec, size_t cap, unsigned long long* d_total, hipStream_t stream,
                const ScanOpts& o) {
  const uint32_t tile = kThreads * kH;
  const uint32_t tiles = (uint32_t)((n + tile - 1) / tile);
  // needle chunk: enough workgroups to fill 256 CUs x 8 waves/SIMD several times over, but each
  // workgroup amortises its 16 KB tile load over >= 1024 needles when there are that many.
  const uint32_t q_chunk = scan_chunk(tiles, nq, 16384, 1024, kQB);
  dim3 grid(tiles, (uint32_t)((nq + q_chunk - 1) / q_chunk)), block(kThreads);
  const uint2* hay = reinterpret_cast<const uint2*>(d_hashes);
#define CBH_SCAN(MODE)                                                                                                  \
  hipLaunchKernelGGL((k_hamm64_scan<kH, kQB, MODE>), grid, block, 0, stream, hay, d_ids, (uint32_t)n, d_q, (uint32_t)nq, \
                     q_chunk, (uint32_t)thresh, d_rec, (unsigned long long)cap, d_total, (uint32_t)o.keep_id0,            \
                     reinterpret_cast<const uint2*>(o.d_qmask))
  if (kernel == Kernel::PopcEq) CBH_SCAN(MODE_EQ);
  else if (kernel == Kernel::PopcPre) CBH_SCAN(MODE_PRE);
  else CBH_SCAN(MODE_FULL);
#undef CBH_SCAN
  CBH_HIP(hipGetLastError());
  return CBH_OK;
}

}  // namespace

bool scan_takes_mfma(size_t n, size_t nq, int thresh) {
  return thresh >= 1 && route(n, nq, thresh, false).kernel == Kernel::Mfma;
}

bool scan_routes_to_join(size_t n, size_t nq, int thresh, bool masked) {
  return thresh >= 1 && n >= 1 && nq >= 1 && route(n, nq, thresh, masked).join != Join::None;
}

ScanVariant scan_pick_pre(const uint64_t* d_hashes, size_t n, size_t n_total, const uint64_t* d_q, size_t nq, int thresh,
                          hipStream_t stream) {
  using V = ScanVariant;
  if (g_pre16 == 1 && thresh <= max_thresh(V::Pre16)) return V::Pre16;
  if (g_pre48 == 1 && thresh <= max_thresh(V::Pre48)) return V::Pre48;
  if (thresh > max_thresh(V::Pre32)) return V::Full;
  if (g_pre_max_thresh >= 0) return thresh <= g_pre_max_thresh ? V::Pre32 : V::Full;
  if (thresh > kProbeMaxThresh) return V::Full;
  double r_cand = 0, r_true = 0, r48 = 0, r16 = 0;
  if ((uint64_t)n_total * (uint64_t)nq < kProbeMinPairs ||
      !probe_fold_rates(d_hashes, n, d_q, nq, thresh, stream, &r_cand, &r_true, &r48, &r16))
    return thresh <= kPreStatic ? V::Pre32 : V::Full;  // the fixed rule
  g_last_rate_e9 = (long long)(r_cand * 1e9);
  g_last_true_e9 = (long long)(r_true * 1e9);
  g_last_rate48_e9 = (long long)(r48 * 1e9);
  g_last_rate16_e9 = (long long)(r16 * 1e9);
  g_n_probe++;
  // modelled times relative to the three-field kernel's
  const double d_pre = kSlopePre * (r_cand - kTrueWeight * r_true - (double)g_pre_rate_max_e9 * 1e-9);
  const bool pre = d_pre <= 0;
  const double t_pre = kBasePre + kSlopePre * r_cand + kTruePre * r_true, t_full = kBaseFull + kTrueFull * r_true;
  // (the 16-bit prefilter only against the 32-bit one: where that has lost already, fold16's candidates are denser still)
  if (g_pre16 != 0 && pre && thresh <= max_thresh(V::Pre16) &&
      kBase16 + kSlopePre * r16 + kTruePre * r_true < kPre16Margin * t_pre)
    return V::Pre16;
  if (g_pre48 != 0) {
    const double t_48 = kBase48 + kSlope48 * r48 + kTrue48 * r_true;
    if (pre ? t_48 < kPre48Margin * t_pre : t_48 < t_full) return V::Pre48;
  }
  return pre ? V::Pre32 : V::Full;
}

namespace {

// the second pass of a call with ScanOpts::zero_needles, behind whichever path took the call
int launch_zero_needles(const uint64_t* d_hashes, const uint32_t* d_ids, size_t n, const uint64_t* d_q, size_t nq,
                        int thresh, cbh_record* d_rec, size_t cap, unsigned long long* d_total, hipStream_t stream,
                        const ScanOpts& o) {
  Scratch scratch(stream);
  uint32_t* list = nullptr;
  CBH_HIP(scratch.get(&list, (nq + 1) * sizeof(uint32_t)));
  CBH_HIP(hipMemsetAsync(list, 0, sizeof(uint32_t), stream));
  hipLaunchKernelGGL(k_zero_needle_list, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, d_q, (uint32_t)nq, list);
  hipLaunchKernelGGL(k_zero_needle_scan, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     reinterpret_cast<const uint2*>(d_hashes), d_ids, (uint32_t)n, list, (uint32_t)thresh, d_rec,
                     (unsigned long long)cap, d_total, (uint32_t)o.keep_id0, reinterpret_cast<const uint2*>(o.d_qmask));
  CBH_HIP(hipGetLastError());
  return CBH_OK;
}

int scan_nonzero_needles(const uint64_t* d_hashes, const uint32_t* d_ids, size_t n, const uint64_t* d_q, size_t nq,
                         int thresh, cbh_record* d_rec, size_t cap, unsigned long long* d_total, hipStream_t stream,
                         const ScanOpts& o);

}  // namespace

int launch_hamm64_scan(const uint64_t* d_hashes, const uint32_t* d_ids, size_t n, const uint64_t* d_q, size_t nq,
                       int thresh, cbh_record* d_rec, size_t cap, unsigned long long* d_total, hipStream_t stream,
                       const ScanOpts& o) {
  if (n == 0 || nq == 0 || thresh <= 0) return CBH_OK;
  if (n > 0xfffffff0ull || nq > CBH_MAX_QUERIES_PER_CALL) return CBH_E_INVAL;
  const int rc = scan_nonzero_needles(d_hashes, d_ids, n, d_q, nq, thresh, d_rec, cap, d_total, stream, o);
  if (rc || !o.zero_needles) return rc;
  return launch_zero_needles(d_hashes, d_ids, n, d_q, nq, thresh, d_rec, cap, d_total, stream, o);
}

namespace {

int scan_nonzero_needles(const uint64_t* d_hashes, const uint32_t* d_ids, size_t n, const uint64_t* d_q, size_t nq,
                         int thresh, cbh_record* d_rec, size_t cap, unsigned long long* d_total, hipStream_t stream,
                         const ScanOpts& o) {
  const Route r = route(n, nq, thresh, o.d_qmask != nullptr);
  if (r.join != Join::None) {
    const bool force = r.join == Join::Forced;
    const int rc = launch_hamm64_join(d_hashes, d_ids, n, d_q, nq, thresh, d_rec, cap, d_total, stream, o, force, r.scan_ms);
    if (rc == CBH_OK || force || (rc != CBH_E_UNSUPPORTED && rc != CBH_E_NOMEM)) return rc;
    // (its scratch is all taken before the first record is written: a join that could not get it, like one whose count
    // said no, leaves the call to the scan)
    if (rc == CBH_E_NOMEM) cbh_clear_error();
  }
  if (r.kernel != Kernel::Mfma) return launch_popc(r.kernel, d_hashes, d_ids, n, d_q, nq, thresh, d_rec, cap, d_total, stream, o);
  const ScanVariant v = o.pre != ScanVariant::Auto ? o.pre : scan_pick_pre(d_hashes, n, n, d_q, nq, thresh, stream);
  if (thresh < 64) note_variant(thresh, v);
  return launch_hamm64_scan_mfma(d_hashes, d_ids, n, d_q, nq, thresh, d_rec, cap, d_total, stream, v, o);
}

}  // namespace

int set_scan_mfma(int mode) {
  if (mode < 0 || mode > 4) return CBH_E_INVAL;
  g_scan_mfma = mode;
  return CBH_OK;
}
int get_scan_mfma() { return g_scan_mfma; }
void set_scan_pre_max(int t) {
  if (t >= -1 && t <= max_thresh(ScanVariant::Pre32)) g_pre_max_thresh = t;
}
void set_scan_pre_rate(int e9) {
  if (e9 >= 0) g_pre_rate_max_e9 = e9;
}
void set_scan_pre48(int v) {
  if (v >= -1 && v <= 1) g_pre48 = v;
}
long long get_scan_pre_mask() { return (long long)(g_variant_mask[(int)ScanVariant::Pre32] | g_variant_mask[(int)ScanVariant::Pre16]); }
int set_scan_pre16(int v) {
  if (v < -1 || v > 1) return CBH_E_INVAL;
  g_pre16 = v;
  return CBH_OK;
}
long long get_scan_pre48_mask() { return (long long)g_variant_mask[(int)ScanVariant::Pre48].load(); }
long long get_scan_pre16_mask() { return (long long)g_variant_mask[(int)ScanVariant::Pre16].load(); }
long long get_scan_probes() { return (long long)g_n_probe.load(); }
long long get_scan_probe_rate_e9() { return g_last_rate_e9.load(); }
long long get_scan_probe_true_e9() { return g_last_true_e9.load(); }
long long get_scan_probe_rate48_e9() { return g_last_rate48_e9.load(); }
long long get_scan_probe_rate16_e9() { return g_last_rate16_e9.load(); }

}  // namespace cbh
